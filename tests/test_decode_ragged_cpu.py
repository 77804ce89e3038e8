"""No GPU: the host side of generate(attention_mask=) -- what engine.ragged_from_mask makes of a mask (positions,
cache slots, per-sample step offsets, last valid rows), its all-ones short-circuit and its argument errors -- and the
pin of the feature's semantics to the reference: the restated masked greedy loop (oracle.restate.llama_forward with
attention_mask and position_ids = cumsum - 1, the loop tests/test_decode_ragged_gpu.py holds generate() to) reproduces
the logits and ids the reference's own cached, masked forward produced (tests/golden/masked_generate.pt, recorded by
scripts/make_golden_masked_generate.py)."""
import os

import pytest
import torch

from golden_util import GOLDEN_DIR, load_case
from oracle import configs, restate

from macaw_llm_amd import engine as eng
from macaw_llm_amd import modeling as Mo


# ------------------------------------------------------------------------------------------- shared helpers --
def masks_of(B, S0):
    """the three padded masks of the generate() tests: left padding, right padding, holes"""
    left = torch.ones((B, S0), dtype=torch.long)
    left[1, :5] = 0
    right = torch.ones((B, S0), dtype=torch.long)
    right[1, S0 - 5:] = 0             # (micro_all, S0 = 29: columns 24 ...)
    holes = torch.ones((B, S0), dtype=torch.long)
    for b in range(B):
        holes[b, 2 + b::7] = 0
    return {"left": left, "right": right, "holes": holes}


def last_valid(mask):
    S = mask.shape[1]
    return torch.where(mask != 0, torch.arange(S).expand_as(mask), torch.full_like(mask, -1)).max(1).values


def restated_masked_greedy(sd, emb, mask, cfg_l, n_new, force_ids=None):
    """greedy decode of a padded batch, restated: oracle.restate.llama_forward with the mask and position_ids =
    cumsum(mask) - 1 (clamped at 0: masked rows only need a valid table row), argmax at the last valid row for token 0
    and at the last row thereafter, the mask extended by a one per step.  Returns (ids [B, n_new], the predicting
    rows' logits [B, n_new, V]); force_ids feeds those ids instead of the argmax (teacher forcing)."""
    E = sd["llm.model.embed_tokens.weight"]
    B = emb.shape[0]
    mask = mask.to(emb.device).long()
    ids, zs = [], []
    for t in range(n_new):
        pos = (mask.cumsum(-1) - 1).clamp(min=0)
        _, logits = restate.llama_forward(sd, "llm.", emb, mask, cfg_l, position_ids=pos)
        row = last_valid(mask.cpu()).to(emb.device) if t == 0 else torch.full((B,), emb.shape[1] - 1, device=emb.device)
        z = logits[torch.arange(B, device=emb.device), row]
        nxt = z.argmax(-1) if force_ids is None else force_ids[:, t].to(emb.device)
        ids.append(nxt)
        zs.append(z)
        emb = torch.cat([emb, torch.nn.functional.embedding(nxt, E).unsqueeze(1).to(emb.dtype)], dim=1)
        mask = torch.cat([mask, torch.ones((B, 1), dtype=mask.dtype, device=mask.device)], dim=1)
    return torch.stack(ids, dim=1), torch.stack(zs, dim=1)


def top2_margin(z):
    t = z.float().topk(2, dim=-1).values
    return (t[..., 0] - t[..., 1]).min().item()


_MEMO = {}


def restated_case(kind):
    """(mask, ids, logits) of the restated loop on micro_all for one of the three masks: computed once, never modified"""
    if kind not in _MEMO:
        fx = load_case("micro_all")
        cfg = configs.get(fx["config_name"])
        mask = masks_of(*fx["inputs_embeds"].shape[:2])[kind]
        with torch.no_grad():
            ids, z = restated_masked_greedy(fx["state"], fx["inputs_embeds"], mask, cfg["llama"], 8)
        _MEMO[kind] = (mask, ids, z)
    return _MEMO[kind]


# ------------------------------------------------------------------------------------------------ host logic --
def _check(mask, want_pos, want_slot, want_toff, want_last):
    B, S0 = mask.shape
    rg, pos, last = eng.ragged_from_mask(mask, B, S0)
    assert rg.kmask.dtype == rg.slot.dtype == rg.t_off.dtype == pos.dtype == torch.int32 and last.dtype == torch.int64
    assert rg.kmask.is_contiguous() and rg.slot.is_contiguous() and rg.t_off.is_contiguous() and pos.is_contiguous()
    assert torch.equal(rg.kmask, (mask != 0).to(torch.int32))
    assert pos.view(B, S0).tolist() == want_pos
    assert rg.slot.tolist() == want_slot
    assert rg.t_off.tolist() == want_toff
    assert last.tolist() == [b * S0 + j for b, j in enumerate(want_last)]


@pytest.mark.parametrize("dtype", [torch.long, torch.int32, torch.bool, torch.uint8])
def test_left_right_holes_and_a_single_valid_token(dtype):
    mask = torch.tensor([[0, 0, 1, 1, 1],          # left padding
                         [1, 1, 1, 0, 0],          # right padding
                         [1, 0, 1, 0, 1],          # holes
                         [0, 0, 0, 1, 0],          # n_b = 1
                         [1, 1, 1, 1, 1]]).to(dtype)
    _check(mask,
           want_pos=[[0, 0, 0, 1, 2], [0, 1, 2, 2, 2], [0, 0, 1, 1, 2], [0, 0, 0, 0, 0], [0, 1, 2, 3, 4]],
           want_slot=[[-1, -1, 0, 1, 2], [0, 1, 2, -1, -1], [0, -1, 1, -1, 2], [-1, -1, -1, 0, -1], [0, 1, 2, 3, 4]],
           want_toff=[-2, -2, -2, -4, 0], want_last=[4, 2, 4, 3, 4])


def test_non_zero_means_valid():
    mask = torch.tensor([[0, 7, -1], [2, 0, 0]])
    _check(mask, want_pos=[[0, 0, 1], [0, 0, 0]], want_slot=[[-1, 0, 1], [0, -1, -1]], want_toff=[-1, -2],
           want_last=[2, 0])


def test_positions_follow_the_reference_rule_on_valid_rows():
    """position_ids = attention_mask.cumsum(-1) - 1 on every valid row (the reference fills masked rows with 1; any
    valid table row serves there), slots are exactly the positions of the valid rows: the cache is compacted in order"""
    g = torch.Generator().manual_seed(3)
    mask = (torch.rand((6, 37), generator=g) < 0.7).long()
    mask[:, 11] = 1
    rg, pos, last = eng.ragged_from_mask(mask, 6, 37)
    ref = mask.cumsum(-1) - 1
    v = mask.bool()
    assert torch.equal(pos.view(6, 37)[v].long(), ref[v]) and int(pos.min()) >= 0
    assert torch.equal(rg.slot[v].long(), ref[v]) and bool((rg.slot[~v] == -1).all())
    for b in range(6):
        n = int(mask[b].sum())
        assert sorted(rg.slot[b][v[b]].tolist()) == list(range(n)) and int(rg.t_off[b]) == n - 37
        assert int(last[b]) == b * 37 + int(torch.nonzero(mask[b]).max())


def test_a_mask_without_a_zero_is_the_unpadded_path():
    for dtype in (torch.long, torch.bool, torch.int32):
        assert eng.ragged_from_mask(torch.ones((3, 9), dtype=dtype), 3, 9) is None
    assert eng.ragged_from_mask(torch.full((2, 4), 5), 2, 4) is None


def test_argument_errors():
    with pytest.raises(ValueError, match="no valid token"):
        eng.ragged_from_mask(torch.tensor([[1, 1, 0], [0, 0, 0]]), 2, 3)
    for bad in (torch.ones((2, 4)), torch.ones((3, 3)), torch.ones((6,)), torch.ones((2, 3, 1))):
        with pytest.raises(ValueError, match="should be of size"):
            eng.ragged_from_mask(bad.long(), 2, 3)
    with pytest.raises(ValueError, match="ragged"):     # no masked attention over a cache: a prefill starts at row 0
        rg = eng.ragged_from_mask(torch.tensor([[0, 1]]), 1, 2)[0]
        eng.llama_layer_cached(torch.zeros((2, 32)), 1, 2, 3, None, 8, None, None, None, 2, 1e-6, *([None] * 9), ragged=rg)


def test_the_multimodal_switch_is_off_by_default():
    assert Mo.GENERATE_MASK[0] is False
    try:
        Mo.MM_LLMs.set_generate_mask(True)
        assert Mo.GENERATE_MASK[0] is True
        Mo.MM_LLMs.set_generate_mask()
        assert Mo.GENERATE_MASK[0] is False
    finally:
        Mo.GENERATE_MASK[0] = False


# --------------------------------------------------------------------------------------------- reference pin --
def test_the_restated_masked_loop_reproduces_the_reference():
    """the reference's own forward under the left mask (its prepare_inputs_for_generation, its KV cache) against the
    restated loop: per-step last-row logits within 5e-6 (the bound of
    test_oracle.test_reference_cached_decode_reproduces_the_committed_ids), ids exactly"""
    rec = torch.load(os.path.join(GOLDEN_DIR, "masked_generate.pt"), weights_only=False)
    fx = load_case("micro_all")
    assert rec["seed"] == fx["seed"] and rec["state_file"] == fx["state_file"] and "reference" in rec["source"]
    mask, ids, z = restated_case("left")
    assert torch.equal(rec["mask"], mask) and rec["ids"].shape == (2, 8)
    err = (z - rec["step_logits"]).abs().max().item()
    print(f"restated masked loop vs the reference ({rec['source'][:60]}...): max |d logits| {err:.3e}")
    assert err < 5e-6, err
    assert torch.equal(ids, rec["ids"])


@pytest.mark.parametrize("kind", ["left", "right", "holes"])
def test_the_restated_ids_are_decidable_and_those_of_each_sample_alone(kind):
    """the smallest top-1 / top-2 margin along the restated path stays above 5e-3 (so an fp32 engine within ~1e-4 of
    these logits must emit the same ids), and each sample run alone on its compacted valid tokens gives the ids it gives
    in the padded batch"""
    fx = load_case("micro_all")
    cfg = configs.get(fx["config_name"])
    mask, ids, z = restated_case(kind)
    m = top2_margin(z)
    print(f"{kind}: smallest top-1 / top-2 margin {m:.3e}")
    assert m > 5e-3, m
    with torch.no_grad():
        for b in range(mask.shape[0]):
            solo = fx["inputs_embeds"][b:b + 1][:, mask[b].bool()]
            one, _ = restated_masked_greedy(fx["state"], solo, torch.ones((1, solo.shape[1]), dtype=torch.long),
                                            cfg["llama"], 8)
            assert torch.equal(one[0], ids[b]), (kind, b, one[0].tolist(), ids[b].tolist())
