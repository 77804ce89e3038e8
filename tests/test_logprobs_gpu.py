"""GPU: token log-probabilities -- ops.token_logprobs (csrc/logprobs.hip) against the fp64 restatement of
tests/logprobs_ref.py (ids exact, values within the derived bound |got - ref| <= 2e-6 + 2^-23 |ref|), the step form
ops.decode_emit_logprobs over scripted steps, and generate(return_logprobs=True, top_logprobs=n) end to end on a
two-layer model: the graph path, the eager path and use_cache=False, a padded mask, sampling, a processor, fp8 weights
and the e4m3 cache.

Largest |got - ref| / bound seen on an MI355X: see DESIGN section 4.6."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import logprobs_ref as R  # noqa: E402

from macaw_llm_amd import modeling as Mo  # noqa: E402
from macaw_llm_amd import ops  # noqa: E402

INF, NAN = float("inf"), float("nan")
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
VS = [1, 7, 1023, 1024, 1025, 32000]            # one, below / at / above a workgroup's width, the model's V
NS = [0, 1, 5, 20]
PITCH = 3                                       # ld = V + 3, the padding holds NaN


def _bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _case(dname, V, rows):
    """(logits [rows, V + PITCH] of the dtype on the CPU, ids [rows], the restatement at n = 20).  Row 0: N(0, 4), in bf16
    full of exact ties at V = 32000, its largest value repeated in six columns (a tie group that n = 1 and n = 5 cut);
    row 1: -inf in a tenth of the columns, as the processors leave them, and NaN in a few; row 2: logits of scale 30"""
    g = torch.Generator().manual_seed(1000 * V + rows)
    x = torch.randn(rows, V, generator=g) * 2
    if V >= 7:
        x[0, torch.randperm(V, generator=g)[:6]] = x[0].max()
    if rows > 1:
        x[1, torch.randperm(V, generator=g)[:max(V // 10, 1)]] = -INF
        if V > 2:
            x[1, torch.randperm(V, generator=g)[:max(V // 100, 1)]] = NAN
        x[2] *= 15
    full = torch.full((rows, V + PITCH), NAN)
    full[:, :V] = x
    full = full.to(DTYPES[dname])
    ids = torch.randint(0, V, (rows,), generator=g)
    return full, ids, R.token_logprobs(full[:, :V], ids, 20)


RATIOS = []


def _compare(got, ref, n, what):
    """got = (lp, top_ids, top_lp) of the kernel, ref = the restatement at n = 20"""
    lp, ti, tl = got
    _, rti, _, rlp64, rtl64 = ref
    ok, ratio = R.within(lp.cpu().numpy(), rlp64)
    print(f"{what}: selected token, largest |got - ref| / bound = {ratio:.3f}")
    assert ok, (what, ratio)
    RATIOS.append(ratio)
    if n == 0:
        assert ti is None and tl is None
        return
    assert np.array_equal(ti.cpu().numpy(), rti[:, :n]), what           # ids are EXACT (the first n of the 20: the same rule)
    ok, ratio = R.within(tl.cpu().numpy(), rtl64[:, :n])
    print(f"{what}: top-{n}, largest |got - ref| / bound = {ratio:.3f}")
    assert ok, (what, ratio)
    RATIOS.append(ratio)


# ------------------------------------------------------------------------------- 1. token_logprobs, the kernel --
@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("dname", list(DTYPES))
def test_token_logprobs_is_the_restatement_ids_exact_values_inside_the_bound(dev, dname, V):
    for rows in (1, 3):
        full, ids, ref = _case(dname, V, rows)
        x = full.to(dev)[:, :V]                                          # pitch V + 3: the NaN padding is never read
        assert x.stride(0) == V + PITCH
        for n in NS:                                                     # n > V included
            got = ops.token_logprobs(x, V, ids.to(dev), n)
            _compare(got, ref, n, f"{dname} V={V} rows={rows} n={n}")
            again = ops.token_logprobs(x, V, ids.to(dev), n)             # the same input twice: the same bits
            assert torch.equal(_bits(got[0]), _bits(again[0]))
            if n:
                assert torch.equal(got[1], again[1]) and torch.equal(_bits(got[2]), _bits(again[2]))
                assert got[1].dtype == torch.long and tuple(got[1].shape) == tuple(got[2].shape) == (rows, n)
            assert got[0].dtype == torch.float32 and tuple(got[0].shape) == (rows,)


@pytest.mark.parametrize("V", [7, 1025])
@pytest.mark.parametrize("dname", list(DTYPES))
def test_token_logprobs_on_the_rows_the_rule_names(dev, dname, V):
    """all -inf, a +inf, NaN columns, fewer non-NaN columns than n, -0 next to +0, ids outside [0, V)"""
    g = torch.Generator().manual_seed(V)
    x = torch.randn(7, V, generator=g) * 3
    x[0] = -INF                                                          # no finite logit: degenerate
    x[1, V // 2] = INF                                                   # a +inf: degenerate
    x[1, 0] = -INF
    x[2, 1::2] = NAN                                                     # NaN columns take no mass and no slot
    x[3] = NAN
    x[3, [1, 4, 6]] = torch.tensor([0.5, -INF, 0.5])                     # three non-NaN columns: V < n for n = 5, 20
    x[4, :4] = torch.tensor([0.0, -0.0, 0.0, -0.0])                      # -0 == +0: ties to the lower column
    x[4, 4:] = -1.0 - x[4, 4:].abs()
    x[5] = x[6]                                                          # ids outside [0, V): NaN, the tops as usual
    full = torch.full((7, V + PITCH), NAN)
    full[:, :V] = x
    full = full.to(DTYPES[dname])
    ids = torch.tensor([0, V // 2, 1, 4, 1, -1, V])
    ids[2] = 1                                                           # a NaN column: NaN
    ref = R.token_logprobs(full[:, :V], ids, 20)
    assert np.isnan(ref[0][[0, 1, 2, 5, 6]]).all() and ref[0][3] == -INF and ref[1][3].tolist()[:4] == [1, 6, 4, -1]
    assert ref[1][4].tolist()[:4] == [0, 1, 2, 3]
    xd = full.to(dev)[:, :V]
    for n in NS:
        _compare(ops.token_logprobs(xd, V, ids.to(dev), n), ref, n, f"{dname} V={V} special n={n}")


# ------------------------------------------------------------------------- 2. decode_emit_logprobs, the step form --
@pytest.mark.parametrize("n_top", [0, 5])
@pytest.mark.parametrize("dname", ["bf16", "fp32"])
def test_decode_emit_logprobs_over_scripted_steps(dev, dname, n_top):
    B, V, n_max, pad, eos = 3, 1025, 4, 1000, 9
    ls = ops.LogprobState(B, n_max, n_top, pad, dev)
    assert not bool(ls.fin.any())
    ls.lp.fill_(7.5)                                                     # sentinels: what is not written keeps them
    if n_top:
        ls.top_ids.fill_(-9)
        ls.top_lp.fill_(7.5)
    g = torch.Generator().manual_seed(n_top)
    state = torch.zeros(4, dtype=torch.int32, device=dev)
    done = torch.zeros(B, dtype=torch.bool, device=dev)
    # (output column the emit wrote, tokens it stored, done flags behind it); sample 1 emits eos at step 1
    script = [(0, [5, 6, 7], [0, 0, 0]), (1, [8, eos, 1024], [0, 1, 0]), (2, [3, pad, 0], [0, 1, 0])]
    want = {}
    for col, toks, dn in script:
        lg = (torch.randn(B, V + PITCH, generator=g) * 3).to(DTYPES[dname]).to(dev)[:, :V]
        tok = torch.tensor(toks, device=dev)
        done.copy_(torch.tensor(dn, dtype=torch.bool))
        state[0], state[1] = 20 + col, col + 1                           # the emit has advanced the column
        before = state.clone()
        ops.decode_emit_logprobs(lg, V, tok, done, state, ls)
        assert torch.equal(state, before) and tok.tolist() == toks and done.tolist() == [bool(d) for d in dn]
        assert ls.fin.tolist() == dn                                     # the latch follows done
        want[col] = ops.token_logprobs(lg, V, tok, n_top)
    for col, (lp, ti, tl) in want.items():                               # bit for bit the stand-alone kernel's row
        live = [b for b in range(B) if not (col == 2 and b == 1)]
        assert torch.equal(_bits(ls.lp[live, col]), _bits(lp[live])), col
        if n_top:
            assert torch.equal(ls.top_ids[live, col], ti[live]) and torch.equal(_bits(ls.top_lp[live, col]), _bits(tl[live]))
    assert bool(torch.isfinite(ls.lp[1, 1])) and float(ls.lp[1, 1]) < 0                    # eos's own log-probability
    assert float(ls.lp[1, 2]) == 0.0                                     # finished BEFORE step 2: 0.0 / pad / 0.0
    if n_top:
        assert ls.top_ids[1, 2].tolist() == [pad] * n_top and ls.top_lp[1, 2].tolist() == [0.0] * n_top
    # a column outside [0, n_max) writes nothing; column 3 was never a step's: every sentinel is still there
    snap = (ls.lp.clone(), None if not n_top else ls.top_ids.clone(), None if not n_top else ls.top_lp.clone())
    lg = (torch.randn(B, V, generator=g) * 3).to(DTYPES[dname]).to(dev)
    tok = torch.tensor([1, 2, 3], device=dev)
    for col in (-1, n_max, n_max + 7):
        state[1] = col + 1
        ops.decode_emit_logprobs(lg, V, tok, done, state, ls)
    assert torch.equal(_bits(ls.lp), _bits(snap[0])) and bool((ls.lp[:, 3] == 7.5).all())
    if n_top:
        assert torch.equal(ls.top_ids, snap[1]) and torch.equal(_bits(ls.top_lp), _bits(snap[2]))
        assert bool((ls.top_ids[:, 3] == -9).all()) and bool((ls.top_lp[:, 3] == 7.5).all())


# ------------------------------------------------------------------------------------------- 3. generate() --
D, HEADS, LAYERS, V16, FF, B, P, N, PAD = 128, 2, 2, 16, 256, 2, 5, 8, 0


@functools.lru_cache(maxsize=None)
def _model(dname):
    """the two-layer model (D = 128, 2 heads of 64, fused projections, V = 16), its prompt [2, 5], the plain greedy ids
    without an eos and an eos that ends exactly one sample early"""
    from transformers import LlamaConfig
    dev = torch.device("cuda:0")
    torch.manual_seed(11)
    Mo.AUTO_FUSE = True
    cfg = LlamaConfig(hidden_size=D, intermediate_size=FF, num_hidden_layers=LAYERS, num_attention_heads=HEADS,
                      num_key_value_heads=HEADS, vocab_size=V16, max_position_embeddings=64)
    lm = Mo.fuse_model(Mo.LlamaForCausalLM(cfg).to(dev).to(DTYPES[dname])).eval()
    ids = torch.randint(3, V16, (B, P), generator=torch.Generator().manual_seed(5)).to(dev)
    free = lm.generate(input_ids=ids, max_new_tokens=N, eos_token_id=-1, pad_token_id=PAD).tolist()
    eos = None
    for b in range(B):                      # a token sample b emits within its first 6 and the other sample never does
        for c in range(N - 2):
            if eos is None and free[b][c] not in free[1 - b]:
                eos = free[b][c]
    assert eos is not None, free
    return lm, ids, eos


def _ends(ids, eos):
    """per sample the number of columns up to and including its eos"""
    W = ids.shape[1]
    return [row.index(eos) + 1 if eos in row else W for row in ids.tolist()]


def _check(out, plain, eos, n, greedy=True, early=True):
    assert isinstance(out, Mo.GenerateLogprobs)
    ids, lp, ti, tl = out
    assert ids.dtype == plain.dtype and torch.equal(ids, plain)                            # bit for bit, same width
    W = ids.shape[1]
    assert lp.dtype == torch.float32 and tuple(lp.shape) == (B, W)
    assert ti.dtype == torch.long and tl.dtype == torch.float32 and tuple(ti.shape) == tuple(tl.shape) == (B, W, n)
    ends = _ends(ids, eos)
    assert not early or min(ends) < N                                    # one sample finished early
    for b, end in enumerate(ends):
        assert bool(torch.isfinite(lp[b, :end]).all()) and bool((lp[b, :end] <= 0).all())
        if greedy:
            assert torch.equal(ids[b, :end], ti[b, :end, 0]) and torch.equal(_bits(lp[b, :end]), _bits(tl[b, :end, 0]))
        v, i = tl[b, :end], ti[b, :end]
        assert bool((v[:, 1:] <= v[:, :-1]).all())                       # sorted descending
        if n == V16:
            assert sorted(i[0].tolist()) == list(range(V16))
            assert float(torch.logsumexp(v.double(), dim=-1).abs().max()) <= V16 * 2e-6
        # the selected token's value is its entry in the tops
        pos = (i == ids[b, :end, None]).float().argmax(-1)
        assert torch.equal(_bits(v.gather(1, pos[:, None])[:, 0]), _bits(lp[b, :end]))
        assert bool((lp[b, end:] == 0).all()) and bool((ti[b, end:] == PAD).all()) and bool((tl[b, end:] == 0).all())
    return ends


PATHS = {"graph": {}, "eager": dict(decode_graph=False), "nocache": dict(use_cache=False)}


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("dname", ["bf16", "fp16"])
def test_generate_returns_the_plain_ids_and_consistent_logprobs(dev, dname, path):
    lm, ids, eos = _model(dname)
    kw = dict(input_ids=ids, max_new_tokens=N, eos_token_id=eos, pad_token_id=PAD, **PATHS[path])
    plain = lm.generate(**kw)
    assert torch.is_tensor(plain)
    out = lm.generate(return_logprobs=True, top_logprobs=V16, **kw)
    ends = _check(out, plain, eos, V16)
    assert min(ends) < max(ends)
    none = lm.generate(return_logprobs=True, **kw)                       # n = 0: the value alone
    assert none.top_ids is None and none.top_logprobs is None and torch.equal(none.ids, plain)
    assert torch.equal(_bits(none.logprobs), _bits(out.logprobs))
    five = lm.generate(return_logprobs=True, top_logprobs=5, **kw)
    assert torch.equal(five.top_ids, out.top_ids[..., :5]) and torch.equal(_bits(five.top_logprobs), _bits(out.top_logprobs[..., :5]))


@pytest.mark.parametrize("dname", ["bf16", "fp16"])
def test_generate_under_a_left_padded_mask_is_bit_identical_on_the_graph_and_the_eager_path(dev, dname):
    lm, ids, eos = _model(dname)
    mask = torch.tensor([[0, 0, 1, 1, 1], [1, 1, 1, 1, 1]], device=dev)
    kw = dict(input_ids=ids, attention_mask=mask, max_new_tokens=N, eos_token_id=eos, pad_token_id=PAD,
              return_logprobs=True, top_logprobs=V16)
    g, e = lm.generate(**kw), lm.generate(decode_graph=False, **kw)
    plain = lm.generate(**{k: v for k, v in kw.items() if k not in ("return_logprobs", "top_logprobs")})
    assert torch.equal(g.ids, plain) and torch.equal(e.ids, plain)
    for a, b in zip(g[1:], e[1:]):                                       # the same launches: the same bits
        assert torch.equal(_bits(a) if a.dtype == torch.float32 else a, _bits(b) if b.dtype == torch.float32 else b)
    assert bool(torch.isfinite(g.logprobs).all())


@pytest.mark.parametrize("path", ["graph", "eager"])
def test_generate_sampling_keeps_the_ids_and_scores_the_unwarped_distribution(dev, path):
    lm, ids, eos = _model("bf16")
    kw = dict(input_ids=ids, max_new_tokens=N, eos_token_id=eos, pad_token_id=PAD, do_sample=True, temperature=1.5, top_k=8,
              seed=1234, **PATHS[path])
    plain = lm.generate(**kw)
    out = lm.generate(return_logprobs=True, top_logprobs=V16, **kw)
    _check(out, plain, eos, V16, greedy=False)                           # every drawn token's log-probability is finite


@pytest.mark.parametrize("path", ["graph", "eager"])
def test_generate_scores_the_logits_behind_the_processors(dev, path):
    lm, ids, eos = _model("bf16")
    kw = dict(input_ids=ids, max_new_tokens=N, eos_token_id=-1, pad_token_id=PAD, return_logprobs=True, top_logprobs=V16,
              **PATHS[path])
    raw = lm.generate(**kw)
    pen = lm.generate(repetition_penalty=1.3, **kw)
    plain = lm.generate(**{k: v for k, v in kw.items() if k not in ("return_logprobs", "top_logprobs")}, repetition_penalty=1.3)
    _check(pen, plain, -1, V16, early=False)
    # the prompt's ids are history: token 0's logits are already rewritten, and with them every value of its row
    assert not torch.equal(_bits(raw.top_logprobs[:, 0]), _bits(pen.top_logprobs[:, 0]))
    assert not torch.equal(_bits(raw.logprobs), _bits(pen.logprobs))


@pytest.mark.parametrize("mode", [dict(decode_weights="fp8"), dict(kv_cache="fp8")], ids=["w-fp8", "kv-fp8"])
def test_generate_composes_with_fp8_weights_and_the_e4m3_cache(dev, mode):
    lm, ids, eos = _model("bf16")
    kw = dict(input_ids=ids, max_new_tokens=N, eos_token_id=eos, pad_token_id=PAD, **mode)
    try:
        plain = lm.generate(**kw)
        _check(lm.generate(return_logprobs=True, top_logprobs=V16, **kw), plain, eos, V16)
    finally:
        ops.clear_fp8_cache()
