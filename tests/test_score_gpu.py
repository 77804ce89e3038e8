"""LlamaForCausalLM.score() on the GPU, on the two micro decoders of tests/test_session_gpu.py (hidden 128, FF 384, 2 layers,
vocab 107, bf16; 2 heads = head size 64 and 4 heads = head size 32): B = 3 prompts of S0 = 21 under the `left` mask with
every sample padded, options of lengths [[6, 1, 4], [2, 6], [5, 3, 3]] -- ragged counts and lengths, a length-1 option and
an absent one.

1. oracle: one oracle.restate.llama_forward per concatenation [valid prompt | option] with the fp32 weights gives z32, the
   same with the bf16 weights z16; lp32 = log_softmax(z32)[target]; per token |got - lp32| <= 2 * 3.0 * max_c |z16 - z32| of
   that row.  3.0 is the project's bf16-noise factor (test_decode_ragged_gpu, test_session_gpu._oracle); the 2 is derived:
   log_softmax(z)[t] = z[t] - logsumexp(z), and both terms move by at most the sup-norm change of z.  The same bound for
   use_cache=False and for an fp32 copy of the model through use_cache=False.
2. exact;  3. with generate();  4. top_logprobs;  5. routing;  6. LoRA;  7. refusals;  8. MM_LLMs.score.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from golden_util import load_case  # noqa: E402
from oracle import configs, restate  # noqa: E402

from macaw_llm_amd import modeling as Mo  # noqa: E402
from macaw_llm_amd import ops  # noqa: E402
from test_session_gpu import _Spy, _eos, _prompts, _small_llama  # noqa: E402

B, S0 = 3, 21
LENGTHS = [[6, 1, 4], [2, 6], [5, 3, 3]]
HEADS = pytest.mark.parametrize("heads", [2, 4], ids=["hd64", "hd32"])


@pytest.fixture(autouse=True)
def _restore_switches():
    yield
    Mo.AUTO_FUSE = True
    Mo.MM_LLMs.set_generate_mask(False)


def _options(V, lengths=LENGTHS, seed=11):
    g = torch.Generator().manual_seed(seed)
    return [[torch.randint(3, V, (n,), generator=g).tolist() for n in row] for row in lengths]


def _valid_ids(ids, mask):
    return [ids[b].cpu()[mask[b].cpu() != 0].tolist() for b in range(ids.shape[0])]


def _oracle(sd32, sd16, cfg_l, prompts, conts, dev):
    """prompts[b]: the valid ids of prompt b; conts[b][j]: option (b, j).  -> (lp32 [b][j] f64 [len], noise [b][j] [len],
    z32 [b][j] [len, V]): the restated log-probability of every option token, the bf16 noise of its logits row, the row"""
    lp32, noise, rows = [], [], []
    for p, opts in zip(prompts, conts):
        lp32.append([]), noise.append([]), rows.append([])
        for o in opts:
            ids = torch.tensor([p + o], device=dev)
            emb = torch.nn.functional.embedding(ids, sd32["llm.model.embed_tokens.weight"])
            with torch.no_grad():
                _, z32 = restate.llama_forward(sd32, "llm.", emb, None, cfg_l)
                _, z16 = restate.llama_forward(sd16, "llm.", emb.to(torch.bfloat16), None, cfg_l)
            z32 = z32[0, len(p) - 1:len(p) + len(o) - 1].float().cpu()          # the rows that predict the option's tokens
            z16 = z16[0, len(p) - 1:len(p) + len(o) - 1].float().cpu()
            t = torch.tensor(o)
            lp32[-1].append(torch.log_softmax(z32.double(), -1)[torch.arange(len(o)), t])
            noise[-1].append((z16 - z32).abs().max(-1).values.double())
            rows[-1].append(z32)
    return lp32, noise, rows


_MEMO = {}


def _case(dev, heads):
    """the model, the prompt, the options and their oracle: computed once per head count, never modified"""
    if heads not in _MEMO:
        lm, cfg_l, sd32, sd16 = _small_llama(dev, heads)
        ids, mask = _prompts(cfg_l, dev)[0]
        conts = _options(cfg_l["vocab_size"])
        _MEMO[heads] = (lm, cfg_l, ids, mask, conts, _oracle(sd32, sd16, cfg_l, _valid_ids(ids, mask), conts, dev))
    return _MEMO[heads]


def _within(res, conts, oracle, what):
    """|got - lp32| <= 2 * 3.0 * noise for every token of every option; prints and returns the worst ratio"""
    lp32, noise, _ = oracle
    got = res.token_logprobs.double().cpu()
    worst = 0.0
    for b, opts in enumerate(conts):
        for j, o in enumerate(opts):
            assert int(res.lengths[b, j]) == len(o)
            err = (got[b, j, :len(o)] - lp32[b][j]).abs()
            bound = 2 * 3.0 * noise[b][j]
            worst = max(worst, float((err / bound.clamp_min(1e-12)).max()))
            assert bool((err <= bound).all()), (what, b, j, err.tolist(), bound.tolist())
            assert bool((got[b, j, len(o):] == 0).all())
            want = float(got[b, j, :len(o)].sum().float())
            assert float(res.sums[b, j]) == pytest.approx(want, rel=1e-6)
    print(f"[score] {what}: worst |got - lp32| / (2 * 3.0 * max|z16 - z32|) = {worst:.3f}")
    return worst


def _same(a, b, what=""):
    for x, y, name in zip(a, b, Mo.ScoreResult._fields):
        assert (x is None) == (y is None), (what, name)
        if x is not None:
            assert x.dtype == y.dtype and x.shape == y.shape, (what, name)
            assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                               y.view(torch.int32) if y.dtype == torch.float32 else y), (what, name)


# ------------------------------------------------------------------------------------------------ 1. oracle --
@HEADS
def test_score_meets_the_fp32_oracle_on_both_paths_and_in_fp32(dev, heads):
    lm, cfg_l, ids, mask, conts, oracle = _case(dev, heads)
    res = lm.score(input_ids=ids, attention_mask=mask, continuations=conts)
    assert res.token_logprobs.dtype == torch.float32 and tuple(res.token_logprobs.shape) == (B, 3, 6)
    assert res.lengths.dtype == torch.int64 and res.lengths.tolist() == [[6, 1, 4], [2, 6, 0], [5, 3, 3]]
    assert res.sums.dtype == torch.float32 and res.top_ids is None and res.top_logprobs is None
    _within(res, conts, oracle, f"heads {heads} use_cache=True")
    _within(lm.score(input_ids=ids, attention_mask=mask, continuations=conts, use_cache=False), conts, oracle,
            f"heads {heads} use_cache=False")
    from transformers import LlamaConfig
    lm32 = Mo.LlamaForCausalLM(LlamaConfig(**cfg_l)).to(dev)
    lm32.load_state_dict({k[4:]: v for k, v in _small_llama(dev, heads)[2].items()})
    _within(lm32.eval().score(input_ids=ids, attention_mask=mask, continuations=conts, use_cache=False), conts, oracle,
            f"heads {heads} fp32 use_cache=False")
    # embeddings in place of ids: the same call
    emb = ops.embedding_fwd(lm.model.embed_tokens.weight, ids.reshape(-1)).view(B, S0, -1)
    _same(lm.score(inputs_embeds=emb, attention_mask=mask, continuations=conts), res, "inputs_embeds")


# ------------------------------------------------------------------------------------------------- 2. exact --
@HEADS
def test_score_is_exact_where_the_rule_says_so(dev, heads):
    lm, cfg_l, ids, mask, conts, _ = _case(dev, heads)
    kw = dict(input_ids=ids, attention_mask=mask, top_logprobs=3)
    res = lm.score(continuations=conts, **kw)
    _same(lm.score(continuations=conts, **kw), res, "the same call twice")
    # permuting a prompt's options permutes its rows
    perm = [2, 0, 1]
    moved = lm.score(continuations=[[conts[0][k] for k in perm], conts[1], conts[2]], **kw)
    for x, y, name in zip(moved, res, Mo.ScoreResult._fields):
        assert torch.equal(x[0], y[0][perm]) and torch.equal(x[1:], y[1:]), name
    # other tokens of the same length in one option leave the other options' values alone
    other = [[list(o) for o in p] for p in conts]
    other[2][1] = [(t + 17) % (cfg_l["vocab_size"] - 3) + 3 for t in other[2][1]]
    swapped = lm.score(continuations=other, **kw)
    keep = torch.ones((B, 3), dtype=torch.bool)
    keep[2, 1] = False
    keep = keep.to(dev)
    for x, y, name in zip(swapped, res, Mo.ScoreResult._fields):
        assert torch.equal(x[keep], y[keep]), name
    assert not torch.equal(swapped.token_logprobs[2, 1], res.token_logprobs[2, 1])
    # list form == tensor form, whatever lies behind an option's end
    cid = torch.full((B, 3, 6), -1, dtype=torch.long)
    cl = torch.zeros((B, 3), dtype=torch.long)
    for b, p in enumerate(conts):
        for j, o in enumerate(p):
            cid[b, j, :len(o)], cl[b, j] = torch.tensor(o), len(o)
    _same(lm.score(continuation_ids=cid.to(dev), continuation_lengths=cl.to(dev), **kw), res, "tensor form")
    _same(lm.score(continuation_ids=cid.to(dev), continuation_lengths=cl.to(dev), use_cache=False, **kw),
          lm.score(continuations=conts, use_cache=False, **kw), "tensor form, use_cache=False")
    # the absent option
    assert int(res.lengths[1, 2]) == 0 and float(res.sums[1, 2]) == float("-inf")
    assert bool((res.token_logprobs[1, 2] == 0).all()) and bool((res.top_ids[1, 2] == -1).all())
    assert bool((res.top_logprobs[1, 2] == 0).all())
    assert bool(torch.isfinite(res.sums[res.lengths > 0]).all()) and bool((res.sums[res.lengths > 0] < 0).all())


# ----------------------------------------------------------------------------------------- 3. with generate --
@HEADS
def test_score_of_generated_tokens_meets_the_oracle_next_to_generates_own_logprobs(dev, heads):
    lm, cfg_l, sd32, sd16 = _small_llama(dev, heads)
    ids, mask = _prompts(cfg_l, dev)[0]
    eos = _eos(dev, heads)
    gen = lm.generate(input_ids=ids, attention_mask=mask, max_new_tokens=6, eos_token_id=eos, pad_token_id=0,
                      return_logprobs=True)
    rows = gen.ids.cpu().tolist()
    ends = [r.index(eos) + 1 if eos in r else len(r) for r in rows]
    conts = [[r[:c]] for r, c in zip(rows, ends)]
    oracle = _oracle(sd32, sd16, cfg_l, _valid_ids(ids, mask), conts, dev)
    res = lm.score(input_ids=ids, attention_mask=mask, continuations=conts)
    _within(res, conts, oracle, f"heads {heads} score of generate()'s tokens")
    lp32 = oracle[0]
    for b, c in enumerate(ends):          # generate()'s own values: the same bound around the same oracle
        err = (gen.logprobs[b, :c].double().cpu() - lp32[b][0]).abs()
        assert bool((err <= 2 * 3.0 * oracle[1][b][0]).all()), (b, err.tolist())
    diff = max(float((res.token_logprobs[b, 0, :c] - gen.logprobs[b, :c]).abs().max()) for b, c in enumerate(ends))
    print(f"[score] heads {heads}: ends {ends}, largest |score - generate| = {diff:.3e}")
    # re-ranking generate's output in the form it comes in: ids on the device and the lengths
    width = gen.ids.shape[1]
    again = lm.score(input_ids=ids, attention_mask=mask, continuation_ids=gen.ids[:, None, :].contiguous(),
                     continuation_lengths=torch.tensor(ends, device=dev)[:, None])
    assert again.token_logprobs.shape[2] == width
    _within(again, conts, oracle, f"heads {heads} the same from generate()'s ids on the device")


# -------------------------------------------------------------------------------------------- 4. top-n --
@HEADS
def test_top_logprobs_are_ordered_masked_and_led_by_the_oracles_argmax(dev, heads):
    lm, cfg_l, ids, mask, conts, oracle = _case(dev, heads)
    res = lm.score(input_ids=ids, attention_mask=mask, continuations=conts, top_logprobs=5)
    plain = lm.score(input_ids=ids, attention_mask=mask, continuations=conts)
    assert torch.equal(res.token_logprobs, plain.token_logprobs) and torch.equal(res.sums, plain.sums)
    assert res.top_ids.dtype == torch.int64 and tuple(res.top_ids.shape) == (B, 3, 6, 5)
    assert res.top_logprobs.dtype == torch.float32 and tuple(res.top_logprobs.shape) == (B, 3, 6, 5)
    ti, tl = res.top_ids.cpu(), res.top_logprobs.cpu()
    _, noise, z32 = oracle
    for b in range(B):
        for j in range(3):
            n = int(res.lengths[b, j])
            assert bool((ti[b, j, n:] == -1).all()) and bool((tl[b, j, n:] == 0).all())
            assert bool((tl[b, j, :n, :-1] >= tl[b, j, :n, 1:]).all()) and bool((tl[b, j, :n] <= 0).all())
            assert bool(((ti[b, j, :n] >= 0) & (ti[b, j, :n] < cfg_l["vocab_size"])).all())
            for g in range(n):
                z = z32[b][j][g]
                assert float(z.max() - z[ti[b, j, g, 0]]) <= 3.0 * float(noise[b][j][g]), (b, j, g)
                hit = (ti[b, j, g] == conts[b][j][g]).nonzero()
                if hit.numel():           # the scored token among the top: the same value
                    assert float(tl[b, j, g, int(hit[0])]) == float(res.token_logprobs[b, j, g])


# ---------------------------------------------------------------------------------------------- 5. routing --
STEP_OPS = ("decode_step_attn", "decode_step_attn_var", "decode_step_attn_shared", "decode_step_attn_multi",
            "decode_step_attn_beam", "decode_linear")


@HEADS
def test_routing_one_prefill_at_b_rows_one_pass_per_layer_and_no_decode_step(dev, heads):
    lm, cfg_l, ids, mask, conts, _ = _case(dev, heads)
    n_layers, D, n, F = cfg_l["num_hidden_layers"], cfg_l["hidden_size"], 3, 5
    with _Spy("score_attn", "kv_append_rows", "flash_attn_fwd", "token_logprobs", *STEP_OPS) as spy:
        lm.score(input_ids=ids, attention_mask=mask, continuations=conts)
    assert len(spy.calls["score_attn"]) == n_layers
    for a in spy.calls["score_attn"]:
        assert a[0].shape[0] == B * n * F and tuple(a[6].shape) == (B, S0, 2 * D) and tuple(a[7].shape) == (B * n, F, 2 * D)
        assert a[8].dtype == torch.int32 and a[8].tolist() == [5, 0, 3, 1, 5, 0, 4, 2, 2] and a[9] is not None
        assert (a[10], a[11], a[12]) == (S0, B, n)
    assert len({a[6].data_ptr() for a in spy.calls["score_attn"]}) == n_layers       # a prompt cache per layer
    assert len(spy.calls["kv_append_rows"]) == n_layers                               # the compacting prefill, at B rows
    for a in spy.calls["kv_append_rows"]:
        assert tuple(a[4].shape) == (B, S0, 2 * D) and a[8] == B
    for a in spy.calls["flash_attn_fwd"]:
        assert a[4] == B
    assert [a[0].shape[0] for a in spy.calls["token_logprobs"]] == [B * n, B * n * F]
    assert all(len(spy.calls[k]) == 0 for k in STEP_OPS)
    # F = 0: token 0 alone, no pass
    with _Spy("score_attn", "token_logprobs", "linear_fwd") as spy:
        one = lm.score(input_ids=ids, attention_mask=mask, continuations=[[o[:1] for o in p] for p in conts])
    assert len(spy.calls["score_attn"]) == 0 and len(spy.calls["token_logprobs"]) == 1
    full = lm.score(input_ids=ids, attention_mask=mask, continuations=conts)
    assert tuple(one.token_logprobs.shape) == (B, 3, 1)
    assert torch.equal(one.token_logprobs[:, :, 0], full.token_logprobs[:, :, 0])     # token 0 does not depend on the rest
    # use_cache=False runs neither
    with _Spy("score_attn", "kv_append_rows") as spy:
        lm.score(input_ids=ids, attention_mask=mask, continuations=conts, use_cache=False)
    assert len(spy.calls["score_attn"]) == 0 and len(spy.calls["kv_append_rows"]) == 0


# ------------------------------------------------------------------------------------------------- 6. LoRA --
def test_a_live_adapter_is_scored_on_its_merged_weights(dev):
    from transformers import LlamaConfig
    from macaw_llm_amd import lora
    lm0, cfg_l, _, _ = _small_llama(dev, 2)
    ids, mask = _prompts(cfg_l, dev)[0]
    conts = _options(cfg_l["vocab_size"])
    torch.manual_seed(0)
    lm = Mo.LlamaForCausalLM(LlamaConfig(**cfg_l)).to(dev).to(torch.bfloat16)
    lm.load_state_dict(lm0.state_dict())
    lm = Mo.fuse_model(lm).eval()
    base = lm.score(input_ids=ids, attention_mask=mask, continuations=conts)
    _same(base, lm0.score(input_ids=ids, attention_mask=mask, continuations=conts), "the copy is the model")
    names = ["q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj"]
    lora.get_peft_model(lm, lora.LoraConfig(r=8, lora_alpha=16, target_modules=names, lora_dropout=0.0))
    g = torch.Generator(device=dev).manual_seed(3)
    with torch.no_grad():
        for n, q in lm.named_parameters():
            if ".lora_B." in n:
                q.copy_(torch.randn(q.shape, generator=g, device=dev) * 0.05)
    lm.eval()
    sd32 = {"llm." + k: v.detach().float() for k, v in lm.state_dict().items() if ".lora_" not in k}
    for name, mod in lm.named_modules():
        if hasattr(mod, "lora_A"):
            sd32[f"llm.{name}.weight"] = (mod.weight.detach().float() +
                                           2.0 * mod.lora_B.weight.detach().float() @ mod.lora_A.weight.detach().float())
    sd16 = {k: v.to(torch.bfloat16) for k, v in sd32.items()}
    oracle = _oracle(sd32, sd16, cfg_l, _valid_ids(ids, mask), conts, dev)
    res = lm.score(input_ids=ids, attention_mask=mask, continuations=conts)
    live = res.lengths > 0
    assert not torch.equal(res.token_logprobs, base.token_logprobs)
    assert float((res.sums[live] - base.sums[live]).abs().max()) > 1e-2
    _within(res, conts, oracle, "LoRA, merged fp32 oracle, use_cache=True")
    _within(lm.score(input_ids=ids, attention_mask=mask, continuations=conts, use_cache=False), conts, oracle,
            "LoRA, merged fp32 oracle, use_cache=False")


# -------------------------------------------------------------------------------------------- 7. refusals --
def test_the_refusals_that_need_the_model(dev):
    from transformers import LlamaConfig
    lm, cfg_l, ids, mask, conts, _ = _case(dev, 2)
    table = lm.config.max_position_embeddings
    n_valid = mask.sum(1).tolist()
    with pytest.raises(ValueError, match="beyond the rotary table"):
        lm.score(input_ids=ids, attention_mask=mask, continuations=[[[5] * (table - n_valid[b] + 1)] for b in range(B)])
    longest = n_valid.index(max(n_valid))                             # the least padded prompt is the first to run out
    with pytest.raises(ValueError, match=rf"prompt\(s\) \[{longest}\]"):
        lens = [table - max(n_valid)] * B
        lens[longest] += 1
        lm.score(input_ids=ids, attention_mask=mask, continuations=[[[5] * n] for n in lens], use_cache=False)
    lm32 = Mo.LlamaForCausalLM(LlamaConfig(**cfg_l)).to(dev).eval()
    with pytest.raises(ValueError, match=r"use_cache=True: fp32 parameters.*use use_cache=False"):
        lm32.score(input_ids=ids, attention_mask=mask, continuations=conts)
    with pytest.raises(ValueError, match="have no valid token"):
        lm.score(input_ids=ids, attention_mask=torch.zeros_like(mask), continuations=conts)
    with pytest.raises(ValueError, match=r"outside \[0, 107\)"):
        lm.score(input_ids=ids, attention_mask=mask, continuations=[[[107]], [[1]], [[2]]])


# --------------------------------------------------------------------------------------------- 8. MM_LLMs --
def test_mm_llms_score_runs_the_towers_once_and_equals_llm_score_on_its_embeddings(dev):
    from test_model_gpu import build_model, to_dev
    fx = load_case("micro_all")
    cfg = configs.get(fx["config_name"])
    model = build_model(cfg, fx["state"], torch.bfloat16, dev, fuse=True).eval()
    Mo.AUTO_FUSE = True
    inp = to_dev(fx["inputs"], dev)
    Bm = inp["input_ids"].shape[0]
    conts = _options(cfg["llama"]["vocab_size"], [[4, 2, 1]] + [[3, 5]] * (Bm - 1), seed=2)
    seen = []
    real = model.encode_image

    def counted(*a, **kw):
        seen.append("encode_image")
        return real(*a, **kw)
    model.encode_image = counted
    try:
        for on in (False, True):
            Mo.MM_LLMs.set_generate_mask(on)
            del seen[:]
            got = model.score(inp, conts, top_logprobs=2)
            assert seen == ["encode_image"]                                  # one tower pass for all the options
            with torch.no_grad():
                emb, ext_mask, _ = model.prepare_inputs_for_generation(inp)
            want = model.llm.score(inputs_embeds=emb, continuations=conts, top_logprobs=2,
                                   attention_mask=ext_mask if on else None)
            _same(got, want, f"mask {on}")
            assert got.lengths.tolist()[0] == [4, 2, 1] and bool(torch.isfinite(got.sums[got.lengths > 0]).all())
    finally:
        del model.encode_image
