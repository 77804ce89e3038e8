"""GPU: classifier-free guidance -- mk_cfg_combine against tests/cfg_ref.py at every path of the kernel, and
generate(guidance_scale=) against a restated loop in fp32, against the fp32 oracle on the bf16 paths, in composition with
the other switches, with the defaults, and through the multimodal forward."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cfg_ref as R  # noqa: E402
from golden_util import load_case  # noqa: E402
from oracle import configs  # noqa: E402
from test_decode_kv8_gpu import _Spy, _small_llama  # noqa: E402
from test_decode_ragged_cpu import restated_masked_greedy  # noqa: E402

from macaw_llm_amd import modeling as Mo  # noqa: E402
from macaw_llm_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu
INF, NAN = float("inf"), float("nan")
DTYPES = {"bfloat16": torch.bfloat16, "float16": torch.float16, "float32": torch.float32}
SCALES = (0.0, 0.5, 1.5, 7.5)
SENTINEL = 7.0


@pytest.fixture(autouse=True)
def _restore_switches():
    yield
    Mo.MM_LLMs.set_guidance()
    Mo.MM_LLMs.set_generate_mask(False)


# --------------------------------------------------------------------------------------------- the kernel --
def _run(x, V, B, s, dev, ld, off=0):
    """x fp-any CPU [2B, V] in the type under test -> (rows [0, B) after the launch as fp64 [B, V], whether everything
    else kept its bits).  The 2B rows lie at pitch ld, `off` elements into a buffer with a guard row at either end; pad
    columns and guard rows hold a sentinel"""
    flat = torch.full(((2 * B + 2) * ld + off,), SENTINEL, dtype=x.dtype)
    rows = flat[off + ld: off + ld + 2 * B * ld].view(2 * B, ld)
    rows[:, :V] = x
    d = flat.to(dev)
    view = d[off + ld: off + ld + 2 * B * ld].view(2 * B, ld)
    out = ops.cfg_combine(view, V, B, s)
    assert out.data_ptr() == view.data_ptr() and tuple(out.shape) == (B, ld) and out.stride(0) == ld
    got = d.cpu()
    g = got[off + ld: off + ld + 2 * B * ld].view(2 * B, ld)
    keep = flat.clone()                                           # the input, with the B x V written values put in
    keep[off + ld: off + ld + 2 * B * ld].view(2 * B, ld)[:B, :V] = g[:B, :V]
    bits = torch.int16 if x.element_size() == 2 else torch.int32
    return g[:B, :V].double().numpy(), torch.equal(got.view(bits), keep.view(bits)), d


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("V", [1, 40, 1023, 1025, 32003])
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_cfg_combine_is_the_restated_rule_and_writes_rows_0_to_b_only(dev, dtype, V, B):
    """ld in (V, V + 5) and s in (0, 0.5, 1.5, 7.5): |got - ref64| <= (|s| + |1 - s|) 2e-6 + u |ref64|, equal -inf / NaN
    patterns, rows [B, 2B), pad columns and the memory around the rows bit for bit, two launches bit-identical"""
    g = torch.Generator().manual_seed(V * 7 + B)
    x = (torch.randn((2 * B, V), generator=g) * 4.0).to(DTYPES[dtype])
    worst = 0.0
    for ld in (V, V + 5):
        for s in SCALES:
            ref = R.combine(x, V, B, s)
            got, same, _ = _run(x, V, B, s, dev, ld)
            again, _, _ = _run(x, V, B, s, dev, ld)
            ok, ratio = R.within(got, ref, s, dtype)
            worst = max(worst, ratio)
            assert ok, (dtype, V, B, ld, s, ratio)
            assert same, (dtype, V, B, ld, s)
            assert np.array_equal(got, again, equal_nan=True), (dtype, V, B, ld, s)
    print(f"{dtype} V={V} B={B}: largest |got - ref| / bound = {worst:.3f}")


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_cfg_combine_masked_columns_nan_and_degenerate_rows(dev, dtype):
    """-inf columns in c, in u and in both, NaN columns in either, a conditional row with +inf, a negative row that is all
    -inf; on the vector path (aligned), with a misaligned base and with an odd pitch"""
    V, B = 1031, 4
    g = torch.Generator().manual_seed(11)
    x = torch.randn((2 * B, V), generator=g) * 4.0
    c, u = x[:B], x[B:]
    c[0, 3::7], u[0, 5::7], c[0, 100:120], u[0, 110:130] = -INF, -INF, -INF, -INF       # in c, in u, in both
    c[1, 17], u[1, 18], c[1, 19], u[1, 19], c[1, 20], u[1, 21] = NAN, NAN, -INF, NAN, NAN, -INF
    c[2, 64] = INF                                               # degenerate conditional row: all NaN
    u[3, :] = -INF                                               # degenerate negative row: NaN, -inf where c is masked
    c[3, 8:16] = -INF
    x = x.to(DTYPES[dtype])
    for ld, off in ((V + 1, 0), (V + 1, 1), (V + 2, 0), (V, 0)):
        for s in (1.5, 0.0):
            ref = R.combine(x, V, B, s)
            assert np.isneginf(ref[0, 3]) and np.isfinite(ref[0, 5]) and np.isneginf(ref[0, 115])
            assert np.isnan(ref[1, 17]) and np.isnan(ref[1, 18]) and np.isneginf(ref[1, 19]) and np.isnan(ref[1, 20])
            assert np.isnan(ref[2]).all() and np.isneginf(ref[3, 8:16]).all() and np.isnan(ref[3, 16:]).all()
            got, same, _ = _run(x, V, B, s, dev, ld, off)
            ok, ratio = R.within(got, ref, s, dtype)
            assert ok and same, (dtype, ld, off, s, ratio)
            # a column the negative prompt rules out is not guided: log_softmax(c) there, whatever the scale
            lc = R.row_lp64(x[0])
            assert np.abs(got[0, 5] - lc[5]) <= 2e-6 + R.ULP[dtype] * abs(lc[5])


def test_cfg_combine_refuses_bad_arguments_without_a_launch(dev):
    x = torch.zeros((4, 8), dtype=torch.bfloat16, device=dev)
    for kw in (dict(V=0), dict(V=9), dict(B=0), dict(scale=INF), dict(scale=NAN)):
        a = dict(dict(V=8, B=2, scale=1.5), **kw)
        rc = ops._L.load().mk_cfg_combine(x.data_ptr(), 8, a["V"], a["B"], a["scale"], ops.dt(x), None)
        assert rc == -1, kw
    with pytest.raises(ops.MacawHipError):
        ops.cfg_combine(x, 8, 3, 1.5)
    torch.cuda.synchronize()
    assert not bool(x.any())


# --------------------------------------------------------------------------------- generate(): fp32, restated --
@pytest.fixture(scope="module")
def micro32(dev):
    from test_model_gpu import build_model
    fx = load_case("micro_all")
    cfg = configs.get(fx["config_name"])
    return build_model(cfg, fx["state"], torch.float32, dev).eval(), fx, cfg


def test_generate_fp32_guided_ids_are_the_restated_loop_and_differ_from_greedy(dev, micro32):
    """use_cache=False in fp32, B = 2, the negative prompt the prompt's last 9 of 29 rows, s = 3: the ids equal a loop
    that runs the model's own forward over the two prefixes separately, combines with cfg_ref and takes the argmax (its
    smallest top-1 / top-2 margin recomputed here and > 5e-3, as in test_decode_ragged_gpu).  The loop's guided ids
    differ from its greedy ids, so a generate() that swallows the arguments fails"""
    model, fx, cfg = micro32
    emb = fx["inputs_embeds"].to(dev)
    B, S0, _ = emb.shape
    neg, s, N = emb[:, 20:].contiguous(), 3.0, 8
    E = model.llm.model.embed_tokens.weight
    V = model.llm.lm_head.weight.shape[0]

    def last_logits(e):
        return model.llm(inputs_embeds=e.contiguous()).logits[:, -1].float()

    c, u, p = emb, neg, emb
    want, greedy, margin = [], [], INF
    with torch.no_grad():
        for _ in range(N):
            g = R.combine(torch.cat([last_logits(c), last_logits(u)]).cpu(), V, B, s)
            top = np.sort(g, axis=1)[:, -2:]
            margin = min(margin, float((top[:, 1] - top[:, 0]).min()))
            nxt = torch.from_numpy(g.argmax(1)).to(dev)
            want.append(nxt)
            e1 = torch.nn.functional.embedding(nxt, E).unsqueeze(1)
            c, u = torch.cat([c, e1], 1), torch.cat([u, e1], 1)
            ng = last_logits(p).argmax(-1)
            greedy.append(ng)
            p = torch.cat([p, torch.nn.functional.embedding(ng, E).unsqueeze(1)], 1)
    want, greedy = torch.stack(want, 1), torch.stack(greedy, 1)
    print(f"guided {want.tolist()}, greedy {greedy.tolist()}, smallest guided top-1 / top-2 margin {margin:.3e}")
    assert not torch.equal(want, greedy) and all(not torch.equal(want[b], greedy[b]) for b in range(B))
    assert margin > 5e-3, margin
    kw = dict(max_new_tokens=N, eos_token_id=-1, pad_token_id=106, use_cache=False)
    got = model.llm.generate(inputs_embeds=emb, negative_inputs_embeds=neg, guidance_scale=s, **kw)
    assert got.dtype == torch.long and torch.equal(got, want), (got.tolist(), want.tolist())
    assert torch.equal(model.llm.generate(inputs_embeds=emb, **kw), greedy)
    # fp32 with use_cache=True: two lengths need the per-sample-position kernels, equal lengths do not
    with pytest.raises(ValueError, match="use_cache=False"):
        model.llm.generate(inputs_embeds=emb, negative_inputs_embeds=neg, guidance_scale=s, **dict(kw, use_cache=True))


# ------------------------------------------------------------------------- generate(): bf16 against the oracle --
def _ids(V, B, S, seed, dev):
    return torch.randint(3, V, (B, S), generator=torch.Generator().manual_seed(seed)).to(dev)


def _oracle_state(lm):
    return {"llm." + k: v.detach().float() for k, v in lm.state_dict().items()}


def _guided_rows(sd, ids, neg, cfg_l, s, got, mask=None, neg_mask=None):
    """the guided scores [B, N, V] (fp64) of the restated loops over the two prompts, teacher-forced on `got`"""
    E = sd["llm.model.embed_tokens.weight"]
    zs = []
    for p, m in ((ids, mask), (neg, neg_mask)):
        m = torch.ones_like(p) if m is None else m
        _, z = restated_masked_greedy(sd, torch.nn.functional.embedding(p, E), m, cfg_l, got.shape[1], force_ids=got)
        zs.append(z.float().cpu())
    B, N, V = zs[0].shape
    return np.stack([R.combine(torch.cat([zs[0][:, t], zs[1][:, t]]), V, B, s) for t in range(N)], axis=1)


def _against_the_oracle(lm, cfg_l, ids, neg, s, outs, **masks):
    """every id is the fp32 oracle's guided argmax, teacher-forced on the path's own ids, or loses to it by no more than
    the bf16 noise there: g32[top] - g32[id] <= 3.0 * max|g16 - g32| (the rule of
    test_decode_ragged_gpu.test_generate_bf16_graph_and_eager_step_ids_against_the_fp32_oracle, on the guided scores)"""
    sd32 = _oracle_state(lm)
    sd16 = {k: v.to(torch.bfloat16) for k, v in sd32.items()}
    with torch.no_grad():
        for tag, got in outs.items():
            g32 = _guided_rows(sd32, ids, neg, cfg_l, s, got, **masks)
            g16 = _guided_rows(sd16, ids, neg, cfg_l, s, got, **masks)
            at = np.take_along_axis(g32, got.cpu().numpy()[..., None], axis=-1)[..., 0]
            margin, noise = g32.max(-1) - at, np.abs(g16 - g32).max(-1)
            print(f"{tag}: ids off the oracle's argmax {(margin > 0).sum()}, worst margin / noise "
                  f"{(margin / np.maximum(noise, 1e-12)).max():.3f}")
            assert (margin <= 3.0 * noise).all(), (tag, margin.tolist(), noise.tolist())


@pytest.mark.parametrize("S_neg", [21, 13])
def test_generate_bf16_graph_eager_step_and_recompute_ids_against_the_fp32_oracle(dev, S_neg):
    """equal lengths (the unpadded path at 2B rows) and two lengths (the padded-batch path): the graph path,
    decode_graph=False and use_cache=False within the bf16 noise of the fp32 oracle.  With two lengths
    decode_graph=False is the eager STEP loop -- the captured launches one by one -- and its ids are the graph's bit
    for bit.  With equal lengths it is the eager cached loop at host positions (rope, copy, flash attention: other
    attention kernels than the step's, as for every unpadded call; test_model_gpu asks 90 % agreement of the two for
    that reason), so only the oracle rule holds there: measured on an MI355X, sample 0 parts at column 4 (45 on the graph
    path, the oracle's argmax; 32 on the eager and the recomputing path, 2.147 x the bf16 noise below it, inside the
    rule's 3.0)."""
    lm, cfg_l = _small_llama(dev)
    B, S0, N, s = 3, 21, 12, 2.0
    nl, V = cfg_l["num_hidden_layers"], cfg_l["vocab_size"]
    ids, neg = _ids(V, B, S0, 3, dev), _ids(V, B, S_neg, 4, dev)
    kw = dict(input_ids=ids, negative_prompt_ids=neg, guidance_scale=s, max_new_tokens=N, eos_token_id=-1, pad_token_id=0)
    step = "decode_step_attn_var" if S_neg != S0 else "decode_step_attn"
    with _Spy("decode_step_attn_var", "decode_step_attn", "cfg_combine") as spy:
        g = lm.generate(**kw)
        assert len(spy.calls[step]) == 2 * nl and len(spy.calls["cfg_combine"]) == 3       # token 0, eager, captured
        e = lm.generate(decode_graph=False, **kw)
        assert len(spy.calls["cfg_combine"]) == 3 + N
        if S_neg != S0:       # (the unpadded eager loop is the host-position one: other attention launches)
            assert len(spy.calls[step]) == (2 + N - 1) * nl
        assert all(tuple(a[0].shape) == (2 * B, V) and a[1:] == (V, B, s) for a in spy.calls["cfg_combine"])
        other = "decode_step_attn" if S_neg != S0 else "decode_step_attn_var"
        assert spy.calls[other] == []
    n = lm.generate(use_cache=False, **kw)
    assert g.shape == e.shape == n.shape == (B, N) and g.dtype == torch.long
    if S_neg != S0:
        assert torch.equal(g, e), (g.tolist(), e.tolist())
    plain = lm.generate(input_ids=ids, max_new_tokens=N, eos_token_id=-1, pad_token_id=0)
    assert not torch.equal(plain, g)
    _against_the_oracle(lm, cfg_l, ids, neg, s, {"graph": g, "eager": e, "recompute": n})


# ------------------------------------------------------------------------------------------------ composition --
COMPOSE = {"kv8": dict(kv_cache="fp8"), "w8": dict(decode_weights="fp8"), "sample": dict(do_sample=True, seed=5),
           "penalty": dict(repetition_penalty=1.2), "logprobs": dict(return_logprobs=True, top_logprobs=3),
           "left": dict(attention_mask="left")}


@pytest.mark.parametrize("case", list(COMPOSE))
def test_generate_guidance_composes_with_the_other_switches(dev, case):
    """one call each: deterministic; graph equals eager step (the two fp8 switches run on the graph path alone);
    sample b's ids are those of sample b run alone with the same lengths (sampling: sample 0, whose random numbers do not
    move); the log-probabilities are ops.token_logprobs of the guided logits"""
    lm, cfg_l = _small_llama(dev)
    B, S0, S_neg, N, s = 3, 21, 13, 12, 2.0
    V = cfg_l["vocab_size"]
    ids, neg = _ids(V, B, S0, 3, dev), _ids(V, B, S_neg, 4, dev)
    mode = dict(COMPOSE[case])
    mask = None
    if mode.pop("attention_mask", None):
        mask = torch.ones((B, S0), dtype=torch.long, device=dev)
        for b in range(B):
            mask[b, :2 + 3 * b] = 0
    kw = dict(guidance_scale=s, max_new_tokens=N, eos_token_id=-1, pad_token_id=0, **mode)

    def call(rows=slice(None), **more):
        m = dict(attention_mask=mask[rows].contiguous()) if mask is not None else {}
        return lm.generate(input_ids=ids[rows].contiguous(), negative_prompt_ids=neg[rows].contiguous(), **m, **kw, **more)

    with _Spy("cfg_combine", "decode_emit_logprobs") as spy:
        out = call()
        assert len(spy.calls["cfg_combine"]) == 3
        assert (len(spy.calls["decode_emit_logprobs"]) == 3) == (case == "logprobs")
    first = out.ids if case == "logprobs" else out
    assert first.shape == (B, N) and first.dtype == torch.long
    again = call()
    assert torch.equal(first, again.ids if case == "logprobs" else again)
    plain = lm.generate(input_ids=ids, max_new_tokens=N, eos_token_id=-1, pad_token_id=0,
                        **{k: v for k, v in mode.items() if k != "return_logprobs" and k != "top_logprobs"},
                        **(dict(attention_mask=mask) if mask is not None else {}))
    assert not torch.equal(plain, first)                          # guidance steers
    if case not in ("kv8", "w8"):
        eager = call(decode_graph=False)
        assert torch.equal(first, eager.ids if case == "logprobs" else eager)
    for b in range(1 if case == "sample" else B):
        one = call(slice(b, b + 1))
        one = one.ids if case == "logprobs" else one
        assert torch.equal(one[0], first[b]), (case, b, one[0].tolist(), first[b].tolist())
    if case == "logprobs":
        assert torch.equal(out.logprobs, eager.logprobs) and torch.equal(out.top_ids, eager.top_ids)
        assert torch.equal(out.top_logprobs, eager.top_logprobs)
        guided = []
        real = ops.cfg_combine

        def keep(*a, **k):
            guided.append(real(*a, **k).clone())
            return guided[-1]
        ops.cfg_combine = keep
        try:
            e2 = call(decode_graph=False)
        finally:
            ops.cfg_combine = real
        assert torch.equal(e2.ids, first) and len(guided) == N
        for t, lg in enumerate(guided):
            assert tuple(lg.shape) == (B, V)
            lp, ti, tl = ops.token_logprobs(lg, V, first[:, t].contiguous(), 3)
            assert torch.equal(lp, out.logprobs[:, t]) and torch.equal(ti, out.top_ids[:, t])
            assert torch.equal(tl, out.top_logprobs[:, t])
        # renormalised: the top value of every step is a log-probability, and the top id is the greedy token
        assert bool((out.top_logprobs <= 0).all()) and torch.equal(out.top_ids[..., 0], first)


def test_generate_guidance_runs_on_the_merged_copies_of_lora_adapters(dev):
    """adapters with non-zero B: the guided call decodes on the per-call merged weights (nothing merged in place), the
    graph path and the eager step loop bit for bit the same, and not the adapted model's plain greedy ids"""
    from test_lora_gpu import _mm_lora
    model, fx = _mm_lora(dev, p=0.0)
    with torch.no_grad():
        for n, q in model.llm.named_parameters():
            if ".lora_B." in n:
                q.copy_(torch.randn_like(q.float()) * 0.05)
    model.eval()
    emb = fx["inputs_embeds"].to(dev).to(torch.bfloat16)
    w0 = {n: q.detach().clone() for n, q in model.llm.named_parameters()}
    kw = dict(inputs_embeds=emb, max_new_tokens=12, eos_token_id=-1, pad_token_id=106)
    guide = dict(negative_inputs_embeds=emb[:, 20:].contiguous(), guidance_scale=2.0)
    with _Spy("cfg_combine", "lora_merge_") as spy:
        g = model.llm.generate(**kw, **guide)
        assert len(spy.calls["cfg_combine"]) == 3 and len(spy.calls["lora_merge_"]) > 0
    e = model.llm.generate(decode_graph=False, **kw, **guide)
    assert g.shape == (emb.shape[0], 12) and torch.equal(g, e), (g.tolist(), e.tolist())
    assert all(torch.equal(w0[n], q) for n, q in model.llm.named_parameters())
    assert not torch.equal(g, model.llm.generate(**kw))


# --------------------------------------------------------------------------------------------------- defaults --
@pytest.mark.parametrize("mode", [dict(), dict(decode_graph=False), dict(use_cache=False)])
def test_generate_with_the_scale_off_is_plain_greedy_and_launches_no_combine(dev, mode):
    lm, cfg_l = _small_llama(dev)
    B, S0, N = 2, 21, 8
    V = cfg_l["vocab_size"]
    ids, neg = _ids(V, B, S0, 3, dev), _ids(V, B, 13, 4, dev)
    kw = dict(input_ids=ids, max_new_tokens=N, eos_token_id=-1, pad_token_id=0, **mode)
    plain = lm.generate(**kw)
    with _Spy("cfg_combine") as spy:
        for off in (dict(), dict(guidance_scale=None), dict(guidance_scale=1.0), dict(guidance_scale=1)):
            got = lm.generate(negative_prompt_ids=neg, negative_prompt_attention_mask=torch.ones_like(neg), **off, **kw)
            assert torch.equal(got, plain), off
        assert spy.calls["cfg_combine"] == []
        on = lm.generate(negative_prompt_ids=neg, guidance_scale=2.0, **kw)
        assert len(spy.calls["cfg_combine"]) > 0 and not torch.equal(on, plain)


# ------------------------------------------------------------------------------------------------- multimodal --
def test_multimodal_forward_under_set_guidance_is_the_explicit_call(dev):
    """micro MM_LLMs with its image, audio and video rows: the inference forward under set_guidance(2.0) equals
    llm.generate(..., negative_inputs_embeds=embed(input_ids), guidance_scale=2.0) bit for bit, with set_generate_mask
    off and on; after set_guidance() the result is today's"""
    from test_model_gpu import build_model, to_dev
    fx = load_case("micro_all")
    cfg = configs.get(fx["config_name"])
    model = build_model(cfg, fx["state"], torch.bfloat16, dev, fuse=True).eval()
    inp = to_dev(fx["inputs"], dev)
    inp["inference"] = True
    Mo.AUTO_FUSE = True
    with torch.no_grad():
        emb, am, _ = model.prepare_inputs_for_generation(inp)
        tids = inp["input_ids"].long()
        text = ops.embedding_fwd(model.llm.model.embed_tokens.weight, tids.reshape(-1)).view(*tids.shape, -1)
        assert text.shape[1] < emb.shape[1]                       # the modal rows are what the negative prompt lacks
        gk = dict(inputs_embeds=emb, max_new_tokens=128, eos_token_id=2, bos_token_id=1, pad_token_id=32006)
        today = model.llm.generate(**gk)
        want_off = model.llm.generate(negative_inputs_embeds=text, guidance_scale=2.0, **gk)
        want_on = model.llm.generate(negative_inputs_embeds=text, guidance_scale=2.0, attention_mask=am,
                                     negative_prompt_attention_mask=inp["attention_mask"], **gk)
        assert torch.equal(model(inputs=inp), today)
        with _Spy("cfg_combine") as spy:
            Mo.MM_LLMs.set_guidance(2.0)
            off = model(inputs=inp)
            assert len(spy.calls["cfg_combine"]) > 0
            Mo.MM_LLMs.set_generate_mask(True)
            on = model(inputs=inp)
            Mo.MM_LLMs.set_generate_mask(False)
            Mo.MM_LLMs.set_guidance()
            n = len(spy.calls["cfg_combine"])
            back = model(inputs=inp)
            assert len(spy.calls["cfg_combine"]) == n
    assert torch.equal(off, want_off) and torch.equal(on, want_on) and torch.equal(back, today)
    assert want_off.shape != today.shape or not torch.equal(want_off, today)      # guidance steers
