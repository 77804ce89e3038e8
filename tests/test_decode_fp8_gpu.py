"""GPU: fp8 weight-only decode (W8A16) -- mk_decode_linear_fp8 against fp32 math on exactly known e4m3 weights and
against the 16-bit kernel on the same values, the quantiser + kernel chain, the C entry point's domain, the fp8
five-launch decode step at LLaMA-7B width, and generate(decode_weights="fp8") end to end (plumbing, the path that
really ran, refusals, LoRA).  Tolerances are those of tests/test_kernels_gpu.py / test_model_gpu.py / test_fullsize_gpu.py
for the 16-bit kernels, taken over unchanged: the fp8 kernel differs only in where the weight bits come from."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from golden_util import load_case  # noqa: E402
from oracle import configs  # noqa: E402
from test_kernels_gpu import DECODE_LINEAR_SHAPES, H16, _close, _rand  # noqa: E402
from test_model_gpu import build_model, to_dev  # noqa: E402

from macaw_llm_amd import engine as eng  # noqa: E402
from macaw_llm_amd import lora as L  # noqa: E402
from macaw_llm_amd import modeling as Mo  # noqa: E402
from macaw_llm_amd import ops  # noqa: E402
from macaw_llm_amd.lib import MacawHipError  # noqa: E402

SHAPES = DECODE_LINEAR_SHAPES + [(24, 4096, 4096)]
FP8 = torch.float8_e4m3fn


@pytest.fixture(autouse=True)
def _restore_switches():
    ops.clear_fp8_cache()
    yield
    Mo.AUTO_FUSE = True
    Mo.DECODE_WEIGHTS[0] = None
    ops.clear_fp8_cache()


def _exact_fp8_weight(N, K, g):
    """random e4m3 bytes (no NaN code) and power-of-two scales 2^-9 ... 2^-4: (Wq uint8, s f32, dequantised f32)"""
    Wq = torch.randint(0, 256, (N, K), generator=g, dtype=torch.int32)
    nan = (Wq & 0x7F) == 0x7F
    while bool(nan.any()):                                      # re-draw 0x7F / 0xFF
        Wq = torch.where(nan, torch.randint(0, 256, (N, K), generator=g, dtype=torch.int32), Wq)
        nan = (Wq & 0x7F) == 0x7F
    Wq = Wq.to(torch.uint8)
    s = torch.pow(2.0, torch.randint(-9, -3, (N,), generator=g).float())
    Wf = Wq.view(FP8).float() * s[:, None]
    assert torch.isfinite(Wf).all()
    return Wq, s, Wf


@pytest.mark.parametrize("dtype", H16)
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_decode_linear_fp8_exact_weights_vs_fp32_and_vs_the_16bit_kernel(M, N, K, dtype):
    """(1) every prologue form against CPU fp32 math on exactly known weights, under test_kernels_gpu._close with the
    scale derived as there from K and the weight magnitude; (2) against mk_decode_linear on the SAME values held in
    the 16-bit type (exact: 3 mantissa bits, power-of-two scales), to the bound that test uses between its two
    routes; two calls on the same inputs are bit-identical.  All nine shapes are inside the fp8 domain (K = 704 is
    11 K-blocks of 64 bytes): nothing falls back, nothing is skipped."""
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(M + N + K)
    x = _rand((M, K), dtype, g)
    Wq, s, Wf = _exact_fp8_weight(N, K, g)
    res = _rand((M, N), dtype, g)
    nw = (1.0 + 0.1 * _rand((K,), torch.float32, g)).to(dtype)
    gu = _rand((M, 2 * K), dtype, g)
    xd, Wqd, sd, resd, nwd, gud = (t.to(dev) for t in (x, Wq, s, res, nw, gu))
    Wd = Wf.to(dtype)
    assert torch.equal(Wd.float(), Wf)                          # the 16-bit type holds every value exactly
    Wd = Wd.to(dev)
    assert ops.decode_linear_fp8_ok(xd, Wqd, 0)                 # the whole list is inside the plain-form domain
    scale = math.sqrt(K) * Wf.std().item() + 1.0

    def versus_16bit(got, want):
        d = (got.float() - want.float()).abs().max().item()
        lim = 0.02 * want.float().abs().max().item() + 1e-3
        same = (got == want).float().mean().item()
        print(f"fp8 vs 16-bit kernel {M}x{N}x{K} {dtype}: max diff {d:.3e} (limit {lim:.3e}), equal {same:.4f}")
        assert d <= lim, d
        assert same > 0.98, same

    # plain
    y0 = ops.decode_linear_fp8(xd, Wqd, sd, residual=resd)
    _close(y0, x.float() @ Wf.t() + res.float(), dtype, scale=scale, what="decode_linear_fp8 plain")
    assert torch.equal(y0, ops.decode_linear_fp8(xd, Wqd, sd, residual=resd))
    versus_16bit(y0, ops.decode_linear(xd, Wd, residual=resd))
    if not ops.decode_linear_fp8_ok(xd, Wqd, 1):                # 17 ... 32 rows: the plain form only
        assert M > 16
        return
    assert ops.decode_linear_ok(xd, Wd, 1)
    # RMSNorm prologue (rounding points of rmsnorm_fwd: y = w * rnd(x * rstd))
    xf = x.float()
    rstd = torch.rsqrt((xf * xf).mean(1, keepdim=True) + 1e-6)
    yn = (nw.float() * (xf * rstd).to(dtype).float()).to(dtype)
    y1 = ops.decode_linear_fp8(xd, Wqd, sd, 1, nwd, 1e-6)
    _close(y1, yn.float() @ Wf.t(), dtype, scale=scale, what="decode_linear_fp8 rmsnorm")
    assert torch.equal(y1, ops.decode_linear_fp8(xd, Wqd, sd, 1, nwd, 1e-6))
    versus_16bit(y1, ops.decode_linear(xd, Wd, 1, nwd, 1e-6))
    # SwiGLU prologue: x2 = [gate | up], a = rnd(rnd(silu(gate)) * up) -- the separate kernel prepares the same rows
    gate, up = gu[:, :K].float(), gu[:, K:].float()
    act = ((gate * torch.sigmoid(gate)).to(dtype).float() * up).to(dtype)
    y2 = ops.decode_linear_fp8(gud, Wqd, sd, 2, residual=resd)
    _close(y2, act.float() @ Wf.t() + res.float(), dtype, scale=scale, what="decode_linear_fp8 swiglu")
    a = ops.swiglu2d_fwd(gud, K)
    assert torch.equal(y2, ops.decode_linear_fp8(gud, Wqd, sd, 2, residual=resd))
    versus_16bit(y2, ops.decode_linear(gud, Wd, 2, residual=resd))
    assert torch.equal(y2, ops.decode_linear_fp8(a, Wqd, sd, residual=resd))    # same token rows, same k order


@pytest.mark.parametrize("M,N,K", [(1, 12288, 4096), (16, 520, 704), (4, 32007, 4096), (24, 4096, 4096), (1, 4096, 11008)])
def test_quantiser_and_fp8_kernel_chain_on_ordinary_weights(M, N, K, dtype=torch.bfloat16):
    """ops.fp8_weight (mk_fp8_quantize_rows: row-major, one scale per output channel) feeding mk_decode_linear_fp8,
    against the quantiser's formula restated on the CPU and the fp32 product"""
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(M + N + K)
    x = _rand((M, K), dtype, g)
    W = (_rand((N, K), dtype, g).float() * 0.05).to(dtype)
    res = _rand((M, N), dtype, g)
    Wdev = W.to(dev)
    Wq, s = ops.fp8_weight(Wdev)
    assert Wq.dtype == torch.uint8 and Wq.shape == (N, K) and Wq.is_contiguous() and s.shape == (N,)
    amax = W.float().abs().amax(1)
    s_ref = amax / 448.0
    sc = torch.full_like(amax, 448.0) / amax                    # (a true fp32 division: `448.0 / tensor` is 448 * reciprocal)
    q_ref = (W.float() * sc[:, None]).clamp(-448.0, 448.0).to(FP8)
    assert torch.allclose(s.cpu(), s_ref, rtol=1e-6, atol=0)
    ref = x.float() @ (q_ref.float() * s_ref[:, None]).t() + res.float()
    got = ops.decode_linear_fp8(x.to(dev), Wq, s, residual=res.to(dev))
    _close(got, ref, dtype, scale=math.sqrt(K) * 0.05 + 1.0, what="fp8_weight -> decode_linear_fp8")


def test_decode_linear_fp8_domain_is_checked_in_the_entry_point(dtype=torch.bfloat16):
    """misaligned pointers, an unsupported K, more than 16 rows with a prologue, more than 32 rows, the LDS budget:
    MK_ERR_UNSUPPORTED through _L.check, and nothing is launched (the output keeps its contents)"""
    dev = torch.device("cuda:0")
    M, N, K = 4, 64, 256
    x = torch.randn((M, K), device=dev).to(dtype)
    Wq = torch.randint(0, 120, (N, K), device=dev, dtype=torch.uint8)
    s = torch.ones(N, device=dev)
    nw = torch.ones(K, device=dev).to(dtype)
    out = torch.full((32, N), 7.0, device=dev).to(dtype)

    def refused(*a, rows=M, **kw):
        with pytest.raises(MacawHipError, match="MK_ERR_UNSUPPORTED"):
            ops.decode_linear_fp8(*a, out=out[:rows], **kw)
        torch.cuda.synchronize()
        assert bool((out == 7.0).all())

    ops.decode_linear_fp8(x, Wq, s, out=out[:M])               # the aligned call is inside the domain
    out.fill_(7.0)
    xbuf = torch.randn(M * K + 8, device=dev).to(dtype)
    refused(xbuf[1:1 + M * K].view(M, K), Wq, s)                # x 2 bytes off a 16-byte boundary
    wbuf = torch.randint(0, 120, (N * K + 16,), device=dev, dtype=torch.uint8)
    refused(x, wbuf[1:1 + N * K].view(N, K), s)                 # Wq 1 byte off
    refused(x, torch.randint(0, 120, (N, K + 8), device=dev, dtype=torch.uint8)[:, :K], s)   # pitch % 16 != 0
    nbuf = torch.ones(K + 8, device=dev).to(dtype)
    refused(x, Wq, s, 1, nbuf[1:1 + K], 1e-6)                   # norm weight misaligned
    refused(x[:, :96], Wq[:, :96].contiguous(), s)              # K % 64 != 0
    x24 = torch.randn((24, K), device=dev).to(dtype)
    refused(x24, Wq, s, 1, nw, 1e-6, rows=24)                   # prologue forms: M <= 16
    refused(torch.randn((24, 2 * K), device=dev).to(dtype), Wq, s, 2, rows=24)
    x40 = torch.randn((40, K), device=dev).to(dtype)
    with pytest.raises(MacawHipError, match="MK_ERR_UNSUPPORTED"):
        ops.decode_linear_fp8(x40, Wq, s)                       # plain: M <= 32
    K2 = 4096                                                   # 8 prepared rows of 4096 exceed the 40 KiB LDS budget
    x8 = torch.randn((8, K2), device=dev).to(dtype)
    Wq2 = torch.randint(0, 120, (N, K2), device=dev, dtype=torch.uint8)
    assert not ops.decode_linear_fp8_ok(x8, Wq2, 1) and ops.decode_linear_fp8_ok(x8, Wq2, 0)
    refused(x8, Wq2, s, 1, torch.ones(K2, device=dev).to(dtype), 1e-6, rows=8)


# ------------------------------------------------------------------------------------------- generate() --
def _snap_fp8_exact(W):
    """W [N, K] -> (values, bytes, scales): every row becomes e4m3 code x power-of-two scale with one element planted
    at +-448 x scale, so that the row maximum re-quantises to that same scale and the quantiser's formula
    (sc = 448 / amax, q = e4m3(x sc)) reproduces the codes exactly"""
    Wf = W.detach().float().cpu()
    amax = Wf.abs().amax(1).clamp_min(2.0 ** -20)
    s = torch.pow(2.0, torch.ceil(torch.log2(amax / 448.0)))
    q = (Wf / s[:, None]).clamp(-448.0, 448.0).to(FP8)
    val = q.float()
    j = Wf.abs().argmax(1)
    rows = torch.arange(Wf.shape[0])
    val[rows, j] = torch.where(Wf[rows, j] < 0, -448.0, 448.0)
    q = val.to(FP8)
    assert torch.equal(q.float(), val)
    return val * s[:, None], q.view(torch.uint8), s


def _snapped_model(dtype, dev):
    fx = load_case("micro_all")
    cfg = configs.get(fx["config_name"])
    model = build_model(cfg, fx["state"], dtype, dev, fuse=True).eval()
    want = []                                                   # (weight as the decode step sees it, bytes, scales)
    with torch.no_grad():
        for lyr in model.llm.model.layers:
            a, m = lyr.self_attn, lyr.mlp
            exp = {}
            for lin in (a.q_proj, a.k_proj, a.v_proj, a.o_proj, m.gate_proj, m.up_proj, m.down_proj):
                v, q, s = _snap_fp8_exact(lin.weight)
                assert torch.equal(v.to(dtype).float(), v)      # exact in the parameter type
                lin.weight.copy_(v.to(dtype).to(dev))
                exp[lin] = (q, s)
            wqkv, wgu = lyr.fused_weights()
            cat = lambda lins: (torch.cat([exp[t][0] for t in lins]), torch.cat([exp[t][1] for t in lins]))  # noqa: E731
            want.append((wqkv, *cat((a.q_proj, a.k_proj, a.v_proj))))
            want.append((a.o_proj.weight, *exp[a.o_proj]))
            want.append((wgu, *cat((m.gate_proj, m.up_proj))))
            want.append((m.down_proj.weight, *exp[m.down_proj]))
        v, q, s = _snap_fp8_exact(model.llm.lm_head.weight)
        model.llm.lm_head.weight.copy_(v.to(dtype).to(dev))
        want.append((model.llm.lm_head.weight, q, s))
    return model, fx, want


@pytest.mark.parametrize("dtype", H16)
def test_generate_fp8_on_fp8_exact_weights_matches_the_16bit_decode(dev, dtype):
    """With every decoder projection and the lm_head snapped to fp8-exact values the quantised copies hold the SAME
    numbers as the 16-bit masters, so generate(decode_weights="fp8") and generate() differ only in the order of fp32
    sums: the project's criterion for two such decode routes (test_generate_hipgraph_decode_matches_eager_loop).
    (The micro model's down projection has K = 352, outside the K % 64 domain of both weight-streaming kernels: it
    keeps the 16-bit GEMM it uses today; test_generate_fp8_really_streams_e4m3 covers all four projections.)"""
    model, fx, want = _snapped_model(dtype, dev)
    for W, q, s in want:                                        # the GPU quantiser reproduces those bytes and scales
        gq, gs = ops.fp8_weight(W)
        gq, q = gq.cpu(), q.clone()
        gq[(gq & 0x7F) == 0], q[(q & 0x7F) == 0] = 0, 0         # (apart from the sign of a zero)
        assert torch.equal(gs.cpu(), s), (gs.cpu() / s).unique()
        assert torch.equal(gq, q), (gq != q).float().mean().item()
    emb = fx["inputs_embeds"].to(dev).to(dtype)
    kw = dict(inputs_embeds=emb, max_new_tokens=24, pad_token_id=106)
    f = model.llm.generate(eos_token_id=-1, decode_weights="fp8", **kw)
    b = model.llm.generate(eos_token_id=-1, **kw)
    assert f.dtype == torch.long and f.shape == b.shape == (emb.shape[0], 24), (f.shape, b.shape)
    agree = (f == b).float().mean().item()
    print(f"generate fp8 vs 16-bit {dtype}: agreement {agree:.3f}")
    assert agree >= 0.9, agree
    # force an early stop: the most frequent greedy token as eos
    e = model.llm.generate(eos_token_id=-1, decode_graph=False, **kw)
    eos = int(e[:, 2:].flatten().mode().values)
    f = model.llm.generate(eos_token_id=eos, decode_weights="fp8", **kw)
    b = model.llm.generate(eos_token_id=eos, **kw)
    assert f.shape == b.shape and (f == b).float().mean().item() >= 0.9, (f.shape, b.shape)


def _small_llama(dev, dtype=torch.bfloat16, seed=0):
    """the micro decoder with FF = 384, so that all four projections are inside the fp8 domain (K % 64 == 0)"""
    from transformers import LlamaConfig
    cfg_l = dict(configs.get(load_case("micro_all")["config_name"])["llama"])
    cfg_l["intermediate_size"] = 384
    torch.manual_seed(seed)
    Mo.AUTO_FUSE = True
    lm = Mo.LlamaForCausalLM(LlamaConfig(**cfg_l)).to(dev).to(dtype)
    return Mo.fuse_model(lm).eval(), cfg_l


class _Spy:
    """wraps ops.<name> for the duration of a with block and records every call's arguments"""

    def __init__(self, *names):
        self.names, self.calls, self.real = names, {n: [] for n in names}, {}

    def __enter__(self):
        for n in self.names:
            self.real[n] = getattr(ops, n)

            def wrapped(*a, _n=n, **kw):
                self.calls[_n].append(a)
                return self.real[_n](*a, **kw)
            setattr(ops, n, wrapped)
        return self

    def __exit__(self, *exc):
        for n in self.names:
            setattr(ops, n, self.real[n])


@pytest.mark.parametrize("B", [2, 8])
def test_generate_fp8_really_streams_e4m3(dev, B):
    """during the decode steps every one of the four projections of every layer and the lm_head goes through
    ops.decode_linear_fp8 with the copy ops.fp8_weight keeps for it, no 16-bit weight-streaming launch happens, the
    copies are made once across calls and again after the weight version moves"""
    lm, cfg_l = _small_llama(dev)
    nl = cfg_l["num_hidden_layers"]
    ids = torch.randint(3, cfg_l["vocab_size"], (B, 21), generator=torch.Generator().manual_seed(B)).to(dev)
    kw = dict(input_ids=ids, max_new_tokens=12, eos_token_id=-1, pad_token_id=0, decode_weights="fp8")
    with _Spy("decode_linear_fp8", "decode_linear", "linear_fwd", "quantize_fp8_rows") as spy:
        out = lm.generate(**kw)
        assert out.shape == (B, 12)
        assert len(spy.calls["quantize_fp8_rows"]) == 4 * nl + 1
        expect = []
        for lyr in lm.model.layers:
            wqkv, wgu = lyr.fused_weights()
            expect += [wqkv, lyr.self_attn.o_proj.weight, wgu, lyr.mlp.down_proj.weight]
        expect.append(lm.lm_head.weight)
        copies = [ops.fp8_weight(W) for W in expect]
        assert len(spy.calls["quantize_fp8_rows"]) == 4 * nl + 1            # ... those were cache hits
        seen = [(a[1].data_ptr(), a[2].data_ptr()) for a in spy.calls["decode_linear_fp8"]]
        step = [(q.data_ptr(), s.data_ptr()) for q, s in copies]
        # token 0: lm_head on the prefill's last row; token 1: one eager step; then ONE captured step
        assert seen == step[-1:] + step + step, (len(seen), len(step))
        assert spy.calls["decode_linear"] == []
        assert [a[0].shape[0] for a in spy.calls["linear_fwd"] if a[0].shape[0] <= 32] == []   # (the prefill has B * 21 rows)
        n_pre = len(spy.calls["linear_fwd"])
        again = lm.generate(**kw)
        assert torch.equal(out, again)                                      # deterministic kernels, same copies
        assert len(spy.calls["quantize_fp8_rows"]) == 4 * nl + 1            # quantised once
        ops.bump_weight_version()
        lm.generate(**kw)
        assert len(spy.calls["quantize_fp8_rows"]) == 2 * (4 * nl + 1)      # the weight version moved: re-made
        assert len(spy.calls["linear_fwd"]) == 3 * n_pre                    # the prefill keeps the 16-bit weights
    ref = lm.generate(**{**kw, "decode_weights": None})
    assert ref.shape == out.shape                                           # (ordinary weights: the ids may differ)


def test_generate_fp8_refusals_and_default(dev, monkeypatch):
    """decode_weights="fp8" raises a ValueError naming the condition that keeps the call off the hipGraph decode path;
    None is today's path; MM_LLMs.set_decode_weights routes inputs["inference"] = True"""
    fx = load_case("micro_all")
    cfg = configs.get(fx["config_name"])
    model = build_model(cfg, fx["state"], torch.bfloat16, dev, fuse=True).eval()
    emb = fx["inputs_embeds"].to(dev).to(torch.bfloat16)
    kw = dict(inputs_embeds=emb, max_new_tokens=8, eos_token_id=-1, pad_token_id=106)
    assert torch.equal(model.llm.generate(**kw), model.llm.generate(decode_weights=None, **kw))
    with pytest.raises(ValueError, match="decode_weights"):
        model.llm.generate(decode_weights="int8", **kw)
    with pytest.raises(ValueError, match="use_cache"):
        model.llm.generate(decode_weights="fp8", use_cache=False, **kw)
    with pytest.raises(ValueError, match="decode_graph"):
        model.llm.generate(decode_weights="fp8", decode_graph=False, **kw)
    with pytest.raises(ValueError, match="max_new_tokens"):
        model.llm.generate(decode_weights="fp8", **{**kw, "max_new_tokens": 2})
    with pytest.raises(ValueError, match="decode_attn_ok"):
        model.llm.generate(decode_weights="fp8", **{**kw, "max_new_tokens": 16000})
    with pytest.raises(ValueError, match="33 sequences"):
        model.llm.generate(decode_weights="fp8", **{**kw, "inputs_embeds": emb[:1].expand(33, -1, -1).contiguous()})
    monkeypatch.setenv("MACAW_NO_DECODE_GRAPH", "1")
    with pytest.raises(ValueError, match="MACAW_NO_DECODE_GRAPH"):
        model.llm.generate(decode_weights="fp8", **kw)
    monkeypatch.delenv("MACAW_NO_DECODE_GRAPH")
    m32 = build_model(cfg, fx["state"], torch.float32, dev).eval()
    with pytest.raises(ValueError, match="fp32"):
        m32.llm.generate(decode_weights="fp8", **{**kw, "inputs_embeds": fx["inputs_embeds"].to(dev)})
    mu = build_model(cfg, fx["state"], torch.bfloat16, dev, fuse=False).eval()      # (lazy fusion off)
    with pytest.raises(ValueError, match="unfused"):
        mu.llm.generate(decode_weights="fp8", **kw)
    # the multimodal entry point: a process-wide switch next to set_fp8
    with pytest.raises(ValueError):
        Mo.MM_LLMs.set_decode_weights("int8")
    inp = to_dev(fx["inputs"], dev)
    inp["inference"] = True
    Mo.AUTO_FUSE = True
    with torch.no_grad():
        base = model(inputs=inp)
        Mo.MM_LLMs.set_decode_weights("fp8")
        with _Spy("decode_linear_fp8") as spy:
            ids = model(inputs=inp)
        Mo.MM_LLMs.set_decode_weights(None)
    assert len(spy.calls["decode_linear_fp8"]) > 0 and ids.dtype == torch.long and ids.shape[0] == base.shape[0]


def test_generate_fp8_with_adapters_matches_merge_and_unload(dev):
    """with LoRA adapters the per-call merged copies are what is quantised (once per call, outside the version-keyed
    cache): the ids agree with the same call on the merged-and-unloaded model"""
    from test_lora_gpu import _mm_lora
    model, fx = _mm_lora(dev, p=0.0)
    with torch.no_grad():
        for n, q in model.llm.named_parameters():
            if ".lora_B." in n:
                q.copy_(torch.randn_like(q.float()) * 0.05)
    model.eval()
    emb = fx["inputs_embeds"].to(dev).to(torch.bfloat16)
    kw = dict(inputs_embeds=emb, max_new_tokens=12, eos_token_id=-1, pad_token_id=106, decode_weights="fp8")
    nl = len(model.llm.model.layers)
    with _Spy("quantize_fp8_rows", "decode_linear_fp8") as spy:
        a = model.llm.generate(**kw)
        n1 = len(spy.calls["quantize_fp8_rows"])
        assert n1 == 3 * nl + 1 and len(spy.calls["decode_linear_fp8"]) > 0   # (down: K = 352 keeps its 16-bit launch)
        model.llm.generate(**kw)
        assert len(spy.calls["quantize_fp8_rows"]) == 2 * n1 - 1             # merged copies again, the lm_head cached
    plain = L.merge_and_unload(model.llm)
    b = plain.generate(**kw)
    assert a.shape == b.shape
    agree = (a == b).float().mean().item()
    print(f"generate fp8 with adapters vs merged model: agreement {agree:.3f}")
    assert agree >= 0.9, agree


# ------------------------------------------------------------------------------------------- real width --
@pytest.mark.parametrize("B", [1, 8])
def test_fp8_decode_step_real_dimension_layer_vs_16bit_step(dev, B):
    """One LLaMA-7B-dimension decode step of a layer: the fp8 five-launch step against the 16-bit five-launch step on
    the dequantised (exactly representable) weights, in the manner and under the bounds of
    test_decode_step_real_dimension_layer_graphable_vs_separate_kernels.  B = 8: the prologue forms exceed the LDS
    budget, the separate RMSNorm / SwiGLU kernels feed the PLAIN fp8 launch."""
    D, FF, H = 4096, 11008, 32
    bf = lambda t: t.to(torch.bfloat16)  # noqa: E731
    g = torch.Generator().manual_seed(11 + B)
    T0, Tmax, hd = 150, 160, D // H

    def weight(N, K):                                           # ~ N(0, 0.02) snapped to fp8-exact rows
        v, q, s = _snap_fp8_exact(torch.randn(N, K, generator=g) * 0.02)
        assert torch.equal(bf(v).float(), v)
        return bf(v).to(dev), (q.to(dev), s.to(dev))

    wqkv, q_qkv = weight(3 * D, D)
    wo, q_o = weight(D, D)
    wgu, q_gu = weight(2 * FF, D)
    wd, q_d = weight(D, FF)
    ln1 = bf(1 + 0.1 * torch.randn(D, generator=g)).to(dev)
    ln2 = bf(1 + 0.1 * torch.randn(D, generator=g)).to(dev)
    x2 = bf(torch.randn(B, D, generator=g)).to(dev)
    cache0 = torch.zeros((B, Tmax, 2 * D), dtype=torch.bfloat16)
    cache0[:, :T0] = bf(torch.randn(B, T0, 2 * D, generator=g))
    inv = 1.0 / (10000.0 ** (torch.arange(0, hd, 2).float() / hd))
    ang = torch.cat((torch.outer(torch.arange(Tmax).float(), inv),) * 2, dim=-1)
    cos, sin = bf(ang.cos()).to(dev), bf(ang.sin()).to(dev)
    pos = torch.full((B,), T0, dtype=torch.int32, device=dev)
    args = (H, 1e-6, wqkv[:D], wqkv[D:2 * D], wqkv[2 * D:], wo, wgu[:FF], wgu[FF:], wd, ln1, ln2, wqkv, wgu)
    kv_b, kv_f = cache0.clone().to(dev), cache0.clone().to(dev)
    t_dev = torch.tensor([T0], dtype=torch.int32, device=dev)
    with torch.no_grad(), _Spy("decode_linear_fp8", "decode_linear", "linear_fwd") as spy:
        out_f = eng.llama_layer_cached(x2, B, 1, 0, kv_f, Tmax, pos, cos, sin, *args, t_dev=t_dev,
                                       w8=(q_qkv, q_o, q_gu, q_d))
        assert [a[3] if len(a) > 3 else 0 for a in spy.calls["decode_linear_fp8"]] == ([1, 0, 1, 2] if B == 1 else [0] * 4)
        assert spy.calls["decode_linear"] == [] and spy.calls["linear_fwd"] == []
        out_b = eng.llama_layer_cached(x2, B, 1, 0, kv_b, Tmax, pos, cos, sin, *args, t_dev=t_dev)
    assert torch.equal(kv_b[:, :T0], kv_f[:, :T0]) and torch.equal(kv_b[:, T0 + 1:], kv_f[:, T0 + 1:])
    same = (kv_b[:, T0] == kv_f[:, T0]).float().mean().item()
    rd = (kv_b[:, T0].float() - kv_f[:, T0].float()).abs().max().item()
    d = (out_b.float() - out_f.float()).abs().max().item()
    ref = out_b.float().abs().max().item()
    print(f"fp8 step vs 16-bit step B={B}: cache row equal {same:.4f}, max diff {rd:.3e}; output diff {d:.3e} of {ref:.3e}")
    assert same > 0.98, same
    assert rd <= 2.0 ** -7 * kv_b[:, T0].float().abs().max().item() + 1e-3, rd
    assert d <= 2.0 ** -6 * ref + 1e-3, (d, ref)
