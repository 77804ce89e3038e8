"""GPU: MXFP4 weight-only decode (W4A16) -- the position of every element in mk_decode_linear_mxfp4's lane mapping, the
kernel against fp32 math on exactly known codes and against the 16-bit kernel on the same values, the quantiser + kernel
chain against tests/mxfp4_ref.py, the C entry point's domain, the mxfp4 five-launch decode step at LLaMA-7B width, and
generate(decode_weights="mxfp4") end to end (plumbing, the path that really ran, refusals, LoRA, composition).
Tolerances are those of tests/test_decode_fp8_gpu.py, taken over unchanged: a de-quantised MXFP4 value is an exact number
of the token type, so the kernel differs from the 16-bit one only in where the weight bits come from."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import mxfp4_ref as R  # noqa: E402
from golden_util import load_case  # noqa: E402
from oracle import configs  # noqa: E402
from test_decode_fp8_gpu import _Spy, _small_llama, _snap_fp8_exact  # noqa: E402
from test_kernels_gpu import DECODE_LINEAR_SHAPES, H16, _close, _rand  # noqa: E402
from test_model_gpu import build_model, to_dev  # noqa: E402

from macaw_llm_amd import engine as eng  # noqa: E402
from macaw_llm_amd import lora as L  # noqa: E402
from macaw_llm_amd import modeling as Mo  # noqa: E402
from macaw_llm_amd import ops  # noqa: E402
from macaw_llm_amd.lib import MacawHipError  # noqa: E402

# K = 704 is outside the K % 128 domain: 640 (five K-blocks) takes its place.  Added: two token tiles (MT = 2), ONE
# K-block with 32 rows, and a ragged N with 17 rows and an odd number of K-blocks (5 over 8 waves: most waves idle).
SHAPES = [(M, N, 640 if K == 704 else K) for M, N, K in DECODE_LINEAR_SHAPES] + [(24, 4096, 4096), (32, 256, 128),
                                                                                   (17, 520, 640)]
_LUT = torch.cat((R.VALUES, -R.VALUES))


@pytest.fixture(autouse=True)
def _restore_switches():
    ops.clear_fp8_cache()
    yield
    Mo.AUTO_FUSE = True
    Mo.DECODE_WEIGHTS[0] = None
    Mo.KV_CACHE[0] = None
    ops.clear_fp8_cache()


def _exact_mxfp4_weight(N, K, g, e_lo=120, e_hi=124):
    """random e2m1 codes (all 16, the negative zero included) and block exponents 2^-7 ... 2^-4: (q uint8 [N, K / 2],
    e uint8 [N, K / 32], de-quantised f32 [N, K])"""
    code = torch.randint(0, 16, (N, K), generator=g, dtype=torch.uint8)
    q = (code[:, 0::2] | (code[:, 1::2] << 4)).contiguous()
    e = torch.randint(e_lo, e_hi, (N, K // 32), generator=g, dtype=torch.uint8)
    Wf = (_LUT[code.int()].view(N, K // 32, 32) * torch.pow(2.0, e.float() - 127.0)[:, :, None]).view(N, K)
    assert torch.equal(Wf[:16], R.dequant(q[:16], e[:16]))      # (the format's restatement, on a slice)
    return q, e, Wf


# ------------------------------------------------------------------------------------------------- position --
@pytest.mark.parametrize("dtype", H16)
def test_every_element_sits_where_the_format_says(dtype):
    """K = 128 (one K-block), N = 16, random codes, block exponents 120 ... 130.  The token rows are rows of the identity,
    so y[m, n] is ONE exact product: it must EQUAL dequant(W)[n, k].  This pins the nibble order inside a byte, the byte
    the conversion's selector picks, and the lane <-> k mapping shared with the token operand -- for the two-tile
    kernel (32 rows) and the one-tile plain kernel (16 rows).  The prologue forms run the same mapping code on token
    rows read from LDS; the exact-weights test covers them."""
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(7)
    q, e, Wf = _exact_mxfp4_weight(16, 128, g, 120, 131)
    assert torch.equal(Wf.to(dtype).float(), Wf)
    eye = torch.eye(128).to(dtype)
    qd, ed = q.to(dev), e.to(dev)
    for rows in (32, 16):
        for j in range(128 // rows):
            x = eye[rows * j:rows * (j + 1)].contiguous().to(dev)
            y = ops.decode_linear_mxfp4(x, qd, ed).float().cpu()
            want = Wf[:, rows * j:rows * (j + 1)].t()
            assert torch.equal(y, want), (rows, j, (y != want).nonzero()[:8].tolist())


# ------------------------------------------------------------------------------------------- exact weights --
@pytest.mark.parametrize("dtype", H16)
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_decode_linear_mxfp4_exact_weights_vs_fp32_and_vs_the_16bit_kernel(M, N, K, dtype):
    """(1) every prologue form against CPU fp32 math on exactly known codes, under test_kernels_gpu._close with the scale
    derived as there from K and the weight magnitude; (2) against mk_decode_linear on the SAME values held in the 16-bit
    type (exact: 1 mantissa bit, power-of-two scales), under the two bounds test_decode_fp8_gpu uses between those
    routes; two calls on the same inputs are bit-identical; the SwiGLU prologue equals swiglu2d_fwd + the plain form."""
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(M + N + K)
    x = _rand((M, K), dtype, g)
    q, e, Wf = _exact_mxfp4_weight(N, K, g)
    res = _rand((M, N), dtype, g)
    nw = (1.0 + 0.1 * _rand((K,), torch.float32, g)).to(dtype)
    gu = _rand((M, 2 * K), dtype, g)
    xd, qd, ed, resd, nwd, gud = (t.to(dev) for t in (x, q, e, res, nw, gu))
    Wd = Wf.to(dtype)
    assert torch.equal(Wd.float(), Wf)                          # the 16-bit type holds every value exactly
    Wd = Wd.to(dev)
    assert ops.decode_linear_mxfp4_ok(xd, qd, 0)                # the whole list is inside the plain-form domain
    scale = math.sqrt(K) * Wf.std().item() + 1.0

    def versus_16bit(got, want):
        d = (got.float() - want.float()).abs().max().item()
        lim = 0.02 * want.float().abs().max().item() + 1e-3
        same = (got == want).float().mean().item()
        print(f"mxfp4 vs 16-bit kernel {M}x{N}x{K} {dtype}: max diff {d:.3e} (limit {lim:.3e}), equal {same:.4f}")
        assert d <= lim, d
        assert same > 0.98, same

    # plain
    y0 = ops.decode_linear_mxfp4(xd, qd, ed, residual=resd)
    _close(y0, x.float() @ Wf.t() + res.float(), dtype, scale=scale, what="decode_linear_mxfp4 plain")
    assert torch.equal(y0, ops.decode_linear_mxfp4(xd, qd, ed, residual=resd))
    versus_16bit(y0, ops.decode_linear(xd, Wd, residual=resd))
    if not ops.decode_linear_mxfp4_ok(xd, qd, 1):               # 17 ... 32 rows: the plain form only
        assert M > 16
        return
    assert ops.decode_linear_ok(xd, Wd, 1)
    # RMSNorm prologue (rounding points of rmsnorm_fwd: y = w * rnd(x * rstd))
    xf = x.float()
    rstd = torch.rsqrt((xf * xf).mean(1, keepdim=True) + 1e-6)
    yn = (nw.float() * (xf * rstd).to(dtype).float()).to(dtype)
    y1 = ops.decode_linear_mxfp4(xd, qd, ed, 1, nwd, 1e-6)
    _close(y1, yn.float() @ Wf.t(), dtype, scale=scale, what="decode_linear_mxfp4 rmsnorm")
    assert torch.equal(y1, ops.decode_linear_mxfp4(xd, qd, ed, 1, nwd, 1e-6))
    versus_16bit(y1, ops.decode_linear(xd, Wd, 1, nwd, 1e-6))
    # SwiGLU prologue: x2 = [gate | up], a = rnd(rnd(silu(gate)) * up) -- the separate kernel prepares the same rows
    gate, up = gu[:, :K].float(), gu[:, K:].float()
    act = ((gate * torch.sigmoid(gate)).to(dtype).float() * up).to(dtype)
    y2 = ops.decode_linear_mxfp4(gud, qd, ed, 2, residual=resd)
    _close(y2, act.float() @ Wf.t() + res.float(), dtype, scale=scale, what="decode_linear_mxfp4 swiglu")
    a = ops.swiglu2d_fwd(gud, K)
    assert torch.equal(y2, ops.decode_linear_mxfp4(gud, qd, ed, 2, residual=resd))
    versus_16bit(y2, ops.decode_linear(gud, Wd, 2, residual=resd))
    assert torch.equal(y2, ops.decode_linear_mxfp4(a, qd, ed, residual=resd))   # same token rows, same k order


# ----------------------------------------------------------------------------------------- quantiser chain --
@pytest.mark.parametrize("M,N,K,dtype", [(1, 1536, 4096, torch.bfloat16), (16, 520, 640, torch.bfloat16),
                                         (24, 512, 4096, torch.bfloat16), (1, 512, 11008, torch.bfloat16),
                                         (3, 264, 256, torch.float16)])
def test_quantiser_and_mxfp4_kernel_chain_on_ordinary_weights(M, N, K, dtype):
    """ops.mxfp4_weight (mk_mxfp4_quantize_rows) on N(0, 0.05) weights held as a PITCHED column slice of a wider buffer,
    with an all-zero block and (fp16: below the clamp of the block exponent) a row of very small values: codes and
    exponents EQUAL tests/mxfp4_ref.quantize apart from the sign of a zero; the kernel on that copy matches
    x dequant^T + res.  The format's relative RMS error is printed, not asserted: nobody has measured it before."""
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(M + N + K)
    x = _rand((M, K), dtype, g)
    buf = (_rand((N, K + 64), dtype, g).float() * 0.05).to(dtype)
    buf[1, 32:64] = 0                                           # an all-zero block
    buf[2] = (buf[2].float() * 2.0 ** -11).to(dtype)            # fp16: amax ~ 2^-13, the exponent clamps at EMIN
    W = buf[:, :K]
    res = _rand((M, N), dtype, g)
    Wdev = buf.to(dev)[:, :K]
    assert Wdev.stride(0) == K + 64
    q, e = ops.mxfp4_weight(Wdev)
    assert q.dtype == e.dtype == torch.uint8 and q.shape == (N, K // 2) and e.shape == (N, K // 32)
    assert q.is_contiguous() and e.is_contiguous()
    q2, _ = ops.mxfp4_weight(Wdev)
    assert q2.data_ptr() == q.data_ptr()                        # cached
    q_ref, e_ref = R.quantize(W, dtype)
    assert torch.equal(e.cpu(), e_ref), (e.cpu() != e_ref).float().mean().item()
    cg, cr = R.unpack(q.cpu()), R.unpack(q_ref)
    cg[(cg & 7) == 0], cr[(cr & 7) == 0] = 0, 0                 # (apart from the sign of a zero)
    assert torch.equal(cg, cr), (cg != cr).float().mean().item()
    assert int(e_ref[1, 1]) == R.emin(dtype) + 127 and bool((cr[1, 32:64] == 0).all())
    if dtype == torch.float16:
        assert int(e_ref[2].min()) == R.emin(dtype) + 127
    Wdq = R.dequant(q.cpu(), e.cpu())
    assert torch.equal(Wdq.to(dtype).float(), Wdq)
    rel = ((Wdq - W.float()).pow(2).mean() / W.float().pow(2).mean()).sqrt().item()
    print(f"mxfp4 round-to-nearest on N(0, 0.05) {N}x{K} {dtype}: relative RMS error {rel:.4f}")
    got = ops.decode_linear_mxfp4(x.to(dev), q, e, residual=res.to(dev))
    _close(got, x.float() @ Wdq.t() + res.float(), dtype, scale=math.sqrt(K) * 0.05 + 1.0, what="mxfp4_weight -> decode_linear_mxfp4")
    ops.clear_fp8_cache()                                       # ... clears the MXFP4 copies too
    q3, e3 = ops.mxfp4_weight(Wdev)
    assert torch.equal(q3, q) and torch.equal(e3, e)            # deterministic


# -------------------------------------------------------------------------------------------------- domain --
def test_decode_linear_mxfp4_domain_is_checked_in_the_entry_point(dtype=torch.bfloat16):
    """misaligned pointers, an unsupported K, bad pitches, more than 16 rows with a prologue, more than 32 rows, the LDS
    budget, fp32 tokens: an error through _L.check, and nothing is launched (the output keeps its contents)"""
    dev = torch.device("cuda:0")
    M, N, K = 4, 64, 256
    x = torch.randn((M, K), device=dev).to(dtype)
    Wq = torch.randint(0, 256, (N, K // 2), device=dev, dtype=torch.uint8)
    e = torch.full((N, K // 32), 122, device=dev, dtype=torch.uint8)
    nw = torch.ones(K, device=dev).to(dtype)
    out = torch.full((32, N), 7.0, device=dev).to(dtype)

    def refused(*a, rows=M, err="MK_ERR_UNSUPPORTED", **kw):
        with pytest.raises(MacawHipError, match=err):
            ops.decode_linear_mxfp4(*a, out=out[:rows], **kw)
        torch.cuda.synchronize()
        assert bool((out == 7.0).all())

    ops.decode_linear_mxfp4(x, Wq, e, out=out[:M])              # the aligned call is inside the domain
    torch.cuda.synchronize()
    assert not bool((out[:M] == 7.0).all())
    out.fill_(7.0)
    refused(x, Wq, e, 3, err="MK_ERR_BAD_ARG")                  # no such prologue
    refused(x, Wq, e, 1, None, 1e-6, err="MK_ERR_BAD_ARG")      # RMSNorm without a weight
    xbuf = torch.randn(M * K + 8, device=dev).to(dtype)
    refused(xbuf[1:1 + M * K].view(M, K), Wq, e)                # x 2 bytes off a 16-byte boundary
    wbuf = torch.randint(0, 256, (N * K // 2 + 16,), device=dev, dtype=torch.uint8)
    refused(x, wbuf[1:1 + N * K // 2].view(N, K // 2), e)       # Wq 1 byte off
    ebuf = torch.full((N * K // 32 + 4,), 122, device=dev, dtype=torch.uint8)
    refused(x, Wq, ebuf[1:1 + N * K // 32].view(N, K // 32))    # e 1 byte off a 4-byte boundary
    refused(x, torch.randint(0, 256, (N, K // 2 + 8), device=dev, dtype=torch.uint8)[:, :K // 2], e)   # ldw % 16 != 0
    refused(x, Wq, torch.full((N, K // 32 + 2), 122, device=dev, dtype=torch.uint8)[:, :K // 32])      # lde % 4 != 0
    nbuf = torch.ones(K + 8, device=dev).to(dtype)
    refused(x, Wq, e, 1, nbuf[1:1 + K], 1e-6)                   # norm weight misaligned
    refused(x[:, :192].contiguous(), Wq[:, :96].contiguous(), e[:, :6].contiguous())    # K = 192: K % 128 != 0
    x17 = torch.randn((17, K), device=dev).to(dtype)
    refused(x17, Wq, e, 1, nw, 1e-6, rows=17)                   # prologue forms: M <= 16
    refused(torch.randn((17, 2 * K), device=dev).to(dtype), Wq, e, 2, rows=17)
    x33 = torch.randn((33, K), device=dev).to(dtype)
    with pytest.raises(MacawHipError, match="MK_ERR_UNSUPPORTED"):
        ops.decode_linear_mxfp4(x33, Wq, e)                     # plain: M <= 32
    with pytest.raises(MacawHipError, match="MK_ERR_UNSUPPORTED"):
        ops.decode_linear_mxfp4(x.float(), Wq, e)               # f32 tokens
    K2 = 4096                                                   # 8 prepared rows of 4096 exceed the 40 KiB LDS budget
    x8 = torch.randn((8, K2), device=dev).to(dtype)
    Wq2 = torch.randint(0, 256, (N, K2 // 2), device=dev, dtype=torch.uint8)
    e2 = torch.full((N, K2 // 32), 122, device=dev, dtype=torch.uint8)
    assert not ops.decode_linear_mxfp4_ok(x8, Wq2, 1) and ops.decode_linear_mxfp4_ok(x8, Wq2, 0)
    refused(x8, Wq2, e2, 1, torch.ones(K2, device=dev).to(dtype), 1e-6, rows=8)
    with pytest.raises(MacawHipError, match="MK_ERR_UNSUPPORTED"):      # the quantiser's own domain
        ops.quantize_mxfp4_rows(torch.randn((4, 144), device=dev).to(dtype)[:, :112])


# ------------------------------------------------------------------------------------------- generate() --
def _snapped_model(dtype, dev):
    """the micro model with every decoder projection with K % 128 == 0 snapped to MXFP4-exact values (the down
    projection, K = 352, keeps its values and its 16-bit GEMM) and the lm_head snapped to e4m3-exact values"""
    fx = load_case("micro_all")
    cfg = configs.get(fx["config_name"])
    model = build_model(cfg, fx["state"], dtype, dev, fuse=True).eval()
    want4 = []                                                  # (weight as the decode step sees it, codes, exponents)
    with torch.no_grad():
        for lyr in model.llm.model.layers:
            a, m = lyr.self_attn, lyr.mlp
            exp = {}
            for lin in (a.q_proj, a.k_proj, a.v_proj, a.o_proj, m.gate_proj, m.up_proj, m.down_proj):
                if lin.weight.shape[1] % 128:
                    continue
                v, q, e = R.snap(lin.weight.cpu(), dtype)
                assert torch.equal(v.to(dtype).float(), v)      # exact in the parameter type
                lin.weight.copy_(v.to(dtype).to(dev))
                exp[lin] = (q, e)
            assert m.down_proj not in exp and len(exp) == 6
            wqkv, wgu = lyr.fused_weights()
            cat = lambda lins: (torch.cat([exp[t][0] for t in lins]), torch.cat([exp[t][1] for t in lins]))  # noqa: E731
            want4.append((wqkv, *cat((a.q_proj, a.k_proj, a.v_proj))))
            want4.append((a.o_proj.weight, *exp[a.o_proj]))
            want4.append((wgu, *cat((m.gate_proj, m.up_proj))))
        v, q, s = _snap_fp8_exact(model.llm.lm_head.weight)
        model.llm.lm_head.weight.copy_(v.to(dtype).to(dev))
    return model, fx, want4, (model.llm.lm_head.weight, q, s)


@pytest.mark.parametrize("dtype", H16)
def test_generate_mxfp4_on_exact_weights_matches_the_16bit_decode(dev, dtype):
    """With the projections snapped to MXFP4-exact and the lm_head to e4m3-exact values the quantised copies hold the
    SAME numbers as the 16-bit masters, so generate(decode_weights="mxfp4") and generate() differ only in the order of
    fp32 sums: the project's criterion for two such decode routes (agreement >= 0.9), also with a forced early eos."""
    model, fx, want4, head = _snapped_model(dtype, dev)
    for W, q, e in want4:                                       # the GPU quantiser reproduces those codes and exponents
        gq, ge = ops.mxfp4_weight(W)
        cg, cr = R.unpack(gq.cpu()), R.unpack(q)
        cg[(cg & 7) == 0], cr[(cr & 7) == 0] = 0, 0             # (apart from the sign of a zero)
        assert torch.equal(ge.cpu(), e) and torch.equal(cg, cr), (cg != cr).float().mean().item()
    gq, gs = ops.fp8_weight(head[0])
    assert torch.equal(gs.cpu(), head[2])
    emb = fx["inputs_embeds"].to(dev).to(dtype)
    kw = dict(inputs_embeds=emb, max_new_tokens=24, pad_token_id=106)
    f = model.llm.generate(eos_token_id=-1, decode_weights="mxfp4", **kw)
    b = model.llm.generate(eos_token_id=-1, **kw)
    assert f.dtype == torch.long and f.shape == b.shape == (emb.shape[0], 24), (f.shape, b.shape)
    agree = (f == b).float().mean().item()
    print(f"generate mxfp4 vs 16-bit {dtype}: agreement {agree:.3f}")
    assert agree >= 0.9, agree
    # force an early stop: the most frequent greedy token as eos
    e = model.llm.generate(eos_token_id=-1, decode_graph=False, **kw)
    eos = int(e[:, 2:].flatten().mode().values)
    f = model.llm.generate(eos_token_id=eos, decode_weights="mxfp4", **kw)
    b = model.llm.generate(eos_token_id=eos, **kw)
    assert f.shape == b.shape and (f == b).float().mean().item() >= 0.9, (f.shape, b.shape)


@pytest.mark.parametrize("B", [2, 8])
def test_generate_mxfp4_really_streams_mxfp4(dev, B):
    """during the decode steps every one of the four projections of every layer goes through ops.decode_linear_mxfp4
    with the copy ops.mxfp4_weight keeps for it and the lm_head through ops.decode_linear_fp8 with its e4m3 copy, no
    16-bit weight-streaming launch happens, the copies are made once across calls and again after the weight version
    moves"""
    lm, cfg_l = _small_llama(dev)
    nl = cfg_l["num_hidden_layers"]
    ids = torch.randint(3, cfg_l["vocab_size"], (B, 21), generator=torch.Generator().manual_seed(B)).to(dev)
    kw = dict(input_ids=ids, max_new_tokens=12, eos_token_id=-1, pad_token_id=0, decode_weights="mxfp4")
    with _Spy("decode_linear_mxfp4", "decode_linear_fp8", "decode_linear", "linear_fwd", "quantize_mxfp4_rows",
              "quantize_fp8_rows") as spy:
        out = lm.generate(**kw)
        assert out.shape == (B, 12)
        assert len(spy.calls["quantize_mxfp4_rows"]) == 4 * nl and len(spy.calls["quantize_fp8_rows"]) == 1
        expect = []
        for lyr in lm.model.layers:
            wqkv, wgu = lyr.fused_weights()
            expect += [wqkv, lyr.self_attn.o_proj.weight, wgu, lyr.mlp.down_proj.weight]
        copies = [ops.mxfp4_weight(W) for W in expect]
        head = ops.fp8_weight(lm.lm_head.weight)
        assert len(spy.calls["quantize_mxfp4_rows"]) == 4 * nl and len(spy.calls["quantize_fp8_rows"]) == 1   # cache hits
        for (q, e), W in zip(copies, expect):
            assert q.shape == (W.shape[0], W.shape[1] // 2) and e.shape == (W.shape[0], W.shape[1] // 32)
        seen = [(a[1].data_ptr(), a[2].data_ptr()) for a in spy.calls["decode_linear_mxfp4"]]
        step = [(q.data_ptr(), e.data_ptr()) for q, e in copies]
        # token 0: lm_head on the prefill's last row; token 1: one eager step; then ONE captured step
        assert seen == step + step, (len(seen), len(step))
        assert [(a[1].data_ptr(), a[2].data_ptr()) for a in spy.calls["decode_linear_fp8"]] == [(head[0].data_ptr(), head[1].data_ptr())] * 3
        assert spy.calls["decode_linear"] == []
        assert [a[0].shape[0] for a in spy.calls["linear_fwd"] if a[0].shape[0] <= 32] == []   # (the prefill has B * 21 rows)
        n_pre = len(spy.calls["linear_fwd"])
        again = lm.generate(**kw)
        assert torch.equal(out, again)                                      # deterministic kernels, same copies
        assert len(spy.calls["quantize_mxfp4_rows"]) == 4 * nl              # quantised once
        ops.bump_weight_version()
        lm.generate(**kw)
        assert len(spy.calls["quantize_mxfp4_rows"]) == 8 * nl and len(spy.calls["quantize_fp8_rows"]) == 2   # re-made
        assert len(spy.calls["linear_fwd"]) == 3 * n_pre                    # the prefill keeps the 16-bit weights
    ref = lm.generate(**{**kw, "decode_weights": None})
    assert ref.shape == out.shape                                           # (ordinary weights: the ids may differ)


def test_generate_mxfp4_refusals_and_default(dev, monkeypatch):
    """decode_weights="mxfp4" raises a ValueError naming the switch value and the condition that keeps the call off the
    hipGraph decode path; None is today's path, launch for launch; MM_LLMs.set_decode_weights routes
    inputs["inference"] = True"""
    fx = load_case("micro_all")
    cfg = configs.get(fx["config_name"])
    model = build_model(cfg, fx["state"], torch.bfloat16, dev, fuse=True).eval()
    emb = fx["inputs_embeds"].to(dev).to(torch.bfloat16)
    kw = dict(inputs_embeds=emb, max_new_tokens=8, eos_token_id=-1, pad_token_id=106)
    with _Spy("decode_linear_mxfp4", "quantize_mxfp4_rows") as spy:
        assert torch.equal(model.llm.generate(**kw), model.llm.generate(decode_weights=None, **kw))
        model.llm.generate(decode_weights="fp8", **kw)
        assert spy.calls["decode_linear_mxfp4"] == [] and spy.calls["quantize_mxfp4_rows"] == []
    with pytest.raises(ValueError, match="decode_weights"):
        model.llm.generate(decode_weights="int4", **kw)
    with pytest.raises(ValueError, match="mxfp4.*use_cache"):
        model.llm.generate(decode_weights="mxfp4", use_cache=False, **kw)
    with pytest.raises(ValueError, match="mxfp4.*decode_graph"):
        model.llm.generate(decode_weights="mxfp4", decode_graph=False, **kw)
    with pytest.raises(ValueError, match="mxfp4.*max_new_tokens"):
        model.llm.generate(decode_weights="mxfp4", **{**kw, "max_new_tokens": 2})
    with pytest.raises(ValueError, match="mxfp4.*decode_attn_ok"):
        model.llm.generate(decode_weights="mxfp4", **{**kw, "max_new_tokens": 16000})
    with pytest.raises(ValueError, match="mxfp4.*33 sequences"):
        model.llm.generate(decode_weights="mxfp4", **{**kw, "inputs_embeds": emb[:1].expand(33, -1, -1).contiguous()})
    monkeypatch.setenv("MACAW_NO_DECODE_GRAPH", "1")
    with pytest.raises(ValueError, match="mxfp4.*MACAW_NO_DECODE_GRAPH"):
        model.llm.generate(decode_weights="mxfp4", **kw)
    monkeypatch.delenv("MACAW_NO_DECODE_GRAPH")
    m32 = build_model(cfg, fx["state"], torch.float32, dev).eval()
    with pytest.raises(ValueError, match="mxfp4.*fp32"):
        m32.llm.generate(decode_weights="mxfp4", **{**kw, "inputs_embeds": fx["inputs_embeds"].to(dev)})
    mu = build_model(cfg, fx["state"], torch.bfloat16, dev, fuse=False).eval()      # (lazy fusion off)
    with pytest.raises(ValueError, match="mxfp4.*unfused"):
        mu.llm.generate(decode_weights="mxfp4", **kw)
    # the multimodal entry point
    with pytest.raises(ValueError):
        Mo.MM_LLMs.set_decode_weights("int4")
    inp = to_dev(fx["inputs"], dev)
    inp["inference"] = True
    Mo.AUTO_FUSE = True
    with torch.no_grad():
        base = model(inputs=inp)
        Mo.MM_LLMs.set_decode_weights("mxfp4")
        with _Spy("decode_linear_mxfp4", "decode_linear_fp8") as spy:
            ids = model(inputs=inp)
        Mo.MM_LLMs.set_decode_weights(None)
    assert len(spy.calls["decode_linear_mxfp4"]) > 0 and len(spy.calls["decode_linear_fp8"]) > 0
    assert ids.dtype == torch.long and ids.shape[0] == base.shape[0]


def test_generate_mxfp4_with_adapters_matches_merge_and_unload(dev):
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
    kw = dict(inputs_embeds=emb, max_new_tokens=12, eos_token_id=-1, pad_token_id=106, decode_weights="mxfp4")
    nl = len(model.llm.model.layers)
    with _Spy("quantize_mxfp4_rows", "quantize_fp8_rows", "decode_linear_mxfp4") as spy:
        a = model.llm.generate(**kw)
        # (down: K = 352 keeps its 16-bit launch; the lm_head has no adapter: its e4m3 copy is cached)
        assert len(spy.calls["quantize_mxfp4_rows"]) == 3 * nl and len(spy.calls["quantize_fp8_rows"]) == 1
        assert len(spy.calls["decode_linear_mxfp4"]) > 0
        model.llm.generate(**kw)
        assert len(spy.calls["quantize_mxfp4_rows"]) == 6 * nl and len(spy.calls["quantize_fp8_rows"]) == 1
    plain = L.merge_and_unload(model.llm)
    b = plain.generate(**kw)
    assert a.shape == b.shape
    agree = (a == b).float().mean().item()
    print(f"generate mxfp4 with adapters vs merged model: agreement {agree:.3f}")
    assert agree >= 0.9, agree


def test_generate_mxfp4_composes_with_the_e4m3_cache_a_padded_batch_and_sampling(dev):
    """one call with kv_cache="fp8", attention_mask= (left and right padding) and seeded sampling runs on the mxfp4 step
    and is repeatable bit for bit"""
    lm, cfg_l = _small_llama(dev)
    B, S0 = 3, 19
    ids = torch.randint(3, cfg_l["vocab_size"], (B, S0), generator=torch.Generator().manual_seed(3)).to(dev)
    mask = torch.ones((B, S0), dtype=torch.long, device=dev)
    mask[0, :5] = 0
    mask[2, -4:] = 0
    kw = dict(input_ids=ids, attention_mask=mask, max_new_tokens=10, eos_token_id=-1, pad_token_id=0,
              decode_weights="mxfp4", kv_cache="fp8", do_sample=True, temperature=0.8, top_k=20, top_p=0.9, seed=1234)
    with _Spy("decode_linear_mxfp4", "decode_step_attn_kv8_var") as spy:
        a = lm.generate(**kw)
        assert len(spy.calls["decode_linear_mxfp4"]) > 0 and len(spy.calls["decode_step_attn_kv8_var"]) > 0
    b = lm.generate(**kw)
    assert a.shape == (B, 10) and a.dtype == torch.long
    assert torch.equal(a, b)
    assert int(a.min()) >= 0 and int(a.max()) < cfg_l["vocab_size"]


# ------------------------------------------------------------------------------------------- real width --
@pytest.fixture(scope="module")
def real_width():
    """LLaMA-7B-dimension weights of one layer, ~ N(0, 0.02) snapped to MXFP4-exact blocks, built once for the module
    (snapped where they will live: tests/mxfp4_ref.py computes on its argument's device)"""
    dev = torch.device("cuda:0")
    D, FF = 4096, 11008
    g = torch.Generator().manual_seed(11)

    def weight(N, K):
        v, q, e = R.snap((torch.randn(N, K, generator=g) * 0.02).to(dev), torch.bfloat16)
        w = v.to(torch.bfloat16)
        assert torch.equal(w.float(), v)
        return w, (q, e)

    ws = dict(wqkv=weight(3 * D, D), wo=weight(D, D), wgu=weight(2 * FF, D), wd=weight(D, FF))
    ws["ln1"] = (1 + 0.1 * torch.randn(D, generator=g)).to(torch.bfloat16).to(dev)
    ws["ln2"] = (1 + 0.1 * torch.randn(D, generator=g)).to(torch.bfloat16).to(dev)
    return ws


@pytest.mark.parametrize("B", [1, 8])
def test_mxfp4_decode_step_real_dimension_layer_vs_16bit_step(dev, B, real_width):
    """One LLaMA-7B-dimension decode step of a layer: the mxfp4 five-launch step against the 16-bit five-launch step on
    the de-quantised (exactly representable) weights, under the bounds of
    test_fp8_decode_step_real_dimension_layer_vs_16bit_step.  B = 1: the prologue forms; B = 8: they exceed the LDS
    budget, the separate RMSNorm / SwiGLU kernels feed the PLAIN mxfp4 launch."""
    D, FF, H = 4096, 11008, 32
    bf = lambda t: t.to(torch.bfloat16)  # noqa: E731
    g = torch.Generator().manual_seed(11 + B)
    T0, Tmax, hd = 150, 160, D // H
    (wqkv, q_qkv), (wo, q_o), (wgu, q_gu), (wd, q_d) = (real_width[k] for k in ("wqkv", "wo", "wgu", "wd"))
    ln1, ln2 = real_width["ln1"], real_width["ln2"]
    if B == 1:                                                  # the device quantiser reproduces the snapped blocks
        gq, ge = ops.mxfp4_weight(wd)
        assert torch.equal(ge, q_d[1])
        cg, cr = R.unpack(gq), R.unpack(q_d[0])
        cg[(cg & 7) == 0], cr[(cr & 7) == 0] = 0, 0
        assert torch.equal(cg, cr)
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
    with torch.no_grad(), _Spy("decode_linear_mxfp4", "decode_linear_fp8", "decode_linear", "linear_fwd") as spy:
        out_f = eng.llama_layer_cached(x2, B, 1, 0, kv_f, Tmax, pos, cos, sin, *args, t_dev=t_dev,
                                       w8=(q_qkv, q_o, q_gu, q_d))
        assert [a[3] if len(a) > 3 else 0 for a in spy.calls["decode_linear_mxfp4"]] == ([1, 0, 1, 2] if B == 1 else [0] * 4)
        assert spy.calls["decode_linear"] == [] and spy.calls["linear_fwd"] == [] and spy.calls["decode_linear_fp8"] == []
        out_b = eng.llama_layer_cached(x2, B, 1, 0, kv_b, Tmax, pos, cos, sin, *args, t_dev=t_dev)
    assert torch.equal(kv_b[:, :T0], kv_f[:, :T0]) and torch.equal(kv_b[:, T0 + 1:], kv_f[:, T0 + 1:])
    same = (kv_b[:, T0] == kv_f[:, T0]).float().mean().item()
    rd = (kv_b[:, T0].float() - kv_f[:, T0].float()).abs().max().item()
    d = (out_b.float() - out_f.float()).abs().max().item()
    ref = out_b.float().abs().max().item()
    print(f"mxfp4 step vs 16-bit step B={B}: cache row equal {same:.4f}, max diff {rd:.3e}; output diff {d:.3e} of {ref:.3e}")
    assert same > 0.98, same
    assert rd <= 2.0 ** -7 * kv_b[:, T0].float().abs().max().item() + 1e-3, rd
    assert d <= 2.0 ** -6 * ref + 1e-3, (d, ref)
