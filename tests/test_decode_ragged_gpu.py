"""GPU: padded-batch decoding, generate(attention_mask=) -- the per-sample-position step kernels against the shipped
ones bit for bit, the compacting cache writes, the entry points' domain, and generate() end to end: fp32 ids against
the restated masked loop (pinned to the reference in tests/test_decode_ragged_cpu.py), the bf16 graph and eager-step
paths against the fp32 oracle teacher-forced (the rule of test_fullsize_gpu), the fp8 modes for batch independence,
the launches that really ran, early stop, the refusals and the multimodal switch."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from golden_util import load_case  # noqa: E402
from oracle import configs  # noqa: E402
from test_decode_kv8_gpu import _Spy, _small_llama, _tables  # noqa: E402
from test_decode_ragged_cpu import masks_of, restated_case, restated_masked_greedy, top2_margin  # noqa: E402
from test_kernels_gpu import DECODE_STEP_SHAPES, H16  # noqa: E402

from macaw_llm_amd import modeling as Mo  # noqa: E402
from macaw_llm_amd import ops  # noqa: E402
from macaw_llm_amd.lib import MacawHipError  # noqa: E402

NEW_OPS = ("decode_step_attn_var", "decode_step_attn_kv8_var", "kv_append_rows", "kv_quant_append_rows")


@pytest.fixture(autouse=True)
def _restore_switches():
    ops.clear_fp8_cache()
    yield
    Mo.AUTO_FUSE = True
    Mo.DECODE_WEIGHTS[0] = None
    Mo.KV_CACHE[0] = None
    Mo.GENERATE_MASK[0] = False
    ops.clear_fp8_cache()


# ------------------------------------------------------------------------------------------------ kernels --
def _four_heads(hd, H, B):
    return hd == 128 and H % 4 == 0 and B * H >= 512


def _positions(hd, H, B, T):
    """p_b per sample: the positions where a lane assignment can go wrong -- both sides of a trip boundary that T allows
    (four heads per workgroup: 8 waves x 8 keys = 64; one head: 8 waves x 64 / (hd / 8) keys per pass x 8 = 256 / 512 /
    1024 / 2048 at hd 128 / 64 / 32 / 16), then 1, T, 0"""
    trip = 64 if _four_heads(hd, H, B) else 8 * 8 * 64 // (hd // 8)
    edge = (trip - 1, trip, trip + 1)
    cand = [p for p in edge if p <= T] + [1, T, 0, T - 1]
    cand = [p for i, p in enumerate(cand) if 0 <= p <= T and p not in cand[:i]]
    return [cand[b % len(cand)] for b in range(B)]


# (the one-head kernels across their trip boundaries: no shape of DECODE_STEP_SHAPES reaches one)
VAR_SHAPES = DECODE_STEP_SHAPES + [(128, 4, 3, 258), (64, 8, 3, 514), (32, 4, 3, 1026), (16, 4, 3, 2050)]


@pytest.mark.parametrize("dtype", H16)
@pytest.mark.parametrize("hd,H,B,T", VAR_SHAPES)
def test_step_attn_var_is_the_shipped_kernel_at_each_samples_position(hd, H, B, T, dtype):
    """sample b of ONE decode_step_attn_var call at *t_dev = T, t_off[b] = p_b - T equals sample b of
    ops.decode_step_attn at *t_dev = p_b (same B, H: the same kernel is selected) in its output row, its appended cache
    row and every other byte of its cache (= the original)"""
    dev = torch.device("cuda:0")
    D, Tmax = H * hd, T + 1
    g = torch.Generator(device=dev).manual_seed(5 * hd + T + B)
    cache0 = torch.randn((B, Tmax, 2 * D), generator=g, device=dev).to(dtype)
    qkv = torch.randn((B, 3 * D), generator=g, device=dev).to(dtype)
    cos, sin = _tables(hd, Tmax, dtype, dev)
    scale = 1.0 / hd ** 0.5
    ps = _positions(hd, H, B, T)
    t_off = torch.tensor([p - T for p in ps], dtype=torch.int32, device=dev)
    cache = cache0.clone()
    out = torch.full((B, D), float("nan"), dtype=dtype, device=dev)
    ops.decode_step_attn_var(qkv, qkv, qkv, 3 * D, cos, sin, cache, torch.tensor([T], dtype=torch.int32, device=dev),
                             t_off, Tmax, B, H, hd, out, scale, k_off=D, v_off=2 * D)
    for p in sorted(set(ps)):
        rc = cache0.clone()
        ro = torch.full((B, D), float("nan"), dtype=dtype, device=dev)
        ops.decode_step_attn(qkv, qkv, qkv, 3 * D, cos, sin, rc, torch.tensor([p], dtype=torch.int32, device=dev), Tmax,
                             B, H, hd, ro, scale, k_off=D, v_off=2 * D)
        for b in [b for b in range(B) if ps[b] == p]:
            assert torch.equal(out[b].view(torch.int16), ro[b].view(torch.int16)), (b, p)
            assert torch.equal(cache[b, p].view(torch.int16), rc[b, p].view(torch.int16)), (b, p)
            rest = [t for t in range(Tmax) if t != p]
            assert torch.equal(cache[b, rest].view(torch.int16), cache0[b, rest].view(torch.int16)), (b, p)
    assert bool(torch.isfinite(out.float()).all())


@pytest.mark.parametrize("dtype", H16)
@pytest.mark.parametrize("hd,H,B,T", VAR_SHAPES)
def test_step_attn_kv8_var_is_the_shipped_kernel_at_each_samples_position(hd, H, B, T, dtype):
    """the same over the e4m3 cache: output row, appended bytes AND scales, every other byte and scale"""
    dev = torch.device("cuda:0")
    D, Tmax = H * hd, T + 1
    g = torch.Generator(device=dev).manual_seed(7 * hd + T + B)
    cache0 = torch.randint(0, 256, (B, Tmax, 2 * D), generator=g, device=dev, dtype=torch.uint8)
    cache0[(cache0 & 0x7F) == 0x7F] = 0                         # (no e4m3 NaN codes: equality is on finite outputs)
    scales0 = torch.rand((B, Tmax, 2 * H), generator=g, device=dev) * 0.01 + 1e-3
    qkv = torch.randn((B, 3 * D), generator=g, device=dev).to(dtype)
    cos, sin = _tables(hd, Tmax, dtype, dev)
    scale = 1.0 / hd ** 0.5
    ps = _positions(hd, H, B, T)
    t_off = torch.tensor([p - T for p in ps], dtype=torch.int32, device=dev)
    cache, scales = cache0.clone(), scales0.clone()
    out = torch.full((B, D), float("nan"), dtype=dtype, device=dev)
    ops.decode_step_attn_kv8_var(qkv, qkv, qkv, 3 * D, cos, sin, cache, scales,
                                 torch.tensor([T], dtype=torch.int32, device=dev), t_off, Tmax, B, H, hd, out, scale,
                                 k_off=D, v_off=2 * D)
    i32 = lambda t: t.view(torch.int32)  # noqa: E731
    for p in sorted(set(ps)):
        rc, rs = cache0.clone(), scales0.clone()
        ro = torch.full((B, D), float("nan"), dtype=dtype, device=dev)
        ops.decode_step_attn_kv8(qkv, qkv, qkv, 3 * D, cos, sin, rc, rs, torch.tensor([p], dtype=torch.int32, device=dev),
                                 Tmax, B, H, hd, ro, scale, k_off=D, v_off=2 * D)
        for b in [b for b in range(B) if ps[b] == p]:
            assert torch.equal(out[b].view(torch.int16), ro[b].view(torch.int16)), (b, p)
            assert torch.equal(cache[b, p], rc[b, p]) and torch.equal(i32(scales[b, p]), i32(rs[b, p])), (b, p)
            rest = [t for t in range(Tmax) if t != p]
            assert torch.equal(cache[b, rest], cache0[b, rest]), (b, p)
            assert torch.equal(i32(scales[b, rest]), i32(scales0[b, rest])), (b, p)
    assert bool(torch.isfinite(out.float()).all())


def _append_case(Sn, Tmax, dev):
    """slots [4, Sn] of an all-skipped sample (one of its slots past the cache: never written), a left-padded, a
    right-padded and a holed one"""
    m = torch.ones((4, Sn), dtype=torch.long)
    m[0] = 0
    m[1, :Sn // 3] = 0
    m[2, Sn - Sn // 3:] = 0
    m[3, 1::3] = 0
    slot = torch.where(m != 0, m.cumsum(1) - 1, torch.full_like(m, -1)).to(torch.int32)
    slot[0, Sn // 2] = Tmax
    return slot.to(dev)


@pytest.mark.parametrize("dtype", H16)
@pytest.mark.parametrize("Sn", [1, 21])
@pytest.mark.parametrize("hd,H", [(128, 4), (64, 8), (32, 4), (16, 4)])
def test_kv_append_rows_compacts_and_touches_nothing_else(hd, H, Sn, dtype):
    """16-bit cache: the written rows are the source rows bit for bit (k and v slices of one fused [B * Sn, 3D] buffer),
    every other byte keeps the pattern the cache was filled with"""
    dev = torch.device("cuda:0")
    B, D, Tmax = 4, H * hd, Sn + 3
    slot = _append_case(Sn, Tmax, dev)
    g = torch.Generator(device=dev).manual_seed(hd + Sn)
    qkv = torch.randn((B * Sn, 3 * D), generator=g, device=dev).to(dtype)
    cache = torch.empty((B, Tmax, 2 * D), dtype=dtype, device=dev)
    cache.view(torch.uint8).fill_(0x5A)
    ops.kv_append_rows(qkv[:, D:2 * D], qkv[:, 2 * D:], 3 * D, Sn * 3 * D, cache, slot, Sn, Tmax, B, H, hd)
    want = torch.empty_like(cache)
    want.view(torch.uint8).fill_(0x5A)
    src = qkv.view(B, Sn, 3 * D)
    written = 0
    for b in range(B):
        for j in range(Sn):
            r = int(slot[b, j])
            if 0 <= r < Tmax:
                want[b, r] = src[b, j, D:]
                written += 1
    assert written == (Sn - Sn // 3) * 2 + Sn - len(range(1, Sn, 3))
    assert torch.equal(cache.view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("dtype", H16)
@pytest.mark.parametrize("Sn", [1, 21])
@pytest.mark.parametrize("hd,H", [(128, 4), (64, 8), (32, 4), (16, 4)])
def test_kv_quant_append_rows_writes_what_kv_quant_append_writes(hd, H, Sn, dtype):
    """e4m3 cache: bytes and scales of the written rows equal those ops.kv_quant_append writes for the same source rows
    into a scratch cache; every other byte and scale keeps its pattern"""
    dev = torch.device("cuda:0")
    B, D, Tmax = 4, H * hd, Sn + 3
    slot = _append_case(Sn, Tmax, dev)
    g = torch.Generator(device=dev).manual_seed(hd + Sn + 1)
    qkv = torch.randn((B * Sn, 3 * D), generator=g, device=dev)
    qkv = (qkv * torch.pow(2.0, torch.randint(-6, 7, (B * Sn, 1), generator=g, device=dev).float())).to(dtype)
    k, v = qkv[:, D:2 * D], qkv[:, 2 * D:]
    sc, ss = ops.kv8_cache(B, Tmax, H, hd, dev)
    ops.kv_quant_append(k, v, 3 * D, Sn * 3 * D, sc, ss, 0, Sn, Tmax, B, H, hd)
    cache, scales = ops.kv8_cache(B, Tmax, H, hd, dev)
    cache.fill_(0x5A)
    scales.fill_(7.0)
    ops.kv_quant_append_rows(k, v, 3 * D, Sn * 3 * D, cache, scales, slot, Sn, Tmax, B, H, hd)
    want_c, want_s = torch.full_like(cache, 0x5A), torch.full_like(scales, 7.0)
    for b in range(B):
        for j in range(Sn):
            r = int(slot[b, j])
            if 0 <= r < Tmax:
                want_c[b, r], want_s[b, r] = sc[b, j], ss[b, j]
    assert torch.equal(cache, want_c)
    assert torch.equal(scales.view(torch.int32), want_s.view(torch.int32))


def test_ragged_domain_is_checked_in_the_entry_points(dtype=torch.bfloat16):
    """null, hd = 48, a misaligned pointer, a pitch that breaks the 16-byte accesses, wrong dtypes of cache / scales /
    slot / t_off: an error from each of the four entry points and nothing is launched (caches, scales and outputs keep
    their contents)"""
    dev = torch.device("cuda:0")
    B, H, hd, Tmax = 2, 4, 64, 8
    D = H * hd
    lib = ops._L.load()

    def fresh(H=H, hd=hd):
        cache, scales = ops.kv8_cache(B, Tmax, H, hd, dev)
        cache.fill_(3)
        scales.fill_(7.0)
        c16 = torch.full((B, Tmax, 2 * H * hd), 7.0, device=dev).to(dtype)
        return cache, scales, c16, torch.full((B, H * hd), 7.0, device=dev).to(dtype)

    def untouched(cache, scales, c16, out):
        torch.cuda.synchronize()
        assert bool((cache == 3).all()) and bool((scales == 7.0).all()) and bool((c16 == 7.0).all()) and bool((out == 7.0).all())

    cos, sin = _tables(hd, Tmax, dtype, dev)
    t_dev = torch.tensor([2], dtype=torch.int32, device=dev)
    t_off = torch.tensor([-1, 0], dtype=torch.int32, device=dev)
    slot = torch.tensor([0, 1], dtype=torch.int32, device=dev)
    buf = torch.randn(B * (3 * D + 8) + 8, device=dev).to(dtype)
    good = buf[:B * 3 * D].view(B, 3 * D)
    off = buf[1:1 + B * 3 * D].view(B, 3 * D)                   # 2 bytes off a 16-byte boundary
    pitched = buf[:B * (3 * D + 4)].view(B, 3 * D + 4)          # sample stride % 8 != 0

    def all_four(x, ld, H=H, hd=hd, cs=(cos, sin), t_off=t_off, slot=slot, err="MK_ERR_UNSUPPORTED"):
        Dh = H * hd
        for op in NEW_OPS:
            c = fresh(H, hd)
            c8, s8 = c[0], c[1]
            with pytest.raises(MacawHipError, match=err):
                if op == "decode_step_attn_var":
                    ops.decode_step_attn_var(x, x, x, ld, *cs, c[2], t_dev, t_off, Tmax, B, H, hd, c[3], 0.125,
                                             k_off=Dh, v_off=2 * Dh)
                elif op == "decode_step_attn_kv8_var":
                    ops.decode_step_attn_kv8_var(x, x, x, ld, *cs, c8, s8, t_dev, t_off, Tmax, B, H, hd, c[3], 0.125,
                                                 k_off=Dh, v_off=2 * Dh)
                elif op == "kv_append_rows":
                    ops.kv_append_rows(x[:, Dh:2 * Dh], x[:, 2 * Dh:], ld, ld, c[2], slot, 1, Tmax, B, H, hd)
                else:
                    ops.kv_quant_append_rows(x[:, Dh:2 * Dh], x[:, 2 * Dh:], ld, ld, c8, s8, slot, 1, Tmax, B, H, hd)
            untouched(*c)

    c = fresh()                                                 # the aligned calls are inside the domain
    ops.decode_step_attn_var(good, good, good, 3 * D, cos, sin, c[2], t_dev, t_off, Tmax, B, H, hd, c[3], 0.125,
                             k_off=D, v_off=2 * D)
    ops.decode_step_attn_kv8_var(good, good, good, 3 * D, cos, sin, c[0], c[1], t_dev, t_off, Tmax, B, H, hd, c[3],
                                 0.125, k_off=D, v_off=2 * D)
    ops.kv_append_rows(good[:, D:2 * D], good[:, 2 * D:], 3 * D, 3 * D, c[2], slot, 1, Tmax, B, H, hd)
    ops.kv_quant_append_rows(good[:, D:2 * D], good[:, 2 * D:], 3 * D, 3 * D, c[0], c[1], slot, 1, Tmax, B, H, hd)
    torch.cuda.synchronize()
    all_four(off, 3 * D)
    all_four(pitched, 3 * D + 4)
    all_four(good, 3 * 4 * 48, H=4, hd=48, cs=_tables(48, Tmax, dtype, dev))       # (B * 3 * 192 elements fit in `good`)
    # wrong dtypes: refused by the wrappers before any entry point is called
    all_four(good, 3 * D, t_off=t_off.long(), slot=slot.long(), err="int32")
    all_four(good, 3 * D, t_off=t_off.float(), slot=slot.float(), err="int32")
    for op in ("kv_append_rows", "decode_step_attn_var"):       # a cache of another element type than the tokens
        c = list(fresh())
        c[2] = torch.full(c[2].shape, 7.0, device=dev, dtype=torch.float16)
        with pytest.raises(MacawHipError, match="cache"):
            if op == "kv_append_rows":
                ops.kv_append_rows(good[:, D:2 * D], good[:, 2 * D:], 3 * D, 3 * D, c[2], slot, 1, Tmax, B, H, hd)
            else:
                ops.decode_step_attn_var(good, good, good, 3 * D, cos, sin, c[2], t_dev, t_off, Tmax, B, H, hd, c[3],
                                         0.125, k_off=D, v_off=2 * D)
        untouched(*c)
    for op in ("kv_quant_append_rows", "decode_step_attn_kv8_var"):     # a 16-bit cache / 16-bit scales for the kv8 ops
        c = fresh()
        with pytest.raises(MacawHipError, match="expected uint8"):
            if op == "kv_quant_append_rows":
                ops.kv_quant_append_rows(good[:, D:2 * D], good[:, 2 * D:], 3 * D, 3 * D, c[2], c[1], slot, 1, Tmax, B, H, hd)
            else:
                ops.decode_step_attn_kv8_var(good, good, good, 3 * D, cos, sin, c[0], c[1].to(dtype), t_dev, t_off, Tmax,
                                             B, H, hd, c[3], 0.125, k_off=D, v_off=2 * D)
        untouched(*c)
    # null arguments and zero sizes at the C entry points: MK_ERR_BAD_ARG
    c = fresh()
    p = lambda t: t.data_ptr()  # noqa: E731
    kp, vp = p(good) + 2 * D, p(good) + 4 * D
    rcs = [
        lib.mk_decode_step_attn_var(p(good), kp, vp, 3 * D, p(cos), p(sin), p(c[2]), p(c[2]) + 2 * D, 2 * D, Tmax * 2 * D,
                                    p(c[3]), D, p(t_dev), None, Tmax, B, H, hd, 0.125, ops.dt(good), None),
        lib.mk_decode_step_attn_kv8_var(p(good), kp, vp, 3 * D, p(cos), p(sin), p(c[0]), p(c[1]), p(c[3]), D, p(t_dev),
                                        None, Tmax, B, H, hd, 0.125, ops.dt(good), None),
        lib.mk_kv_append_rows(kp, vp, 3 * D, 3 * D, p(c[2]), None, 1, Tmax, B, H, hd, ops.dt(good), None),
        lib.mk_kv_quant_append_rows(kp, vp, 3 * D, 3 * D, p(c[0]), p(c[1]), None, 1, Tmax, B, H, hd, ops.dt(good), None),
        lib.mk_kv_append_rows(kp, vp, 3 * D, 3 * D, None, p(slot), 1, Tmax, B, H, hd, ops.dt(good), None),
        lib.mk_kv_append_rows(kp, vp, 3 * D, 3 * D, p(c[2]), p(slot), 0, Tmax, B, H, hd, ops.dt(good), None),
        lib.mk_kv_quant_append_rows(kp, vp, 3 * D, 3 * D, p(c[0]), None, p(slot), 1, Tmax, B, H, hd, ops.dt(good), None),
        lib.mk_kv_quant_append_rows(kp, vp, 3 * D, 3 * D, p(c[0]), p(c[1]), p(slot), 0, Tmax, B, H, hd, ops.dt(good), None),
        lib.mk_decode_step_attn_var(p(good), kp, vp, 3 * D, p(cos), p(sin), p(c[2]), p(c[2]) + 2 * D, 2 * D, Tmax * 2 * D,
                                    p(c[3]), D, None, p(t_off), Tmax, B, H, hd, 0.125, ops.dt(good), None),
        lib.mk_decode_step_attn_kv8_var(p(good), kp, vp, 3 * D, p(cos), p(sin), p(c[0]), p(c[1]), p(c[3]), D, p(t_dev),
                                        p(t_off), 0, B, H, hd, 0.125, ops.dt(good), None),
    ]
    for i, rc in enumerate(rcs):
        with pytest.raises(MacawHipError, match="MK_ERR_BAD_ARG"):
            ops._L.check(rc, f"call {i}")
    untouched(*c)


# --------------------------------------------------------------------------------------------- generate() --
@pytest.fixture(scope="module")
def micro32(dev):
    from test_model_gpu import build_model
    fx = load_case("micro_all")
    cfg = configs.get(fx["config_name"])
    return build_model(cfg, fx["state"], torch.float32, dev).eval(), fx, cfg


@pytest.mark.parametrize("kind", ["left", "right", "holes"])
def test_generate_fp32_ids_are_the_restated_masked_loops(dev, micro32, kind):
    """use_cache=False in fp32 on micro_all: the ids of the restated masked loop bit for bit (its smallest top-1 /
    top-2 margin recomputed here and > 5e-3, the fp32 engine within ~1e-4 of those logits), each sample alone on its
    compacted valid tokens gives the same ids, and -- what fails without the feature -- the left mask changes sample 1"""
    model, fx, cfg = micro32
    mask, want, z = restated_case(kind)
    m = top2_margin(z)
    print(f"{kind}: restated ids {want.tolist()}, smallest top-1 / top-2 margin {m:.3e}")
    assert m > 5e-3, m
    emb = fx["inputs_embeds"].to(dev)
    kw = dict(max_new_tokens=8, eos_token_id=-1, pad_token_id=106, use_cache=False)
    got = model.llm.generate(inputs_embeds=emb, attention_mask=mask.to(dev), **kw)
    assert got.dtype == torch.long and torch.equal(got.cpu(), want), (got.tolist(), want.tolist())
    for b in range(emb.shape[0]):
        solo = emb[b:b + 1][:, mask[b].bool().to(dev)].contiguous()
        one = model.llm.generate(inputs_embeds=solo, **kw)
        assert torch.equal(one[0].cpu(), want[b]), (b, one[0].tolist(), want[b].tolist())
    if kind == "left":
        plain = model.llm.generate(inputs_embeds=emb, **kw)
        assert torch.equal(plain[0], got[0]) and not torch.equal(plain[1], got[1]), (plain.tolist(), got.tolist())
        assert got[1, :4].tolist() == [60, 84, 4, 62] and plain[1, :3].tolist() == [98, 4, 41]
        for m_bool in (mask.bool(), mask.to(torch.int32)):      # any integer or bool dtype
            assert torch.equal(model.llm.generate(inputs_embeds=emb, attention_mask=m_bool.to(dev), **kw), got)


def _lm_masks(B, S0):
    """left / right / holes for a [B, S0] prompt, every sample padded somewhere in `left`"""
    ms = masks_of(B, S0)
    for b in range(B):
        ms["left"][b, :2 + 3 * b] = 0
    return ms


def _oracle_state(lm):
    return {"llm." + k: v.detach().float() for k, v in lm.state_dict().items()}


@pytest.mark.parametrize("kind", ["left", "right", "holes"])
def test_generate_bf16_graph_and_eager_step_ids_against_the_fp32_oracle(dev, kind):
    """every id emitted on the hipGraph path and on the kernel-by-kernel step loop is the fp32 oracle's argmax,
    teacher-forced on the path's own ids with the mask and the cumsum positions, or loses to it by no more than the bf16
    noise there (the rule of test_fullsize_gpu.test_generate_at_7b_dimensions_...):
        z32[top] - z32[id] <= 3.0 * max|z16 - z32|,   z16 = the same restatement in eager bf16"""
    lm, cfg_l = _small_llama(dev)
    B, S0, N = 3, 21, 12
    ids = torch.randint(3, cfg_l["vocab_size"], (B, S0), generator=torch.Generator().manual_seed(B)).to(dev)
    mask = _lm_masks(B, S0)[kind].to(dev)
    kw = dict(input_ids=ids, attention_mask=mask, max_new_tokens=N, eos_token_id=-1, pad_token_id=0)
    with _Spy("decode_step_attn_var") as spy:
        g = lm.generate(**kw)
        n_graph = len(spy.calls["decode_step_attn_var"])
        e = lm.generate(decode_graph=False, **kw)
        n_eager = len(spy.calls["decode_step_attn_var"]) - n_graph
    nl = cfg_l["num_hidden_layers"]
    assert g.shape == e.shape == (B, N) and n_graph == 2 * nl and n_eager == (N - 1) * nl
    assert torch.equal(g, e)                    # the same launches, replayed or one by one
    sd32 = _oracle_state(lm)
    sd16 = {k: v.to(torch.bfloat16) for k, v in sd32.items()}
    emb = torch.nn.functional.embedding(ids, sd32["llm.model.embed_tokens.weight"])
    with torch.no_grad():
        for tag, got in (("graph", g), ("eager", e)):
            _, z32 = restated_masked_greedy(sd32, emb, mask, cfg_l, N, force_ids=got)
            _, z16 = restated_masked_greedy(sd16, emb.to(torch.bfloat16), mask, cfg_l, N, force_ids=got)
            z32, z16 = z32.float(), z16.float()
            margin = z32.max(-1).values - z32.gather(-1, got[..., None]).squeeze(-1)
            noise = (z16 - z32).abs().max(-1).values
            print(f"{kind} {tag}: ids off the oracle's argmax {(margin > 0).sum().item()}, worst margin / noise "
                  f"{(margin / noise.clamp_min(1e-12)).max().item():.3f}")
            assert (margin <= 3.0 * noise).all(), (tag, margin.tolist(), noise.tolist())


@pytest.mark.parametrize("mode", [dict(kv_cache="fp8"), dict(decode_weights="fp8"),
                                  dict(kv_cache="fp8", decode_weights="fp8")])
def test_generate_fp8_modes_take_the_mask_and_do_not_depend_on_the_batch(dev, mode):
    """shape, determinism, and the ids of a left-padded batch equal those of its samples run alone left-padded to the
    same S0 (same kernels, same reduction order)"""
    lm, cfg_l = _small_llama(dev)
    B, S0, N = 3, 21, 12
    ids = torch.randint(3, cfg_l["vocab_size"], (B, S0), generator=torch.Generator().manual_seed(B)).to(dev)
    mask = _lm_masks(B, S0)["left"].to(dev)
    kw = dict(max_new_tokens=N, eos_token_id=-1, pad_token_id=0, **mode)
    want = "decode_step_attn_kv8_var" if "kv_cache" in mode else "decode_step_attn_var"
    with _Spy(*NEW_OPS, "decode_linear_fp8") as spy:
        out = lm.generate(input_ids=ids, attention_mask=mask, **kw)
        assert len(spy.calls[want]) == 2 * cfg_l["num_hidden_layers"]
        assert ("decode_weights" in mode) == (len(spy.calls["decode_linear_fp8"]) > 0)
    assert out.shape == (B, N) and out.dtype == torch.long
    assert torch.equal(out, lm.generate(input_ids=ids, attention_mask=mask, **kw))
    for b in range(B):
        one = lm.generate(input_ids=ids[b:b + 1].contiguous(), attention_mask=mask[b:b + 1].contiguous(), **kw)
        assert torch.equal(one[0], out[b]), (b, one[0].tolist(), out[b].tolist())


def test_generate_routes_a_padded_batch_through_the_new_launches_only(dev):
    lm, cfg_l = _small_llama(dev)
    nl, D = cfg_l["num_hidden_layers"], cfg_l["hidden_size"]
    B, S0, N = 3, 21, 12
    ids = torch.randint(3, cfg_l["vocab_size"], (B, S0), generator=torch.Generator().manual_seed(B)).to(dev)
    mask = _lm_masks(B, S0)["holes"].to(dev)
    kw = dict(input_ids=ids, max_new_tokens=N, eos_token_id=-1, pad_token_id=0)
    old = ("decode_step_attn", "decode_step_attn_kv8", "kv_quant_append", "copy2d")

    def into_a_cache(calls):
        return [a for a in calls if tuple(a[1].shape) == (B, S0 + N, 2 * D)]

    with _Spy(*NEW_OPS, *old) as spy:
        lm.generate(attention_mask=mask, **kw)
        assert len(spy.calls["kv_append_rows"]) == nl and len(spy.calls["decode_step_attn_var"]) == 2 * nl
        assert spy.calls["decode_step_attn"] == [] and into_a_cache(spy.calls["copy2d"]) == []
        assert spy.calls["kv_quant_append_rows"] == [] and spy.calls["decode_step_attn_kv8_var"] == []
    with _Spy(*NEW_OPS, *old) as spy:
        lm.generate(attention_mask=mask, kv_cache="fp8", **kw)
        assert len(spy.calls["kv_quant_append_rows"]) == nl and len(spy.calls["decode_step_attn_kv8_var"]) == 2 * nl
        assert spy.calls["decode_step_attn"] == [] and spy.calls["decode_step_attn_kv8"] == []
        assert spy.calls["kv_quant_append"] == [] and into_a_cache(spy.calls["copy2d"]) == []
        assert spy.calls["kv_append_rows"] == [] and spy.calls["decode_step_attn_var"] == []
    with _Spy(*NEW_OPS, *old) as spy:
        none = lm.generate(**kw)
        ones = lm.generate(attention_mask=torch.ones_like(mask), **kw)
        assert all(spy.calls[n] == [] for n in NEW_OPS)
        assert len(spy.calls["decode_step_attn"]) == 4 * nl and len(into_a_cache(spy.calls["copy2d"])) == 2 * nl
        assert torch.equal(none, ones)


def test_generate_padded_early_stop_is_the_same_on_the_graph_and_the_eager_step_path(dev):
    """an early eos (the most frequent greedy token): a finished sample emits pad from then on, the output stops at the
    column at which every sample has finished, identically on both paths"""
    lm, cfg_l = _small_llama(dev)
    B, S0, N = 4, 21, 24
    ids = torch.randint(3, cfg_l["vocab_size"], (B, S0), generator=torch.Generator().manual_seed(B)).to(dev)
    mask = _lm_masks(B, S0)["left"].to(dev)
    kw = dict(input_ids=ids, attention_mask=mask, max_new_tokens=N, pad_token_id=0)
    free = lm.generate(eos_token_id=-1, **kw)
    eos = int(free[:, 2:].flatten().mode().values)
    f = lm.generate(eos_token_id=eos, **kw)
    e = lm.generate(eos_token_id=eos, decode_graph=False, **kw)
    assert torch.equal(f, e), (f.tolist(), e.tolist())
    assert f.dtype == torch.long and f.shape[0] == B and f.shape[1] <= N
    hit = (f == eos).cumsum(1) > 0
    assert bool(hit[:, -1].all()) or f.shape[1] == N
    if 2 <= f.shape[1] < N:
        assert not bool(hit[:, -2].all())
    after = torch.zeros_like(hit)
    after[:, 1:] = hit[:, :-1]
    assert bool(after.any()) and bool((f[after] == 0).all())    # pad after a sample's eos
    assert torch.equal(f[~after], free[:, :f.shape[1]][~after])  # and the unconstrained ids before it


def test_generate_mask_refusals_and_the_multimodal_switch(dev, micro32):
    from test_model_gpu import build_model, to_dev
    m32, fx, cfg = micro32
    emb32 = fx["inputs_embeds"].to(dev)
    B, S0 = emb32.shape[:2]
    left = masks_of(B, S0)["left"].to(dev)
    kw = dict(max_new_tokens=8, eos_token_id=-1, pad_token_id=106)
    with _Spy(*NEW_OPS) as spy:
        dead = left.clone()
        dead[0] = 0
        with pytest.raises(ValueError, match="no valid token"):
            m32.llm.generate(inputs_embeds=emb32, attention_mask=dead, **kw)
        for bad in (left[:, :-1], left[:1], left.view(-1)):
            with pytest.raises(ValueError, match="should be of size"):
                m32.llm.generate(inputs_embeds=emb32, attention_mask=bad, **kw)
        with pytest.raises(ValueError, match="use_cache=False"):            # fp32, padded, cached
            m32.llm.generate(inputs_embeds=emb32, attention_mask=left, **kw)
        with pytest.raises(ValueError, match="use_cache=False"):
            m32.llm.generate(inputs_embeds=emb32, attention_mask=left, decode_graph=False, **kw)
        # an all-ones mask in fp32 is today's call
        assert torch.equal(m32.llm.generate(inputs_embeds=emb32, attention_mask=torch.ones_like(left), **kw),
                           m32.llm.generate(inputs_embeds=emb32, **kw))
        assert all(spy.calls[n] == [] for n in NEW_OPS)
    model = build_model(cfg, fx["state"], torch.bfloat16, dev, fuse=True).eval()
    with pytest.raises(ValueError, match="decode_attn_ok"):                 # 16-bit, outside the step kernels' lengths
        model.llm.generate(inputs_embeds=emb32.to(torch.bfloat16), attention_mask=left, **{**kw, "max_new_tokens": 16000})
    # the multimodal entry point: off by default (the reference drops its mask), on = generate(attention_mask=extended)
    inp = to_dev(fx["inputs"], dev)
    inp["inference"] = True
    Mo.AUTO_FUSE = True
    with torch.no_grad():
        emb, am, _ = model.prepare_inputs_for_generation(inp)
        assert bool((am == 0).any())                                        # (micro_all: a padded tail on the odd rows)
        gk = dict(inputs_embeds=emb, max_new_tokens=128, eos_token_id=2, bos_token_id=1, pad_token_id=32006)
        want_off, want_on = model.llm.generate(**gk), model.llm.generate(attention_mask=am, **gk)
        with _Spy(*NEW_OPS) as spy:
            base = model(inputs=inp)
            assert all(spy.calls[n] == [] for n in NEW_OPS)
            Mo.MM_LLMs.set_generate_mask(True)
            ids = model(inputs=inp)
            assert len(spy.calls["decode_step_attn_var"]) > 0 and len(spy.calls["kv_append_rows"]) > 0
            Mo.MM_LLMs.set_generate_mask(False)
            again = model(inputs=inp)
    assert torch.equal(base, want_off) and torch.equal(again, want_off) and torch.equal(ids, want_on)
