"""fp64 reference of the decode attention kernels (mk_decode_step_attn and its _var, _beam, _multi, _kv8, _kv8_var forms,
mk_decode_attn), shared by tests/test_decode_attn_edges_gpu.py, tests/test_decode_attn_ref_cpu.py and the two older
step-attention tests:  o = softmax(scale q . k_t) v  over the cache rows given, from the bits AS STORED, widened exactly to
float64, together with  o_abs = sum_t p_t |v_t|,  the natural scale of the accumulation error.

The query is the RoPE-rotated query (mk_rope is pinned elsewhere), the cache is the cache as it stands AFTER the call (the
append is pinned bit for bit elsewhere).  `scale` is rounded to fp32 first: the entry points take a float.

The module also holds the kernels' geometry, the positions at which a lane assignment can go wrong, the seeded input
families, and the bound the kernels are held to.  Everything is torch on the CPU.
"""
import collections
import math

import torch

import fp8_ref

# ---------------------------------------------------------------------------------------------------- geometry --
# A body's key -> lane map, restated from the template parameters of csrc/decode_impl.inc and csrc/decode_kv8_impl.inc:
#   decode_step_attn_body<HD, NWV = 8> and decode_step_attn_kv8_kernel<HD, E = 8, HG = 1, NWV = 8>  (one head per workgroup):
#       LPK = HD / 8 lanes per key, KPW = 64 / LPK keys per wave and pass, KPP = NWV * KPW keys per pass, NB = 8 keys per lane
#       group in flight: a trip of the online softmax is KPP * NB keys
#   decode_step_attn4_kernel<NWV = 8>  (four heads per workgroup, hd 128, B * H >= 512, H % 4 == 0): a wave holds ONE key of
#       four heads, KPP = NWV, trip = NWV * NB
#   decode_step_attn_kv8_kernel<128, E = 16, HG = 4, NWV = 8>: LPK = 8, KPW = 64 / (LPK * HG) = 2, KPP = 16, trip = 128
#   decode_attn_kernel<HD>  (mk_decode_attn: 4 waves, three passes, scores in LDS): KPW as one head, KPP = 4 * KPW, no trip;
#       its second pass strides by the 256 threads
Body = collections.namedtuple("Body", "name hd kpw kpp trip")
NB, NWV = 8, 8


def one_head(hd):
    kpw = 64 // (hd // 8)
    return Body(f"one-head hd{hd}", hd, kpw, NWV * kpw, NWV * kpw * NB)


FOUR16 = Body("four-heads 16-bit", 128, 1, NWV, NWV * NB)
FOUR8 = Body("four-heads kv8", 128, 2, 2 * NWV, 2 * NWV * NB)


def attn3(hd):
    kpw = 64 // (hd // 8)
    return Body(f"mk_decode_attn hd{hd}", hd, kpw, 4 * kpw, None)


ATTN3_STRIDE = 256                      # threads of decode_attn_kernel: the stride of its pass 2
ATTN3_T_MAX = 60 * 1024 // 4            # its scores live in 60 KiB of LDS


def four_heads(hd, H, B):
    """the entry points' selection of the four-heads-per-workgroup bodies"""
    return hd == 128 and H % 4 == 0 and B * H >= 512


def edge_positions(body):
    """last-key indices p (T = p + 1) at which a key can be skipped, read twice or paired with the wrong value row: the
    first key, both sides of a wave's share, of a pass and of a trip (p = trip - 1: the last full trip; p = trip: the new
    key alone in a trip; p = trip + 1: a cached key alone in front of it), the second trip, and a third one with a ragged
    pass.  Sorted, unique."""
    k, pp, tr = body.kpw, body.kpp, body.trip
    return sorted({0, 1, k - 1, k, pp - 1, pp, pp + 1, tr - 2, tr - 1, tr, tr + 1, 2 * tr - 1, 2 * tr, 2 * tr + pp + 1})


def attn3_lengths(body):
    """T of mk_decode_attn: one key, both sides of a pass, both sides of the second pass's stride, three strides + a
    ragged pass"""
    pp = body.kpp
    return sorted({1, pp - 1, pp, pp + 1, ATTN3_STRIDE - 1, ATTN3_STRIDE, ATTN3_STRIDE + 1, 2 * ATTN3_STRIDE + pp + 1})


def census_length(body):
    """a full trip, a full pass and a ragged rest"""
    return body.trip + body.kpp + 3


# ------------------------------------------------------------------------------------------------------- bound --
# |out - ref| <= u * max(|ref|, tiny) + a * o_abs  per output element.
#   u     unit round-off of the ONE rounding the header promises (fp32 quotient -> output type)
#   tiny  the output type's smallest normal number: below it that rounding is absolute (half a subnormal step = u * tiny),
#         not relative -- an expectation of 1e-15 (the K census's leak) is 0 in f16, correctly
#   a     fp32 accumulation and __expf, measured against this reference over every case of
#         tests/test_decode_attn_edges_gpu.py (table in that module's docstring) and set to 4x the largest value seen;
#         A_CAP = 2^-14 (one eighth of f16's u) is what the census's sharpness is proven for in test_decode_attn_ref_cpu.py
U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
A_CAP = 2.0 ** -14
A = 4 * 4.88e-6                 # = 1.95e-5 = 2^-15.6; largest measured: 4.88e-6 (four heads per workgroup, kv8, f16)


def bound(ref, o_abs, dtype, a=None):
    a = A if a is None else a
    return U[dtype] * ref.abs().clamp_min(torch.finfo(dtype).tiny) + a * o_abs


def measured_a(out, ref, o_abs, dtype):
    """the smallest a under which `out` meets the bound (<= 0: the rounding term alone covers it); inf if an element
    without accumulation scale (o_abs = 0) is off"""
    exc = (out.double() - ref).abs() - bound(ref, o_abs, dtype, a=0.0)
    if not bool(torch.isfinite(exc).all()):
        return float("inf")
    live = o_abs > 0
    if bool((exc[~live] > 0).any()):
        return float("inf")
    return (exc[live] / o_abs[live]).max().item() if bool(live.any()) else 0.0


def assert_within(out, ref, o_abs, dtype, what, a=None):
    """prints the measured a, then asserts the bound element by element"""
    out = out.detach().double().cpu()
    m = measured_a(out, ref, o_abs, dtype)
    print(f"[decode-attn] {what} {str(dtype).split('.')[-1]}: measured a {m:.3e}")
    err = (out - ref).abs()
    ok = err <= bound(ref, o_abs, dtype, a)
    assert bool(ok.all()), (what, m, int((~ok).sum()), err[~ok].max().item() if bool((~ok).any()) else float("nan"))
    return m


# --------------------------------------------------------------------------------------------------- reference --
def _f32(x):
    return float(torch.tensor(x, dtype=torch.float32))


def _attend(q, k, v, scale):
    """q [B, H, hd], k, v [B, T, H, hd], float64 -> (o, o_abs) [B, H * hd]"""
    B, H, hd = q.shape
    s = torch.einsum("bhd,bthd->bht", q, k) * _f32(scale)
    p = torch.softmax(s, dim=-1)
    o = torch.einsum("bht,bthd->bhd", p, v)
    o_abs = torch.einsum("bht,bthd->bhd", p, v.abs())
    return o.reshape(B, H * hd), o_abs.reshape(B, H * hd)


def ref16(q_rot, cache_rows, H, hd, scale):
    """q_rot [B, H * hd], cache_rows [B, T, 2 * H * hd] = [keys | values] per row, both 16-bit -> (o, o_abs) float64"""
    B, T, D2 = cache_rows.shape
    D = H * hd
    assert D2 == 2 * D and q_rot.shape == (B, D)
    kv = cache_rows.double().reshape(B, T, 2, H, hd)
    return _attend(q_rot.double().reshape(B, H, hd), kv[:, :, 0], kv[:, :, 1], scale)


def dequant_kv8(q_bytes, scales, hd):
    """float64 values of an e4m3 cache: code x scale; bytes [..., n * hd] uint8, scales [..., n] float32"""
    return (fp8_ref.decode_bytes(q_bytes).reshape(*scales.shape, hd) * scales.double()[..., None]).reshape(q_bytes.shape)


def ref_kv8(q_rot, q_bytes, scales, H, hd, scale):
    """the same over an e4m3 cache: bytes [B, T, 2 * H * hd] uint8, scales [B, T, 2 * H] float32"""
    B, T, D2 = q_bytes.shape
    D = H * hd
    assert D2 == 2 * D and scales.shape == (B, T, 2 * H) and q_rot.shape == (B, D)
    kv = dequant_kv8(q_bytes, scales, hd).reshape(B, T, 2, H, hd)
    return _attend(q_rot.double().reshape(B, H, hd), kv[:, :, 0], kv[:, :, 1], scale)


def rope16(x, cos, sin, pos, hd):
    """RoPE of x [R, n * hd] at table rows pos [R], with the kernels' rounding points (each product and the sum rounded
    to the 16-bit type); cos, sin [positions, hd] in that type"""
    dt = x.dtype
    R = x.shape[0]
    xf = x.float().reshape(R, -1, hd)
    c, s = cos[pos.long()].float()[:, None, :], sin[pos.long()].float()[:, None, :]
    half = hd // 2
    partner = torch.cat((-xf[..., half:], xf[..., :half]), dim=-1)
    a = (xf * c).to(dt).float()
    b = (partner * s).to(dt).float()
    return (a + b).to(dt).reshape(x.shape)


def tables(hd, n, dtype):
    """the model's RoPE tables (LlamaRotaryEmbedding) in the 16-bit type, [n, hd]"""
    inv = 1.0 / (10000.0 ** (torch.arange(0, hd, 2).float() / hd))
    ang = torch.outer(torch.arange(n).float(), inv)
    ang = torch.cat((ang, ang), dim=-1)
    return ang.cos().to(dtype), ang.sin().to(dtype)


# ------------------------------------------------------------------------------------------------------ inputs --
FAMILIES = ("random", "ramp_up", "ramp_down", "v_census", "k_census")
NAN_BYTE = 0x7F                 # the e4m3 NaN code
PAD_ROWS = 3                    # NaN rows behind the largest position


def _nan_bits(dtype):
    return torch.tensor(float("nan"), dtype=dtype).view(torch.int16).item()


def windows(T, hd):
    return -(-T // (4 * hd))


def window_of(r, T, hd):
    """[lo, hi) of head row r (= sample * H + head): windows of 4 * hd keys, assigned round-robin"""
    j = r % windows(T, hd)
    return j * 4 * hd, min((j + 1) * 4 * hd, T)


def census_counts(lo, hi, hd):
    """[hd] float64: keys t of [lo, hi) with t mod hd == d"""
    return torch.bincount(torch.arange(lo, hi) % hd, minlength=hd).double()


def v_census_expect(lo, hi, T, hd):
    return census_counts(lo, hi, hd) / T


def k_census_expect(lo, hi, hd):
    return census_counts(lo, hi, hd) / (hi - lo)


Case = collections.namedtuple(
    "Case", "family dtype hd H B ps Tmax scale qkv cos sin q_rot rows cache cbytes cscales expect")


def make_case(family, dtype, hd, H, ps, seed, kv8=False):
    """One launch's inputs: sample b at position ps[b] (T_b = ps[b] + 1).
      qkv      [B, 3D]  the new q | k | v rows (unrotated), 16-bit
      q_rot    [B, D]   rope16 of q at ps (the GPU tests take ops.rope_'s instead)
      rows     [B, Tmax, 2D] 16-bit: the cache AS IT WILL STAND after the step where row ps[b] holds rope16(k_new) | v_new;
               rows behind ps[b] are zero here
      cache    [B, Tmax, 2D] 16-bit cache BEFORE the step: rows >= ps[b] hold NaN bits              (kv8: None)
      cbytes, cscales  the e4m3 cache before the step: NaN codes and NaN scales at rows >= ps[b]    (16-bit: None)
      expect   [B, D] float64 closed form of the census families, else None
    Census families need B * H >= the number of windows of every sample."""
    assert family in FAMILIES
    g = torch.Generator().manual_seed(seed)
    B, D = len(ps), H * hd
    Tmax = max(ps) + 1 + PAD_ROWS
    scale = 1.0 / math.sqrt(hd)
    cos, sin = tables(hd, Tmax, dtype)
    pos = torch.tensor(ps)
    Tb = pos + 1
    t = torch.arange(Tmax)
    live = (t[None, :] < Tb[:, None])                                  # [B, Tmax]: rows 0 ... p_b
    is_p = (t[None, :] == pos[:, None])

    def blocks(shape):                  # random rows; kv8: a power of two 2^-6 ... 2^6 per (row, key or value, head) block, as
        x = torch.randn(shape, generator=g)          # test_decode_kv8_gpu._random_kv draws them
        if kv8:
            x = x * torch.pow(2.0, torch.randint(-6, 7, (*shape[:-1], 1), generator=g).float())
        return x.to(dtype)

    qmul = 2.0 if family == "k_census" else 1.0
    q = (torch.randn((B, H, hd), generator=g) * qmul).to(dtype)
    q_rot = rope16(q.reshape(B, D), cos, sin, pos, hd).view(B, H, hd)
    n2 = q_rot.double().pow(2).sum(-1)                                 # [B, H]
    k = torch.zeros((B, Tmax, H, hd), dtype=dtype)                     # rotated keys of every row, row p_b included
    v = torch.zeros((B, Tmax, H, hd), dtype=dtype)
    k_new = torch.zeros((B, H, hd), dtype=dtype)                       # unrotated new key
    expect = None
    if family == "random":
        k, v = blocks((B, Tmax, H, hd)), blocks((B, Tmax, H, hd))
        k_new = blocks((B, H, hd))
        k[is_p] = rope16(k_new.reshape(B, D), cos, sin, pos, hd).view(B, H, hd)
    elif family in ("ramp_up", "ramp_down"):
        sgn = 1.0 if family == "ramp_up" else -1.0
        c = sgn * (2.0 * t[None, :].double() / (Tb[:, None] - 1).clamp_min(1).double() - 1.0)        # [B, Tmax]
        coef = 60.0 / (_f32(scale) * n2)                                                              # [B, H]
        k = (c[:, :, None, None] * coef[:, None, :, None] * q_rot.double()[:, None]).to(dtype)
        c_p = c[is_p]                                                                                 # [B]
        k_new = (c_p[:, None, None] * coef[:, :, None] * q.double()).to(dtype)
        k[is_p] = rope16(k_new.reshape(B, D), cos, sin, pos, hd).view(B, H, hd)
        v = torch.randn((B, Tmax, H, hd), generator=g).to(dtype)
    else:
        expect = torch.zeros((B, H, hd), dtype=torch.float64)
        onehot = (t[:, None] % hd == torch.arange(hd)[None, :]).to(dtype)                             # [Tmax, hd]
        kappa = torch.pow(2.0, torch.ceil(torch.log2(32.0 / (_f32(scale) * n2))))                    # [B, H]
        for b in range(B):
            T = int(Tb[b])
            assert B * H >= windows(T, hd), "every key needs a head row that owns it"
            for h in range(H):
                lo, hi = window_of(b * H + h, T, hd)
                if family == "v_census":
                    v[b, lo:hi, h] = onehot[lo:hi]
                    expect[b, h] = v_census_expect(lo, hi, T, hd)
                else:
                    kq = (kappa[b, h] * q_rot[b, h].double())
                    assert bool((kq.to(dtype).double() == kq).all()), "kappa * q_rot is exact"
                    k[b, lo:hi, h] = kq.to(dtype)
                    if lo <= ps[b] < hi:
                        k_new[b, h] = (kappa[b, h] * q[b, h].double()).to(dtype)
                    v[b, :, h] = onehot
                    expect[b, h] = k_census_expect(lo, hi, hd)
        expect = expect.reshape(B, D)
        if kv8:                         # a one-hot value row is stored as code 448 x scale fp32(1 / 448): not exactly 1
            expect = expect * (448.0 * float(torch.tensor(1.0) / 448.0))
    v_new = v[is_p].clone()                                            # [B, H, hd]
    keep = live[:, :, None, None]
    k, v = torch.where(keep, k, torch.zeros((), dtype=dtype)), torch.where(keep, v, torch.zeros((), dtype=dtype))
    rows = torch.cat((k.reshape(B, Tmax, D), v.reshape(B, Tmax, D)), dim=-1)
    qkv = torch.cat((q.reshape(B, D), k_new.reshape(B, D), v_new.reshape(B, D)), dim=-1)
    cached = (live & ~is_p)[:, :, None]                                # rows 0 ... p_b - 1
    cache = cbytes = cscales = None
    if kv8:
        qb, sc = fp8_ref.quant_rows_bytes(rows.reshape(-1, hd))
        qb, sc = qb.reshape(B, Tmax, 2 * D), sc.reshape(B, Tmax, 2 * H)
        cbytes = torch.where(cached, qb, torch.full((), NAN_BYTE, dtype=torch.uint8))
        cscales = torch.where(cached, sc, torch.full((), float("nan")))
    else:
        cache = torch.where(cached, rows.view(torch.int16), torch.full((), _nan_bits(dtype), dtype=torch.int16)).view(dtype)
    return Case(family, dtype, hd, H, B, list(ps), Tmax, scale, qkv, cos, sin, q_rot.reshape(B, D), rows, cache, cbytes,
                cscales, expect)


def case_reference(case, q_rot=None, rows=None, cbytes=None, cscales=None):
    """(o, o_abs) [B, D] of a Case, sample by sample over rows 0 ... ps[b]; by default from the case's own rope16 query
    and the cache it predicts (kv8: the project's row quantiser over the predicted rows), else from what is given"""
    q_rot = case.q_rot if q_rot is None else q_rot
    H, hd = case.H, case.hd
    kv8 = case.cbytes is not None
    if kv8 and cbytes is None:
        cbytes, cscales = fp8_ref.quant_rows_bytes(case.rows.reshape(-1, hd))
        cbytes, cscales = cbytes.reshape(case.B, case.Tmax, -1), cscales.reshape(case.B, case.Tmax, 2 * H)
    rows = case.rows if rows is None else rows
    o, o_abs = [], []
    for b, p in enumerate(case.ps):
        if kv8:
            r = ref_kv8(q_rot[b:b + 1], cbytes[b:b + 1, :p + 1], cscales[b:b + 1, :p + 1], H, hd, case.scale)
        else:
            r = ref16(q_rot[b:b + 1], rows[b:b + 1, :p + 1], H, hd, case.scale)
        o.append(r[0])
        o_abs.append(r[1])
    return torch.cat(o), torch.cat(o_abs)
