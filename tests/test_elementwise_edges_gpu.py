"""GPU: every branch of the pointwise, gather and e4m3 quantisation kernels of csrc/elementwise.hip that the one small,
aligned, contiguous shape per kernel of tests/test_kernels_gpu.py does not select -- vector path, scalar fallback, tail
loop and the second trip of the grid-stride loop (a grid is at most 2048 blocks x 256 threads: 524 288 work items) --
against the float64 / bit-exact restatements and the per-element bound of tests/elementwise_ref.py (themselves checked
on the CPU by tests/test_elementwise_ref_cpu.py):
  - mk_rope: the shift-and-mask index path at heads = 32 with both chunk slots of a trip live and a second trip
    (test_rope_large_grids, forward and inverse), the 64-bit division path past one trip, a small power-of-two shape,
    fp32 vector (hd = 8) and scalar (hd = 4) (test_rope_small_shapes); the k slice of a fused q|k|v buffer, the same
    slice behind a misaligned pointer and behind a pitch that is no multiple of the vector
    (test_rope_on_a_slice_of_the_fused_qkv_buffer); random non-monotone positions everywhere; inverse after forward
    (test_rope_inverse_undoes_forward_fp32);
  - mk_swiglu_fwd / mk_swiglu_bwd: n below one vector, one vector, a scalar tail, the grid-stride trip; +-20, +-88,
    +-100 in g, 0, -0 and the largest finite T in u (test_swiglu_1d_sizes_and_planted_values);
  - mk_act_fwd / mk_act_bwd per element over [-12, 12] and past one trip (test_activations_per_element); mk_add with
    period 0 and a broadcast row past one trip (test_add_flat_and_broadcast_row); mk_fill in all three dtypes, inexact
    value, guard element (test_fill_every_dtype_with_guard); mk_cast over all six pairs with ties of both parities,
    fp16 overflow, subnormals, signed zeros, infinities and NaN (test_cast_every_pair_ties_overflow_subnormals);
  - mk_embedding_fwd: second trip of the row loop, scalar path by dim and by pitch, pitched out, negative and
    out-of-range ids (test_embedding_fwd_paths_pitch_and_bad_ids);
  - mk_col2im1d against the autograd of the CPU im2col: channels-first, channels-last, pad > 0, stride 2, odd T
    (test_col2im1d_is_the_transpose_of_im2col); mk_im2col1d, mk_patchify, mk_unpatchify past one trip
    (test_im2col1d_past_one_trip_with_pad_columns, test_patchify_past_one_trip_and_non_square);
  - mk_copy2d: 16-byte vector, scalar 2-byte and 4-byte, batch, broadcast source, second trip
    (test_copy2d_branches);
  - mk_fp8_quantize_rows byte for byte with torch at every instantiation 1, 2, 3, 4, 8 with full and ragged last
    chunks, the two-pass fallback, fp16, pitched input and output (test_fp8_quantize_rows_every_instantiation,
    test_fp8_quantize_rows_pitched_in_and_out); mk_fp8_quantize_cols_t at cols > 256, rows % 64 != 0, rows < 32, pitched
    (test_fp8_quantize_cols_t_shapes); mk_fp8_quantize past 4096 blocks (test_fp8_quantize_per_tensor) and its refusal
    of n % 8 != 0 (test_fp8_quantize_refuses_a_length_that_is_no_multiple_of_8)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_kernels_gpu import DTYPES, H16  # noqa: E402

import elementwise_ref as R  # noqa: E402
import fp8_ref  # noqa: E402
from macaw_llm_amd import ops  # noqa: E402
from macaw_llm_amd.lib import MacawHipError  # noqa: E402

ONE_TRIP = 2048 * 256
IVIEW = {2: torch.int16, 4: torch.int32}


def _same_bits(got, want, what):
    """bit-exact (signed zeros told apart); NaN positions must agree, their payload need not"""
    got = got.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.shape} {got.dtype}"
    gn, wn = torch.isnan(got), torch.isnan(want)
    assert torch.equal(gn, wn), f"{what}: NaN at {(gn != wn).nonzero()[:4].tolist()}"
    iv = IVIEW[got.element_size()]
    bad = ((got.view(iv) != want.view(iv)) & ~wn).nonzero()
    assert bad.numel() == 0, (f"{what}: {bad.shape[0]} of {got.numel()} differ, first at {bad[0].tolist()}: "
                              f"{got[tuple(bad[0])].item()!r} != {want[tuple(bad[0])].item()!r}")


# ------------------------------------------------------------------------------------------- RoPE --
def _check_rope(got, x, cos, sin, pos, heads, hd, inverse, what):
    dtype = x.dtype
    got = got.cpu()
    if dtype == torch.float32:           # |err| <= 2^-22 (|a cos| + |b sin|): R.rope_f64
        ref, mag = R.rope_f64(x, cos, sin, pos, heads, hd, inverse)
        err = (got.double() - ref).abs()
        assert torch.isfinite(got).all() and bool((err <= 2.0 ** -22 * mag).all()), \
            f"{what}: worst err / (|a cos| + |b sin|) = {float((err / mag.clamp_min(1e-300)).max()):.3e} > 2^-22"
    else:                                # products of two 16-bit values are exact in fp32; rounded where the reference rounds
        _same_bits(got, R.rope_ref(x, cos, sin, pos, heads, hd, inverse), what)


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("dtype", H16)
def test_rope_large_grids(dev, dtype, inverse):
    """heads = 32 (shift-and-mask indices), 1 049 344 chunks: both slots live on trip 1, the first slot of 768 threads
    on trip 2; heads = 12 (64-bit divisions), 528 000 chunks: the second slot is live for some threads only"""
    for name in ("pow2_two_trips",) + (() if inverse else ("div_second_slot",)):
        heads, hd, tokens = R.ROPE_SHAPES[name]
        assert tokens * heads * (hd // 16) > ONE_TRIP and ((heads & (heads - 1)) == 0) == name.startswith("pow2")
        x, cos, sin, pos = R.rope_inputs(name, dtype)
        xd = x.to(dev).clone()
        assert xd.data_ptr() % 16 == 0
        ops.rope_(xd, cos.to(dev), sin.to(dev), pos.to(dev), heads, hd, inverse=inverse)
        _check_rope(xd, x, cos, sin, pos, heads, hd, inverse, f"rope {name}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["pow2_small", "f32_vec", "f32_scalar"])
def test_rope_small_shapes(dev, dtype, name):
    """heads = 4: the shift path in one partly filled block; hd = 8 is the fp32 vector path with one chunk per
    head-half (scalar for 16-bit), hd = 4 the scalar kernel for every dtype"""
    heads, hd, _ = R.ROPE_SHAPES[name]
    x, cos, sin, pos = R.rope_inputs(name, dtype)
    for inverse in (False, True):
        xd = x.to(dev).clone()
        ops.rope_(xd, cos.to(dev), sin.to(dev), pos.to(dev), heads, hd, inverse=inverse)
        _check_rope(xd, x, cos, sin, pos, heads, hd, inverse, f"rope {name} inverse={inverse}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", ["aligned", "shifted_pointer", "odd_pitch"])
def test_rope_on_a_slice_of_the_fused_qkv_buffer(dev, dtype, layout):
    """x = the k third of a [tokens, 3 H hd] buffer: pitched vector path; the same slice one element further (the
    pointer fails the host's 16-byte check) and in a buffer of pitch 3 H hd + 1 (ld % N != 0): the scalar kernel.
    q, v and the slack are bit-unchanged."""
    heads, hd, tokens = R.ROPE_SHAPES["qkv_slice"]
    x, cos, sin, pos = R.rope_inputs("qkv_slice", dtype)
    D = heads * hd
    ld = 3 * D + (1 if layout == "odd_pitch" else 0)
    shift = 1 if layout == "shifted_pointer" else 0
    g = torch.Generator().manual_seed(ld + shift)
    flat = torch.randn(tokens * ld + 8, generator=g).to(dtype)
    flat[shift: shift + tokens * ld].view(tokens, ld)[:, D: 2 * D] = x
    fd = flat.to(dev).clone()
    buf = fd[shift: shift + tokens * ld].view(tokens, ld)
    k = buf[:, D: 2 * D]
    assert fd.data_ptr() % 16 == 0 and (k.data_ptr() % 16 == 0) == (shift == 0) and k.stride(0) == ld
    ops.rope_(k, cos.to(dev), sin.to(dev), pos.to(dev), heads, hd)
    _check_rope(k, x, cos, sin, pos, heads, hd, False, f"rope qkv slice {layout}")
    want = flat.clone()
    got = fd.cpu()
    want[shift: shift + tokens * ld].view(tokens, ld)[:, D: 2 * D] = got[shift: shift + tokens * ld].view(tokens, ld)[:, D: 2 * D]
    _same_bits(got, want, f"outside the k slice ({layout})")


@pytest.mark.parametrize("name", ["pow2_small", "f32_vec", "f32_scalar", "qkv_slice"])
def test_rope_inverse_undoes_forward_fp32(dev, name):
    """bound(k = 2) of the input element.  fp32 only: in a 16-bit type the reference itself is outside (the error of a
    rotated pair is a spacing of its larger element; tests/test_elementwise_ref_cpu.py) -- there both directions are
    pinned bit for bit above."""
    heads, hd, _ = R.ROPE_SHAPES[name]
    x, cos, sin, pos = R.rope_inputs(name, torch.float32)
    xd = x.to(dev).clone()
    ops.rope_(xd, cos.to(dev), sin.to(dev), pos.to(dev), heads, hd)
    assert not torch.equal(xd.cpu(), x)
    ops.rope_(xd, cos.to(dev), sin.to(dev), pos.to(dev), heads, hd, inverse=True)
    R.assert_close_elementwise(xd, x.double(), torch.float32, 2, f"rope round trip {name}")


# ---------------------------------------------------------------------- SwiGLU, activations, add --
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("size", range(4))
def test_swiglu_1d_sizes_and_planted_values(dev, dtype, size):
    """n = 3 (no vector chunk: tail loop only), N, N * 1453 + 5 (chunks + tail), 2048 * 256 * N + 2405 (second trip +
    tail).  Forward within k = 3 of rnd_T(silu(g)) * u, dg / du within k = 1 of float64 autograd; all finite except the
    one planted element whose reference overflows T, which must be inf."""
    n = R.pointwise_sizes(dtype)[size]
    g, u, da = R.swiglu_inputs(n, dtype)
    gd, ud, dad = g.to(dev), u.to(dev), da.to(dev)
    a = ops.swiglu_fwd(gd, ud)
    novf = R.assert_close_or_overflow(a, R.silu_mul(g, u), dtype, R.K_SWIGLU_FWD, f"swiglu fwd n={n}")
    dg, du = ops.swiglu_bwd(gd, ud, dad)
    dg64, du64 = R.swiglu_grads(g, u, da)
    novf += R.assert_close_or_overflow(dg, dg64, dtype, R.K_ONCE, f"swiglu dg n={n}")
    R.assert_close_elementwise(du, du64, dtype, R.K_ONCE, f"swiglu du n={n}")
    assert novf == (2 if n >= 32 else 0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("act", [1, 2])
def test_activations_per_element(dev, dtype, act):
    """GELU (erf form) and quick-GELU, forward and backward, each element against its own bound (k = 1): a dense sweep
    of [-12, 12] -- GELU's negative tail is 1e-2 .. 1e-30 and invisible to a bound taken from the largest element --
    and 600 000 random values for the second trip"""
    x, dy = R.act_inputs(dtype)
    assert x.numel() > ONE_TRIP
    fwd, grad = R.ACTS[act]
    R.assert_close_elementwise(ops.act_fwd(x.to(dev), act), fwd(x), dtype, R.K_ONCE, f"act {act} fwd")
    R.assert_close_elementwise(ops.act_bwd(x.to(dev), dy.to(dev), act), dy.double() * grad(x), dtype, R.K_ONCE, f"act {act} bwd")


@pytest.mark.parametrize("dtype", DTYPES)
def test_add_flat_and_broadcast_row(dev, dtype):
    a, b, row = R.add_inputs(dtype)
    assert a.numel() > ONE_TRIP
    R.assert_close_elementwise(ops.add(a.to(dev), b.to(dev)), a.double() + b.double(), dtype, R.K_ONCE, "add period 0")
    got = ops.add(a.to(dev), row.to(dev), period=R.ADD_PERIOD)
    R.assert_close_elementwise(got, a.double() + row.double().repeat(R.ADD_ROWS), dtype, R.K_ONCE, "add broadcast row")
    # a sum of two values of T rounded once is the correctly rounded sum when fp32 holds it exactly: torch agrees bit for bit
    _same_bits(got, (a.float() + row.float().repeat(R.ADD_ROWS)).to(dtype), "add broadcast row against torch")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1, ONE_TRIP + 1])
def test_fill_every_dtype_with_guard(dev, dtype, n):
    buf = torch.full((n + 1,), -7.0, dtype=dtype, device=dev)
    ops.fill_(buf[:n], 0.1)                                    # inexact in every T
    want = torch.full((n + 1,), 0.1, dtype=dtype)
    want[n] = -7.0
    _same_bits(buf, want, "fill")


# ------------------------------------------------------------------------------------------- cast --
def _cast_inputs(src):
    t8, t11 = 2.0 ** -8, 2.0 ** -11
    sp = [0.0, -0.0, float("inf"), float("-inf"), float("nan"), 1.0, -1.0,
          # exact ties between bf16 neighbours: 1 | 1 + 2^-7 (down to even), 1 + 2^-7 | 1 + 2^-6 (up to even)
          1 + t8, 1 + 3 * t8, -(1 + t8), -(1 + 3 * t8), 1 + t8 + 2.0 ** -20, 1 + t8 - 2.0 ** -20,
          # the same between fp16 neighbours (exact in fp32 only), and just off the tie
          1 + t11, 1 + 3 * t11, -(1 + t11), -(1 + 3 * t11), 1 + t11 + 2.0 ** -23, 1 + 3 * t11 - 2.0 ** -23,
          # fp16 overflow: the largest finite, just below the tie to inf, the tie (-> inf), beyond
          65504.0, 65519.99, 65520.0, -65519.99, -65520.0, 65536.0, 1e5, -3e38,
          # fp16 subnormals: smallest, ties 0 | 2^-24 (-> 0) and 2^-24 | 2^-23 (-> 2^-23), just above a tie, largest
          2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -10), -(2.0 ** -25), 2.0 ** -14 - 2.0 ** -24,
          2.0 ** -14, 5 * 2.0 ** -24, 2.0 ** -26,
          # bf16 subnormals (fp32's too): smallest, ties 0 | 2^-133 and 2^-133 | 2^-132, fp32's smallest, bf16's largest
          2.0 ** -133, 2.0 ** -134, 3 * 2.0 ** -134, -(3 * 2.0 ** -134), 2.0 ** -149, 2.0 ** -140, 2.0 ** -126 - 2.0 ** -133,
          2.0 ** -126, 2.0 ** -127,
          # the top of bf16: its largest finite, the tie to inf (-> inf, even), fp32's largest
          3.3895313892515355e38, 3.3961775292304610e38, 3.4028234663852886e38, -3.4028234663852886e38]
    g = torch.Generator().manual_seed(6)
    rnd = torch.randn(600000, generator=g) * torch.exp2(torch.randint(-30, 18, (600000,), generator=g).float())
    return torch.cat((torch.tensor(sp, dtype=torch.float32), rnd)).to(src)


@pytest.mark.parametrize("src,dst", [(s, d) for s in DTYPES for d in DTYPES if s != d])
def test_cast_every_pair_ties_overflow_subnormals(dev, src, dst):
    """from_f32<T> is round-to-nearest-even with overflow to inf and gradual underflow, as tensor.to(T) on the CPU:
    bit-exact over planted ties of both parities, the fp16 overflow edge, fp16 / bf16 / fp32 subnormals, signed zeros
    and infinities (NaN stays NaN), and 600 000 random values over 48 binades (second trip)"""
    x = _cast_inputs(src)
    assert x.numel() > ONE_TRIP
    if src == torch.float32:                                   # the planted values are what they claim
        assert torch.isinf(x[:64].to(torch.float16)).sum() > 4 and x[19:21].to(torch.float16).tolist() == [65504.0, 65504.0]
        h, b = x[:64].to(torch.float16).float(), x[:64].to(torch.bfloat16).float()
        assert float(b[7]) == 1.0 and float(b[8]) == 1 + 2.0 ** -6 and float(h[13]) == 1.0 and float(h[14]) == 1 + 2.0 ** -9
    _same_bits(ops.cast(x.to(dev), dst), x.to(dst), f"cast {src} -> {dst}")


# -------------------------------------------------------------------------------------- embedding --
EMB_CASES = [(torch.bfloat16, 4096, None)] + \
            [(dt, dim, None) for dt in DTYPES for dim in (100, 101)] + \
            [(dt, 128, ld) for dt in DTYPES for ld in (160, 161)]


@pytest.mark.parametrize("dtype,dim,ld", EMB_CASES)
def test_embedding_fwd_paths_pitch_and_bad_ids(dev, dtype, dim, ld):
    """dim = 4096 bf16: 512 vectors per row, a second trip of the 256-thread row loop; dim = 100 / 101: the scalar
    path (100 % 4 == 0 keeps fp32 on vectors, 101 does not); dim = 128 into columns 8 .. 136 of a buffer of pitch 160
    (vector path, 16-byte aligned slice) and of pitch 161 (ld_out % N != 0: scalar).  id -1 leaves its row untouched,
    id >= vocab reads row 0, the slack columns keep the sentinel."""
    g = torch.Generator().manual_seed(dim + (ld or 0))
    V, tokens, off = 107, 41, 8
    table = torch.randn((V, dim), generator=g).to(dtype)
    ids = torch.randint(1, V, (tokens,), generator=g)
    ids[3] = ids[17] = -1
    ids[5] = ids[tokens - 1] = V + 3
    ids[9] = ids[10] = 7
    width = ld or dim
    wide = torch.full((tokens, width), -123.0, dtype=dtype, device=dev)
    out = wide[:, off: off + dim] if ld else wide
    if ld:
        assert out.data_ptr() % 16 == 0 and out.stride(0) == ld
    ret = ops.embedding_fwd(table.to(dev), ids.to(dev), out=out)
    assert ret.data_ptr() == out.data_ptr()
    want = torch.full((tokens, width), -123.0, dtype=dtype)
    rows = table[torch.where(ids >= V, torch.zeros_like(ids), ids).clamp_min(0)]
    rows[ids < 0] = -123.0
    want[:, (off if ld else 0): (off if ld else 0) + dim] = rows
    _same_bits(wide, want, "embedding fwd")
    assert torch.equal(wide.cpu()[5, (off if ld else 0): (off if ld else 0) + dim], table[0])


# ------------------------------------------------------------------- im2col / col2im / patchify --
# (layout, kw, stride, pad, T): Whisper conv1's adjoint (channels-first k3 p1), conv2's (channels-last k3 s2 p1),
# the overlapping projection windows channels-first, and an odd T whose last sample no window of stride 2 centres on
COL2IM_CASES = [("cf", 3, 1, 1, 40), ("cl", 3, 2, 1, 40), ("cf", 6, 5, 0, 40), ("cl", 3, 2, 1, 41), ("cf", 3, 2, 1, 41)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout,kw,stride,pad,T", COL2IM_CASES)
def test_col2im1d_is_the_transpose_of_im2col(dev, dtype, layout, kw, stride, pad, T):
    """random dcols straight into mk_col2im1d (no GEMM in the comparison) against the float64 autograd of the CPU
    im2col (= F.conv1d's input gradient: test_elementwise_ref_cpu.py); sums of at most 3 terms rounded once: k = 1.
    The pad columns of dcols hold NaN: reading one shows."""
    g = torch.Generator().manual_seed(kw * 100 + T + stride)
    B, C = 2, 10
    K, ld = C * kw, ops.pad8(C * kw)
    x0 = torch.zeros((B, C, T), dtype=torch.float64, requires_grad=True)
    cols, Lout = R.im2col1d_cpu(x0, kw, stride, pad)
    dcols = torch.full((B * Lout, ld), float("nan")).to(dtype)
    dcols[:, :K] = torch.randn((B * Lout, K), generator=g).to(dtype)
    (ref,) = torch.autograd.grad(cols, x0, dcols[:, :K].double())
    if layout == "cf":
        dx = ops.col2im1d(dcols.to(dev), B, C, T, kw, stride, pad, Lout, C * T, T, 1, (B, C, T))
    else:
        dx = ops.col2im1d(dcols.to(dev), B, C, T, kw, stride, pad, Lout, T * C, 1, C, (B, T, C)).transpose(1, 2)
    R.assert_close_elementwise(dx.contiguous(), ref, dtype, R.K_ONCE, f"col2im {layout} k{kw} s{stride} p{pad} T{T}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_im2col1d_past_one_trip_with_pad_columns(dev, dtype):
    """Whisper conv1 at full size: B = 2, C = 80, T = 1500, k3 p1 into a pitch of 248: 744 000 output elements.
    Bit-exact against the CPU gather; the 8 pad columns and the two padded window taps are exactly +0."""
    g = torch.Generator().manual_seed(1500)
    B, C, T, kw, ld = 2, 80, 1500, 3, 248
    x = torch.randn((B, C, T), generator=g).to(dtype)
    cols, Lout = ops.im2col1d(x.to(dev), B, C, T, kw, 1, 1, C * T, T, 1, ld_out=ld)
    assert Lout == T and cols.shape == (B * T, ld) and cols.numel() > ONE_TRIP
    want = torch.zeros((B * T, ld), dtype=dtype)
    want[:, : C * kw] = R.im2col1d_cpu(x, kw, 1, 1)[0]
    _same_bits(cols, want, "im2col1d")
    # channels-last, stride 2 (conv2) through the same long grid
    xl = x.transpose(1, 2).contiguous()
    cols, Lout = ops.im2col1d(xl.to(dev), B, C, T, kw, 2, 1, T * C, 1, C, ld_out=ld)
    want = torch.zeros((B * Lout, ld), dtype=dtype)
    want[:, : C * kw] = R.im2col1d_cpu(x, kw, 2, 1)[0]
    _same_bits(cols, want, "im2col1d channels-last s2")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,H,W", [(4, 224, 224), (2, 28, 56)])
def test_patchify_past_one_trip_and_non_square(dev, dtype, B, H, W):
    """4 x 3 x 224 x 224, P = 14: 1024 rows of pitch 592 = 606 208 elements forward, 602 112 back; 28 x 56: gy != gx.
    Bit-exact, pad columns +0, unpatchify(patchify) is the identity."""
    g = torch.Generator().manual_seed(H + W)
    P, K = 14, 3 * 14 * 14
    img = torch.randn((B, 3, H, W), generator=g).to(dtype)
    cols = ops.patchify(img.to(dev), P)
    want = torch.zeros((B * (H // P) * (W // P), ops.pad8(K)), dtype=dtype)
    want[:, :K] = R.patchify_cpu(img, P)
    _same_bits(cols, want, "patchify")
    _same_bits(ops.unpatchify(cols, B, 3, H, W, P), img, "unpatchify")


# ----------------------------------------------------------------------------------------- copy2d --
# name -> (element bytes, rows, cols, ld_src, ld_dst, batch, s_src, s_dst, src_off, dst_off, vector path?)
COPY2D_CASES = {
    "vec2": (2, 5, 64, 72, 80, 1, 0, 0, 8, 16, True),
    "scalar2_src_off_1": (2, 5, 64, 72, 80, 1, 0, 0, 1, 16, False),
    "scalar2_cols_100_odd_pitches": (2, 7, 100, 101, 103, 1, 0, 0, 0, 3, False),
    "vec4": (4, 5, 32, 36, 40, 1, 0, 0, 4, 8, True),
    "scalar4_dst_off_1": (4, 5, 32, 36, 40, 1, 0, 0, 4, 1, False),
    "batch3_vec": (2, 4, 32, 40, 48, 3, 4 * 40 + 8, 4 * 48 + 16, 8, 8, True),
    "batch3_scalar_stride": (2, 4, 32, 40, 48, 3, 4 * 40 + 3, 4 * 48 + 16, 8, 8, False),
    "batch3_broadcast_src": (2, 4, 32, 40, 48, 3, 0, 4 * 48 + 8, 8, 8, True),
    "batch3_broadcast_src_4": (4, 4, 30, 31, 33, 3, 0, 4 * 33 + 1, 2, 5, False),
    "second_trip": (2, 2050, 2048, 2048, 2056, 1, 0, 0, 0, 8, True),
}


@pytest.mark.parametrize("case", list(COPY2D_CASES))
def test_copy2d_branches(dev, case):
    """dst[z][r][:cols] = src[z][r][:cols] against torch strided views, the rest of dst (sentinel) untouched"""
    es, rows, cols, ld_s, ld_d, batch, s_s, s_d, off_s, off_d, vec = COPY2D_CASES[case]
    dtype = torch.bfloat16 if es == 2 else torch.float32
    n_src = off_s + (batch - 1) * s_s + (rows - 1) * ld_s + cols + 5
    n_dst = off_d + (batch - 1) * s_d + (rows - 1) * ld_d + cols + 5
    g = torch.Generator().manual_seed(rows * cols + batch)
    src = torch.randn(n_src, generator=g).to(dtype)
    dst = torch.full((n_dst,), -9.0, dtype=dtype)
    sd, dd = src.to(dev), dst.to(dev)
    al = all(v * es % 16 == 0 for v in (cols, ld_s, ld_d, s_s, s_d, off_s, off_d)) and sd.data_ptr() % 16 == 0 and dd.data_ptr() % 16 == 0
    assert al == vec, "the case selects the branch it names"
    if case == "second_trip":
        assert rows * cols * es // 16 > ONE_TRIP
    ops.copy2d(sd, dd, rows, cols, ld_s, ld_d, batch=batch, s_src=s_s, s_dst=s_d, src_off=off_s, dst_off=off_d)
    torch.as_strided(dst, (batch, rows, cols), (s_d, ld_d, 1), off_d).copy_(
        torch.as_strided(src, (batch, rows, cols), (s_s, ld_s, 1), off_s))
    _same_bits(dd, dst, f"copy2d {case}")


# ----------------------------------------------------------------------------------- e4m3 quantisers --
def _same_bytes(q, s, x_ref, what):
    qr, sr = fp8_ref.quant_rows_bytes(x_ref)
    q, s = q.cpu(), s.cpu()
    bad = (q != qr).nonzero()
    assert bad.numel() == 0, (f"{what}: {bad.shape[0]} of {q.numel()} bytes differ, first at {bad[0].tolist()}: "
                              f"{int(q[tuple(bad[0])]):#04x} != {int(qr[tuple(bad[0])]):#04x}")
    assert torch.equal(s.view(torch.int32), sr.view(torch.int32)), f"{what}: scales {s} != {sr}"


@pytest.mark.parametrize("dtype", H16)
@pytest.mark.parametrize("cols", R.FP8_ROW_COLS)
def test_fp8_quantize_rows_every_instantiation(dev, dtype, cols):
    """chunks of 8 per row: 1 (CH 1, one live thread), 255 (CH 1, ragged), 257 and 512 (CH 2, ragged and full), 640
    (CH 3), 769 and 1024 (CH 4), 1025, 1536 and 2048 (CH 8), 2049 (the two-pass kernel).  Rows span 2^-20 amax .. amax
    (e4m3 zeros by underflow, subnormals, +-448), one is all zero, one has its maximum at the last element."""
    x = R.fp8_rows(R.FP8_ROWS, cols, dtype)
    q, s = ops.quantize_fp8_rows(x.to(dev))
    _same_bytes(q, s, x, f"fp8 rows {cols}")


@pytest.mark.parametrize("dtype", H16)
def test_fp8_quantize_rows_pitched_in_and_out(dev, dtype):
    cols, off, wide = 5120, 8, 5120 + 64
    x = R.fp8_rows(R.FP8_ROWS, cols, dtype, seed=1)
    xw = torch.full((R.FP8_ROWS, wide), 1e4, dtype=dtype)         # larger than every amax: reading the slack shows
    xw[:, off: off + cols] = x
    qw = torch.full((R.FP8_ROWS, wide), 0x55, dtype=torch.uint8, device=dev)
    xs, qs = xw.to(dev)[:, off: off + cols], qw[:, off: off + cols]
    assert xs.data_ptr() % 16 == 0 and qs.data_ptr() % 8 == 0
    q, s = ops.quantize_fp8_rows(xs, out=qs)
    assert q.data_ptr() == qs.data_ptr()
    _same_bytes(q, s, x, "fp8 rows pitched")
    slack = qw.cpu()
    assert bool((slack[:, :off] == 0x55).all()) and bool((slack[:, off + cols:] == 0x55).all())


@pytest.mark.parametrize("rows,cols,wide", [(8, 8, None), (24, 520, None), (328, 520, None), (1000, 264, None), (328, 520, 1024)])
def test_fp8_quantize_cols_t_shapes(dev, rows, cols, wide):
    """8 x 8: one partly filled block of either pass; 24 x 520: rows < 32 skip the four-rows-in-flight loop, cols > 256
    give fp8_colamax_kernel three x-blocks; 328 x 520: rows % 64 = 8; 1000 x 264: sixteen row slabs meet in one
    atomicMax per column; 328 x 520 inside a 328 x 1024 buffer: pitched input.  Column 3 is all zero, column 4 has its
    maximum in the last row."""
    W = R.fp8_rows(cols, rows, torch.bfloat16, seed=2).t().contiguous()
    assert bool((W[:, 3] == 0).all()) and int(W[:, 4].float().abs().argmax()) == rows - 1
    if wide:
        Ww = torch.full((rows, wide), 1e4, dtype=torch.bfloat16)
        Ww[:, 8: 8 + cols] = W
        Wd = Ww.to(dev)[:, 8: 8 + cols]
        assert Wd.stride(0) == wide and Wd.data_ptr() % 16 == 0
    else:
        Wd = W.to(dev)
    qt, s = ops.quantize_fp8_cols_t(Wd)
    assert qt.shape == (cols, rows)
    _same_bytes(qt, s, W.t().contiguous(), f"fp8 cols_t {rows}x{cols}")


@pytest.mark.parametrize("dtype,n", [(torch.bfloat16, 8), (torch.float32, 8), (torch.bfloat16, 8 * 256 * 4096 + 8000),
                                     (torch.float32, 8 * 256 * 4096 + 8000)])
def test_fp8_quantize_per_tensor(dev, dtype, n):
    """n = 8: one chunk; n / 8 = 4096 * 256 + 1000 chunks: the grid-stride loop past the 4096-block cap, with the
    maximum of the tensor in its last 8 elements (both passes must reach the end)"""
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=g) * torch.exp2(-12.0 * torch.rand(n, generator=g))
    x[n - 3] = -17.0
    x = x.to(dtype)
    q, s = ops.quantize_fp8(x.to(dev))
    assert q.shape == (n,) and s.shape == (1,)
    _same_bytes(q.view(1, n), s, x.view(1, n), f"fp8 per tensor {n}")
    assert int(q.cpu()[n - 3]) == 0xFE


def test_fp8_quantize_refuses_a_length_that_is_no_multiple_of_8(dev):
    with pytest.raises(MacawHipError):
        ops.quantize_fp8(torch.zeros(12, dtype=torch.bfloat16, device=dev))
