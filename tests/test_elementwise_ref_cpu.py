"""The references, bounds and inputs that tests/test_elementwise_edges_gpu.py holds csrc/elementwise.hip to
(tests/elementwise_ref.py) are themselves checked here, on the CPU:
  - ulp() is torch.nextafter's spacing over subnormals, powers of two and their neighbours in every dtype;
  - rope_ref is oracle.restate.apply_rope bit for bit in bf16 AND fp16 at the GPU file's shapes, forward and inverse (the
    CPU half of the claim that a kernel which multiplies in fp32 and rounds where the reference does is bit-exact);
  - every pointwise formula evaluated in fp32 (torch.exp / torch.erf) and rounded to T stays inside bound() with the k
    the GPU file uses, on the very inputs it uses: a correct fp32 kernel passes, and a later choice of inputs for which
    that is not so fails here first;
  - im2col1d_cpu (whose autograd is the col2im reference) reproduces F.conv1d, patchify_cpu reproduces F.conv2d;
  - the e4m3 rows really hold subnormals, zeros by underflow and +-448, an all-zero row and a row led by its last
    element.
The inverse-after-forward round trip of RoPE is held to bound(k = 2) in fp32 only: in a 16-bit type the error of a
rotated pair is a spacing of the LARGER of the two elements (and the rounded table has cos^2 + sin^2 = 1 +- 2^-8), which
no per-element multiple of ulp(input) covers -- rope_ref itself misses it, as
test_rope_round_trip_bound_holds_in_fp32_only records.  The 16-bit round trip is pinned by bit-exactness in both
directions instead."""
import pytest
import torch
import torch.nn.functional as F

import elementwise_ref as R
import fp8_ref
from oracle import restate

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
H16 = [torch.bfloat16, torch.float16]


@pytest.mark.parametrize("dtype", DTYPES)
def test_ulp_is_the_nextafter_spacing(dtype):
    p, emin = R.FORMATS[dtype]
    fi = torch.finfo(dtype)
    tiny = 2.0 ** (emin - p)                                   # the smallest subnormal
    vals = [0.0, tiny, 3 * tiny, 2.0 ** emin - tiny, 2.0 ** emin, 2.0 ** emin + tiny, fi.max / 2]
    for e in (emin + 1, -9, -1, 0, 1, 7, 14):                 # a power of two, its lower and upper neighbour, 1.5 x
        vals += [2.0 ** e, 2.0 ** e * (1 - 2.0 ** (-p - 1)), 2.0 ** e * (1 + 2.0 ** -p), 2.0 ** e * 1.5]
    g = torch.Generator().manual_seed(0)
    sweep = torch.cat((torch.tensor(vals, dtype=torch.float64),
                       torch.randn(2000, generator=g, dtype=torch.float64) * torch.exp2(torch.randint(-30, 15, (2000,), generator=g))))
    v = sweep.to(dtype).abs()
    assert torch.equal(v[: len(vals)].double(), torch.tensor(vals, dtype=torch.float64)), "the sweep is exact in the dtype"
    up = torch.nextafter(v, torch.full_like(v, float("inf")))
    assert torch.isfinite(up).all()
    assert torch.equal(R.ulp(v, dtype), up.double() - v.double())
    assert torch.equal(R.ulp(-v, dtype), R.ulp(v, dtype))
    assert float(R.ulp(torch.zeros(1), dtype)) == tiny


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("dtype", H16)
@pytest.mark.parametrize("name", ["pow2_two_trips", "div_second_slot", "pow2_small", "qkv_slice"])
def test_rope_ref_is_the_oracle_bit_for_bit(name, dtype, inverse):
    heads, hd, tokens = R.ROPE_SHAPES[name]
    x, cos, sin, pos = R.rope_inputs(name, dtype)
    assert (pos[1:] < pos[:-1]).any() and (pos[1:] > pos[:-1]).any(), "positions are not monotone"
    q = x.view(1, tokens, heads, hd).transpose(1, 2)
    want, _ = restate.apply_rope(q, q, cos, -sin if inverse else sin, pos.long()[None])
    got = R.rope_ref(x, cos, sin, pos, heads, hd, inverse)
    assert got.dtype == dtype
    assert torch.equal(got.view(tokens, heads, hd), want[0].transpose(0, 1))


@pytest.mark.parametrize("dtype", DTYPES)
def test_rope_ref_meets_the_fp32_bound_and_the_exact_rotation(dtype):
    for name in ("pow2_small", "f32_vec", "f32_scalar"):
        heads, hd, _ = R.ROPE_SHAPES[name]
        x, cos, sin, pos = R.rope_inputs(name, dtype)
        for inverse in (False, True):
            ref, mag = R.rope_f64(x, cos, sin, pos, heads, hd, inverse)
            err = (R.rope_ref(x, cos, sin, pos, heads, hd, inverse).double() - ref).abs()
            if dtype == torch.float32:
                assert bool((err <= 2.0 ** -22 * mag).all()), float((err / mag).max())
            else:                                             # three roundings to T of values no larger than mag
                assert bool((err <= 3 * R.ulp(mag, dtype)).all())


def test_rope_round_trip_bound_holds_in_fp32_only():
    k = 2
    for name in ("pow2_small", "f32_vec", "f32_scalar", "qkv_slice"):
        heads, hd, _ = R.ROPE_SHAPES[name]
        x, cos, sin, pos = R.rope_inputs(name, torch.float32)
        back = R.rope_ref(R.rope_ref(x, cos, sin, pos, heads, hd), cos, sin, pos, heads, hd, inverse=True)
        R.assert_close_elementwise(back, x.double(), torch.float32, k, f"fp32 round trip {name}")
    # the reason the GPU file does not ask it of the 16-bit types: the reference itself is outside
    heads, hd, _ = R.ROPE_SHAPES["qkv_slice"]
    for dtype in H16:
        x, cos, sin, pos = R.rope_inputs("qkv_slice", dtype)
        back = R.rope_ref(R.rope_ref(x, cos, sin, pos, heads, hd), cos, sin, pos, heads, hd, inverse=True)
        err = (back.double() - x.double()).abs()
        assert bool((err > R.bound(x, dtype, k)).any())


@pytest.mark.parametrize("dtype", DTYPES)
def test_f32_swiglu_stays_inside_the_bounds(dtype):
    for n in R.pointwise_sizes(dtype):
        g, u, da = R.swiglu_inputs(n, dtype)
        assert g.numel() == n and g.dtype == dtype
        novf = R.assert_close_or_overflow(R.silu_mul_f32(g, u), R.silu_mul(g, u), dtype, R.K_SWIGLU_FWD, f"swiglu fwd {n}")
        dg64, du64 = R.swiglu_grads(g, u, da)
        dg, du = R.swiglu_grads_f32(g, u, da)
        novf += R.assert_close_or_overflow(dg, dg64, dtype, R.K_ONCE, f"swiglu dg {n}")
        R.assert_close_elementwise(du, du64, dtype, R.K_ONCE, f"swiglu du {n}")
        if n >= 32:                                            # the inputs do what they claim
            assert novf == 2
            assert {20.0, -20.0, 88.0, -88.0, 100.0, -100.0} <= set(g[:6].tolist()) | set(g[-3:].tolist())
            assert float(u[8]) == torch.finfo(dtype).max and float(u[9]) == -torch.finfo(dtype).max
            assert float(u[6]) == 0 and not torch.signbit(u[6]) and float(u[7]) == 0 and torch.signbit(u[7])
            assert n % R.vec_n(dtype) != 0


@pytest.mark.parametrize("act", [1, 2])
@pytest.mark.parametrize("dtype", DTYPES)
def test_f32_activations_stay_inside_the_bound(dtype, act):
    x, dy = R.act_inputs(dtype)
    assert x.numel() > 2048 * 256 and float(x.min()) <= -12 and float(x.max()) >= 12
    fwd, grad = R.ACTS[act]
    R.assert_close_elementwise(R.act_f32(x, act), fwd(x), dtype, R.K_ONCE, f"act {act} fwd")
    R.assert_close_elementwise(R.act_grad_f32(x, dy, act), dy.double() * grad(x), dtype, R.K_ONCE, f"act {act} bwd")
    # GELU's negative tail is inside the bound's reach: on (-3, -2), where gelu is -0.004 .. -0.045, the bound is a few
    # per cent of the value (one limit for the whole tensor, 8e-3 (1 + max |y|), is larger than the whole tail)
    if act == 1:
        tail = (x.double() > -3) & (x.double() < -2)
        assert bool((R.bound(fwd(x)[tail], dtype, R.K_ONCE) < 0.05 * fwd(x)[tail].abs()).all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_f32_add_stays_inside_the_bound(dtype):
    a, b, row = R.add_inputs(dtype)
    assert a.numel() > 2048 * 256
    R.assert_close_elementwise((a.float() + b.float()).to(dtype), a.double() + b.double(), dtype, R.K_ONCE, "add")
    bc = row.repeat(R.ADD_ROWS)
    R.assert_close_elementwise((a.float() + bc.float()).to(dtype), a.double() + bc.double(), dtype, R.K_ONCE, "add row")


@pytest.mark.parametrize("kw,stride,pad,T", [(3, 1, 1, 40), (3, 2, 1, 40), (6, 5, 0, 40), (3, 2, 1, 41)])
def test_im2col_cpu_is_conv1d_and_its_autograd_is_col2im(kw, stride, pad, T):
    g = torch.Generator().manual_seed(kw + T)
    B, C, O = 2, 10, 6
    x = torch.randn((B, C, T), generator=g, dtype=torch.float64, requires_grad=True)
    W = torch.randn((O, C, kw), generator=g, dtype=torch.float64)
    cols, Lout = R.im2col1d_cpu(x, kw, stride, pad)
    ref = F.conv1d(x, W, stride=stride, padding=pad)
    assert ref.shape[2] == Lout
    assert torch.allclose(cols @ W.reshape(O, -1).t(), ref.transpose(1, 2).reshape(B * Lout, O), rtol=1e-12, atol=1e-12)
    dy = torch.randn((B, O, Lout), generator=g, dtype=torch.float64)
    (dx_conv,) = torch.autograd.grad(ref, x, dy, retain_graph=True)
    (dx_cols,) = torch.autograd.grad(cols, x, dy.transpose(1, 2).reshape(B * Lout, O) @ W.reshape(O, -1))
    assert torch.allclose(dx_cols, dx_conv, rtol=1e-12, atol=1e-12)


def test_patchify_cpu_is_conv2d():
    g = torch.Generator().manual_seed(14)
    img = torch.randn((2, 3, 28, 56), generator=g, dtype=torch.float64)
    W = torch.randn((5, 3, 14, 14), generator=g, dtype=torch.float64)
    ref = F.conv2d(img, W, stride=14).flatten(2).transpose(1, 2).reshape(-1, 5)
    assert torch.allclose(R.patchify_cpu(img, 14) @ W.reshape(5, -1).t(), ref, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("dtype", H16)
@pytest.mark.parametrize("cols", R.FP8_ROW_COLS)
def test_fp8_rows_hold_subnormals_underflow_and_saturation(cols, dtype):
    x = R.fp8_rows(R.FP8_ROWS, cols, dtype)
    q, s = fp8_ref.quant_rows_bytes(x)
    mag = q & 0x7F
    live = x.float() != 0
    assert bool(((mag == 0) & live).any()), "no non-zero input underflows to an e4m3 zero"
    assert bool(((mag > 0) & (mag < 8)).any()), "no e4m3 subnormal"
    assert bool((q == 0x7E).any()) and bool((q == 0xFE).any()), "+448 and -448"
    assert not bool((mag == 0x7F).any()), "no NaN code"
    assert bool((x[3] == 0).all()) and float(s[3]) == 1.0
    assert int(x[4].float().abs().argmax()) == cols - 1 and int((x[4].float().abs() == x[4].float().abs().max()).sum()) == 1
    assert int(mag[4, cols - 1]) == 0x7E
    if cols >= 2040:                                           # the span: every binade from amax 2^-20 up is there
        r = x[0].float().abs()
        assert float(r[r > 0].min()) < 4.0 * 2.0 ** -19 and float(r.max()) == 4.0
