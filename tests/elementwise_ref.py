"""Plain torch restatements of the pointwise / gather kernels of csrc/elementwise.hip, the per-element error bound they
are held to, and the seeded inputs that tests/test_elementwise_edges_gpu.py feeds the kernels and
tests/test_elementwise_ref_cpu.py feeds the restatements.  References are computed in float64 from the ROUNDED inputs
(the values the kernel reads), so the only differences left are the kernel's fp32 intermediates and its final rounding.

The bound.  A kernel that evaluates its formula in fp32 and rounds to the storage type T ONCE is off by at most half a
spacing of T at the value it computed; that value may sit just above a power of two that the exact value sits just
below, where the spacing doubles -- so by at most ONE spacing of T at the reference: k = 1.  The fp32 evaluation itself
(__expf, the Abramowitz-Stegun mk_erf with absolute error 1.5e-7, a handful of fp32 products) is given the project's own
fp32 tolerance, test_kernels_gpu._tol(torch.float32): a + r |ref|.

SwiGLU forward rounds twice, a = rnd_T(rnd_T(silu(g)) * u), as the eager reference does (silu is its own op there).
rnd_T(silu) of the kernel's fp32 silu may land on a NEIGHBOUR of the value silu_mul() below rounds to when the exact silu
is within fp32 error of a rounding tie: a relative change of one spacing of T in one factor.  One spacing at silu is at
most 2^-p |silu|, so the exact product moves by at most 2^-p |silu u| <= 2 spacings of T at the product (a spacing is
never less than 2^-(p+1) of the value).  The product is then rounded once more: 1 spacing by the argument above.
k = 2 + 1 = 3.
"""
import math

import torch
import torch.nn.functional as F

from test_kernels_gpu import _tol

# (p, emin): explicit mantissa bits and the exponent of the smallest normal number
FORMATS = {torch.bfloat16: (7, -126), torch.float16: (10, -14), torch.float32: (23, -126)}
A32, R32 = _tol(torch.float32)["atol"], _tol(torch.float32)["rtol"]
K_ONCE = 1           # rounded to T once: activations fwd / bwd, SwiGLU bwd, add, col2im sums of <= 8 terms
K_SWIGLU_FWD = 3     # derivation: module docstring


def ulp(ref, dtype):
    """spacing of `dtype` at |ref| (float64): 2^(max(floor(log2 |ref|), emin) - p); the smallest subnormal at 0"""
    p, emin = FORMATS[dtype]
    a = ref.double().abs()
    _, ex = torch.frexp(a)                                   # a = m 2^ex with m in [0.5, 1): floor(log2 a) = ex - 1
    e = torch.where(a == 0, torch.full_like(ex, emin), (ex - 1).clamp_min(emin))
    return torch.ldexp(torch.ones_like(a), e - p)


def bound(ref, dtype, k):
    ref = ref.double()
    return k * ulp(ref, dtype) + A32 + R32 * ref.abs()


def assert_close_elementwise(got, ref64, dtype, k, what):
    """every element of got finite and within bound(ref64, dtype, k) of ref64; the message names the worst index"""
    got = got.detach().cpu().double().reshape(-1)
    ref = ref64.detach().double().reshape(-1)
    assert got.shape == ref.shape, f"{what}: {tuple(got.shape)} elements against {tuple(ref.shape)}"
    assert torch.isfinite(ref).all(), f"{what}: the reference itself is not finite"
    bad = (~torch.isfinite(got)).nonzero()
    assert bad.numel() == 0, f"{what}: {bad.numel()} non-finite outputs, first at {int(bad[0])} (ref {float(ref[bad[0]]):.6g})"
    err, lim = (got - ref).abs(), bound(ref, dtype, k)
    i = int((err / lim).argmax())
    assert bool((err <= lim).all()), (f"{what}: {int((err > lim).sum())} of {err.numel()} outside k = {k}; worst at {i}: "
                                      f"got {float(got[i]):.9g}, ref {float(ref[i]):.9g}, err {float(err[i]):.3e} > "
                                      f"{float(lim[i]):.3e}")


def overflows(ref64, dtype):
    """where the float64 reference rounds to +-inf in `dtype`.  The planted inputs keep every reference value either
    below half the largest finite number or above twice it (asserted), so the verdict never hangs on a rounding."""
    big = torch.finfo(dtype).max
    a = ref64.double().abs()
    assert not bool(((a > 0.5 * big) & (a < 2.0 * big)).any()), "an input puts a reference value at the overflow edge"
    return a > big


def assert_close_or_overflow(got, ref64, dtype, k, what):
    """assert_close_elementwise on every element whose reference is finite in `dtype`; the others must be the
    infinity of the reference's sign.  Returns how many those were."""
    got, ref = got.detach().cpu().reshape(-1), ref64.detach().double().reshape(-1)
    ovf = overflows(ref, dtype)
    want = torch.where(ref[ovf] > 0, float("inf"), float("-inf")).to(torch.float64)
    assert torch.equal(got[ovf].double(), want), f"{what}: {got[ovf]} where the reference overflows to {want}"
    assert_close_elementwise(got[~ovf], ref[~ovf], dtype, k, what)
    return int(ovf.sum())


# ------------------------------------------------------------------------------------- formulas --
def _r(t, dtype):
    return t.to(dtype).double()


def silu_mul(g, u):
    """float64 rnd_T(silu(g)) * u: silu is rounded to the storage type before the product, as in the kernel and in
    the eager reference (F.silu(g) * u in T)"""
    g64, u64 = g.double(), u.double()
    return _r(g64 * torch.sigmoid(g64), g.dtype) * u64


def swiglu_grads(g, u, da):
    """(dg, du) of silu(g) * u by float64 autograd"""
    g64, u64 = g.double().requires_grad_(True), u.double().requires_grad_(True)
    (F.silu(g64) * u64).backward(da.double())
    return g64.grad, u64.grad


def gelu(x):
    x = x.double()
    return 0.5 * x * torch.special.erfc(-x / math.sqrt(2.0))          # erfc: no cancellation in the negative tail


def gelu_grad(x):
    x = x.double()
    return 0.5 * torch.special.erfc(-x / math.sqrt(2.0)) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def quick_gelu(x):
    x = x.double()
    return x * torch.sigmoid(1.702 * x)


def quick_gelu_grad(x):
    x = x.double()
    s = torch.sigmoid(1.702 * x)
    return s * (1.0 + 1.702 * x * (1.0 - s))


ACTS = {1: (gelu, gelu_grad), 2: (quick_gelu, quick_gelu_grad)}     # mk_act_* codes


# the same formulas the way a correct fp32 kernel evaluates them (torch.exp / torch.erf in fp32), for the CPU test
def silu_mul_f32(g, u):
    gf = g.float()
    return ((gf / (1.0 + torch.exp(-gf))).to(g.dtype).float() * u.float()).to(g.dtype)


def swiglu_grads_f32(g, u, da):
    gf, uf, df = g.float(), u.float(), da.float()
    s = 1.0 / (1.0 + torch.exp(-gf))
    return (df * uf * s * (1.0 + gf * (1.0 - s))).to(g.dtype), (df * gf * s).to(g.dtype)


def act_f32(x, act):
    v = x.float()
    y = 0.5 * v * (1.0 + torch.erf(v * 0.70710678118654752440)) if act == 1 else v / (1.0 + torch.exp(-1.702 * v))
    return y.to(x.dtype)


def act_grad_f32(x, dy, act):
    v = x.float()
    if act == 1:
        gr = 0.5 * (1.0 + torch.erf(v * 0.70710678118654752440)) + v * 0.3989422804014327 * torch.exp(-0.5 * v * v)
    else:
        s = 1.0 / (1.0 + torch.exp(-1.702 * v))
        gr = s * (1.0 + 1.702 * v * (1.0 - s))
    return (dy.float() * gr).to(x.dtype)


# ----------------------------------------------------------------------------------------- RoPE --
def rope_ref(x, cos, sin, pos, heads, hd, inverse=False):
    """half-split rotation of x [tokens, heads * hd] (type T) with the kernel's rounding points: each product rounded
    to T, then the sum rounded to T; fp32 arithmetic with explicit .to(T) round trips.  cos / sin [P, hd] in T, pos
    int [tokens]; inverse negates sin."""
    T = x.dtype
    tokens, half = x.shape[0], hd // 2
    xv = x.reshape(tokens, heads, hd)
    a, b = xv[..., :half].float(), xv[..., half:].float()
    c = cos[pos.long()][:, None, :half].float()
    s = sin[pos.long()][:, None, :half].float()
    if inverse:
        s = -s

    def r(t):
        return t.to(T).float()

    o1 = r(r(a * c) + r(-b * s))
    o2 = r(r(b * c) + r(a * s))
    return torch.cat((o1, o2), dim=-1).to(T).reshape(tokens, heads * hd)


def rope_f64(x, cos, sin, pos, heads, hd, inverse=False):
    """(exact rotation, sum of the magnitudes of the two products) in float64, for the fp32 bound
    |err| <= 2^-22 (|a cos| + |b sin|): two products and one sum, each within 2^-24 relative, FMA contraction or not"""
    tokens, half = x.shape[0], hd // 2
    xv = x.double().reshape(tokens, heads, hd)
    a, b = xv[..., :half], xv[..., half:]
    c = cos[pos.long()][:, None, :half].double()
    s = sin[pos.long()][:, None, :half].double() * (-1.0 if inverse else 1.0)
    out = torch.cat((a * c - b * s, b * c + a * s), dim=-1).reshape(tokens, heads * hd)
    mag = torch.cat(((a * c).abs() + (b * s).abs(), (b * c).abs() + (a * s).abs()), dim=-1).reshape(tokens, heads * hd)
    return out, mag


ROPE_POSITIONS = 600
# name -> (heads, hd, tokens).  Chunks of 16 bytes per head-half cph = hd / 2 / N (N = 8 for 16-bit, 4 for fp32); a
# grid is at most 2048 blocks x 256 threads, and a thread handles chunks idx and idx + 524288 per trip.
ROPE_SHAPES = {
    # 4099 * 32 * 8 = 1 049 344 chunks: trip 1 has both slots live, trip 2 the first slot for 768 threads only
    "pow2_two_trips": (32, 128, 4099),
    # heads not a power of two: the 64-bit division path; 11000 * 12 * 4 = 528 000 chunks > 524 288
    "div_second_slot": (12, 64, 11000),
    "pow2_small": (4, 32, 7),
    "qkv_slice": (4, 128, 37),
    "f32_vec": (4, 8, 7),         # fp32: half = 4 = N, cph = 1
    "f32_scalar": (4, 4, 7),      # half = 2 < N: scalar kernel
}


def rope_inputs(name, dtype):
    """(x [tokens, heads * hd], cos, sin [P, hd], pos int32 [tokens]: random, not monotone) for ROPE_SHAPES[name]"""
    from oracle import restate
    heads, hd, tokens = ROPE_SHAPES[name]
    g = torch.Generator().manual_seed(1000 * heads + hd + tokens)
    cos, sin = restate.rotary_tables(hd, ROPE_POSITIONS)
    x = torch.randn((tokens, heads * hd), generator=g).to(dtype)
    pos = torch.randint(0, ROPE_POSITIONS, (tokens,), generator=g).to(torch.int32)
    return x, cos.to(dtype), sin.to(dtype), pos


# ------------------------------------------------------------------------------ pointwise inputs --
def vec_n(dtype):
    return 4 if dtype == torch.float32 else 8


def pointwise_sizes(dtype):
    """fewer elements than one 16-byte chunk; exactly one chunk; chunks plus a scalar tail of 5 (1 for fp32: 5 % 4);
    more than 2048 x 256 chunks (the grid-stride trip) plus a tail"""
    N = vec_n(dtype)
    return [3, N, N * 1453 + 5, 2048 * 256 * N + 2405]


def swiglu_inputs(n, dtype):
    """g, u = randn * 3, da = randn, with the values where silu / exp misbehave planted in g (+-20, +-88, +-100), zeros
    of both signs and the largest finite T in u.  Where u is the largest finite number, g and da are chosen so that
    the output and the fp32 product da * u the backward kernel forms first are either well inside the range (|.| <=
    0.5 max) or overflow together with the reference (20 max, 3 max): the tests assert inf there."""
    g_ = torch.Generator().manual_seed(n)
    g, u, da = torch.randn(n, generator=g_) * 3, torch.randn(n, generator=g_) * 3, torch.randn(n, generator=g_)
    big = torch.finfo(dtype).max
    if n >= 32:
        g[0:6] = torch.tensor([20.0, -20.0, 88.0, -88.0, 100.0, -100.0])
        u[6], u[7] = 0.0, -0.0
        g[8], u[8], da[8] = 0.5, big, 0.5
        g[9], u[9], da[9] = -0.5, -big, -0.5
        g[10], u[10], da[10] = 20.0, big, 3.0                 # overflows in the reference too
        g[n - 1], g[n - 2], g[n - 3] = -20.0, 88.0, -100.0    # the scalar tail loop sees them too
        u[n - 4] = -0.0
    else:
        g[0], g[1] = 20.0, -88.0
        g[2], u[2], da[2] = 0.5, big, 0.5
    return g.to(dtype), u.to(dtype), da.to(dtype)


def act_inputs(dtype):
    """a dense sweep of [-12, 12] (GELU's negative tail, both saturations) and 600 000 random values: 648 001 elements,
    more than one trip of the 2048 x 256 grid"""
    g_ = torch.Generator().manual_seed(12)
    x = torch.cat((torch.linspace(-12.0, 12.0, 48001), torch.randn(600000, generator=g_) * 3))
    return x.to(dtype), torch.randn(x.numel(), generator=g_).to(dtype)


ADD_ROWS, ADD_PERIOD = 1500, 352      # 528 000 > 524 288 elements


def add_inputs(dtype):
    g_ = torch.Generator().manual_seed(352)
    n = ADD_ROWS * ADD_PERIOD
    return (torch.randn(n, generator=g_) * 3).to(dtype), (torch.randn(n, generator=g_) * 3).to(dtype), \
        (torch.randn(ADD_PERIOD, generator=g_) * 3).to(dtype)


# ---------------------------------------------------------------------------------- conv columns --
def im2col1d_cpu(x_bct, kw, stride, pad):
    """x [B, C, T] -> [B * Lout, C * kw], column c * kw + t = x[b, c, j * stride + t - pad] (0 outside): F.unfold's
    order for a 1-D convolution.  Differentiable: its autograd is col2im."""
    B, C, T = x_bct.shape
    Lout = (T + 2 * pad - kw) // stride + 1
    xp = F.pad(x_bct, (pad, pad))
    idx = torch.arange(Lout)[:, None] * stride + torch.arange(kw)[None, :]
    return xp[:, :, idx].permute(0, 2, 1, 3).reshape(B * Lout, C * kw), Lout


def patchify_cpu(img, P):
    B, C, H, W = img.shape
    return img.reshape(B, C, H // P, P, W // P, P).permute(0, 2, 4, 1, 3, 5).reshape(B * (H // P) * (W // P), C * P * P)


# ------------------------------------------------------------------------------------ e4m3 rows --
# cols -> chunks of 8 per thread (fp8_rowquant_reg_kernel<CH>) / ragged last chunk row / the two-pass kernel
FP8_ROW_COLS = [8, 2040, 2056, 4096, 5120, 6152, 8192, 8200, 12288, 16384, 16392]
FP8_ROWS = 5


def fp8_rows(rows, cols, dtype, seed=0):
    """[rows, cols]: row r spans amax_r 2^-20 .. amax_r in magnitude with random signs (quantised with 448 / amax_r that
    is e4m3 zero by underflow, e4m3 subnormals, and +-448).  Row 3 is all zero; the only maximum of row 4 is its last
    element.  Planted so that even 8 columns hold every class: x[0, 0] = amax 2^-20 (-> 0), x[0, 1] = amax 2^-15
    (-> subnormal), x[0, 2] = -amax (-> -448), x[1, 0] = +amax (-> +448)."""
    assert rows >= 5 and cols >= 4
    g_ = torch.Generator().manual_seed(cols * 31 + rows + seed)
    amax = torch.tensor([4.0, 0.37, 96.0, 0.0, 1.5] + [2.0] * (rows - 5))[:, None]
    x = amax * torch.exp2(-20.0 * torch.rand((rows, cols), generator=g_))
    x = x * (torch.randint(0, 2, (rows, cols), generator=g_) * 2 - 1)
    x[0, 0], x[0, 1], x[0, 2] = 4.0 * 2.0 ** -20, 4.0 * 2.0 ** -15, -4.0
    x[1, 0] = 0.37
    x[4, cols - 1] = 3.0
    return x.to(dtype)
