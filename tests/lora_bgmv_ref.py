"""fp64 restatement of the mixed-adapter LoRA kernels (csrc/lora_bgmv.hip: mk_lora_bgmv_shrink / mk_lora_bgmv_expand) and of
the stacking of lora.AdapterBank, with the error bounds the GPU tests hold the kernels to.

    shrink   U[m, c] = rnd16( sum_k p(x)[m, k] A[idx[m]][c, k] )                                  c < G r
    expand   Y[m, i N + n] = rnd16( Y[m, i N + n] + s[idx[m]] sum_j U[m, i r + j] B[idx[m]][i N + n, j] )

A [n, G r, K], B [n, G N, r], s [n]; a row with idx[m] outside [0, n) gives a zero row of U and keeps its row of Y.  p is the
token prologue of the stream kernels (0 none, 1 RMSNorm, 2 SwiGLU of [gate | up]) with their rounding points: rows(x, ...)
restates it in fp32 with explicit round trips, SwiGLU through tests/elementwise_ref.py's restatement.

Bounds (fp32 accumulation of n terms in any order: |err| <= n u sum |terms| to first order, u = 2^-24; the factor 2 is
the head room the issue grants for an MFMA's undocumented inner order, kept although these kernels sum with plain FMAs):
    shrink   |U - ref| <= g + ulp16(|ref| + g) / 2,  g = 2 K u sum_k |p_k a_k|
    expand   the same form with g = 2 (r + 2) u (|Y0| + |s| sum_j |U_j B_nj|), on the kernel's own U"""
import torch

from elementwise_ref import silu_mul_f32, ulp

U32 = 2.0 ** -24
BASE = "__base__"
GROUPS = (("qkv", (0, 1, 2)), ("o", (3,)), ("gu", (4, 5)), ("down", (6,)))      # engine.LORA_GROUPS, restated


# ------------------------------------------------------------------------------------------------ prologues --
def rmsnorm_rows(x, w, eps):
    """w * rnd(x * rstd) rounded to x's type, rstd = rsqrt(mean(x^2) + eps) in fp32: rmsnorm_fwd_kernel's rounding points
    (the sum of squares in fp64 here; the kernels' fp32 order is pinned bit for bit on the GPU, not restated)"""
    xf = x.float()
    rstd = torch.rsqrt((x.double() ** 2).mean(1, keepdim=True) + eps).float()
    return (w.float() * (xf * rstd).to(x.dtype).float()).to(x.dtype)


def rows(x, pro, w=None, eps=0.0):
    """the prepared token rows p(x) in x's type"""
    if pro == 0:
        return x
    if pro == 1:
        return rmsnorm_rows(x, w, eps)
    FF = x.shape[1] // 2
    return silu_mul_f32(x[:, :FF], x[:, FF:])


# -------------------------------------------------------------------------------------------------- kernels --
def in_range(idx, n):
    return [0 <= int(i) < n for i in idx]


def shrink64(xp, A, idx):
    """(exact U [M, G r], sum of the products' magnitudes) in fp64 for the prepared rows xp; zero rows outside the bank"""
    M, GR = xp.shape[0], A.shape[1]
    ref, mag = torch.zeros((M, GR), dtype=torch.float64), torch.zeros((M, GR), dtype=torch.float64)
    for m, ok in enumerate(in_range(idx, A.shape[0])):
        if ok:
            a, x = A[int(idx[m])].double(), xp[m].double()
            ref[m], mag[m] = a @ x, a.abs() @ x.abs()
    return ref, mag


def shrink(xp, A, idx, dtype=None):
    """U rounded to dtype (None: left in fp64)"""
    ref, _ = shrink64(xp, A, idx)
    return ref if dtype is None else ref.to(dtype)


def expand64(U, B, s, idx, Y0, G):
    """(exact Y [M, G N] before its rounding, magnitude |Y0| + |s| sum_j |U_j B_nj|, rows touched) in fp64"""
    M = U.shape[0]
    n, GN, r = B.shape
    N = GN // G
    ref, mag = Y0[:, :GN].double().clone(), Y0[:, :GN].double().abs()
    touched = in_range(idx, n)
    for m, ok in enumerate(touched):
        if not ok:
            continue
        a = int(idx[m])
        for i in range(G):
            u, b = U[m, i * r:(i + 1) * r].double(), B[a, i * N:(i + 1) * N].double()
            ref[m, i * N:(i + 1) * N] += float(s[a]) * (b @ u)
            mag[m, i * N:(i + 1) * N] += abs(float(s[a])) * (b.abs() @ u.abs())
    return ref, mag, touched


def expand(U, B, s, idx, Y0, G, dtype=None):
    ref, _, _ = expand64(U, B, s, idx, Y0, G)
    return ref if dtype is None else ref.to(dtype)


def shrink_bound(ref, mag, K, dtype):
    g = 2.0 * K * U32 * mag
    return g + 0.5 * ulp(ref.abs() + g, dtype)


def expand_bound(ref, mag, r, dtype):
    g = 2.0 * (r + 2) * U32 * mag
    return g + 0.5 * ulp(ref.abs() + g, dtype)


# ------------------------------------------------------------------------------------------------- the bank --
def name_indices(names, bank_names):
    return [-1 if n == BASE else bank_names.index(n) for n in names]


def runs(indices):
    """the maximal runs (b0, b1, a) of consecutive samples with the same adapter a >= 0"""
    out, b0 = [], 0
    for b in range(1, len(indices) + 1):
        if b == len(indices) or indices[b] != indices[b0]:
            if indices[b0] >= 0:
                out.append((b0, b, indices[b0]))
            b0 = b
    return tuple(out)


def stack(adapters, layer, members, N, K, dtype):
    """the stacks of one (layer, group): adapters = [(r, lora_alpha, {(layer, module): (A [r, K], B [N, r])})].  Returns
    (A [n, G rmax, K], B [n, G N, rmax], s [n]) or None where no adapter targets a member at this layer"""
    if not any((layer, mi) in ws for _, _, ws in adapters for mi in members):
        return None
    n, G, rmax = len(adapters), len(members), max(r for r, _, _ in adapters)
    A, B = torch.zeros((n, G * rmax, K), dtype=dtype), torch.zeros((n, G * N, rmax), dtype=dtype)
    for a, (r, _, ws) in enumerate(adapters):
        for i, mi in enumerate(members):
            if (layer, mi) in ws:
                A[a, i * rmax:i * rmax + r], B[a, i * N:(i + 1) * N, :r] = ws[(layer, mi)]
    return A, B, torch.tensor([alpha / r for r, alpha, _ in adapters], dtype=torch.float32)
