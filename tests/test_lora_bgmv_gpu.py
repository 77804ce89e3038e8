"""GPU: mk_lora_bgmv_shrink / mk_lora_bgmv_expand (csrc/lora_bgmv.hip) against the fp64 restatement of
tests/lora_bgmv_ref.py, inside the bounds that follow from fp32 accumulation, and bit for bit where the contract says so:
a second launch, row m of a batch against M = 1 on that row, a prologue on x against prologue 0 on the prepared rows,
rows outside the bank, pad columns, a zero B."""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

import lora_bgmv_ref as R  # noqa: E402

from macaw_llm_amd import lib as L  # noqa: E402
from macaw_llm_amd import ops  # noqa: E402

EPS = 1e-5
N_AD = 3
MS = (1, 5, 16, 17, 32)
SHAPES = ((128, 128, 3), (128, 352, 2), (352, 128, 1), (1000, 1032, 3))
RANKS = (8, 24, 64, 128)
DTYPES = (torch.bfloat16, torch.float16)
IDX_KINDS = ("mixed", "equal", "base", "outside")


def _idx(kind, M):
    if kind == "mixed":
        return [(3 * m + 1) % N_AD for m in range(M)]
    if kind == "equal":
        return [1] * M
    if kind == "base":
        return [-1] * M
    return [(N_AD, -7, 0, 2, -1, 1)[m % 6] for m in range(M)]      # the first index past the bank, a negative one


def _bits(t):
    return t.contiguous().view(torch.int16)


def _inputs(dtype, M, K, N, G, r, pro, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((M, 2 * K if pro == 2 else K), generator=g).to(dtype)
    w = (1 + 0.1 * torch.randn(K, generator=g)).to(dtype)
    A = (torch.randn((N_AD, G * r, K), generator=g) * 0.5).to(dtype)
    B = (torch.randn((N_AD, G * N, r), generator=g) * 0.1).to(dtype)
    s = torch.tensor([2.0, 0.5, 1.25])
    Y0 = torch.randn((M, G * N), generator=g).to(dtype)
    return x, w, A, B, s, Y0


def _pitched(M, cols, pad, dtype, dev, fill=None):
    """an [M, cols] view of an [M, cols + pad] buffer whose pad columns hold a sentinel"""
    buf = torch.full((M, cols + pad), -1234.0, dtype=dtype, device=dev)
    if fill is not None:
        buf[:, :cols] = fill
    return buf, buf[:, :cols]


def _check(dev, dtype, M, K, N, G, r, pro, kind, seed=0):
    x, w, A, B, s, Y0 = (t.to(dev) for t in _inputs(dtype, M, K, N, G, r, pro, seed))
    idx_l = _idx(kind, M)
    idx = torch.tensor(idx_l, dtype=torch.int32, device=dev)
    inside = R.in_range(idx_l, N_AD)
    assert ops.lora_bgmv_ok(x, A, pro)
    # ---- shrink, into a pitched U with poisoned pad columns
    Ubuf, U = _pitched(M, G * r, 8, dtype, dev)
    ops.lora_bgmv_shrink(x, A, idx, G, pro, w if pro == 1 else None, EPS, out=U)
    xp = x if pro == 0 else (ops.rmsnorm_fwd(x, w, EPS)[1] if pro == 1 else ops.swiglu2d_fwd(x, K))
    ref, mag = R.shrink64(xp.cpu(), A.cpu(), idx_l)
    err, bound = (U.cpu().double() - ref).abs(), R.shrink_bound(ref, mag, K, dtype)
    assert bool((err <= bound).all()), f"shrink: worst error / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}"
    assert bool((Ubuf[:, G * r:] == -1234.0).all())
    for m, ok in enumerate(inside):
        if not ok:
            assert bool((_bits(U[m]) == 0).all()), m
    # a second launch, a prologue against the prepared rows, a row alone
    U2buf, U2 = _pitched(M, G * r, 8, dtype, dev)
    ops.lora_bgmv_shrink(x, A, idx, G, pro, w if pro == 1 else None, EPS, out=U2)
    assert torch.equal(_bits(Ubuf), _bits(U2buf))
    if pro:
        assert torch.equal(_bits(ops.lora_bgmv_shrink(xp, A, idx, G)), _bits(U))
    for m in range(M):
        one = ops.lora_bgmv_shrink(x[m:m + 1], A, idx[m:m + 1], G, pro, w if pro == 1 else None, EPS)
        assert torch.equal(_bits(one[0]), _bits(U[m])), m
    # ---- expand, on the kernel's own U, into a pitched Y with poisoned pad columns
    Ybuf, Y = _pitched(M, G * N, 16, dtype, dev, Y0)
    ops.lora_bgmv_expand_(U, B, s.to(dev), idx, Y, G)
    ref, mag, _ = R.expand64(U.cpu(), B.cpu(), s, idx_l, Y0.cpu(), G)
    err, bound = (Y.cpu().double() - ref).abs(), R.expand_bound(ref, mag, r, dtype)
    assert bool((err <= bound).all()), f"expand: worst error / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}"
    assert bool((Ybuf[:, G * N:] == -1234.0).all())
    for m, ok in enumerate(inside):
        if not ok:
            assert torch.equal(_bits(Y[m]), _bits(Y0[m])), m
        else:
            assert not torch.equal(_bits(Y[m]), _bits(Y0[m])), m
    Y2buf, Y2 = _pitched(M, G * N, 16, dtype, dev, Y0)
    ops.lora_bgmv_expand_(U, B, s.to(dev), idx, Y2, G)
    assert torch.equal(_bits(Ybuf), _bits(Y2buf))
    for m in range(M):
        one = Y0[m:m + 1].clone()
        ops.lora_bgmv_expand_(U[m:m + 1], B, s.to(dev), idx[m:m + 1], one, G)
        assert torch.equal(_bits(one[0]), _bits(Y[m])), m
    # a zero B leaves Y as it is
    Y3 = Y0.clone()
    ops.lora_bgmv_expand_(U, torch.zeros_like(B), s.to(dev), idx, Y3, G)
    assert torch.equal(_bits(Y3), _bits(Y0))


# every M at every small shape; rank, type, prologue and index pattern cycle so that each value meets each shape
GRID = [(M, shape, RANKS[(i + j) % 4], DTYPES[(i + j) % 2], (i + 2 * j) % 3, IDX_KINDS[(i + j // 2) % 4])
        for i, M in enumerate(MS) for j, shape in enumerate(SHAPES)]
# every rank x prologue x type at the shape whose N = FF = 352 is no multiple of 64, M = 17
RANKED = [(17, SHAPES[1], r, dtype, pro, "mixed") for r, dtype, pro in itertools.product(RANKS, DTYPES, (0, 1, 2))]
# every index pattern at every M
PATTERNS = [(M, SHAPES[0], 24, torch.bfloat16, 1, kind) for M in MS for kind in IDX_KINDS]


def test_the_grid_covers_what_it_claims():
    for col, want in ((0, set(MS)), (1, set(SHAPES)), (2, set(RANKS)), (3, set(DTYPES)), (4, {0, 1, 2}), (5, set(IDX_KINDS))):
        assert {c[col] for c in GRID} == want, col
    for shape in SHAPES:
        assert {c[4] for c in GRID if c[1] == shape} == {0, 1, 2}, shape


@pytest.mark.parametrize("M,shape,r,dtype,pro,kind", GRID + RANKED + PATTERNS)
def test_bgmv_against_fp64_and_bit_for_bit(dev, M, shape, r, dtype, pro, kind):
    _check(dev, dtype, M, *shape, r, pro, kind, seed=M + r)


@pytest.mark.parametrize("M,shape,r,dtype,pro", [(32, (4096, 4096, 3), 16, torch.bfloat16, 1),
                                                 (5, (11008, 4096, 1), 64, torch.float16, 2)])
def test_bgmv_at_the_7b_widths(dev, M, shape, r, dtype, pro):
    _check(dev, dtype, M, *shape, r, pro, "outside", seed=7)


def test_outside_the_domain_returns_codes_not_launches(dev):
    x = torch.zeros((2, 64), dtype=torch.bfloat16, device=dev)
    A = torch.zeros((1, 8, 64), dtype=torch.bfloat16, device=dev)
    B = torch.zeros((1, 64, 8), dtype=torch.bfloat16, device=dev)
    idx = torch.zeros(2, dtype=torch.int32, device=dev)
    s = torch.ones(1, device=dev)
    U = torch.zeros((2, 8), dtype=torch.bfloat16, device=dev)
    Y = torch.zeros((2, 64), dtype=torch.bfloat16, device=dev)
    lib = L.load()
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()  # noqa: E731

    def shrink(M=2, K=64, G=1, r=8, pro=0, w=None, dtype=1, xp=None, ldx=64, ldu=8):
        return lib.mk_lora_bgmv_shrink(p(x) if xp is None else xp, ldx, M, K, p(A), 1, G, r, p(idx), pro, w, 0.0, p(U), ldu,
                                       dtype, st)

    def expand(M=2, G=1, r=8, N=64, dtype=1, ldy=64, yp=None):
        return lib.mk_lora_bgmv_expand(p(U), 8, M, G, r, p(B), p(s), 1, p(idx), p(Y) if yp is None else yp, ldy, N, dtype, st)

    assert shrink() == 0 and expand() == 0
    bad, uns = -1, -2
    assert shrink(M=0) == bad and shrink(G=4) == bad and shrink(r=12) == bad and shrink(r=136) == bad
    assert shrink(pro=3) == bad and shrink(pro=1) == bad and shrink(ldu=4) == bad and shrink(pro=2) == bad   # ldx < 2 K
    assert shrink(M=33) == uns and shrink(dtype=0) == uns and shrink(K=60, ldx=64) == uns and shrink(xp=p(x) + 2) == uns
    assert expand(M=0) == bad and expand(G=0) == bad and expand(r=4) == bad and expand(ldy=32) == bad
    assert expand(M=33) == uns and expand(dtype=0) == uns and expand(N=60) == uns and expand(yp=p(Y) + 2) == uns
    torch.cuda.synchronize()
    with pytest.raises(ops.MacawHipError):
        ops.lora_bgmv_shrink(x, A, idx.long(), 1)
    assert not ops.lora_bgmv_ok(torch.zeros((33, 64), dtype=torch.bfloat16, device=dev), A)
    assert not ops.lora_bgmv_ok(x.float(), A) and not ops.lora_bgmv_ok(x, A, 2) and ops.lora_bgmv_ok(x, A)
