"""GPU: the 288 x 256 x 64 tile of gemm_v9 (kernel configuration 21, gemm_bf16_tile288_kernel; loop: gemm_v9_loop288.inc, its
slot / wait protocol simulated in tests/test_v9_gen288_cpu.py) against configurations 11 (gemm_v7) and 15 (gemm_v9's 256 tile).

Every output element is summed over K by the same MFMA in the same order on all three, so the comparison is BIT for bit; against
torch's fp32 product of the same 16-bit inputs the bound is tests/test_kernels_gpu.py's (the final 16-bit rounding: rtol 8e-3 of
the largest reference value + 8e-3 of the output scale 0.1 sqrt(K) (+ 1 with a residual)).

Shapes: M in {288, 576, 2304} (one tile row, two, nine = a wave's upper and lower 144 rows in every tile), N in {256, 512},
K in {128, 192, 256, 320, 1024} = 2, 3, 4, 5, 16 K-tiles (no trip of the steady-state body, one, two, three = the two-slot
rings wrap, many laps).  The operands are row slices of one buffer per dtype, so lda = ldb = 1024 >= K.  The profile's cfg
column says which kernel ran: a forced 21 must not be a silent fallback, and outside its domain it must be one."""
import csv
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from macaw_llm_amd import engine as eng  # noqa: E402
from macaw_llm_amd import lib as L  # noqa: E402
from macaw_llm_amd import ops  # noqa: E402

H16 = [torch.bfloat16, torch.float16]
MMAX, NMAX, KMAX, PITCH = 2304, 512, 1024, 516      # PITCH: rows of C / R 8- but not 16-byte aligned


@pytest.fixture(scope="module")
def data(dev):
    out = {}
    for dtype in H16:
        g = torch.Generator().manual_seed(288 + (dtype == torch.float16))
        r = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).to(dtype).to(dev)  # noqa: E731
        out[dtype] = dict(A=r(MMAX + 12, KMAX), B=r(NMAX, KMAX, scale=0.1), R=r(MMAX + 12, PITCH))
    return out


def _close(got, ref, K, residual, what):
    got, ref = got.float(), ref.float()
    err = (got - ref).abs().max().item()
    lim = 8e-3 * (0.1 * math.sqrt(K) + (1.0 if residual else 0.0)) + 8e-3 * ref.abs().max().item()
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    assert err <= lim, f"{what}: max abs err {err:.3e} > {lim:.3e}"


def _run(lib, cfg, d, M, N, K, ldc, alpha, residual):
    lib.mk_gemm_set_cfg(cfg)
    C = torch.full((M, ldc), float("nan"), dtype=d["A"].dtype, device=d["A"].device)
    ops.gemm_raw(d["A"], d["B"], C, M, N, K, KMAX, KMAX, ldc, R=d["R"] if residual else None, ldr=PITCH if residual else 0,
                 alpha=alpha)
    return C


def _cfgs_of_profile(path):
    with open(path) as f:
        return [(int(r["cfg"]), int(r["launches"])) for r in csv.DictReader(f) if r["kind"] == "gemm"]


@pytest.mark.parametrize("dtype", H16)
@pytest.mark.parametrize("M", [288, 576, 2304])
@pytest.mark.parametrize("N", [256, 512])
@pytest.mark.parametrize("K", [128, 192, 256, 320, 1024])
def test_tile288_is_bit_equal_to_the_256_tiles(dev, data, tmp_path, dtype, M, N, K):
    lib = L.load()
    assert lib.mk_gemm_has_cfg(21)
    d = data[dtype]
    prod = d["A"][:M, :K].float() @ d["B"][:N, :K].float().t()
    path = str(tmp_path / "prof.csv")
    n21 = 0
    ops.prof_begin()
    try:
        for alpha in (1.0, 0.375):
            for residual in (False, True):
                for ldc in (N, PITCH):          # (the residual always has the pitch; C has it in two of the four forms)
                    if ldc == PITCH and (alpha == 1.0) == residual:
                        continue
                    what = f"{dtype} {M}x{N}x{K} alpha {alpha} residual {residual} ldc {ldc}"
                    got = _run(lib, 21, d, M, N, K, ldc, alpha, residual)
                    n21 += 1
                    ref = alpha * prod + (d["R"][:M, :N].float() if residual else 0.0)
                    _close(got[:, :N], ref, K, residual, what)
                    assert torch.isnan(got[:, N:].float()).all(), f"{what}: pad columns of C written"
                    for other in (11, 15) if M % 256 == 0 else (11,):
                        assert torch.equal(got[:, :N], _run(lib, other, d, M, N, K, ldc, alpha, residual)[:, :N]), \
                            f"{what}: differs from configuration {other}"
        ops.prof_report(path)
    finally:
        ops.prof_end()
        lib.mk_gemm_set_cfg(-1)
    assert sum(n for c, n in _cfgs_of_profile(path) if c == 21) == n21, "a forced configuration 21 ran on another kernel"


@pytest.mark.parametrize("dtype", H16)
def test_walking_workgroups_over_several_tiles_twice_in_a_row(dev, data, dtype):
    """8 planned CUs (mk_gemm_set_cus); M = 2304 is 8 tile rows of 288, N = 512 two columns: 16 tiles = two whole rounds of 8
    walking workgroups (each requests its second tile before the first one's epilogue; the second runs the loop's
    walking form).  Run twice in a row: nothing of a launch is left behind in LDS or registers.
    Here configuration 15 really runs gemm_v9's 256 tile (18 tiles on 8 CUs; in the test above 256 CUs outnumber the tiles and
    the launcher sends a forced 15 to gemm_v7).  Its epilogue lets hipcc contract alpha * acc + R into one fma and, in fp16,
    alpha * acc and the conversion into one v_fma_mixlo_f16, so it matches gemm_v7 where the product with alpha is exact (a
    power of two, as in tests/test_kernels_gpu.py); the 288 tile rounds step by step as gemm_v7 does, so at alpha = 0.375 it is
    compared with configuration 11 alone."""
    lib = L.load()
    d = data[dtype]
    M, N, K = 2304, 512, 1024
    prev = lib.mk_gemm_set_cus(8)
    try:
        prod = d["A"][:M, :K].float() @ d["B"][:N, :K].float().t()
        for alpha, others in ((0.5, (11, 15)), (0.375, (11,))):
            for residual in (False, True):
                a = _run(lib, 21, d, M, N, K, N, alpha, residual)
                b = _run(lib, 21, d, M, N, K, N, alpha, residual)
                assert torch.equal(a, b), "not reproducible run to run"
                for other in others:
                    assert torch.equal(a, _run(lib, other, d, M, N, K, N, alpha, residual)), \
                        f"alpha {alpha} residual {residual}: differs from configuration {other}"
                ref = alpha * prod + (d["R"][:M, :N].float() if residual else 0.0)
                _close(a, ref, K, residual, f"walking {dtype} alpha {alpha} residual {residual}")
    finally:
        lib.mk_gemm_set_cus(prev)
        lib.mk_gemm_set_cfg(-1)


def test_outside_its_domain_configuration_21_falls_back(dev, data, tmp_path):
    """M = 300 is no multiple of 288; a reduction-major operand, an activation and an accumulating C have no 288 kernel either:
    a forced 21 runs what a forced 11 runs, the profile says so, and the result is configuration 11's."""
    lib = L.load()
    d = data[torch.bfloat16]
    N, K = 256, 256
    path = str(tmp_path / "prof.csv")
    ops.prof_begin()
    try:
        got = _run(lib, 21, d, 300, N, K, N, 1.0, False)
        assert torch.equal(got, _run(lib, 11, d, 300, N, K, N, 1.0, False))
        _close(got, d["A"][:300, :K].float() @ d["B"][:N, :K].float().t(), K, False, "M = 300")
        outs = {}
        for cfg in (21, 11):
            lib.mk_gemm_set_cfg(cfg)
            At = d["A"][:K, :288]                      # A as [K][M]: reduction-major
            C1 = torch.empty((288, N), dtype=torch.bfloat16, device=dev)
            ops.gemm_raw(At, d["B"], C1, 288, N, K, KMAX, KMAX, N, a_red=True)
            C2 = torch.empty((288, N), dtype=torch.bfloat16, device=dev)
            ops.gemm_raw(d["A"], d["B"], C2, 288, N, K, KMAX, KMAX, N, act=1)
            C3 = torch.ones((288, N), dtype=torch.bfloat16, device=dev)
            ops.gemm_raw(d["A"], d["B"], C3, 288, N, K, KMAX, KMAX, N, accumulate=True)
            outs[cfg] = (C1, C2, C3)
        for a, b in zip(outs[21], outs[11]):
            assert torch.equal(a, b)
        ops.prof_report(path)
    finally:
        ops.prof_end()
        lib.mk_gemm_set_cfg(-1)
    assert all(c != 21 for c, _ in _cfgs_of_profile(path))


# ---- one decoder layer, forward + backward, configuration 21 forced against configuration 11 forced ------------------------
B_, S_, D_, H_, FF_ = 3, 192, 512, 4, 1024          # M = 576 rows = two tile rows of 288
NAMES = ["wq", "wk", "wv", "wo", "wg", "wu", "wd", "ln1", "ln2"]


def _layer(dev, dtype):
    g = torch.Generator().manual_seed(21)
    r = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).to(dtype).to(dev)  # noqa: E731
    wqkv, wgu = r(3 * D_, D_, scale=D_ ** -0.5), r(2 * FF_, D_, scale=D_ ** -0.5)
    w = {"wq": wqkv[:D_], "wk": wqkv[D_:2 * D_], "wv": wqkv[2 * D_:], "wo": r(D_, D_, scale=D_ ** -0.5), "wg": wgu[:FF_],
         "wu": wgu[FF_:], "wd": r(D_, FF_, scale=FF_ ** -0.5), "ln1": 1 + r(D_, scale=0.1), "ln2": 1 + r(D_, scale=0.1)}
    w = {k: v.detach().requires_grad_(True) for k, v in w.items()}
    hd = D_ // H_
    inv = 1.0 / (10000 ** (torch.arange(0, hd, 2).float() / hd))
    emb = torch.cat((torch.einsum("i,j->ij", torch.arange(S_).float(), inv),) * 2, dim=-1)
    return dict(w=w, wqkv=wqkv, wgu=wgu, x=r(B_, S_, D_).requires_grad_(True), dout=r(B_, S_, D_),
                cos=emb.cos().to(dtype).to(dev), sin=emb.sin().to(dtype).to(dev),
                pos=torch.arange(S_, dtype=torch.int32).repeat(B_).to(dev))


def _fwd_bwd(c):
    w = c["w"]
    y = eng.LlamaLayerFn.apply(c["x"], None, c["pos"], c["cos"], c["sin"], H_, 1e-6, w["wq"], w["wk"], w["wv"], w["wo"], w["wg"],
                               w["wu"], w["wd"], w["ln1"], w["ln2"], c["wqkv"], c["wgu"], False)
    return [y.detach()] + list(torch.autograd.grad(y, [c["x"]] + [w[n] for n in NAMES], c["dout"]))


def test_decoder_layer_forward_and_backward_are_bit_equal_under_configuration_21(dev, tmp_path):
    """LlamaLayerFn at D = 512, FF = 1024, M = 576: the four forward projections (q|k|v 576 x 1536 x 512, o 576 x 512 x 512 +
    residual, gate|up 576 x 2048 x 512, down 576 x 512 x 1024 + residual) run on the 288 tile (the profile says so), the
    backward's reduction-major GEMMs where configuration 11 sends them: the output and all ten gradients are the same bits."""
    lib = L.load()
    c = _layer(dev, torch.bfloat16)
    path = str(tmp_path / "prof.csv")
    outs = {}
    try:
        for cfg in (21, 11):
            lib.mk_gemm_set_cfg(cfg)
            if cfg == 21:
                ops.prof_begin()
            try:
                outs[cfg] = [t.clone() for t in _fwd_bwd(c)]
                if cfg == 21:
                    ops.prof_report(path)
            finally:
                if cfg == 21:
                    ops.prof_end()
    finally:
        lib.mk_gemm_set_cfg(-1)
        ops.GRAD_DST.clear()
        ops.GRAD_DST_TAKEN.clear()
    for n, a, b in zip(["y", "dx"] + NAMES, outs[21], outs[11]):
        assert a.shape == b.shape and torch.equal(a, b), f"{n} differs"
        assert torch.isfinite(a.float()).all(), f"{n} not finite"
    with open(path) as f:
        rows = [r for r in csv.DictReader(f) if r["kind"] == "gemm" and int(r["cfg"]) == 21]
    assert sorted((int(r["N"]), int(r["K"])) for r in rows) == sorted([(3 * D_, D_), (D_, D_), (2 * FF_, D_), (D_, FF_)]), rows
    assert all(int(r["M"]) == B_ * S_ and int(r["layout"]) == 0 for r in rows)
