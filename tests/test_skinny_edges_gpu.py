"""GPU: the weight-streaming decode linears held to the EXACT result at every K-loop edge -- every instantiation of
gemm_skinny16_kernel, decode_linear_fp8_kernel, decode_linear_mxfp4_kernel, gemm_skinny32p_kernel and gemm_skinny_kernel
that a launcher can send (tests/skinny_ref.py FORMS, pinned to the sources by tests/test_skinny_ref_cpu.py), on census inputs
whose every partial sum is an exact fp32 number: the output must equal RNE(exact * scale + residual) bit for bit, with the
cancelling residual that makes one quantum of error in the sum visible, and once more without a residual.  Outputs go to a
NaN-filled buffer of 32 rows and a pitch of N rounded up to 64: rows >= M and columns >= N must stay NaN.  A mismatch here is
a kernel fault by construction (Census.check() has shown on the CPU that the expectation has no rounding freedom).  The
ordinary-input tests at the end keep the non-census rounding points covered at the new shapes under the project's own
bounds.

Edge lists run (nkb = K blocks; N = 40 unless noted; largest K in brackets):
  <16,2,P,2> e16 / e4m3 wide, cfg 18     M = 3: 1 15 16 17 31 32 33 47 48 49 63 64                       [K = 4096]
  <8,2,P,3>  e16 / e4m3 narrow, cfg 17   M = 3: 1, 8 j - 1, 8 j, 8 j + 1 for j = 1 ... 13 (to 105)       [K = 6720; N = 4097, cfg 17: 40]
  <8,2,0,2,2> cfg 19, e4m3 two tiles; <8,2,0,2> cfg 13                      the same list to 73         [K = 4672]
  gemm_skinny32p_kernel<8,1,3> cfg 22    to 49 [K = 3136];   gemm_skinny_kernel<8> cfg 12   to 41 [K = 2624]
  MXFP4 <16,1,0,3> and <16,2,P,2> wide   1 15 16 17 31 32                                                [K = 4096]
  MXFP4 <8,1,0,4> narrow                 1, 8 j - 1, 8 j, 8 j + 1 for j = 1 ... 8 (to 65)                [K = 8320; N = 4097]
  MXFP4 <8,2,P,3> narrow                 M = 3 to 49 [K = 6272: three prepared rows end at 53 blocks], M = 1 from 55 to 105 [K = 13440]
  MXFP4 <8,1,0,2,2> two tiles            to 33                                                           [K = 4224]
  one-tile forms also M = 1, 15, 16 at nkb = 1, NW + 1, NW U + 1 (as far as the prepared rows fit), the prologue forms M = 16
  at the largest K inside 40 KiB (19 blocks, MXFP4 9), the narrow decode forms once more reached through K (N = 33, 65 blocks
  of 64 / 33 of 128); the two-tile and 32-row forms M = 17, 31, 32 (mk_gemm forms also 3) over their lists.
Measured on an MI355X: the 98 tests of this file take 22 s together; the slowest parametrised test is
test_ordinary_inputs_at_the_edge_shapes_keep_the_existing_bounds[fp8-narrow] at 1.4 s (the CPU side of _exact_fp8_weight at
4097 x 4160), the slowest census test 0.72 s (MXFP4 <8,2,P,3>, K to 13440) -- below the existing decode-linear tests at the
workload's shapes, so nothing is split.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import skinny_ref as R  # noqa: E402
from test_decode_fp8_gpu import _exact_fp8_weight  # noqa: E402
from test_decode_mxfp4_gpu import _exact_mxfp4_weight  # noqa: E402
from test_kernels_gpu import _close, _rand  # noqa: E402

from macaw_llm_amd import lib as L  # noqa: E402
from macaw_llm_amd import ops  # noqa: E402
from macaw_llm_amd.lib import MacawHipError  # noqa: E402

DEV = torch.device("cuda:0")
FORM_IDS = [f.name.replace(" ", "_") for f in R.FORMS]
DT_IDS = ["bf16", "f16"]


# ------------------------------------------------------------------------------------------------- launching --
class _Operands:
    """the operands of a census on the device; at(nkb) gives the leading-K launch arguments"""

    def __init__(self, c):
        self.c = c
        self.x = tuple(t.to(DEV) for t in c.x) if c.form.PRO == 2 else c.x.to(DEV)
        self.w = {k: v.to(DEV) for k, v in c.weights.items()}
        self.nw = c.norm_w.to(DEV) if c.norm_w is not None else None

    def at(self, nkb):
        f = self.c.form
        K = nkb * f.kblk
        if f.PRO == 2:
            x = torch.cat((self.x[0][:, :K], self.x[1][:, :K]), 1)
        else:
            x = self.x[:, :K]                                   # a pitched view: ldx = the census K
        if f.fmt == "e16":
            w = (self.w["W"][:, :K].contiguous(),)
        elif f.fmt == "fp8":
            w = (self.w["Wq"][:, :K].contiguous(), self.w["s"])
        else:
            w = (self.w["q"][:, :K // 2].contiguous(), self.w["e"][:, :K // 32].contiguous())
        return x, w, (self.nw[:K] if self.nw is not None else None)


def _call(fmt, x, w, pro=0, nw=None, residual=None, out=None):
    fn = {"e16": ops.decode_linear, "fp8": ops.decode_linear_fp8, "mxfp4": ops.decode_linear_mxfp4}[fmt]
    return fn(x, *w, pro, nw, R.EPS if pro == 1 else 0.0, residual=residual, out=out)


def _nan_out(M, N, dtype):
    full = torch.full((32, -(-N // 64) * 64), float("nan"), dtype=dtype, device=DEV)
    return full, full[:M, :N]


def _assert_bits(full, want, M, N, what):
    got = full.cpu()
    gb, wb = R.bits16(got[:M, :N]), R.bits16(want)
    if not torch.equal(gb, wb):
        bad = (gb != wb).nonzero()
        m, n = bad[0].tolist()
        raise AssertionError(f"{what}: {bad.shape[0]} of {M * N} outputs differ; rows {sorted(set(bad[:, 0].tolist()))[:8]}, "
                             f"columns {bad[:12, 1].tolist()} ...; at ({m}, {n}) got {got[m, n].item()!r}, exact "
                             f"expectation {want[m, n].item()!r}")
    guard = got.float()
    guard[:M, :N] = float("nan")
    assert bool(torch.isnan(guard).all()), f"{what}: wrote outside [:{M}, :{N}]"


def _run_decode(o, nkb, M, N, dtype, what):
    c, f = o.c, o.c.form
    x, w, nw = o.at(nkb)
    v = c.exact(nkb) * c.oscale
    res = R.residual(v, dtype, nkb)
    full, out = _nan_out(M, N, dtype)
    _call(f.fmt, x, w, f.PRO, nw, res.to(DEV), out)
    _assert_bits(full, R.expected(v, dtype, res), M, N, f"{what} nkb={nkb} with the cancelling residual")
    full, out = _nan_out(M, N, dtype)
    _call(f.fmt, x, w, f.PRO, nw, None, out)
    _assert_bits(full, R.expected(v, dtype), M, N, f"{what} nkb={nkb} without a residual")


def _gemm(x, W, out, M, N, K, **kw):
    ops.gemm_raw(x, W, out, M, N, K, x.stride(0) if M > 1 else max(x.stride(0), K), K, out.stride(0), **kw)


def _run_gemm(o, nkb, M, N, dtype, what, extras):
    """mk_gemm under the forced cfg: residual / none, and (extras) alpha with an integer row bias, accumulate onto a
    cancelling C"""
    c = o.c
    x, (W,), _ = o.at(nkb)
    K = nkb * 64
    v = c.exact(nkb)
    res = R.residual(v, dtype, nkb)
    resd = res.to(DEV)
    full, out = _nan_out(M, N, dtype)
    _gemm(x, W, out, M, N, K, R=resd, ldr=N)
    _assert_bits(full, R.expected(v, dtype, res), M, N, f"{what} nkb={nkb} residual")
    full, out = _nan_out(M, N, dtype)
    _gemm(x, W, out, M, N, K)
    _assert_bits(full, R.expected(v, dtype), M, N, f"{what} nkb={nkb} plain")
    if not extras:
        return
    bias = torch.randint(-3, 4, (N,), generator=torch.Generator().manual_seed(nkb)).to(dtype)
    for alpha in (0.5, 2.0):
        va = alpha * v + bias.double()[None, :]
        ra = R.residual(va, dtype, nkb + 1)
        full, out = _nan_out(M, N, dtype)
        _gemm(x, W, out, M, N, K, R=ra.to(DEV), ldr=N, bias=bias.to(DEV), bias_mode=1, alpha=alpha)
        _assert_bits(full, R.expected(va, dtype, ra), M, N, f"{what} nkb={nkb} alpha={alpha} + row bias + residual")
    full, out = _nan_out(M, N, dtype)
    out.copy_(resd)
    _gemm(x, W, out, M, N, K, accumulate=True)
    _assert_bits(full, R.expected(v, dtype, res), M, N, f"{what} nkb={nkb} accumulate onto a cancelling C")


# ------------------------------------------------------------------------------------------ the census, exact --
@pytest.mark.parametrize("dtype", R.H16, ids=DT_IDS)
@pytest.mark.parametrize("form", R.FORMS, ids=FORM_IDS)
def test_census_outputs_equal_the_exact_result_at_every_edge(form, dtype):
    lib = L.load()
    try:
        if form.reach != "decode":
            lib.mk_gemm_set_cfg(form.reach)
        for M, N, nkbs in R.census_runs(form):
            c = R.census(form.name, dtype, M, N, max(nkbs))
            o = _Operands(c)
            what = f"{form.name} {dtype} M={M} N={N}"
            for nkb in nkbs:
                if form.reach == "decode":
                    assert form.mmax == 32 or R.wide(N, nkb * form.kblk) == form.wide
                    _run_decode(o, nkb, M, N, dtype, what)
                else:
                    _run_gemm(o, nkb, M, N, dtype, what, extras=M in (3, 17))
    finally:
        lib.mk_gemm_set_cfg(-1)


@pytest.mark.parametrize("dtype", R.H16, ids=DT_IDS)
@pytest.mark.parametrize("N,cfg", [(40, 19), (8191, 19), (8192, 22), (8193, 22)])
def test_17_to_32_rows_through_decode_linear_take_cfg_19_below_n_8192_and_22_from_there(N, cfg, dtype):
    """ops.decode_linear with 17 rows sends skinny32_cfg(N)'s kernel; both are exact on the census, so what this adds to the
    forced-cfg runs is the route (and the 32-row kernel's ragged last workgroup at N = 8193: one real weight row of 32)"""
    assert R.skinny32_cfg(N) == cfg
    form = R.BY_NAME["e16 cfg22 32 x 32" if cfg == 22 else "e16 cfg19 two tiles"]
    nkbs = [1, form.NW + 1, form.NW * form.U * form.NBUF + 1]
    c = R.census(form.name, dtype, 17, N, max(nkbs))
    c.check()
    o = _Operands(c)
    for nkb in nkbs:
        _run_decode(o, nkb, 17, N, dtype, f"decode_linear 17 x {N} (cfg {cfg})")


@pytest.mark.parametrize("dtype", R.H16, ids=DT_IDS)
@pytest.mark.parametrize("pro,width", [(p, w) for p in (0, 1, 2) for w in ("wide", "narrow")])
def test_the_three_formats_give_identical_bits_on_the_same_values(pro, width, dtype):
    """the MXFP4 census (integers times block scales 1/2, 1, 2) is also a set of e4m3 codes with scale 1 and of 16-bit values:
    the three kernels must agree bit for bit (each already equals the exact expectation: a consistency check, not the oracle)"""
    f4 = R.BY_NAME[f"mxfp4 {width} pro{pro}"]
    N = R.census_N(f4)
    for nkb in sorted({1, f4.NW + 1, min(R.nkb_reach(f4, 3), 2 * f4.NW * f4.U + 1)}):
        c = R.census(f4.name, dtype, 3, N, nkb)
        o = _Operands(c)
        x, w4, nw = o.at(nkb)
        v = c.exact(nkb)
        res = R.residual(v, dtype, nkb).to(DEV)
        W16 = c.weff.to(dtype).to(DEV)
        W8 = c.weff.to(R.FP8).view(torch.uint8).to(DEV)
        assert torch.equal(W8.cpu().view(R.FP8).float(), c.weff)
        one = torch.ones(N, dtype=torch.float32, device=DEV)
        assert R.wide(N, c.K) == (width == "wide")
        y4 = _call("mxfp4", x, w4, pro, nw, res)
        y8 = _call("fp8", x, (W8, one), pro, nw, res)
        y16 = _call("e16", x, (W16,), pro, nw, res)
        want = R.bits16(R.expected(v, dtype, R.residual(v, dtype, nkb)))
        for name, y in (("mxfp4", y4), ("e4m3", y8), ("16-bit", y16)):
            assert torch.equal(R.bits16(y.cpu()), want), (name, pro, width, nkb)


@pytest.mark.parametrize("dtype", R.H16, ids=DT_IDS)
def test_k_1280_with_16_rows_is_refused_alike_by_the_ok_rules_and_the_entry_points(dtype):
    """16 prepared rows of K = 1280 are 41216 bytes: past the 40 KiB the prologue forms may take.  K = 1216 (1152 for MXFP4)
    is the largest that fits, and the census runs it."""
    M, N, K = 16, 40, 1280
    assert not R.prologue_fits(M, K) and R.prologue_fits(M, 1216)
    x = torch.ones((M, 2 * K), dtype=dtype, device=DEV)
    nw = torch.ones(K, dtype=dtype, device=DEV)
    W = torch.ones((N, K), dtype=dtype, device=DEV)
    Wq, s = torch.zeros((N, K), dtype=torch.uint8, device=DEV), torch.ones(N, device=DEV)
    q, e = torch.zeros((N, K // 2), dtype=torch.uint8, device=DEV), torch.full((N, K // 32), 127, dtype=torch.uint8, device=DEV)
    for pro in (1, 2):
        xx = x if pro == 2 else x[:, :K]
        assert not ops.decode_linear_ok(xx, W, pro) and not ops.decode_linear_fp8_ok(xx, Wq, pro)
        assert not ops.decode_linear_mxfp4_ok(xx, q, pro)
        for fmt, w in (("e16", (W,)), ("fp8", (Wq, s)), ("mxfp4", (q, e))):
            with pytest.raises(MacawHipError):
                _call(fmt, xx, w, pro, nw)
    assert ops.decode_linear_ok(x[:, :K], W, 0) and ops.decode_linear_ok(x[:, :1216], W[:, :1216].contiguous(), 1)
    _call("e16", x[:, :K], (W,))                                # the plain form takes it


# ------------------------------------------------------------------------------- ordinary inputs, edge shapes --
def _ordinary_weight(fmt, N, K, dtype, g):
    """(kernel operands, f32 values, their magnitude): the generators of the existing decode-linear tests"""
    if fmt == "e16":
        W = (_rand((N, K), dtype, g).float() * 0.05).to(dtype)
        return (W.to(DEV),), W.float(), 0.05
    if fmt == "fp8":
        Wq, s, Wf = _exact_fp8_weight(N, K, g)
        return (Wq.to(DEV), s.to(DEV)), Wf, Wf.std().item()
    q, e, Wf = _exact_mxfp4_weight(N, K, g)
    return (q.to(DEV), e.to(DEV)), Wf, Wf.std().item()


@pytest.mark.parametrize("dtype", R.H16, ids=DT_IDS)
@pytest.mark.parametrize("width", ["wide", "narrow"])
@pytest.mark.parametrize("fmt", ["e16", "fp8", "mxfp4"])
def test_ordinary_inputs_at_the_edge_shapes_keep_the_existing_bounds(fmt, width, dtype):
    """N(0, 1) tokens and the existing weight generators at nkb = 1, NW - 1, NW U + 1, (NBUF + 1) NW U + 1 of each form:
    the plain form under test_kernels_gpu._close against fp32 math, PRO 2 equal to swiglu2d_fwd + the plain form bit for
    bit, PRO 1 against rmsnorm_fwd + the plain form under the two bounds of
    test_decode_linear_prologues_match_the_separate_kernels (the share of equal outputs over M N >= 4096 of them)"""
    M, N = 3, 1366 if width == "wide" else 4097
    assert M * N >= 4096
    for pro in (0, 1, 2):
        f = R.BY_NAME[f"{fmt} {width} pro{pro}"]
        lim = R.nkb_reach(f, M)
        for nkb in sorted({n for n in (1, f.NW - 1, f.NW * f.U + 1, (f.NBUF + 1) * f.NW * f.U + 1) if n <= lim}):
            K = nkb * f.kblk
            assert R.wide(N, K) == (width == "wide")
            g = torch.Generator().manual_seed(M + N + K + pro)
            w, Wf, wstd = _ordinary_weight(fmt, N, K, dtype, g)
            res = _rand((M, N), dtype, g)
            resd = res.to(DEV)
            if pro == 0:
                x = _rand((M, K), dtype, g)
                y = _call(fmt, x.to(DEV), w, residual=resd)
                _close(y, x.float() @ Wf.t() + res.float(), dtype, scale=math.sqrt(K) * wstd + 1.0, what=f"{f.name} nkb={nkb}")
            elif pro == 1:
                x = _rand((M, K), dtype, g).to(DEV)
                nw = (1.0 + 0.1 * _rand((K,), torch.float32, g)).to(dtype).to(DEV)
                _, yn, _ = ops.rmsnorm_fwd(x, nw, R.EPS)
                want = _call(fmt, yn, w)
                got = _call(fmt, x, w, 1, nw)
                d = (got.float() - want.float()).abs().max().item()
                assert d <= 0.02 * want.float().abs().max().item() + 1e-3, (f.name, nkb, d)
                assert (got == want).float().mean().item() > 0.98, (f.name, nkb)
            else:
                gu = _rand((M, 2 * K), dtype, g).to(DEV)
                want = _call(fmt, ops.swiglu2d_fwd(gu, K), w, residual=resd)
                got = _call(fmt, gu, w, 2, residual=resd)
                assert torch.equal(got, want), (f.name, nkb)


@pytest.mark.parametrize("dtype", R.H16, ids=DT_IDS)
@pytest.mark.parametrize("name", ["e16 cfg19 two tiles", "e16 cfg22 32 x 32", "e16 cfg13", "e16 cfg12", "fp8 two tiles",
                                  "mxfp4 two tiles"])
def test_ordinary_inputs_on_the_two_tile_32_row_and_forced_forms(name, dtype):
    """the same four K-block counts, plain form, under test_kernels_gpu._close"""
    f = R.BY_NAME[name]
    M, N = (16 if f.mmax == 16 else 31), 1366
    lib = L.load()
    try:
        if f.reach != "decode":
            lib.mk_gemm_set_cfg(f.reach)
        for nkb in sorted({1, f.NW - 1, f.NW * f.U + 1, (f.NBUF + 1) * f.NW * f.U + 1}):
            K = nkb * f.kblk
            g = torch.Generator().manual_seed(M + N + K)
            w, Wf, wstd = _ordinary_weight(f.fmt, N, K, dtype, g)
            x, res = _rand((M, K), dtype, g), _rand((M, N), dtype, g)
            if f.reach == "decode":
                y = _call(f.fmt, x.to(DEV), w, residual=res.to(DEV))
            else:
                y = ops.linear_fwd(x.to(DEV), w[0], residual=res.to(DEV))
            _close(y, x.float() @ Wf.t() + res.float(), dtype, scale=math.sqrt(K) * wstd + 1.0, what=f"{name} nkb={nkb}")
    finally:
        lib.mk_gemm_set_cfg(-1)
