"""mk_gemm's launcher paths that depend on the PLANNED CU count (mk_gemm_set_cus) and on a batch, on the MFMA tile kernels.

Every round size, the spatial tail of the 256 x 256 kernels, the walking grid and the K-split of the 128 x 128 kernels are
computed from n_cus; the step runtime plans for (CUs - collective channels) while collectives overlap the backward, and the
engine's batched products reach the 128 x 128 kernels with the batch index folded into the linear tile index.  With 8
planned CUs every one of those branches is reached at a few hundred rows; the cases and the plan each is meant to hit are
in tests/gemm_cases.py (checked against the restated rules by tests/test_gemm_cases_cpu.py).

For every case:
  * inputs: seeded normal values rounded to the element type on the CPU, B scaled by 0.1
  * reference: float64 on the CPU from the same buffers by explicit index arithmetic (gemm_cases.Problem.reference)
  * bounds: the two of tests/test_kernels_gpu.py, unchanged -- its `_close` against the reference with
    scale = 0.1 sqrt(K) + the magnitude of the added terms, and max|diff| <= 2^-7 max|ref| + 1e-6 against cfg 0 (the
    generic kernel) on the same inputs
  * C has a pitch wider than N, guard rows between batch slices, NaN everywhere outside what accumulate reads: every element
    outside the logical outputs must be bit-unchanged
  * a forced kernel runs twice, bit-identical
  * after every launch the arrival counters (first 4 KiB of the workspace) are zero again
  * the in-library profile must name the kernel the case pins (cfg 15 with fewer whole tiles than planned CUs reports 11,
    as csrc/gemm.hip documents; the f32 kernel reports -1: it has no configurations)

Deliberately not covered: the launcher's fallback for more tail tiles than counters (R * 4 > 4096 bytes).  R < slots <= 4 x
256 CUs = 1024 counters, so no device with at most 256 CUs reaches it.
"""
import csv

import pytest
import torch

pytestmark = pytest.mark.gpu

from macaw_llm_amd import lib as L  # noqa: E402
from macaw_llm_amd import ops  # noqa: E402
from test_kernels_gpu import _close  # noqa: E402
import gemm_cases as G  # noqa: E402

H16 = [torch.bfloat16, torch.float16]


def _bits(t):
    return t.reshape(-1).view(torch.int32 if t.dtype == torch.float32 else torch.int16)


class _Planned:
    """forces a kernel configuration and a planned CU count; always restores the automatic choice and all CUs"""

    def __init__(self, cfg, cus):
        self.cfg, self.cus, self.lib = cfg, cus, L.load()

    def __enter__(self):
        self.lib.mk_gemm_set_cfg(self.cfg)
        self.lib.mk_gemm_set_cus(self.cus)
        return self

    def __exit__(self, *exc):
        self.lib.mk_gemm_set_cfg(-1)
        self.lib.mk_gemm_set_cus(0)


def _launch(p, dev, tmp_path):
    """one mk_gemm of problem p under the current cfg / CU plan -> (flat C on the CPU, cfg the profile reports)"""
    dv = {k: (getattr(p, k).to(dev) if getattr(p, k) is not None else None) for k in ("A", "B", "C", "R", "bias")}
    path = str(tmp_path / "prof.csv")
    ops.prof_begin()
    try:
        ops.gemm_raw(dv["A"], dv["B"], dv["C"], p.M, p.N, p.K, p.lda, p.ldb, p.ldc, R=dv["R"], bias=dv["bias"],
                     **p.gemm_args())
        ops.prof_report(path)
    finally:
        ops.prof_end()
    with open(path) as f:
        rows = [r for r in csv.DictReader(f) if r["kind"] == "gemm"]
    assert len(rows) == 1 and int(rows[0]["launches"]) == 1, rows
    assert (int(rows[0]["M"]), int(rows[0]["N"]), int(rows[0]["K"]), int(rows[0]["batch"])) == (p.M, p.N, p.K, p.nbatch)
    assert not ops._workspace(dev)[:G.COUNTER_BYTES].any().item(), f"{p.name}: arrival counters not left zero"
    return dv["C"].cpu().reshape(-1), int(rows[0]["cfg"])


def _check(p, got, what):
    """reference bound on the logical outputs, everything else bit-unchanged"""
    idx, ref = p.reference()
    print(f"{what}: max|err| {(got[idx].double() - ref).abs().max().item():.3e}  max|ref| {ref.abs().max().item():.3e}")
    _close(got[idx], ref, p.dtype, scale=p.scale, what=what)
    outside = torch.ones(got.numel(), dtype=torch.bool)
    outside[idx] = False
    assert torch.equal(_bits(got)[outside], _bits(p.C)[outside]), f"{what}: wrote outside the logical outputs"


def _pinned(p, dev, tmp_path, cfg, cus, want_cfg=None, generic=None):
    """the common method: forced kernel twice (bit-identical), the profile's cfg, both bounds; returns the generic result"""
    want_cfg = cfg if want_cfg is None else want_cfg
    what = f"{p.name} cfg {cfg} cus {cus}"
    with _Planned(cfg, cus):
        got, seen = _launch(p, dev, tmp_path)
        again, _ = _launch(p, dev, tmp_path)
    assert seen == want_cfg, f"{what}: ran cfg {seen}, meant to pin {want_cfg}"
    assert torch.equal(_bits(got), _bits(again)), f"{what}: not reproducible run to run"
    _check(p, got, what)
    if generic is None:
        with _Planned(0, cus):
            generic, seen0 = _launch(p, dev, tmp_path)
        assert seen0 == 0
        _check(p, generic, what + " (generic kernel)")
    idx, ref = p.reference()
    d = (got[idx].float() - generic[idx].float()).abs().max().item()
    print(f"{what}: max|diff to cfg 0| {d:.3e}")
    assert d <= 2 ** -7 * ref.abs().max().item() + 1e-6, f"{what}: {d:.3e} from the generic kernel"
    return generic


# ------------------------------------------------------ A: 256 x 256 kernels --
@pytest.mark.parametrize("row", G.A_ROWS, ids=G.A_IDS)
def test_v7_planned_cu_plans(dev, tmp_path, row):
    """cfg 11 under a planned CU count: exact rounds, eighth / quarter tails, walking workgroups and both in one grid, CU
    counts that are no multiple of 8 -- every operand layout, bf16 and f16, plain and with alpha + column bias + residual
    + accumulate."""
    n, M, N, K, ldc = row[:5]
    for i, (a_red, b_red) in enumerate(G.LAYOUTS):
        for j, dtype in enumerate(H16):
            for epi in ("plain", "alpha+bias+residual+accumulate"):
                _pinned(G.single(dtype, M, N, K, a_red, b_red, epi, ldc=ldc, seed=4 * i + j), dev, tmp_path, 11, n)


@pytest.mark.parametrize("row", [r for r in G.A_ROWS if r[7]], ids=[i for i, r in zip(G.A_IDS, G.A_ROWS) if r[7]])
def test_v9_planned_cu_plans(dev, tmp_path, row):
    """cfg 15 with the epilogues it keeps (plain on a 16-byte aligned C; alpha + residual on a C pitch that is only 8-byte
    aligned): whole tiles on gemm_v9 -- walking where they are whole rounds -- and the tail as a second launch on v7."""
    n, M, N, K = row[:4]
    for i, (a_red, b_red) in enumerate(G.LAYOUTS):
        for j, dtype in enumerate(H16):
            for epi, ldc in (("plain", N + 8), ("alpha+residual", N + 4)):
                _pinned(G.single(dtype, M, N, K, a_red, b_red, epi, ldc=ldc, seed=4 * i + j + 1), dev, tmp_path, 15, n)


def test_v9_with_bias_falls_back_to_v7_and_says_so(dev, tmp_path):
    """gemm_v9's register epilogue has no bias form: forced cfg 15 must run (and report) cfg 11, walking on 8 planned CUs"""
    for dtype in H16:
        _pinned(G.single(dtype, 1024, 1024, 192, False, True, "bias"), dev, tmp_path, 15, 8, want_cfg=11)


def test_automatic_choice_under_planned_cus(dev, tmp_path):
    """cfg = -1 with 8 planned CUs, 9 / 16 / 17 tiles: right whatever pick_cfg chose, and it reports a kernel that exists"""
    lib = L.load()
    for M, N, K in G.AUTO_SHAPES:
        for i, (a_red, b_red) in enumerate(G.LAYOUTS):
            p = G.single(H16[i % 2], M, N, K, a_red, b_red, seed=i)
            what = f"{p.name} automatic, 8 CUs"
            with _Planned(-1, 8):
                got, seen = _launch(p, dev, tmp_path)
            with _Planned(0, 8):
                generic, _ = _launch(p, dev, tmp_path)
            print(f"{what}: chose cfg {seen}")
            assert lib.mk_gemm_has_cfg(seen) == 1, f"{what}: reports cfg {seen}"
            _check(p, got, what)
            idx, ref = p.reference()
            d = (got[idx].float() - generic[idx].float()).abs().max().item()
            assert d <= 2 ** -7 * ref.abs().max().item() + 1e-6, what


def test_set_cus_returns_the_previous_value_and_zero_means_all(dev, tmp_path):
    lib = L.load()
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    p = G.single(torch.bfloat16, 768, 768, 192, False, False)
    try:
        lib.mk_gemm_set_cfg(11)
        before, _ = _launch(p, dev, tmp_path)              # no mk_gemm_set_cus call in effect
        assert lib.mk_gemm_set_cus(8) == 0
        eight, _ = _launch(p, dev, tmp_path)
        assert lib.mk_gemm_set_cus(cus) == 8
        at_all, _ = _launch(p, dev, tmp_path)
        assert lib.mk_gemm_set_cus(cus + 16) == cus
        above, _ = _launch(p, dev, tmp_path)
        assert lib.mk_gemm_set_cus(-3) == cus + 16         # negative values are stored as 0
        assert lib.mk_gemm_set_cus(0) == 0
        after, _ = _launch(p, dev, tmp_path)
        assert lib.mk_gemm_set_cus(0) == 0
    finally:
        lib.mk_gemm_set_cfg(-1)
        lib.mk_gemm_set_cus(0)
    for name, got in (("the CU count", at_all), ("more than the CU count", above), ("0 again", after)):
        assert torch.equal(_bits(got), _bits(before)), f"planning for {name} differs from the default plan"
    _check(p, before, "768 x 768, all CUs")
    _check(p, eight, "768 x 768, 8 CUs")


# ------------------------------------------- B: K-split of the 128 x 128 kernels --
@pytest.mark.parametrize("row", G.B_ROWS, ids=G.B_IDS)
def test_k_split_tail_under_planned_cus(dev, tmp_path, row):
    """one tail tile beside a full round of 8 planned CUs' slots: even pieces, a shorter last piece, an empty last piece,
    and a K too short to split -- plain, and with bias + GELU + residual + accumulate (applied once, by the last arriver)."""
    cfg, n, M, N, K = row[:5]
    for i, (a_red, b_red) in enumerate(G.b_layouts(cfg)):
        for j, dtype in enumerate(H16):
            for epi in ("plain", "bias+gelu+residual+accumulate"):
                _pinned(G.single(dtype, M, N, K, a_red, b_red, epi, seed=4 * i + j + 2), dev, tmp_path, cfg, n)


@pytest.mark.parametrize("cfg", [5, 7])
def test_k_split_needs_its_whole_workspace_or_runs_unsplit(dev, tmp_path, monkeypatch, cfg):
    """workspace edges: counters only (the launcher must run the tail tile unsplit), and exactly the bytes the split needs
    in front of a guard that must stay intact"""
    n, M, N, K = [r for r in G.B_ROWS if r[0] == cfg][0][1:5]
    a_red = b_red = cfg == 7
    plan = G.plan128(n, M, N, K, a_red, b_red)
    assert plan["sp"] >= 2
    for dtype in H16:
        p = G.single(dtype, M, N, K, a_red, b_red, "bias+gelu+residual+accumulate", seed=5)
        small = torch.zeros(G.COUNTER_BYTES, dtype=torch.uint8, device=dev)
        monkeypatch.setattr(ops, "_workspace", lambda device: small)
        generic = _pinned(p, dev, tmp_path, cfg, n)
        assert not small.any().item()

        need, guard = plan["need"], 64 << 10
        buf = torch.empty(need + guard, dtype=torch.uint8, device=dev)
        buf[:G.COUNTER_BYTES] = 0
        buf[G.COUNTER_BYTES:need] = 0xFF                   # (fp32 NaN: a slab that is read without being written shows)
        buf[need:] = 0xA5
        monkeypatch.setattr(ops, "_workspace", lambda device: buf[:need])
        _pinned(p, dev, tmp_path, cfg, n, generic=generic)
        assert (buf[need:] == 0xA5).all().item(), "the K-split wrote past the workspace it was given"
        assert (buf[G.COUNTER_BYTES:need] != 0xFF).any().item(), "the K-split did not run"
        assert not buf[:G.COUNTER_BYTES].any().item()
        monkeypatch.undo()


# ----------------------------------------------------- C: batched products --
@pytest.mark.parametrize("cus", [0, 8], ids=["all-cus", "8-cus"])
@pytest.mark.parametrize("name", list(G.C_PATTERNS))
def test_batched_engine_patterns_on_the_128_tile_kernels(dev, tmp_path, name, cus):
    """the engine's batched products on cfg 5 / cfg 7: with all CUs the K-split takes the whole problem (batch folded into
    the linear tile index), with 8 planned CUs whole tiles and tail tiles lie in different batches.  A wrong (z1, z2)
    decomposition lands in another head's columns or another sample's rows: all of those must be bit-unchanged."""
    for dtype in H16:
        p = G.c_problem(name, dtype)
        _pinned(p, dev, tmp_path, 5, cus, want_cfg=7 if (p.a_red and p.b_red) else 5)


@pytest.mark.parametrize("name", list(G.C_PATTERNS))
def test_batched_engine_patterns_in_f32(dev, tmp_path, name):
    """the same patterns on the exact-f32 kernel (batch through blockIdx.z)"""
    p = G.c_problem(name, torch.float32)
    with _Planned(-1, 0):
        got, seen = _launch(p, dev, tmp_path)
    assert seen == -1
    _check(p, got, p.name)


@pytest.mark.parametrize("name", list(G.C_V7))
def test_batched_engine_patterns_on_the_256_tile_kernel(dev, tmp_path, name):
    """the same patterns where cfg 11 is legal: batch through blockIdx.z, whole tiles and the spatial tail per batch"""
    sizes, cus = G.C_V7[name]
    _pinned(G.c_problem(name, H16[len(name) % 2], sizes), dev, tmp_path, 11, cus)
