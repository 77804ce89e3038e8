"""mk_gemm_grouped (include/macaw_hip.h): one launch of whole 256 x 256 v9 tiles of a grad-input GEMM and the grad-weight GEMMs
queued behind it, on one persistent workgroup per planned CU.

Everything runs with mk_gemm_set_cus(8), so a round is 8 tiles (one case repeats the method at 16, 24 and 12).  For every case
  * the problems come from tests/gemm_cases.py (`single`: seeded inputs rounded on the CPU, C pitched wider than N and NaN
    everywhere -- the NaN is the sentinel for "not written")
  * the grouped result is compared BIT FOR BIT with the same problem run alone through mk_gemm with configuration 15 forced
    under the same 8 planned CUs (its partial round runs as v7 sub-tiles; fewer whole tiles than CUs run on v7 altogether)
  * and against gemm_cases' float64 reference at that file's bound (test_kernels_gpu._close, scale = 0.1 sqrt(K))
  * tiles that a launch reports as not taken keep the sentinel; nothing outside the logical outputs is ever written.
The tile order of a filler is tile_from_index with 8-row groups (csrc/gemm_common.h), restated in `_tile_rc`.
What a balancing launch takes is the planner's rule (csrc/gemm_group_plan.h, checked by tests/test_gemm_group_plan_cpu.py):
main 768 x 768 = 9 tiles on 8 workgroups leaves 7 workgroups one main tile short; a K = 768 filler tile costs 12 + 6.8
K-tiles, a K = 192 main tile 3 + 6.8 (more than half a filler tile: each idle workgroup takes one), a K = 128 main tile
2 + 6.8 (less than half: none is taken)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from macaw_llm_amd import lib as L  # noqa: E402
from macaw_llm_amd import ops  # noqa: E402
from test_kernels_gpu import _close  # noqa: E402
import gemm_cases as G  # noqa: E402

H16 = [torch.bfloat16, torch.float16]
CUS = 8
FILL_K = 768
FILL_SHAPES = {4: (512, 512), 5: (256, 1280), 27: (768, 2304)}     # tiles -> (M, N) of a grad-weight problem
_PROBLEMS, _ALONE = {}, {}


def _bits(t):
    return t.reshape(-1).view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _problem(dtype, M, N, K, a_red, epilogue="plain", seed=0):
    key = (dtype, M, N, K, a_red, epilogue, seed)
    if key not in _PROBLEMS:
        _PROBLEMS[key] = G.single(dtype, M, N, K, a_red, True, epilogue, seed=seed)
    return _PROBLEMS[key]


def _main(dtype, K, M=768, N=768):
    return _problem(dtype, M, N, K, False)


def _filler(dtype, tiles, seed=0):
    return _problem(dtype, *FILL_SHAPES[tiles], FILL_K, True, seed=seed)


class _Dev:
    """a problem's buffers on the device and its descriptor"""

    def __init__(self, p, dev):
        self.p = p
        self.t = {k: (getattr(p, k).to(dev) if getattr(p, k) is not None else None) for k in ("A", "B", "C", "R", "bias")}
        self.d = ops.gemm_desc(self.t["A"], self.t["B"], self.t["C"], p.M, p.N, p.K, p.lda, p.ldb, p.ldc, R=self.t["R"],
                               bias=self.t["bias"], **p.gemm_args())

    def c(self):
        return self.t["C"].cpu().reshape(-1)


def _alone(p, dev):
    """flat C of the problem run alone: mk_gemm, configuration 15 forced, under the planned CUs (computed once per problem)"""
    if id(p) not in _ALONE:      # (whatever CU count is planned at that moment: the result does not depend on it)
        lib = L.load()
        dv = _Dev(p, dev)
        lib.mk_gemm_set_cfg(15)
        try:
            L.check(lib.mk_gemm(C.byref(dv.d), torch.cuda.current_stream().cuda_stream), "mk_gemm")
        finally:
            lib.mk_gemm_set_cfg(-1)
        _ALONE[id(p)] = dv.c()
    return _ALONE[id(p)]


def _grouped(main, fills, firsts, drain):
    """-> (return code, tiles taken per filler)"""
    lib = L.load()
    arr = (L.GroupFill * max(len(fills), 1))()
    for f, dv, first in zip(arr, fills, firsts):
        f.d, f.first_tile, f.taken = dv.d, first, -7
    rc = lib.mk_gemm_grouped(C.byref(main.d) if main is not None else None, arr, len(fills), int(drain),
                             torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, [arr[i].taken for i in range(len(fills))]


def _tile_rc(i, tiles_m, tiles_n):
    per = 8 * tiles_n
    grp = i // per
    first_m = grp * 8
    gsize = min(tiles_m - first_m, 8)
    in_g = i - grp * per
    return first_m + in_g % gsize, in_g // gsize


def _written(p, done):
    """mask over the flat C: the elements of the first `done` tiles of p's tile order"""
    m = torch.zeros((p.M, p.ldc), dtype=torch.bool)
    for i in range(done):
        r, c = _tile_rc(i, p.M // 256, p.N // 256)
        m[256 * r:256 * r + 256, 256 * c:256 * c + 256] = True
    return m.reshape(-1)


def _check(dv, dev, done, what):
    """the first `done` tiles equal the problem run alone, bit for bit, and meet the float64 bound; every other element of C
    still holds what it held before"""
    p = dv.p
    got, alone, mask = dv.c(), _alone(p, dev), _written(p, done)
    assert torch.equal(_bits(got)[mask], _bits(alone)[mask]), f"{what}: differs from mk_gemm cfg 15"
    assert torch.equal(_bits(got)[~mask], _bits(p.C.reshape(-1))[~mask]), f"{what}: wrote outside the tiles it reported"
    if done == (p.M // 256) * (p.N // 256):
        idx, ref = p.reference()
        print(f"{what}: max|err| {(got[idx].double() - ref).abs().max().item():.3e}  max|ref| {ref.abs().max().item():.3e}")
        _close(got[idx], ref, p.dtype, scale=p.scale, what=what)


@pytest.fixture(autouse=True)
def _eight_cus():
    lib = L.load()
    lib.mk_gemm_set_cus(CUS)
    yield
    lib.mk_gemm_set_cus(0)
    lib.mk_gemm_set_cfg(-1)


@pytest.mark.parametrize("dtype", H16, ids=["bf16", "f16"])
@pytest.mark.parametrize("k_main", [128, 192])
@pytest.mark.parametrize("tiles", [4, 5, 27])
def test_filler_behind_a_partial_round_then_the_rest_in_a_second_launch(dev, dtype, k_main, tiles):
    """9 main tiles on 8 workgroups.  Launch 1 balances: with K = 192 each of the 7 idle workgroups takes one filler tile (all
    of them when only 4 or 5 are queued: fewer fillers than idle workgroups), with K = 128 none does.  The remainder is
    reported as not taken and untouched.  Launch 2 has no main problem and drains the filler from its first-tile offset; both
    launches together equal the filler run alone."""
    main, fill = _Dev(_main(dtype, k_main), dev), _Dev(_filler(dtype, tiles), dev)
    rc, (t1,) = _grouped(main, [fill], [0], False)
    assert rc == 0
    assert t1 == (min(tiles, 7) if k_main == 192 else 0)
    _check(main, dev, 9, f"main K={k_main} {dtype}")
    _check(fill, dev, t1, f"filler {tiles} tiles after launch 1")
    rc, (t2,) = _grouped(None, [fill], [t1], True)
    assert rc == 0 and t1 + t2 == tiles
    _check(fill, dev, tiles, f"filler {tiles} tiles after launch 2 (offset {t1})")


@pytest.mark.parametrize("dtype", H16, ids=["bf16", "f16"])
def test_whole_rounds_of_main_tiles_take_no_filler_unless_drained(dev, dtype):
    main, fill = _Dev(_main(dtype, 128, 1024, 1024), dev), _Dev(_filler(dtype, 5), dev)
    rc, taken = _grouped(main, [fill], [0], False)
    assert rc == 0 and taken == [0]
    _check(main, dev, 16, "16 main tiles")
    _check(fill, dev, 0, "untouched filler")
    main2 = _Dev(main.p, dev)
    rc, taken = _grouped(main2, [fill], [0], True)
    assert rc == 0 and taken == [5]
    _check(main2, dev, 16, "16 main tiles, drain")
    _check(fill, dev, 5, "drained filler")


@pytest.mark.parametrize("dtype", H16, ids=["bf16", "f16"])
def test_drain_runs_every_queued_problem_and_the_profile_counts_the_tiles(dev, dtype, tmp_path):
    """main + two fillers (5 and 27 tiles, the second partly done: offset 3) with drain: everything is taken.  The in-library
    profile shows ONE kind-0 launch with configuration id 16 and the FLOPs of the executed tiles."""
    import csv
    main = _Dev(_main(dtype, 192), dev)
    f5, f27 = _Dev(_filler(dtype, 5, seed=1), dev), _Dev(_filler(dtype, 27), dev)
    rc, first = _grouped(None, [f27], [0], False)        # no main, no drain: whole rounds of the queue = 24 of 27
    assert rc == 0 and first == [24]
    _check(f27, dev, 24, "filler only, whole rounds")
    path = str(tmp_path / "prof.csv")
    ops.prof_begin()
    try:
        rc, taken = _grouped(main, [f5, f27], [0, 24], True)
        ops.prof_report(path)
    finally:
        ms, flops, launches = ops.prof_end()
    assert rc == 0 and taken == [5, 3]
    assert launches == 1 and flops == 2.0 * 256 * 256 * (9 * 192 + 8 * FILL_K)
    with open(path) as f:
        rows = [r for r in csv.DictReader(f) if r["kind"] == "gemm"]
    assert len(rows) == 1 and int(rows[0]["cfg"]) == 16 and int(rows[0]["launches"]) == 1, rows
    assert (int(rows[0]["M"]), int(rows[0]["N"]), int(rows[0]["K"]), int(rows[0]["layout"])) == (768, 768, 192, 1)
    _check(main, dev, 9, "main")
    _check(f5, dev, 5, "first filler")
    _check(f27, dev, 27, "second filler, 24 + 3")


# 8 planned CUs make every XCD group of workgroups ONE workgroup wide, where the round-by-round dealing of a group's span
# (csrc/gemm_v9_impl.inc GrpCursor: ballot over the members' counts, the mask of the members before this one, the advance
# of the round's base) is the same as one contiguous run.  16 and 24 planned CUs have groups of 2 and 3 members; 12 is no
# multiple of 8: rank = workgroup index and ONE short group of 12.  A tile that the device dealt twice or not at all
# shows as a sentinel left in a taken tile, or as a write into a tile reported as not taken.
@pytest.mark.parametrize("cus", [16, 24, 12])
@pytest.mark.parametrize("dtype", H16, ids=["bf16", "f16"])
def test_groups_of_several_workgroups_deal_their_span_round_by_round(dev, dtype, cus):
    """main 1280 x 1024 = 20 tiles of K = 192.  16 CUs: 4 workgroups run two main tiles, 12 one -> 12 filler tiles in the
    balancing launch; 24 CUs: 4 workgroups have no main tile -> 4; 12 CUs: 8 run two, 4 one -> 4.  The second launch has a
    9-tile main problem, the rest of the 27-tile filler and a 5-tile one, and drains: unequal counts inside every group."""
    lib = L.load()
    lib.mk_gemm_set_cus(cus)
    main, f27 = _Dev(_main(dtype, 192, 1280, 1024), dev), _Dev(_filler(dtype, 27), dev)
    rc, (t1,) = _grouped(main, [f27], [0], False)
    assert rc == 0 and t1 == {16: 12, 24: 4, 12: 4}[cus]
    _check(main, dev, 20, f"20 main tiles, {cus} CUs")
    _check(f27, dev, t1, f"27-tile filler after the balancing launch, {cus} CUs")
    main2, f5 = _Dev(_main(dtype, 192), dev), _Dev(_filler(dtype, 5, seed=1), dev)
    rc, taken = _grouped(main2, [f27, f5], [t1, 0], True)
    assert rc == 0 and taken == [27 - t1, 5]
    _check(main2, dev, 9, f"9 main tiles, {cus} CUs")
    _check(f27, dev, 27, f"27-tile filler drained from offset {t1}, {cus} CUs")
    _check(f5, dev, 5, f"5-tile filler, {cus} CUs")
    # filler only, whole rounds of the queue: 27 tiles on `cus` workgroups
    g27 = _Dev(f27.p, dev)
    rc, (t3,) = _grouped(None, [g27], [0], False)
    assert rc == 0 and t3 == 27 // cus * cus
    _check(g27, dev, t3, f"filler only, {cus} CUs")


def test_a_member_outside_the_domain_is_not_grouped_and_nothing_is_written(dev):
    bf = torch.bfloat16
    good_main, good_fill = _main(bf, 192), _filler(bf, 5)
    bad = {
        "bias": (_problem(bf, 768, 768, 192, False, "bias"), good_fill),
        "ragged N": (G.single(bf, 768, 760, 192, False, True), good_fill),
        "fp32": (G.single(torch.float32, 768, 768, 192, False, True), good_fill),
        "fp32 filler": (good_main, G.single(torch.float32, 512, 512, FILL_K, True, True)),
        "ragged filler": (good_main, G.single(bf, 500, 512, FILL_K, True, True)),
    }
    for name, (pm, pf) in bad.items():
        main, fill = _Dev(pm, dev), _Dev(pf, dev)
        rc, taken = _grouped(main, [fill], [0], True)
        assert rc == L.NOT_GROUPED and taken == [0], (name, rc, taken)
        for dv in (main, fill):
            assert torch.equal(_bits(dv.c()), _bits(dv.p.C)), f"{name}: a refused launch wrote to C"
    # a first-tile offset past the problem is a bad argument, not a fallback
    main, fill = _Dev(good_main, dev), _Dev(good_fill, dev)
    rc, _ = _grouped(main, [fill], [6], True)
    assert rc == -1
