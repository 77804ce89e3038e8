"""CPU: tests/skinny_ref.py checked against itself and against the sources -- the trip model partitions K, the edge list holds
every kind of edge, the form table equals what the launchers' MK_LAUNCH lines and selection rules say (and stops doing so when
a template argument is edited), every census the GPU test launches meets its exactness conditions and sharpness caps, the
exact sum equals a second formulation in integers, and mutations of the trip model (a dropped, doubled, skipped or late K
block) move the expected output bits in every 16-row tile: the sharpness of tests/test_skinny_edges_gpu.py, shown without
running a broken kernel."""
import shutil

import pytest
import torch

import mxfp4_ref
import skinny_ref as R

FORM_IDS = [f.name.replace(" ", "_") for f in R.FORMS]


def _trips(form, w, nkb):
    return len(R.blocks(form, w, nkb))


# ------------------------------------------------------------------------------------------------ trip model --
@pytest.mark.parametrize("form", R.FORMS, ids=FORM_IDS)
def test_blocks_partition_k_exactly_once(form):
    for nkb in range(1, 2 * max(R.edges(form, 1)) + 1):
        got = sorted(b for w in range(form.NW) for trip in R.blocks(form, w, nkb) for b in trip)
        assert got == list(range(nkb)), (form.name, nkb)
        for w in range(form.NW):
            for trip in R.blocks(form, w, nkb):
                assert 1 <= len(trip) <= form.U and all(b % form.NW == w for b in trip)


@pytest.mark.parametrize("form", R.FORMS, ids=FORM_IDS)
def test_edges_hold_every_kind_of_edge(form):
    ed = R.edges(form, 1 if form.mmax == 16 else 17)
    lim = R.nkb_reach(form, 1)
    assert ed == sorted(set(ed)) and ed[0] == 1 and ed[-1] <= lim
    assert any(any(not R.blocks(form, w, n) for w in range(form.NW)) for n in ed)          # a wave without a block
    if form.U == 2:                                                                         # a clamped, skipped u = 1 block
        assert any(any(len(trip) == 1 for w in range(form.NW) for trip in R.blocks(form, w, n)) for n in ed)
    for want in (form.NBUF - 1, form.NBUF, form.NBUF + 1, 2 * form.NBUF + 1):              # the ring fills, wraps, wraps twice
        if want >= 1 and (want - 1) * form.NW * form.U + 1 <= lim:
            assert any(_trips(form, 0, n) == want and _trips(form, form.NW - 1, n) == want - 1 for n in ed), (form.name, want)
    for n in (form.NW - 1, form.NW + 1, form.NW * form.U - 1, form.NW * form.U + 1):
        assert n in ed or n > lim or n < 1
    if form.wide:
        assert R.WIDE_K // form.kblk in R.edges(form, 3)
    # the lists the issue names
    if (form.NW, form.U, form.NBUF) == (8, 2, 3) and form.fmt != "mxfp4":
        assert R.edges(form, 3)[-1] == 105
    if (form.NW, form.U, form.NBUF) == (8, 1, 4):
        assert R.edges(form, 3)[-1] == 65


def test_census_runs_stay_inside_every_entry_point_domain():
    for form in R.FORMS:
        for M, N, nkbs in R.census_runs(form):
            assert nkbs and 1 <= M <= form.mmax
            for nkb in nkbs:
                K = nkb * form.kblk
                if form.PRO:
                    assert R.prologue_fits(M, K), (form.name, M, nkb)
                if form.reach == "decode" and form.mmax == 16:
                    assert R.wide(N, K) == form.wide, (form.name, N, K)
    assert R.prologue_fits(3, 6818) and not R.prologue_fits(3, 6819)
    assert R.prologue_fits(16, 1216) and not R.prologue_fits(16, 1280)


# ------------------------------------------------------------------------------------------------ source pin --
def _pin(csrc):
    """the mismatches between the form table and the sources under csrc"""
    bad = []
    table = R.launch_table(csrc)
    claimed = {}
    for form in R.FORMS:
        for site in form.sites:
            claimed.setdefault(site, []).append(form)
    for site in sorted(set(table) | set(claimed)):
        if site not in table or site not in claimed:
            bad.append(f"{site}: in the {'table' if site in claimed else 'source'} only")
            continue
        kernel, args, threads, wrows, kblk = table[site]
        for form in claimed[site]:
            got = (kernel, threads, wrows, kblk) + tuple(args[k] for k in sorted(args))
            want = (form.kernel, 64 * form.NW, form.wrows, form.kblk) + tuple(getattr(form, k) for k in sorted(args))
            if got != want:
                bad.append(f"{site} / {form.name}: source {got}, table {want}")
    r = R.source_rules(csrc)
    want = {"wide_n": R.WIDE_N, "wide_k": R.WIDE_K, "lds_bytes": R.LDS_BYTES, "mmax": (16, 32),
            "skinny32": (R.SKINNY32_N, 22, 19), "mk_gemm": (R.WIDE_N, R.WIDE_K, 18, 17),
            "forced": ((12, 19, 22), (13, 17, 18)), "cfg12_loop": True}
    bad += [f"rule {k}: source {r[k]}, table {want[k]}" for k in want if r[k] != want[k]]
    return bad


def test_form_table_equals_the_launchers_and_rules():
    assert _pin(R.CSRC) == []
    assert len(R.launch_table()) == 26
    assert R.skinny32_cfg(8191) == 19 and R.skinny32_cfg(8192) == 22
    assert R.wide(4096, 4096) and not R.wide(4097, 64) and not R.wide(33, 4160)


@pytest.mark.parametrize("fname,old,new", [
    ("gemm_impl.inc", "gemm_skinny16_kernel<8, 2, 1, 3>", "gemm_skinny16_kernel<8, 2, 1, 4>"),
    ("gemm_impl.inc", "gemm_skinny32p_kernel<8, 1, 3>", "gemm_skinny32p_kernel<8, 2, 2>"),
    ("gemm_impl.inc", "template <int NW, int U, int PRO, int NBUF = 2, int MT = 1>", "template <int NW, int U, int PRO, int NBUF = 3, int MT = 1>"),
    ("decode_fp8_impl.inc", "decode_linear_fp8_kernel<16, 2, 0>), g16, dim3(1024)", "decode_linear_fp8_kernel<8, 2, 0>), g16, dim3(512)"),
    ("decode_mxfp4_impl.inc", "decode_linear_mxfp4_kernel<8, 1, 0, 4>", "decode_linear_mxfp4_kernel<8, 2, 0, 3>"),
    ("common.h", "K <= 4096;", "K <= 8192;"),
    ("gemm.hip", "return N >= 8192 ? 22 : 19;", "return N >= 4096 ? 22 : 19;"),
])
def test_the_pin_fails_when_the_source_is_retuned(tmp_path, fname, old, new):
    csrc = tmp_path / "csrc"
    shutil.copytree(R.CSRC, csrc, ignore=shutil.ignore_patterns("_obj"))
    text = (csrc / fname).read_text()
    assert text.count(old) == 1, old
    (csrc / fname).write_text(text.replace(old, new))
    assert _pin(str(csrc)) != []


# ------------------------------------------------------------------------------------------------- the census --
@pytest.mark.parametrize("dtype", R.H16, ids=["bf16", "f16"])
@pytest.mark.parametrize("form", R.FORMS, ids=FORM_IDS)
def test_every_census_the_gpu_test_launches_meets_its_conditions(form, dtype):
    for M, N, nkbs in R.census_runs(form):
        c = R.census(form.name, dtype, M, N, max(nkbs))
        figs = c.check()
        print(f"{form.name} {dtype} M={M} N={N} K={c.K}: {figs}")


@pytest.mark.parametrize("dtype", R.H16, ids=["bf16", "f16"])
@pytest.mark.parametrize("name", ["e16 wide pro0", "fp8 wide pro1", "mxfp4 wide pro2", "mxfp4 two tiles", "e16 cfg12"])
def test_exact_sum_equals_an_integer_formulation_and_the_stored_weights(name, dtype):
    """the exact result recomputed in int64 from the operands as the kernel gets them, de-quantised by the formats' own
    restatements: independent of Census.partials and of its f32 arithmetic"""
    form = R.BY_NAME[name]
    M = 17 if form.mmax == 32 and form.reach == "decode" else 3
    c = R.census(name, dtype, M, None, None)
    if form.fmt == "e16":
        W = c.weights["W"].double()
    elif form.fmt == "fp8":
        W = c.weights["Wq"].view(R.FP8).double()
    else:
        W = mxfp4_ref.dequant(c.weights["q"], c.weights["e"]).double()
    assert torch.equal(W.float(), c.weff)
    if form.PRO == 0:
        tok, q = c.x.double(), 1
    elif form.PRO == 1:
        x = c.x.double()
        rstd = 1 / torch.sqrt((x * x).mean(1, keepdim=True) + R.EPS)
        tok, q = c.norm_w.double() * (x * rstd).float().to(dtype).double(), 4
    else:
        g, up = c.x[0].double(), c.x[1].double()
        tok, q = ((g / (1 + torch.exp(-g))).float().to(dtype).double() * up).float().to(dtype).double(), None
    for nkb in sorted({1, c.nkb // 2, c.nkb}):
        K = nkb * form.kblk
        if q is None:                                           # SwiGLU: s_m times an integer sum
            ti = torch.round(tok[:, :K] / c.s_row[:, None]).long()
            assert torch.equal(ti.double() * c.s_row[:, None], tok[:, :K])
            want = (ti @ torch.round(W[:, :K] * 2).long().t()).double() * c.s_row[:, None] / 2
        else:
            want = (torch.round(tok[:, :K] * q).long() @ torch.round(W[:, :K] * 2).long().t()).double() / (2 * q)
        assert torch.equal(c.exact(nkb), want)
        assert torch.equal(c.by_trips(nkb), want)


# --------------------------------------------------------------------------------------------------- sharpness --
def _drop(form, w, nkb):                                        # wave 1's (or 0's) last trip loses its first block
    t = R.blocks(form, w, nkb)
    if w == min(1, nkb - 1):
        t[-1] = t[-1][1:]
    return t


def _double(form, w, nkb):                                      # ... multiplies it twice
    t = R.blocks(form, w, nkb)
    if w == min(1, nkb - 1):
        t[-1] = t[-1] + t[-1][:1]
    return t


def _skip_u1(form, w, nkb):                                     # the u = 1 block of wave 0's first trip is taken for clamped
    t = R.blocks(form, w, nkb)
    if w == 0 and len(t[0]) == 2:
        t[0] = t[0][:1]
    return t


def _late(form, w, nkb):                                        # the last wave with a block starts one block late
    t = R.blocks(form, w, nkb)
    if w == min(form.NW, nkb) - 1:
        t[0] = t[0][1:]
    return t


MUTATIONS = {"drop": _drop, "double": _double, "skip_u1": _skip_u1, "late": _late}


@pytest.mark.parametrize("dtype", R.H16, ids=["bf16", "f16"])
@pytest.mark.parametrize("name", ["e16 wide pro0", "e16 narrow pro1", "fp8 wide pro2", "mxfp4 wide pro1", "mxfp4 narrow pro0",
                                  "fp8 two tiles", "e16 cfg22 32 x 32", "e16 cfg12"])
def test_mutations_of_the_trip_model_move_output_bits_in_every_tile(name, dtype):
    """a K block dropped, multiplied twice, skipped as if clamped, or lost to a late start: under the cancelling residual
    every tile of weight rows then holds an output whose BITS differ from the expectation -- at every edge, for M = 3 (and
    17 for the forms that start there)."""
    form = R.BY_NAME[name]
    M = 17 if form.mmax == 32 and form.reach == "decode" else 3
    c = R.census(name, dtype, M, None, None)
    tiles = -(-c.N // form.wrows)
    pad = tiles * form.wrows - c.N
    total = 0
    for nkb in R.edges(form, M):
        v = c.exact(nkb) * c.oscale
        res = R.residual(v, dtype, nkb)
        want = R.bits16(R.expected(v, dtype, res))
        for what, fn in MUTATIONS.items():
            if fn(form, 0, nkb) == R.blocks(form, 0, nkb) and all(fn(form, w, nkb) == R.blocks(form, w, nkb) for w in range(form.NW)):
                continue                                        # (no u = 1 block at this nkb)
            vm = c.by_trips(nkb, fn) * c.oscale
            moved = R.bits16(R.expected(vm, dtype, res)) != want
            moved = torch.cat((moved, torch.zeros(M, pad, dtype=torch.bool)), 1).view(M, tiles, form.wrows)
            assert bool(moved.any(2).any(0).all()), (name, nkb, what)
            total += 1
    print(f"{name} {dtype}: {total} mutations, every tile moved")


@pytest.mark.parametrize("dtype", R.H16, ids=["bf16", "f16"])
def test_a_clamped_token_lane_feeds_no_stored_output(dtype):
    """The MFMA's token operand is its N dimension: token lane j contributes to output column j alone, and columns >= M are
    not stored.  Which row a CLAMPED lane (r16 >= M) reads -- M - 1 as written, or row M by an off-by-one -- therefore cannot
    move a stored output: that mutation is invisible to every output comparison (it can only read out of bounds), and the
    GPU test is no check of it.  Shown here on the model with a NaN row M, so that nobody takes it for one."""
    form = R.BY_NAME["e16 wide pro0"]
    c = R.census(form.name, dtype, 3, None, None)
    x = torch.cat((c.tok, torch.full((1, c.K), float("nan"))), 0)           # row M exists and holds NaN
    for clamp_to in (c.M - 1, c.M):
        lanes = x[[min(j, clamp_to) for j in range(16)]].double()            # the 16 token lanes of the MFMA
        d = lanes @ c.weff.double().t()                                      # D[j][n]
        assert torch.equal(d[:c.M], c.exact(c.nkb))                          # stored: j < M
