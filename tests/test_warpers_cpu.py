"""CPU: the four warpers behind top-p -- min_p, typical_p, epsilon_cutoff, eta_cutoff (rule 6 next to mk_sample_rows in
include/macaw_hip.h).  The float64 reference of tests/warpers_ref.py against transformers' MinPLogitsWarper,
TypicalLogitsWarper, EpsilonLogitsWarper and EtaLogitsWarper chained in HF's order behind top-k and top-p; designed rows
held exactly; the leave-out condition of the GPU test (tests/test_warpers_gpu.py) checked on the reference alone; the
three new C entries and their bad-argument codes; the arguments of generate() / MM_LLMs.set_sampling that need no
device."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import warpers_ref as R
from test_sampling_cpu import filter_row

# (temperature, top_k, top_p, min_p, typical_p, epsilon_cutoff, eta_cutoff)
HF_TUPLES = [(1.0, 0, 1.0, .05, 1.0, 0.0, 0.0),
             (1.0, 0, 1.0, 0.0, .9, 0.0, 0.0),
             (1.0, 0, 1.0, 0.0, .2, 0.0, 0.0),                       # drops the maximum
             (1.0, 0, 1.0, 0.0, 1.0, 3e-3, 0.0),
             (1.0, 0, 1.0, 0.0, 1.0, 0.0, 2e-3),
             (1.0, 0, 1.0, 0.0, 1.0, .9, 0.0),                       # falls back to the maximum
             (1.0, 0, 1.0, 0.0, 1.0, 0.0, .9),                       # falls back to the maximum
             (.8, 40, .95, .02, .9, 1e-2, 0.0),
             (1.3, 0, .9, .01, .95, 3e-3, 2e-3),
             (.7, 50, 1.0, .1, .5, 0.0, 5e-2)]


def _hf_kept(lg, T, k, p, min_p, typ, eps, eta):
    tg = pytest.importorskip("transformers.generation.logits_process")
    scores = torch.from_numpy(lg) / T
    chain = [(k, lambda: tg.TopKLogitsWarper(top_k=k)), (p < 1, lambda: tg.TopPLogitsWarper(top_p=p)),
             (min_p > 0, lambda: tg.MinPLogitsWarper(min_p=min_p)), (typ < 1, lambda: tg.TypicalLogitsWarper(mass=typ)),
             (eps > 0, lambda: tg.EpsilonLogitsWarper(epsilon=eps)), (eta > 0, lambda: tg.EtaLogitsWarper(epsilon=eta))]
    for on, make in chain:
        if on:
            scores = make()(None, scores)
    return torch.isfinite(scores).numpy()


@pytest.mark.parametrize("tup", HF_TUPLES, ids=[str(i) for i in range(len(HF_TUPLES))])
def test_reference_agrees_with_the_transformers_warpers(tup):
    """180 rows: V = 997 and 5, sigma 1 to 3, three rows each, ten tuples.  A row without an undecided column must give
    HF's kept set exactly; with one (HF's fp32 softmax a rounding error from a threshold) HF's set is an alternative."""
    exact = dropped_max = fell_back = 0
    for V in (997, 5):
        for sigma in (1.0, 2.0, 3.0):
            lg = (torch.randn(3, V, generator=torch.Generator().manual_seed(int(10 * sigma) + V)) * sigma).numpy()
            hf = _hf_kept(lg, *tup)
            for r in range(3):
                w = R.warp_row(lg[r], V, *tup)
                if not w["undecided"]:
                    assert np.array_equal(w["kept"], hf[r]), (V, sigma, r)
                    exact += 1
                else:
                    assert w["alternatives"] is not None and any(np.array_equal(a, hf[r]) for a in w["alternatives"])
                dropped_max += not w["kept"][int(np.argmax(lg[r]))]
                fell_back += int(w["kept"].sum()) == 1
    assert exact >= 12                                                # of 18: the exact comparison is the rule
    if tup[4] == .2:
        assert dropped_max > 0
    if tup[5] == .9:
        assert fell_back == 18                                        # (a maximum of probability >= 0.9 stays alone too)
    if tup[6] == .9:
        assert fell_back > 0                                          # where the entropy is low: min(eta, ...) = eta


def test_designed_rows_are_held_exactly():
    row = np.log(np.array([.4, .15, .15, .15, .15])).astype(np.float32)
    w = R.warp_row(row, 5, typical_p=0.5)
    assert np.nonzero(w["kept"])[0].tolist() == [1, 2, 3, 4]          # a band: the maximum goes, the tie group whole
    tie = np.array([5, 3, 3, 3, 1], dtype=np.float32)
    w = R.warp_row(tie, 5, min_p=float(np.exp(-2.5)))
    assert np.nonzero(w["kept"])[0].tolist() == [0, 1, 2, 3]
    w = R.warp_row(np.array([1, 7, 2, 7, 7, 0], dtype=np.float32), 6, min_p=1.0)
    assert np.nonzero(w["kept"])[0].tolist() == [1, 3, 4]             # the tie group of the maximum
    # every stage keeps at least one column, and epsilon / eta fall back to the whole tie group of the maximum
    for kw in (dict(epsilon_cutoff=.9), dict(eta_cutoff=.9)):
        w = R.warp_row(np.array([0, 2, 2, 1], dtype=np.float32), 4, **kw)
        assert np.nonzero(w["kept"])[0].tolist() == [1, 2]
    # all off: filter_row's kept set, no stage, one alternative
    lg = (torch.randn(300, generator=torch.Generator().manual_seed(5)) * 3).numpy()
    w = R.warp_row(lg, 300, .8, 40, 1.0)
    assert np.array_equal(w["kept"], filter_row(lg, 300, .8, 40, 1.0)["kept"]) and len(w["alternatives"]) == 1
    assert R.warp_row(np.array([-np.inf, np.nan], dtype=np.float32), 2, min_p=.1) is None
    # NaN and -inf never survive a stage
    bad = np.array([np.nan, -np.inf, 0.5, np.nan, 0.25, -np.inf, 0.0], dtype=np.float32)
    for tup in R.TUPLES:
        assert not R.warp_row(bad, 7, *tup)["kept"][[0, 1, 3, 5]].any()


def test_few_rows_of_the_gpu_fixtures_are_left_out():
    """the condition under which tests/test_warpers_gpu.py may leave a row out, on the reference alone: at most a
    quarter of a case's rows and at most 2 % of all rows have more than 4 undecided columns"""
    per_case = []
    for V, rows, ld in R.SHAPES:
        for sigma in R.SIGMAS:
            for dtype in R.DTYPES:
                for tup in R.TUPLES:
                    res = R.case(V, rows, ld, sigma, dtype, tup)
                    per_case.append((sum(alts is None for _, alts, _ in res), rows))
    ok, figures = R.left_out_ok(per_case)
    print("left out: %d of %d rows, worst case %.3f" % figures)
    assert ok, figures


# --------------------------------------------------------------------------------------------------------- ABI --
def test_abi_has_the_three_entries_and_refuses_bad_arguments():
    from macaw_llm_amd import build, lib as L
    build.build()
    lib = L.load()
    assert lib.mk_abi_version() == 11 and L.ABI_VERSION == 11
    for name in ("mk_sample_rows_warp", "mk_decode_emit_sample_warp", "mk_sample_keep_rows"):
        assert hasattr(lib, name) and name in L.SIGNATURES
    buf = (C.c_char * 64)()
    p = C.addressof(buf)                                             # never dereferenced: every call is refused first
    off = dict(mp=0.0, ty=1.0, ep=0.0, et=0.0)

    def rows(logits=p, ld=8, V=8, T=1.0, k=0, tp=1.0, out=p, dtype=1, **w):
        w = {**off, **w}
        return lib.mk_sample_rows_warp(logits, ld, 1, V, T, k, tp, w["mp"], w["ty"], w["ep"], w["et"], 0, 0, out, dtype,
                                       None)

    def emit(logits=p, ld=8, V=8, T=1.0, k=0, tp=1.0, out=p, dtype=1, **w):
        w = {**off, **w}
        return lib.mk_decode_emit_sample_warp(logits, ld, V, 1, 0, 2, p, p, out, 4, p, T, k, tp, w["mp"], w["ty"],
                                              w["ep"], w["et"], 0, dtype, None)

    def keep(logits=p, ld=8, V=8, T=1.0, k=0, tp=1.0, out=p, dtype=1, keep_ld=8, **w):
        w = {**off, **w}
        return lib.mk_sample_keep_rows(logits, ld, 1, V, T, k, tp, w["mp"], w["ty"], w["ep"], w["et"], out, keep_ld,
                                       dtype, None)

    nan, inf = float("nan"), float("inf")
    for f in (rows, emit, keep):
        assert f(logits=None) == -1 and f(out=None) == -1 and f(V=0) == -1 and f(ld=7) == -1
        assert f(T=0.0) == -1 and f(tp=0.0) == -1 and f(k=-1) == -1   # the old arguments, as in the old entries
        for bad in (dict(mp=-.1), dict(mp=1.0001), dict(mp=nan), dict(mp=inf),
                    dict(ty=0.0), dict(ty=-.5), dict(ty=1.0001), dict(ty=nan), dict(ty=inf),
                    dict(ep=-.1), dict(ep=1.0), dict(ep=nan), dict(ep=inf),
                    dict(et=-.1), dict(et=1.0), dict(et=nan), dict(et=inf)):
            assert f(**bad) == -1, (f.__name__, bad)
        assert f(dtype=7) == -2                                       # MK_ERR_UNSUPPORTED, after the argument checks
        assert f(dtype=7, mp=1.0, ty=.5, ep=.999, et=.999) == -2      # the ends of the ranges are inside
    assert keep(keep_ld=7) == -1
    # the old two entries take their old arguments
    assert lib.mk_sample_rows(p, 8, 1, 8, 1.0, 0, 1.0, 0, 0, p, 7, None) == -2
    assert lib.mk_decode_emit_sample(p, 8, 8, 1, 0, 2, p, p, p, 4, p, 1.0, 0, 1.0, 0, 7, None) == -2
    assert lib.mk_sample_rows(p, 8, 1, 8, 1.0, 0, 1.5, 0, 0, p, 1, None) == -1


# ------------------------------------------------------------------------------------------------------ Python --
NAMES = ("min_p", "typical_p", "epsilon_cutoff", "eta_cutoff")


def test_generate_and_set_sampling_name_the_four_and_validate():
    from macaw_llm_amd import modeling as Mo
    from macaw_llm_amd import ops
    for fn in (Mo.LlamaForCausalLM.generate, Mo.MM_LLMs.set_sampling):
        sig = inspect.signature(fn).parameters
        assert [sig[n].default for n in NAMES] == [None, 1.0, 0.0, 0.0]
    for fn in (ops.sample_rows_warp, ops.decode_emit_sample_warp, ops.sample_keep_rows):
        sig = inspect.signature(fn).parameters
        assert [sig[n].default for n in NAMES] == [0.0, 1.0, 0.0, 0.0]
    for fn in (ops.sample_rows, ops.decode_emit_sample):             # the old two as they were: launch traces bind to them
        assert not set(NAMES) & set(inspect.signature(fn).parameters)
    try:
        Mo.MM_LLMs.set_sampling(True, 0.7, None, 0.9, 5, min_p=.05, eta_cutoff=1e-3)
        assert Mo.SAMPLING[0] == dict(do_sample=True, temperature=0.7, top_k=None, top_p=0.9, seed=5)   # the five keys
        assert Mo.SAMPLING_WARPERS[0] == dict(min_p=.05, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=1e-3)
        nan, inf = float("nan"), float("inf")
        for name, bads in (("min_p", (-.1, 1.5, nan, inf, True)), ("typical_p", (0.0, 1.5, nan, inf, True, None)),
                           ("epsilon_cutoff", (-.1, 1.0, nan, inf, False, None)),
                           ("eta_cutoff", (-.1, 1.0, nan, inf, False, None))):
            for bad in bads:
                with pytest.raises(ValueError, match=name):
                    Mo.MM_LLMs.set_sampling(True, **{name: bad})
                with pytest.raises(ValueError, match=name):
                    Mo._warpers_check("generate", **{**dict(min_p=None, typical_p=1.0, epsilon_cutoff=0.0,
                                                            eta_cutoff=0.0), name: bad})
        Mo.MM_LLMs.set_sampling(False, min_p=7.0, typical_p=-1.0)    # ignored without do_sample
        assert Mo._warpers_check("generate", None, 1.0, 0.0, 0.0) == ()       # all off: the 4-tuple stays
        assert Mo._warpers_check("generate", 0, 1, 0, 0) == ()
        assert Mo._warpers_check("generate", .1, 1.0, 0.0, 0.0) == (.1, 1.0, 0.0, 0.0)
    finally:
        Mo.MM_LLMs.set_sampling()
    assert Mo.SAMPLING[0]["do_sample"] is False and Mo.SAMPLING_WARPERS[0]["min_p"] is None
