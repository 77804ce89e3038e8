"""CPU: the reference of sampled decoding (mk_sample_rows / mk_decode_emit_sample, include/macaw_hip.h) as a NumPy float64
restatement of its five rules -- temperature, candidates, top-k with ties to the lower column, top-p by value, the
counter-hash draw -- which tests/test_sampling_gpu.py imports, and tests of that reference itself: against transformers'
TopKLogitsWarper / TopPLogitsWarper where no tie sits at a threshold, top_k = 1 = argmax, the tie rule, the range of u,
and empirical frequencies against the probabilities.  Also the bad-argument codes of the two C entry points and the
argument checks of generate() / MM_LLMs.set_sampling that need no device."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

MASK64 = (1 << 64) - 1


def hash32(seed, idx):
    """mk_hash32 (csrc/common.h) on Python integers, 64-bit wrap-around"""
    z = (idx * 0x9E3779B97F4A7C15 + seed) & MASK64
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & MASK64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & MASK64
    z ^= z >> 31
    return (z >> 16) & 0xFFFFFFFF


def uniform(seed, step, row):
    """rule 5's u in (0, 1): 24 hash bits, centred in their cell"""
    return ((hash32(seed & MASK64, ((step & 0xFFFFFFFF) << 32) | row) >> 8) + 0.5) * 2.0 ** -24


def greedy(logits):
    """torch.argmax order (mk_argmax_better): the first NaN, else the first maximum"""
    nan = np.isnan(logits)
    return int(np.argmax(nan)) if nan.any() else int(np.argmax(logits))


def filter_row(logits, V, temperature=1.0, top_k=0, top_p=1.0, p_slack=0.0):
    """rules 1-4 for one row (any float array, columns [V:] ignored) -> None when the row has no finite logit, else a
    dict: x (fp32 scaled values), kept (bool [V]), e (float64 masses exp(x - x_max), 0 outside the top-k survivors),
    Zk (their sum over the top-k survivors), above (per column the mass strictly above its value among the survivors),
    topk (bool [V], the survivors of rules 2-3).  p_slack relaxes the top-p rule to above < (p + p_slack) * Zk."""
    lg = np.asarray(logits, dtype=np.float32)[:V]
    if not np.isfinite(lg).any():
        return None
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        x = (lg / np.float32(temperature)).astype(np.float32)
    cand = ~np.isnan(lg) & (lg != -np.inf)
    cols = np.nonzero(cand)[0]
    xs = x[cols] + np.float32(0)                                     # -0 -> +0: equal values compare and sort as equal
    surv = cols
    if top_k and 0 < top_k < len(cols):
        order = np.lexsort((cols, -xs.astype(np.float64)))           # value descending, then column ascending
        surv = np.sort(cols[order[:top_k]])
    topk = np.zeros(V, dtype=bool)
    topk[surv] = True
    x64 = x.astype(np.float64)
    xmax = x64[surv].max()
    e = np.zeros(V, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        e[surv] = np.where(x64[surv] == xmax, 1.0, np.exp(x64[surv] - xmax))
    Zk = e[surv].sum()
    vals, inv = np.unique(x64[surv], return_inverse=True)             # ascending
    mass = np.zeros(len(vals))
    np.add.at(mass, inv, e[surv])
    above_v = np.concatenate([np.cumsum(mass[::-1])[::-1][1:], [0.0]])    # mass of the strictly larger values
    above = np.full(V, np.inf)
    above[surv] = above_v[inv]
    kept = topk.copy()
    if top_p < 1.0:
        kept &= above < (float(np.float32(top_p)) + p_slack) * Zk
    return dict(x=x, kept=kept, e=e, Zk=Zk, above=above, topk=topk)


def sample_row(logits, V, temperature=1.0, top_k=0, top_p=1.0, seed=0, step=0, row=0):
    """the token of one row by the five rules"""
    f = filter_row(logits, V, temperature, top_k, top_p)
    if f is None:
        return greedy(np.asarray(logits, dtype=np.float32)[:V])
    kept = np.nonzero(f["kept"])[0]
    cum = np.cumsum(f["e"][kept])
    hit = np.nonzero(cum > uniform(seed, step, row) * cum[-1])[0]
    return int(kept[hit[0]] if len(hit) else kept[-1])


# ------------------------------------------------------------------------------------------ the reference itself --
def _rows(n, V, sigma, seed):
    return (torch.randn(n, V, generator=torch.Generator().manual_seed(seed)) * sigma).numpy()


@pytest.mark.parametrize("T,k,p", [(1.0, 50, 1.0), (0.7, 5, 1.0), (1.0, 0, 0.9), (0.8, 40, 0.95), (1.3, 0, 0.5)])
def test_filters_agree_with_the_transformers_warpers(T, k, p):
    tg = pytest.importorskip("transformers.generation.logits_process")
    lg = _rows(6, 997, 3.0, 1)
    scores = torch.from_numpy(lg) / T
    if k:
        scores = tg.TopKLogitsWarper(top_k=k)(None, scores)
    if p < 1:
        scores = tg.TopPLogitsWarper(top_p=p)(None, scores)
    hf = torch.isfinite(scores).numpy()
    for r in range(lg.shape[0]):
        f = filter_row(lg[r], 997, T, k, p)
        # fp32 softmax + cumsum against float64: skip rows whose top-p threshold is a rounding error away from a column
        if p < 1 and np.abs(f["above"][f["topk"]] - float(np.float32(p)) * f["Zk"]).min() < 1e-4 * f["Zk"]:
            continue
        assert np.array_equal(f["kept"], hf[r]), r


def test_top_k_1_is_argmax_and_ties_go_to_the_lower_column():
    lg = _rows(16, 300, 4.0, 2)
    lg[3, 17] = lg[3, 250] = lg[3].max() + 1                         # duplicated maximum
    for r in range(16):
        for step in range(4):
            assert sample_row(lg[r], 300, 0.6, 1, 1.0, seed=9, step=step, row=r) == int(np.argmax(lg[r]))
    tie = np.array([5, 3, 3, 3, 1], dtype=np.float32)
    f = filter_row(tie, 5, 1.0, 2, 1.0)
    assert f["kept"].tolist() == [True, True, False, False, False]
    f = filter_row(tie, 5, 1.0, 3, 1.0)
    assert f["kept"].tolist() == [True, True, True, False, False]
    assert {sample_row(tie, 5, 1.0, 2, 1.0, seed=1, step=s) for s in range(64)} == {0, 1}
    # top-p keeps or drops a tie group whole, and always keeps the top value
    f = filter_row(tie, 5, 1.0, 0, 1e-6)
    assert f["kept"].tolist() == [True, False, False, False, False]
    f = filter_row(tie, 5, 1.0, 0, 0.9)
    assert f["kept"].tolist() == [True, True, True, True, False]


def test_nan_and_minus_inf_are_never_drawn_and_a_row_without_finite_logits_is_greedy():
    row = np.array([np.nan, -np.inf, 0.5, np.nan, 0.25, -np.inf], dtype=np.float32)
    assert {sample_row(row, 6, 1.0, 0, 1.0, seed=3, step=s) for s in range(200)} == {2, 4}
    assert sample_row(np.array([-np.inf, -np.inf], dtype=np.float32), 2) == 0
    assert sample_row(np.array([-np.inf, np.nan, np.nan], dtype=np.float32), 3) == 1
    assert sample_row(np.array([1.0, 2.0, 1e4], dtype=np.float32), 2, seed=5) in (0, 1)      # columns [V:] are not read


def test_u_lies_strictly_inside_the_unit_interval():
    us = [uniform(s, t, r) for s in (0, 1, 2 ** 63 - 1, MASK64) for t in range(64) for r in range(8)]
    assert 0.0 < min(us) and max(us) < 1.0
    assert uniform(0, 0, 0) != uniform(0, 1, 0) != uniform(0, 0, 1) and uniform(0, 0, 0) != uniform(1, 0, 0)
    assert 0.0 < 0.5 * 2.0 ** -24 and (2 ** 24 - 0.5) * 2.0 ** -24 < 1.0                       # the two extreme cells
    # the hash against the array form the dropout tests use
    with np.errstate(over="ignore"):
        z = np.uint64(7) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(123)
        z ^= z >> np.uint64(30); z *= np.uint64(0xBF58476D1CE4E5B9)
        z ^= z >> np.uint64(27); z *= np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
    assert hash32(123, 7) == int(z >> np.uint64(16)) & 0xFFFFFFFF


def test_empirical_frequencies_match_the_probabilities():
    row = np.array([1.0, 0.0, 2.0, -1.0, 0.5, 1.5], dtype=np.float32)
    n = 20000
    for T, k, p in [(1.0, 0, 1.0), (0.7, 4, 1.0), (1.0, 0, 0.8)]:
        f = filter_row(row, 6, T, k, p)
        prob = np.where(f["kept"], f["e"], 0.0)
        prob /= prob.sum()
        cnt = np.bincount([sample_row(row, 6, T, k, p, seed=11, step=s) for s in range(n)], minlength=6)
        # five standard deviations of a binomial count (a uniform u: P(false alarm) < 1e-5 over all cells)
        assert (np.abs(cnt - n * prob) <= 5 * np.sqrt(n * prob * (1 - prob)) + 1e-9).all(), (T, k, p, cnt, n * prob)
        assert (cnt[~f["kept"]] == 0).all()


# --------------------------------------------------------------------------------------------------------- ABI --
def test_bad_arguments_return_error_codes():
    from macaw_llm_amd import build, lib as L
    build.build()
    lib = L.load()
    buf = (C.c_char * 64)()
    p = C.addressof(buf)                                             # never dereferenced: every call is refused first

    def rows(logits=p, ld=8, n=1, V=8, T=1.0, k=0, tp=1.0, out=p, dtype=1):
        return lib.mk_sample_rows(logits, ld, n, V, T, k, tp, 0, 0, out, dtype, None)

    def emit(logits=p, ld=8, V=8, B=1, tok=p, done=p, out=p, state=p, T=1.0, k=0, tp=1.0, dtype=1):
        return lib.mk_decode_emit_sample(logits, ld, V, B, 0, 2, tok, done, out, 4, state, T, k, tp, 0, dtype, None)

    for f in (rows, emit):
        assert f(logits=None) == -1
        assert f(out=None) == -1
        assert f(V=0) == -1 and f(V=-3) == -1
        assert f(ld=7) == -1
        for T in (0.0, -1.0, float("inf"), float("nan")):
            assert f(T=T) == -1, T
        for tp in (0.0, -0.1, 1.0001, float("nan")):
            assert f(tp=tp) == -1, tp
        assert f(k=-1) == -1
        assert f(dtype=7) == -2                                       # MK_ERR_UNSUPPORTED, after the argument checks
    assert rows(n=0) == -1 and emit(B=0) == -1
    assert emit(tok=None) == -1 and emit(done=None) == -1 and emit(state=None) == -1


def test_generate_names_the_sampling_arguments_and_set_sampling_validates():
    from macaw_llm_amd import modeling as Mo
    sig = inspect.signature(Mo.LlamaForCausalLM.generate).parameters
    assert [sig[n].default for n in ("do_sample", "temperature", "top_k", "top_p", "seed")] == [False, 1.0, 50, 1.0, None]
    sig = inspect.signature(Mo.MM_LLMs.set_sampling).parameters
    assert [sig[n].default for n in ("do_sample", "temperature", "top_k", "top_p", "seed")] == [False, 1.0, 50, 1.0, None]
    try:
        Mo.MM_LLMs.set_sampling(True, 0.7, None, 0.9, 5)
        assert Mo.SAMPLING[0] == dict(do_sample=True, temperature=0.7, top_k=None, top_p=0.9, seed=5)
        for bad, name in ((dict(temperature=0.0), "temperature"), (dict(top_p=0.0), "top_p"), (dict(top_p=1.5), "top_p"),
                          (dict(top_k=-1), "top_k")):
            with pytest.raises(ValueError, match=name):
                Mo.MM_LLMs.set_sampling(True, **bad)
        Mo.MM_LLMs.set_sampling(False, temperature=-1.0)             # ignored without do_sample
    finally:
        Mo.MM_LLMs.set_sampling()
    assert Mo.SAMPLING[0]["do_sample"] is False
