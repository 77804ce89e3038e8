"""The rule of include/macaw_hip.h ("Token log-probabilities") restated in numpy, fp64 -- what mk_token_logprobs and
mk_decode_emit_logprobs are pinned to.

For a row of logits x[0:V) (the stored values, widened exactly):
  1. m = the maximum over the columns that are neither NaN nor -inf; S = sum of exp(x_c - m) over the same columns;
     lse = m + log(S), all in fp64 (the kernels take expf in fp32 and accumulate in fp64: inside the tests' bound).
  2. logprob(c) = float32(x_c - lse): one rounding.  -inf gives -inf, NaN gives NaN.
  3. A row with no finite logit, or with a +inf in it, is degenerate: every log-probability is NaN.
  4. Top-n: the n columns with the largest x_c, NaN columns excluded (-inf columns are columns like any other, -0 == +0),
     descending, ties to the LOWER column.  Fewer than n non-NaN columns: the remaining slots are id -1 with
     log-probability -inf.  In a degenerate row the ids are still the n largest, the values NaN.
An id outside [0, V) has log-probability NaN."""
import numpy as np


def _row64(x):
    """a row of logits (numpy of any float type, or a torch tensor of bf16 / f16 / f32) -> float64, exactly"""
    if hasattr(x, "detach"):
        x = x.detach().double().cpu().numpy()
    return np.asarray(x, dtype=np.float64)


def lse(x):
    """-> (lse in fp64, degenerate)"""
    x = _row64(x)
    ok = ~np.isnan(x) & (x != -np.inf)
    if not ok.any() or np.isposinf(x[ok]).any():
        return np.nan, True
    m = x[ok].max()
    return m + np.log(np.exp(x[ok] - m).sum()), False


def row_logprobs(x):
    """log-probability of every column of one row -> float32 [V] (rule 2 and 3), and the fp64 values before the
    rounding (for the tolerance of a comparison)"""
    x = _row64(x)
    l, deg = lse(x)
    if deg:
        full = np.full(x.shape, np.nan)
    else:
        with np.errstate(invalid="ignore"):
            full = x - l
    return full.astype(np.float32), full


def top(x, n):
    """the n best columns of one row (rule 4) -> ids int64 [n] with -1 behind the last non-NaN column"""
    x = _row64(x)
    cols = [c for c in range(x.shape[0]) if not np.isnan(x[c])]
    cols.sort(key=lambda c: (-x[c], c))           # python's sort is stable and -0.0 == 0.0: ties to the lower column
    ids = cols[:n] + [-1] * max(n - len(cols), 0)
    return np.asarray(ids, dtype=np.int64)


def token_logprobs(x, ids, n=0):
    """rows x [R, V] (columns beyond V already cut), ids [R] -> (lp f32 [R], top_ids int64 [R, n], top_lp f32 [R, n],
    lp64 [R], top_lp64 [R, n]); the last two are the unrounded fp64 values"""
    R = len(x)
    lp, lp64 = np.empty(R, np.float32), np.empty(R, np.float64)
    ti, tl, tl64 = np.empty((R, n), np.int64), np.empty((R, n), np.float32), np.empty((R, n), np.float64)
    for r in range(R):
        row = _row64(x[r])
        v32, v64 = row_logprobs(row)
        i = int(ids[r])
        inside = 0 <= i < row.shape[0]
        lp[r], lp64[r] = (v32[i], v64[i]) if inside else (np.nan, np.nan)
        ti[r] = top(row, n)
        for j, c in enumerate(ti[r]):
            tl[r, j], tl64[r, j] = (v32[c], v64[c]) if c >= 0 else (-np.inf, -np.inf)
    return lp, ti, tl, lp64, tl64


def within(got, ref64):
    """the tests' bound |got - ref| <= 2e-6 + 2^-23 |ref| on the finite entries, equal -inf / +inf / NaN patterns
    elsewhere -> (ok, the largest |got - ref| / bound)"""
    got, ref64 = np.asarray(got, dtype=np.float64), np.asarray(ref64, dtype=np.float64)
    fin = np.isfinite(ref64)
    same = (np.array_equal(np.isnan(got), np.isnan(ref64)) and np.array_equal(np.isfinite(got), fin)
            and np.array_equal(got[~fin & ~np.isnan(ref64)], ref64[~fin & ~np.isnan(ref64)]))
    if not fin.any():
        return same, 0.0
    ratio = np.abs(got[fin] - ref64[fin]) / (2e-6 + 2.0 ** -23 * np.abs(ref64[fin])) if same else np.array([np.inf])
    return bool(same and ratio.max() <= 1.0), float(ratio.max())
