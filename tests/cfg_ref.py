"""The rule of include/macaw_hip.h ("Classifier-free guidance") restated in numpy, fp64 -- what mk_cfg_combine is pinned to.

For sample b of a guided step, c is row b of the step's logits (scored on the prompt) and u is row B + b (scored on the
negative prompt), columns [0, V), the stored values widened exactly; s is the fp32 scale widened exactly:
  1. lc = c - lse(c), lu = u - lse(u): the rule of "Token log-probabilities" (logprobs_ref.row_logprobs) without its
     rounding -- lse in fp64 over the columns that are neither NaN nor -inf; a row with no finite logit, or with +inf in
     it, is all NaN.
  2. g = lu + s * (lc - lu), in fp64.
  3. Where lc or lu is -inf, g = lc: a masked conditional column stays masked, a column the negative prompt rules out is
     not guided.
  4. NaN propagates (rule 3 first: lc = -inf next to lu = NaN is -inf).
  5. g is rounded ONCE to the logits' type and stored into row b; nothing else is written.

The bound against HF (hf_bound).  transformers' UnbatchedClassifierFreeGuidanceLogitsProcessor computes, all in fp32
(eps = 2^-24, the unit roundoff; first order in eps, the dropped terms are O((V eps)^2) < 4e-9 for V <= 1025):
  log_softmax of a row x, out_j = fl(fl(x_j - m) - fl(log(S))), S = fl(sum_k fl(exp(fl(x_k - m)))), m = max x exactly:
    fl(x_k - m)            one rounding: relative eps, absolute <= eps R, R = m - min x over the finite columns
    exp                    <= 1 ulp = 2 eps relative, plus the argument's absolute error eps R as a relative one
    the sum of V terms     non-negative terms, any order: <= (V - 1) eps relative
      => S is off by <= (V + 1 + R) eps relative, log(S) by that much absolutely
    log                    <= 1 ulp: 2 eps |log S| <= 2 eps log V
    the outer subtraction  one rounding: eps |out_j| <= eps (R + log V); its left operand carries eps R
    => |out_j - exact| <= E(V, R) = eps (V + 1 + 3 R + 3 log V)
  hf = fl(fl(s * fl(lc' - lu')) + lu') with lc', lu' those fp32 log-softmax values (lu' the same value in both places, so
  its error enters as (1 - s) e_u):
    |hf - g| <= |s| E_c + |1 - s| E_u + eps (2 |s| |lc - lu| + |g|)
  (the subtraction and the product round once each, relative to |s (lc - lu)|; the sum once, relative to |g|)."""
import numpy as np

import logprobs_ref as LR

EPS32 = 2.0 ** -24
ULP = {"float32": 2.0 ** -23, "float16": 2.0 ** -10, "bfloat16": 2.0 ** -8}     # one unit in the last place, relative


def row_lp64(x):
    """log-probability of every column of one row in fp64, unrounded (rule 1)"""
    return LR.row_logprobs(x)[1]


def combine_row(c, u, s):
    """rules 1 - 4 for one sample: c, u [V] (any float type or torch tensor) -> g in fp64 [V]"""
    lc, lu = row_lp64(c), row_lp64(u)
    s = float(np.float32(s))
    with np.errstate(invalid="ignore"):
        g = lu + s * (lc - lu)
    return np.where(np.isneginf(lc) | np.isneginf(lu), lc, g)


def combine(logits, V, B, s):
    """logits [2B, >= V] -> g in fp64 [B, V]"""
    return np.stack([combine_row(LR._row64(logits[b])[:V], LR._row64(logits[B + b])[:V], s) for b in range(B)])


def round_to(g64, dtype):
    """rule 5: fp64 -> the values of `dtype` ("float32", "float16", "bfloat16"), ONE rounding to nearest even, as fp64"""
    g64 = np.asarray(g64, dtype=np.float64)
    if dtype == "float32":
        return g64.astype(np.float32).astype(np.float64)
    if dtype == "float16":
        with np.errstate(over="ignore"):
            return g64.astype(np.float16).astype(np.float64)       # numpy converts double -> half directly
    assert dtype == "bfloat16", dtype
    out = g64.copy()
    fin = np.isfinite(g64) & (g64 != 0)
    _, e = np.frexp(g64[fin])                                      # |x| in [2^(e-1), 2^e)
    q = np.exp2(np.maximum(e - 8, -133).astype(np.float64))        # 8 significant bits; subnormals below 2^-126
    r = np.rint(g64[fin] / q) * q                                  # exact scaling, rint is to nearest even
    r[np.abs(r) >= 2.0 ** 128] = np.sign(r[np.abs(r) >= 2.0 ** 128]) * np.inf
    out[fin] = r
    return out


def within(got, ref64, s, dtype):
    """the tests' bound |got - ref64| <= (|s| + |1 - s|) 2e-6 + u |ref64| on the finite entries (the lse bound of
    logprobs_ref.within for each of the two rows, weighted, and one unit in the last place of the logits' type), equal
    -inf / +inf / NaN patterns elsewhere -> (ok, the largest |got - ref| / bound)"""
    got, ref64 = np.asarray(got, dtype=np.float64), np.asarray(ref64, dtype=np.float64)
    s = float(np.float32(s))
    fin = np.isfinite(ref64)
    same = (np.array_equal(np.isnan(got), np.isnan(ref64)) and np.array_equal(np.isfinite(got), fin)
            and np.array_equal(got[~fin & ~np.isnan(ref64)], ref64[~fin & ~np.isnan(ref64)]))
    if not same:
        return False, float("inf")
    if not fin.any():
        return True, 0.0
    ratio = np.abs(got[fin] - ref64[fin]) / ((abs(s) + abs(1 - s)) * 2e-6 + ULP[dtype] * np.abs(ref64[fin]))
    return bool(ratio.max() <= 1.0), float(ratio.max())


def _lse_err(x):
    """E(V, R) of the module docstring for one fp32 row"""
    x = LR._row64(x)
    f = x[np.isfinite(x)]
    R = float(f.max() - f.min())
    return EPS32 * (len(x) + 1 + 3 * R + 3 * np.log(len(x)))


def hf_bound(c, u, s):
    """the bound of the module docstring on |HF's fp32 result - g| for one sample -> fp64 [V] (finite rows)"""
    s = float(np.float32(s))
    lc, lu = row_lp64(c), row_lp64(u)
    g = lu + s * (lc - lu)
    return abs(s) * _lse_err(c) + abs(1 - s) * _lse_err(u) + EPS32 * (2 * abs(s) * np.abs(lc - lu) + np.abs(g))
