"""The float64 reference of the four warpers behind top-p -- min_p, typical_p, epsilon_cutoff, eta_cutoff (rule 6 next to
mk_sample_rows in include/macaw_hip.h) -- on test_sampling_cpu.filter_row's conventions: fp32 scaling, candidates, top-k
with ties to the lower column, parameters rounded to fp32 as the C entry takes them.  No test in here:
tests/test_warpers_cpu.py checks this reference against transformers and tests/test_warpers_gpu.py holds the kernel to it.

warp_row() returns the kept mask and, per stage, every column's criterion and the threshold.  From these it derives the
UNDECIDED columns: those whose keep decision at some stage flips when that stage's threshold moves by the window
W = 2^-16 relative (4 W for the probability floors; top-p: p +- W, the relaxed rule of tests/test_sampling_gpu.py) or,
for typical_p, when D moves by W * max(1, D) -- W is the EPS of tests/test_sampling_gpu.py, about three times the
worst-case fp32 error of a 32k-term sum plus the error of exp, so an EPS-accurate kernel decides every other column as
the reference does.  The ALTERNATIVES are the kept sets obtained by deciding each undecided column either way and running
the later stages on the result.  A row with more than MAX_UNDECIDED undecided columns is left out (alternatives None)."""
import functools
import itertools

import numpy as np

from test_sampling_cpu import filter_row

W = 2.0 ** -16
MAX_UNDECIDED = 4
TINY = 2.0 ** -40                                                     # one unit of the kernel's fixed-point masses
OFF = (0.0, 1.0, 0.0, 0.0)


def f32(v):
    return float(np.float32(v))


class _LeftOut(Exception):
    pass


def _floor_stage(name, crit, thr, surv, e, win):
    """keep c iff crit_c >= thr; no survivor passes: the survivors of the largest value stay"""
    keep = surv & (crit >= thr)
    if not keep.any():
        keep = surv & (e == e[surv].max())
    und = surv & (crit >= thr * (1 - win)) & (crit < thr * (1 + win))
    return dict(stage=name, crit=crit, thr=thr, keep=keep, undecided=np.nonzero(und)[0])


def _typical_keep(d, e, surv, D, target):
    """keep c iff the mass of the survivors with t strictly below t_c is below target, t = |d - D|"""
    cols = np.nonzero(surv)[0]
    t = np.abs(d[cols] - D)
    order = np.argsort(t, kind="stable")
    ts, ms = t[order], e[cols][order]
    cum = np.cumsum(ms)
    first = np.searchsorted(ts, ts, side="left")                      # the first position of each tie group in t
    below = np.where(first > 0, cum[np.maximum(first - 1, 0)], 0.0)
    keep = np.zeros(len(d), dtype=bool)
    keep[cols[order[below < target]]] = True
    tcol = np.full(len(d), np.inf)
    tcol[cols] = t
    return keep, tcol


def _stages(base, p, min_p, typical_p, eps, eta):
    """the stage functions behind top-k, each surv -> dict(stage, crit, thr, keep, undecided), in HF's order"""
    e = base["e"]
    x64 = base["x"].astype(np.float64)
    xmax = x64[base["topk"]].max()
    with np.errstate(invalid="ignore"):
        d = np.where(x64 == xmax, 0.0, xmax - x64)
    out = []
    if p < 1.0:
        def top_p(surv):
            Zk, above = base["Zk"], base["above"]
            keep = surv & (above < p * Zk)
            und = surv & (above >= (p - W) * Zk) & (above < (p + W) * Zk)
            return dict(stage="top_p", crit=above, thr=p * Zk, keep=keep, undecided=np.nonzero(und)[0])
        out.append(top_p)
    if min_p > 0.0:
        out.append(lambda surv: _floor_stage("min_p", e, min_p, surv, e, 4 * W))
    if typical_p < 1.0:
        out.append(lambda surv: _floor_stage("mass0", e, TINY, surv, e, 4 * W))

        def typical(surv):
            Z = e[surv].sum()
            D = (e[surv] * d[surv]).sum() / Z
            keep, t = _typical_keep(d, e, surv, D, typical_p * Z)
            und = np.zeros(len(e), dtype=bool)
            dD = W * max(1.0, D)
            for D2 in (D - dD, D, D + dD):
                for tg in (typical_p * Z * (1 - W), typical_p * Z, typical_p * Z * (1 + W)):
                    if D2 != D or tg != typical_p * Z:
                        und |= _typical_keep(d, e, surv, D2, tg)[0] != keep
            return dict(stage="typical_p", crit=t, thr=t[keep].max(), D=D, keep=keep, undecided=np.nonzero(und)[0])
        out.append(typical)
    if eps > 0.0:
        out.append(lambda surv: _floor_stage("epsilon_cutoff", e / e[surv].sum(), eps, surv, e, 4 * W))
    if eta > 0.0:
        def eta_stage(surv):
            Z = e[surv].sum()
            H = np.log(Z) + (e[surv] * d[surv]).sum() / Z
            return _floor_stage("eta_cutoff", e / Z, min(eta, np.sqrt(eta) * np.exp(-H)), surv, e, 4 * W)
        out.append(eta_stage)
    return out


def warp_row(logits, V, temperature=1.0, top_k=0, top_p=1.0, min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0,
             eta_cutoff=0.0):
    """rules 1-3 and 6 for one row -> None when it has no finite logit, else a dict: kept (bool [V]), e (float64 masses
    exp(x - x_max), 0 outside the top-k survivors), stages (per stage that is on: stage, crit [V], thr, keep, undecided),
    undecided (sorted columns, over every branch explored), alternatives (list of bool [V], the nominal kept set first;
    None when the row is left out)."""
    base = filter_row(logits, V, temperature, top_k, 1.0)
    if base is None:
        return None
    fns = _stages(base, f32(top_p), f32(0.0 if min_p is None else min_p), f32(typical_p), f32(epsilon_cutoff),
                  f32(eta_cutoff))
    memo = {}

    def stage(i, surv):                                               # one evaluation per (stage, survivors)
        key = (i, surv.tobytes())
        if key not in memo:
            memo[key] = fns[i](surv)
        return memo[key]

    surv, stages = base["topk"].copy(), []
    for i in range(len(fns)):
        stages.append(stage(i, surv))
        surv = stages[-1]["keep"]
    seen = set()

    def walk(i, surv):
        if i == len(fns):
            return [surv]
        st = stage(i, surv)
        und = st["undecided"]
        seen.update(int(c) for c in und)
        if len(seen) > MAX_UNDECIDED:
            raise _LeftOut
        outs = []
        for bits in itertools.product((False, True), repeat=len(und)):
            k2 = st["keep"].copy()
            k2[und] = bits
            if k2.any():                                              # every stage keeps at least one column
                outs += walk(i + 1, k2)
        return outs

    try:
        alts = {a.tobytes(): a for a in [surv] + walk(0, base["topk"].copy())}
        alts = list(alts.values())
    except _LeftOut:
        alts = None
    return dict(kept=surv, e=base["e"], x=base["x"], stages=stages, undecided=sorted(seen), alternatives=alts)


# ------------------------------------------------------------------------------------------------- the fixtures --
SHAPES = [(32007, 8, 32064), (1000, 3, 1000), (1, 2, 1), (8193, 33, 8193)]          # V, rows, pitch (test_sampling_gpu.py)
SIGMAS = [3.0, 6.0]
DTYPES = ["bf16", "fp16", "fp32"]
# (temperature, top_k, top_p, min_p, typical_p, epsilon_cutoff, eta_cutoff)
TUPLES = [(1.0, 0, 1.0, .05, 1.0, 0.0, 0.0),
          (1.0, 0, 1.0, 0.0, .9, 0.0, 0.0),
          (1.0, 0, 1.0, 0.0, .2, 0.0, 0.0),
          (1.0, 0, 1.0, 0.0, 1.0, 3e-3, 0.0),
          (1.0, 0, 1.0, 0.0, 1.0, 0.0, 2e-3),
          (.8, 40, .95, .02, .9, 1e-2, 0.0),
          (1.3, 0, .9, .01, .95, 3e-3, 2e-3)]


def logits_host(V, rows, ld, sigma, dtype, seed=0):
    """test_sampling_gpu._logits without the device: randn * sigma rounded to dtype, pad columns [V, ld) = +1e4 ->
    (torch tensor [rows, ld] of dtype, fp32 numpy [rows, V])"""
    import torch
    tdt = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[dtype]
    x = torch.randn(rows, V, generator=torch.Generator().manual_seed(seed + V)) * sigma
    full = torch.full((rows, ld), 1e4)
    full[:, :V] = x
    full = full.to(tdt)
    return full, full[:, :V].float().numpy()


@functools.lru_cache(maxsize=None)
def case(V, rows, ld, sigma, dtype, tup):
    """the reference of one fixture under one parameter tuple, computed once per process and shared by the tests that
    need it: per row (kept, alternatives or None, undecided) of warp_row"""
    _, xh = logits_host(V, rows, ld, sigma, dtype)
    out = []
    for r in range(rows):
        w = warp_row(xh[r], V, *tup)
        out.append((w["kept"], w["alternatives"], w["undecided"]))
    return tuple(out)


def left_out_ok(per_case):
    """the leave-out caps over [(rows left out, rows)] per case: at most a quarter of a case's rows, at most 2 % of all"""
    worst = all(4 * lo <= n for lo, n in per_case)
    tot_lo, tot = sum(lo for lo, _ in per_case), sum(n for _, n in per_case)
    return worst and 50 * tot_lo <= tot, (tot_lo, tot, max((lo / n for lo, n in per_case), default=0.0))
