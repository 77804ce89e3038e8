"""The restatement of the per-row sampling table (include/macaw_hip.h, "Per-row sampling table": mk_sample_rows_table,
mk_decode_emit_sample_table) on top of the restatements the scalar entries already have: test_sampling_cpu's greedy,
sample_row and uniform (rules 1-4) and warpers_ref.warp_row (rule 6).  No test in here: tests/test_sampling_params_cpu.py
checks it, tests/test_sampling_params_gpu.py holds the kernels to the project's scalar kernels bit for bit.

A record is None (greedy) or a dict with the keys of ops.SampleTable: temperature, top_k (0 = off), top_p, min_p,
typical_p, epsilon_cutoff, eta_cutoff, seed, stream -- a missing one takes its off value."""
import math
import struct

import numpy as np

from test_sampling_cpu import greedy, sample_row, uniform
from warpers_ref import OFF, warp_row

RECORD = struct.Struct("<fifffffIQii")            # the header's 48 bytes
FIELDS = ("temperature", "top_k", "top_p", "min_p", "typical_p", "epsilon_cutoff", "eta_cutoff", "stream", "seed", "mode")
DEFAULTS = dict(temperature=1.0, top_k=0, top_p=1.0, min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0,
                seed=0, stream=0)


def full(rec):
    """a record with every key"""
    return None if rec is None else {**DEFAULTS, **rec}


def pack(rec):
    """the 48 bytes of one record: mode 0 and the off values for a greedy row"""
    r = full(rec) or DEFAULTS
    return RECORD.pack(r["temperature"], r["top_k"], r["top_p"], r["min_p"], r["typical_p"], r["epsilon_cutoff"],
                       r["eta_cutoff"], r["stream"], r["seed"] & (2 ** 64 - 1), int(rec is not None), 0)


def unpack(raw):
    """48 bytes -> the record as a dict with `mode`"""
    return dict(zip(FIELDS, RECORD.unpack(bytes(raw))))


def in_domain(r):
    """the domain of the scalar entries (MK_ERR_BAD_ARG outside it): a record outside it is greedy"""
    return (math.isfinite(r["temperature"]) and r["temperature"] > 0 and 0 < r["top_p"] <= 1 and r["top_k"] >= 0
            and 0 <= r["min_p"] <= 1 and 0 < r["typical_p"] <= 1 and 0 <= r["epsilon_cutoff"] < 1
            and 0 <= r["eta_cutoff"] < 1)


def warpers(r):
    return (r["min_p"], r["typical_p"], r["epsilon_cutoff"], r["eta_cutoff"])


def form(rec):
    """which of the three forms a row takes: "greedy", "sample" (sample_row<T, false>) or "warp" (sample_row<T, true>)"""
    r = full(rec)
    if r is None or r.get("mode", 1) != 1 or not in_domain(r):
        return "greedy"
    return "sample" if tuple(float(v) for v in warpers(r)) == OFF else "warp"


def table_row(logits, V, rec, step=0):
    """the token of one row of logits under its record at `step`: the place of the row in the batch is no argument"""
    lg = np.asarray(logits, dtype=np.float32)[:V]
    f, r = form(rec), full(rec)
    if f == "greedy":
        return greedy(lg)
    if f == "sample":
        return sample_row(lg, V, r["temperature"], r["top_k"], r["top_p"], r["seed"], step, row=r["stream"])
    w = warp_row(lg, V, r["temperature"], r["top_k"], r["top_p"], *warpers(r))
    if w is None:
        return greedy(lg)
    kept = np.nonzero(w["kept"])[0]
    cum = np.cumsum(w["e"][kept])
    hit = np.nonzero(cum > uniform(r["seed"], step, r["stream"]) * cum[-1])[0]
    return int(kept[hit[0]] if len(hit) else kept[-1])


def table_rows(logits, V, recs, step=0):
    return [table_row(row, V, rec, step) for row, rec in zip(logits, recs)]


def emit(logits, V, recs, pad, eos, tok, done, out, state, select=None):
    """mk_decode_emit_sample_table on host lists / arrays, in place: select(step) -> the ids of every row at that step
    (None: table_rows)"""
    col = state[1]
    ids = select(col) if select is not None else table_rows(logits, V, recs, col)
    for b in range(len(recs)):
        nxt = pad if done[b] else int(ids[b])
        out[b][col] = nxt
        if nxt == eos:
            done[b] = True
        tok[b] = nxt
    state[0] += 1
    state[1] = col + 1
    state[2] = 0
