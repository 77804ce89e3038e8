"""The host side of generate(num_beams=K): the argument check (a plain function, no GPU) and the one pass over the
device's books after the loop -- finalisation of the unfinished samples, the sort of the pool and the backtracking of
the (token, parent) history into id sequences.  The rule is written down in include/macaw_hip.h ("Beam search") and
restated in tests/beam_ref.py; every step of it runs on the device (csrc/beam.hip)."""
from __future__ import annotations

import numbers

import torch

MAX_BEAMS = 16


def beam_check(where, num_beams, num_return_sequences=1, vocab=None, do_sample=False, kv_cache=None, padded=False,
               length_penalty=1.0):
    """the beam arguments of generate() / set_beam_search -> num_beams as an int.  ValueError naming the condition for
    num_beams not an integer in [1, 16]; with num_beams > 1 also for num_return_sequences outside [1, num_beams], a
    vocabulary below 2 * num_beams (vocab=None: not checked), do_sample=True, kv_cache="fp8" and a padded
    attention_mask (the last two are not built yet: DESIGN 4.6).  num_beams = 1 ignores every other argument."""
    if isinstance(num_beams, bool) or not isinstance(num_beams, numbers.Integral) or not 1 <= num_beams <= MAX_BEAMS:
        raise ValueError(f"{where}: num_beams must be an integer in [1, {MAX_BEAMS}], got {num_beams!r}")
    K = int(num_beams)
    if K == 1:
        return K
    if (isinstance(num_return_sequences, bool) or not isinstance(num_return_sequences, numbers.Integral)
            or num_return_sequences < 1):
        raise ValueError(f"{where}: num_return_sequences must be an integer >= 1, got {num_return_sequences!r}")
    if num_return_sequences > K:
        raise ValueError(f"{where}: num_return_sequences={num_return_sequences} > num_beams={K}")
    if not isinstance(length_penalty, numbers.Real) or length_penalty != length_penalty or abs(length_penalty) == float("inf"):
        raise ValueError(f"{where}: length_penalty must be a finite number, got {length_penalty!r}")
    if vocab is not None and vocab < 2 * K:
        raise ValueError(f"{where}: a vocabulary of {vocab} is below 2 * num_beams = {2 * K} (a step ranks 2 * num_beams "
                         "candidates)")
    if do_sample:
        raise ValueError(f"{where}: do_sample=True with num_beams={K} > 1 (beam-sample decoding is not built)")
    if kv_cache == "fp8":
        raise ValueError(f"{where}: kv_cache='fp8' with num_beams={K} > 1 (there is no beam step over the e4m3 cache)")
    if padded:
        raise ValueError(f"{where}: a padded attention_mask with num_beams={K} > 1 (there is no beam step over the "
                         "ragged cache)")
    return K


def _pool_insert(pool, K, score, seq, item):
    """rule 4: append while fewer than K entries, else replace the worst if strictly greater (among equal worst scores
    the latest inserted).  pool: list of (score, seq, item)"""
    if len(pool) < K:
        pool.append((score, seq, item))
        return
    w = 0
    for e in range(1, len(pool)):
        if pool[e][0] < pool[w][0] or (pool[e][0] == pool[w][0] and pool[e][1] > pool[w][1]):
            w = e
    if score > pool[w][0]:
        pool[w] = (score, seq, item)


def beam_result(hist, scores, pool_score, pool_info, done, n_cols, length_penalty, num_return_sequences, pad, eos):
    """The books of ops.BeamState after n_cols steps, as CPU tensors -> (ids int64 [B * nret, width], scores f32
    [B * nret]): every sample not done adds its running beams with a finite score to its pool in beam order with
    s_k / n_cols ** length_penalty (fp32, the device's arithmetic); the pool is sorted by score descending, ties to the
    earlier insertion; the first nret hypotheses are backtracked through hist and padded with pad behind their eos to
    the longest one returned.  A sample with fewer than nret hypotheses (beams that could not be filled) returns rows
    of pad with score -inf."""
    _, B, K, _ = hist.shape
    nret = num_return_sequences
    hist = hist.tolist()

    def back(col, k):               # the tokens of beam k at output column col
        seq = []
        for i in range(col, -1, -1):
            t, k = hist[i][b][k]
            seq.append(t)
        return seq[::-1]

    pen = torch.tensor(float(n_cols), dtype=torch.float32) ** torch.tensor(float(length_penalty), dtype=torch.float32)
    rows, out_scores = [], []
    for b in range(B):
        n, seq = int(pool_info[b, K, 0]), int(pool_info[b, K, 1])
        pool = [(float(pool_score[b, e]), int(pool_info[b, e, 2]), ("eos", int(pool_info[b, e, 0]), int(pool_info[b, e, 1])))
                for e in range(n)]
        if not bool(done[b]):
            for k in range(K):
                s = scores[b * K + k]
                if bool(torch.isfinite(s)):
                    _pool_insert(pool, K, float(s / pen), seq, ("run", n_cols - 1, k))
                    seq += 1
        pool.sort(key=lambda e: (-e[0], e[1]))
        for e in range(nret):
            if e < len(pool):
                sc, _, (kind, col, k) = pool[e]
                rows.append(back(col - 1, k) + [eos] if kind == "eos" else back(col, k))
                out_scores.append(sc)
            else:
                rows.append([])
                out_scores.append(float("-inf"))
    width = max(1, max(len(r) for r in rows))
    ids = torch.full((B * nret, width), pad, dtype=torch.long)
    for i, r in enumerate(rows):
        ids[i, :len(r)] = torch.tensor(r, dtype=torch.long)
    return ids, torch.tensor(out_scores, dtype=torch.float32)
