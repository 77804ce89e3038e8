"""The token-sequence rules of include/macaw_hip.h ("Token-sequence matching") restated in plain torch on the CPU: integers
and -inf only.  tests/test_stopping_cpu.py pins the ban rule, for fp32 logits, to the installed transformers'
NoBadWordsLogitsProcessor bit for bit wherever every sequence has L >= n, and checks both rules by hand;
tests/test_stopping_gpu.py pins ops.seq_ban and ops.stop_match to them exactly."""
import torch


def ban_row(logits, history, seqs):
    """logits [V] (bf16 / fp16 / fp32, CPU), history = prompt ++ generated (a list of ints), seqs: the banned sequences
    -> a new row of the same type: for every q of n ids, column q[n - 1] is -inf when n == 1, and when L >= n - 1 and
    the history's last n - 1 ids are q[:n - 1].  An id outside [0, V) names no column"""
    V = logits.shape[0]
    out = logits.clone()
    h = [int(c) for c in history]
    L = len(h)
    for q in seqs:
        q = [int(c) for c in q]
        n = len(q)
        if n == 1 or (L >= n - 1 and h[L - (n - 1):] == q[:n - 1]):
            if 0 <= q[-1] < V:
                out[q[-1]] = float("-inf")
    return out


def ban(logits, prompts, generated, seqs):
    """logits [B, V]; prompts: per row a list of ids (or None: no prompt history); generated: per row this call's ids so
    far -> [B, V]"""
    return torch.stack([ban_row(logits[b], ([] if prompts is None else list(prompts[b])) + list(generated[b]), seqs)
                        for b in range(logits.shape[0])])


def drop_eos(seqs, eos):
    """HF's rule: a banned sequence equal to [eos] is dropped"""
    return [list(q) for q in seqs if list(q) != [eos]]


def stops_row(generated, seqs):
    """whether the generated ids (a list of ints; never the prompt) end with one of the sequences"""
    g = [int(c) for c in generated]
    return any(len(q) <= len(g) and g[len(g) - len(q):] == [int(c) for c in q] for q in seqs)


def stop_match(out, n, seqs, done):
    """out: per row the output ids, n: the generated count, done: per row a flag -> the flags behind the match: a
    finished row is not examined and stays finished"""
    return [bool(d) or stops_row(list(row)[:n], seqs) for row, d in zip(out, done)]


def finish_column(row, seqs, eos):
    """the column at which a row of plain ids finishes by eos or by a stop sequence, or None"""
    row = [int(c) for c in row]
    for c in range(len(row)):
        if row[c] == eos or stops_row(row[:c + 1], seqs):
            return c
    return None


def cut(ids, seqs, eos, pad):
    """plain ids [B, W] (a tensor; stopping changes no logit) -> what generate(stop_sequences=seqs) returns: every row
    kept up to its finish column, pad behind it, the width that of the last row to finish (W if one never does)"""
    rows = [[int(c) for c in r] for r in ids.tolist()]
    ends = [finish_column(r, seqs, eos) for r in rows]
    W = len(rows[0]) if any(e is None for e in ends) else max(ends) + 1
    return torch.tensor([[c if e is None or i <= e else pad for i, c in enumerate(r[:W])] for r, e in zip(rows, ends)],
                        dtype=torch.long)
