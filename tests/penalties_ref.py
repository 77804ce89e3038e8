"""The rule of include/macaw_hip.h, "Per-request penalties" (frequency_penalty, presence_penalty, logit_bias), restated
in torch: `penalize`, step by step in fp32 with the roundings where the header puts them -- the reference the kernel
(mk_logits_penalize) and generate() are pinned to bit for bit -- and `penalize_dense`, an independent formulation
(torch.bincount, a dense bias row, fp64 arithmetic) that agrees with it wherever fp64 and the stepwise fp32 provably give
the same number: integer-valued logits, penalties and biases, every intermediate far below 2^24.

Inputs, per row b: the generated ids gen[b, :n] (the prompt is never counted; an id outside [0, V) names no column), f[b]
and p[b] (None: all zeros), and bias[b], a dict {column: value} or None (bias None: no row has one)."""
import torch

F32 = torch.float32


def counts(gen, n, V):
    """cnt int64 [B, V]: how often gen[b, :n] holds each column"""
    B = gen.shape[0]
    cnt = torch.zeros((B, V), dtype=torch.long)
    for b in range(B):
        for c in gen[b, :n].tolist():
            if 0 <= c < V:
                cnt[b, c] += 1
    return cnt


def touched(B, V, gen, n, f=None, p=None, bias=None):
    """bool [B, V]: the columns the rule reads and writes -- a bias entry, or generated at least once in a row whose f or
    p is not zero (as float32)"""
    n = max(0, min(int(n), gen.shape[1]))
    cnt = counts(gen.cpu(), n, V)
    t = torch.zeros((B, V), dtype=torch.bool)
    for b in range(B):
        fb = torch.tensor(0.0 if f is None else float(f[b]), dtype=F32)
        pb = torch.tensor(0.0 if p is None else float(p[b]), dtype=F32)
        if bool(fb != 0) or bool(pb != 0):
            t[b] = cnt[b] > 0
        for c in (bias[b] if bias is not None else None) or {}:
            t[b, c] = True
    return t


def penalize(logits, V, gen, n, f=None, p=None, bias=None):
    """logits [B, ld >= V] of any float type, gen int64 [B, n_max], n clamped into [0, n_max] -> the rewritten matrix (a
    new tensor).  A column is read and written only when it is touched; every other column, the padding [V, ld)
    included, keeps its bits (clone, then indexed stores).  A touched NaN stays a NaN; which NaN (sign, payload) is
    whatever torch's scalar arithmetic and conversion leave, and is not part of the rule."""
    logits, gen = logits.cpu(), gen.cpu()
    out = logits.clone()
    n = max(0, min(int(n), gen.shape[1]))
    cnt = counts(gen, n, V)
    for b in range(logits.shape[0]):
        fb = torch.tensor(0.0 if f is None else float(f[b]), dtype=F32)
        pb = torch.tensor(0.0 if p is None else float(p[b]), dtype=F32)
        row_bias = (bias[b] if bias is not None else None) or {}
        pen = bool(fb != 0) or bool(pb != 0)
        for c in sorted(set(row_bias) | (set(torch.nonzero(cnt[b]).flatten().tolist()) if pen else set())):
            x = logits[b, c].to(F32)                                   # x = float(logit[c])
            if c in row_bias:
                x = x + torch.tensor(row_bias[c], dtype=F32)           # one fp32 addition
            if cnt[b, c] > 0:
                x = x - fb * cnt[b, c].to(F32)                         # one fp32 product, one fp32 subtraction
                x = x - pb                                             # one fp32 subtraction, also when p is 0
            out[b, c] = x.to(logits.dtype)                             # one rounding, to nearest even
    return out


def penalize_dense(logits, V, gen, n, f=None, p=None, bias=None):
    """the same result another way: torch.bincount per row, a dense bias row and fp64 arithmetic, selected into the
    touched columns.  Equal to `penalize` bit for bit when the logits, f, p and the bias values are integers (every
    intermediate is then exact in fp32 and in fp64); -inf, +inf and NaN columns agree as well."""
    logits, gen = logits.cpu(), gen.cpu()
    B = logits.shape[0]
    n = max(0, min(int(n), gen.shape[1]))
    out = logits.clone()
    for b in range(B):
        g = gen[b, :n]
        g = g[(g >= 0) & (g < V)]
        cnt = torch.bincount(g, minlength=V)
        dense = torch.zeros(V, dtype=torch.float64)
        has = torch.zeros(V, dtype=torch.bool)
        for c, v in ((bias[b] if bias is not None else None) or {}).items():
            dense[c], has[c] = v, True
        fb = 0.0 if f is None else float(f[b])
        pb = 0.0 if p is None else float(p[b])
        touched = has | ((cnt > 0) & bool(fb != 0 or pb != 0))
        x = logits[b, :V].to(torch.float64) + dense - fb * cnt.to(torch.float64) - pb * (cnt > 0).to(torch.float64)
        out[b, :V] = torch.where(touched, x.to(F32).to(logits.dtype), logits[b, :V])
    return out

