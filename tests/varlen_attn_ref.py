"""fp32 reference of the variable-length causal forward (mk_flash_attn_varlen_fwd), shared by
tests/test_flash_varlen_gpu.py and tests/test_varlen_attn_ref_cpu.py.

The rule (macaw_hip.h): with ql_b = clamp(q_len[b], 0, Lq) and kl_b = clamp(k_len[b], 0, Lk), query row i < ql_b of
sample b sees key j iff j < kl_b and j <= i + (kl_b - ql_b); every other row -- i >= ql_b, and the first ql_b - kl_b
rows where kl_b < ql_b -- gets o = 0 and lse = -inf.  The reference is attn_ref.attention_ref, sample by sample, on
q[b, :ql_b], k[b, :kl_b], v[b, :kl_b] with causal=True: rows of k / v at or past kl_b and rows of q at or past ql_b never
enter it, so they may hold anything.

Tensors are token-major: q [B, Lq, H * hd]; k, v [B, Lk, H * hd]; o [B, Lq, H * hd]; lse [B, H, Lq].
"""
import torch

import attn_ref as R

# (Lq; (q_len, k_len) per sample): chosen to cross the 64-key tile, the 32-key sub-block, the 32-row wave slice and the
# 128-row block; Lk = max k_len (the GPU test adds rows that are never written behind it)
CASES = [
    (5, [(5, 333), (1, 1), (3, 64), (0, 17)]),
    (40, [(40, 40), (32, 96), (31, 95), (33, 97)]),
    (130, [(130, 300), (129, 129), (33, 65), (1, 257)]),
    (70, [(70, 40), (64, 64), (2, 129)]),          # the first sample has 30 dead leading rows
]


def clamp_lens(q_len, k_len, Lq, Lk):
    return [min(max(int(x), 0), Lq) for x in q_len], [min(max(int(x), 0), Lk) for x in k_len]


def visible(q_len, k_len, Lq, Lk):
    """[B, Lq, Lk] bool: key j visible to query i of sample b, by the rule above"""
    ql, kl = clamp_lens(q_len, k_len, Lq, Lk)
    i = torch.arange(Lq)[:, None]
    j = torch.arange(Lk)[None, :]
    return torch.stack([(i < a) & (j < b) & (j <= i + (b - a)) for a, b in zip(ql, kl)])


def varlen_ref(q, k, v, H, scale, q_len, k_len):
    """dict(o [B, Lq, D] fp32, lse [B, H, Lq] fp32)"""
    B, Lq, D = q.shape
    Lk = k.shape[1]
    ql, kl = clamp_lens(q_len, k_len, Lq, Lk)
    o = torch.zeros(B, Lq, D, dtype=torch.float32)
    lse = torch.full((B, H, Lq), float("-inf"), dtype=torch.float32)
    for b in range(B):
        if ql[b] == 0 or kl[b] == 0:
            continue
        r = R.attention_ref(q[b:b + 1, :ql[b]], k[b:b + 1, :kl[b]], v[b:b + 1, :kl[b]], H, scale, causal=True)
        o[b, :ql[b]] = r["o"][0]
        lse[b, :, :ql[b]] = r["lse"][0]
    return {"o": o, "lse": lse}


def census_expect(v, H, q_len, k_len, Lq):
    """q = 0: every visible score is exactly 0, so lse = log(n_visible) and o is the mean of the visible v rows.
    Rows of v at or past k_len[b] are excluded by the select (they may be NaN).
    Returns (n [B, Lq] int64, lse [B, H, Lq] float64 with -inf at n = 0, o [B, Lq, D] float64)."""
    B, Lk, D = v.shape
    vis = visible(q_len, k_len, Lq, Lk)
    _, kl = clamp_lens(q_len, k_len, Lq, Lk)
    vv = v.double().clone()
    for b in range(B):
        vv[b, kl[b]:] = 0
    n = vis.sum(-1)
    lse = torch.where(n > 0, torch.log(n.double().clamp(min=1)), torch.full((), float("-inf"), dtype=torch.float64))
    o = (vis.double() @ vv) / n.clamp(min=1)[..., None].double()
    return n, lse[:, None, :].expand(B, H, Lq).contiguous(), o
