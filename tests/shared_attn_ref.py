"""What mk_decode_step_attn_shared is pinned to, shared by tests/test_shared_attn_gpu.py and
tests/test_shared_attn_ref_cpu.py: the gather that builds the plain kernel's cache for one row of a parallel-sampling
step, and the table of (S0, p) edges at which the shared kernel can go wrong.  Everything is torch on the CPU (the gather
works on device tensors too).

Layout (include/macaw_hip.h): prompt [B, S0, 2D] holds each prompt's keys and values once, tail [B * n, Tn, 2D] the rows'
own tokens; row r = b * n + j is sample j of prompt b.  A step at *t_dev runs row r at position p = L_b + i with
i = clamp(*t_dev - S0, 0, Tn - 1) and L_b = clamp(S0 + t_off[b], 0, S0), over prompt rows 0 ... L_b - 1 of prompt b and
tail rows 0 ... i of row r.  The contract: row r's output and appended key are bit for bit mk_decode_step_attn's, called
for the row alone at *t_dev = p over the gathered cache below.
"""
import collections

import decode_attn_ref as dref


def tail_row(t_dev, S0, Tn):
    """i of the rule"""
    return min(max(t_dev - S0, 0), Tn - 1)


def prompt_len(S0, off):
    """L_b of the rule (off = t_off[b], 0 without a t_off)"""
    return min(max(S0 + off, 0), S0)


def gather_cache(prompt, tail, r, n, L, i, rows):
    """the plain kernel's cache of row r, [1, rows, 2D]: prompt rows 0 ... L - 1 of prompt r // n, then tail rows 0 ... i - 1
    of row r, then rows the plain call must not read (row L + i is the one it appends), filled with NaN bits"""
    assert rows > L + i
    D2 = prompt.shape[-1]
    out = prompt.new_full((1, rows, D2), float("nan"))
    out[0, :L] = prompt[r // n, :L]
    out[0, L:L + i] = tail[r, :i]
    return out


def gather_caches(prompt, tail, b, n, L, i, rows):
    """gather_cache for the n rows of prompt b at once, [n, rows, 2D]: slice [j : j + 1] is row b * n + j's cache"""
    assert rows > L + i
    out = prompt.new_full((n, rows, prompt.shape[-1]), float("nan"))
    out[:, :L] = prompt[b, :L]
    out[:, L:L + i] = tail[b * n:(b + 1) * n, :i]
    return out


# ------------------------------------------------------------------------------------------------------- edges --
Edge = collections.namedtuple("Edge", "S0 p")


def edge_table(body):
    """(S0, p) for p over decode_attn_ref.edge_positions(body) and S0 over {0, 1, kpp - 1, kpp, kpp + 1, trip - 1, trip,
    trip + 1, p - 1, p}, kept where 0 <= S0 <= p.  S0 = p: the first step (the tail is the new key alone); S0 = 0: no
    prompt.  Sorted, unique."""
    pp, tr = body.kpp, body.trip
    out = set()
    for p in dref.edge_positions(body):
        for S0 in (0, 1, pp - 1, pp, pp + 1, tr - 1, tr, tr + 1, p - 1, p):
            if 0 <= S0 <= p:
                out.add(Edge(S0, p))
    return sorted(out)


def trips(body, p):
    """the key ranges [lo, hi) of the online softmax's trips at last key p"""
    return [(lo, min(lo + body.trip, p + 1)) for lo in range(0, p + 1, body.trip)]


def wave_trip_keys(body, trip_lo, wave):
    """every key index a wave's lanes hold in the trip that starts at trip_lo (whether or not it exists): lane group grp of
    wave w holds trip_lo + w * kpw + grp + j * kpp, j < NB"""
    return [trip_lo + wave * body.kpw + g + j * body.kpp for g in range(body.kpw) for j in range(dref.NB)]


def trip_kinds(body, S0, p):
    """per trip 'prompt' (every key < S0), 'tail' (every key >= S0) or 'straddle'"""
    out = []
    for lo, hi in trips(body, p):
        out.append("prompt" if hi <= S0 else "tail" if lo >= S0 else "straddle")
    return out


def wave_sources(body, S0, p):
    """per (trip, wave): the caches the wave's EXISTING keys of the trip come from -- a subset of {'prompt', 'tail'} (the new
    key p counts as tail; empty: the wave holds no key of the trip)"""
    out = []
    for lo, _ in trips(body, p):
        row = []
        for w in range(dref.NWV):
            ks = [k for k in wave_trip_keys(body, lo, w) if k <= p]
            row.append({"prompt" if k < S0 else "tail" for k in ks})
        out.append(row)
    return out
