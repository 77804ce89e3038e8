"""The rules of include/macaw_hip.h, "Grammar-constrained decoding", restated in numpy / torch for the tests: the byte
walk that makes a token table, the token trim, the flags, the mask and the advance.  Written from the header alone, in
the plainest form that is still fast enough (loops over tokens, rows and columns); it imports nothing of the package's
grammar module."""
import numpy as np
import torch

INF = float("inf")


def token_table(char_next, vocab):
    """char_next int [S, 256] (-1 dead), vocab a list of bytes | None -> next int32 [S, V]: entry (s, t) is char_next walked
    over token t's bytes from s, -1 on a dead byte transition or an empty (or None) token.  One token at a time, all
    start states together"""
    char_next = np.asarray(char_next)
    S = char_next.shape[0]
    out = np.full((S, len(vocab)), -1, dtype=np.int32)
    for t, tok in enumerate(vocab):
        if not tok:
            continue
        cur = np.arange(S, dtype=np.int64)
        for byte in tok:
            cur = np.where(cur >= 0, char_next[np.maximum(cur, 0), byte], -1)
        out[:, t] = cur
    return out


def live_states(nxt, accepting):
    """the states from which an accepting state can be reached by the table's tokens: a breadth-first search backwards"""
    nxt = np.asarray(nxt)
    S = nxt.shape[0]
    preds = [set() for _ in range(S)]
    for s in range(S):
        for d in np.unique(nxt[s][nxt[s] >= 0]).tolist():
            preds[d].add(s)
    live = [bool(a) for a in accepting]
    queue = [s for s in range(S) if live[s]]
    while queue:
        d = queue.pop()
        for s in preds[d]:
            if not live[s]:
                live[s] = True
                queue.append(s)
    return np.array(live, dtype=bool)


def trim(nxt, accepting):
    """-> (the token-trimmed table, flags uint8 [S]): a transition into a state that is not live is -1; bit 0 accepting,
    bit 1 terminal = accepting with no allowed token"""
    nxt = np.array(nxt, dtype=np.int32, copy=True)
    live = live_states(nxt, accepting)
    nxt[(nxt >= 0) & ~live[np.maximum(nxt, 0)]] = -1
    acc = np.asarray(accepting, dtype=bool)
    flags = acc.astype(np.uint8) | ((acc & ~(nxt >= 0).any(1)).astype(np.uint8) << 1)
    return nxt, flags


def mask(logits, V, nxt, flags, state, done, eos):
    """logits [rows, ld] (any float dtype, CPU) -> the masked copy.  eos None or outside [0, V): absent"""
    out = logits.clone()
    n_states = len(flags)
    ninf = torch.tensor(-INF, dtype=logits.dtype)
    for b in range(logits.shape[0]):
        s = int(state[b])
        if bool(done[b]) or s < 0 or s >= n_states:
            continue
        for c in range(V):
            banned = not (int(flags[s]) & 1) if (eos is not None and c == eos) else int(nxt[s][c]) < 0
            if banned:
                out[b, c] = ninf
    return out


def mask_fast(logits, V, nxt, flags, state, done, eos):
    """mask() with the columns of a row taken together (the large shapes)"""
    out = logits.clone()
    n_states = len(flags)
    for b in range(logits.shape[0]):
        s = int(state[b])
        if bool(done[b]) or s < 0 or s >= n_states:
            continue
        banned = torch.as_tensor(np.asarray(nxt[s][:V]) < 0).clone()
        if eos is not None and 0 <= eos < V:
            banned[eos] = not (int(flags[s]) & 1)
        out[b, :V][banned] = -INF
    return out


def advance(out, n, V, nxt, flags, state, done, end):
    """one step behind the emit: out [B][n_max] ids, n generated tokens -> (state, done, end) as lists"""
    n_max = len(out[0])
    n = min(max(n, 0), n_max)
    state, done, end = [int(s) for s in state], [int(d) for d in done], [int(e) for e in end]
    n_states = len(flags)
    for b in range(len(out)):
        if done[b] or state[b] < 0:
            continue
        s, sn = state[b], -1
        if n >= 1 and s < n_states:
            t = int(out[b][n - 1])
            if 0 <= t < V:
                sn = int(nxt[s][t])
            if sn >= n_states:
                sn = -1
        if sn >= 0:
            state[b] = sn
            if int(flags[sn]) & 2:
                done[b], end[b] = 1, n
        else:
            state[b], done[b], end[b] = -2, 1, n
    return state, done, end


def walk(nxt, ids, start=0):
    """the state behind ids on a (trimmed) table, None when a token is not allowed"""
    s = start
    for t in ids:
        if not 0 <= int(t) < nxt.shape[1] or nxt[s][int(t)] < 0:
            return None
        s = int(nxt[s][int(t)])
    return s


def synthetic_vocab(V, seed, alphabet=None, n_special=3, lengths=(2, 17)):
    """3 specials (None), the 256 single bytes, then random pieces of 2 to 17 bytes over `alphabet` (default: all bytes)"""
    rng = np.random.default_rng(seed)
    alphabet = np.frombuffer(bytes(range(256)) if alphabet is None else alphabet, dtype=np.uint8)
    vocab = [None] * n_special + [bytes([i]) for i in range(256)]
    while len(vocab) < V:
        vocab.append(bytes(rng.choice(alphabet, size=int(rng.integers(lengths[0], lengths[1] + 1))).tolist()))
    return vocab[:V]
