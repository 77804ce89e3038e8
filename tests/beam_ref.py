"""The beam-search rule of include/macaw_hip.h ("Beam search") restated in numpy float64 -- the reference that
mk_beam_emit (csrc/beam.hip) and generate(num_beams=K) are pinned to -- and the input generator of the GPU selection
test (tests/test_beam_gpu.py), whose precondition tests/test_beam_cpu.py asserts.

BeamRef holds the books of B samples in plain arrays with the device's layout, so that a test can load a prepared
mid-search state into both and compare every field after a step."""
import numpy as np


def candidates(scores, logits):
    """cand(k, c) = s_k + (x_kc - lse_k) in float64, [K_in, V]; -inf wherever it is not finite (a NaN or -inf logit, a
    -inf score, a row without a finite logit or with +inf in it)"""
    x = np.asarray(logits, dtype=np.float64)
    s = np.asarray(scores, dtype=np.float64)[:x.shape[0]]
    out = np.full(x.shape, -np.inf)
    for k in range(x.shape[0]):
        ok = ~np.isnan(x[k]) & (x[k] != -np.inf)
        if not ok.any() or not np.isfinite(x[k][ok]).all() or not np.isfinite(s[k]):
            continue
        m = x[k][ok].max()
        lse = m + np.log(np.exp(x[k][ok] - m).sum())
        out[k][ok] = s[k] + (x[k][ok] - lse)
    out[~np.isfinite(out)] = -np.inf
    return out


def ranked(cand, n):
    """the n best finite candidates as flat indices k * V + c, by value descending, ties to the lower flat index"""
    flat = cand.reshape(-1)
    idx = np.flatnonzero(np.isfinite(flat))
    order = idx[np.lexsort((idx, -flat[idx]))]
    return order[:n]


class BeamRef:
    def __init__(self, B, K, n_max, pad, eos, length_penalty=1.0, early_stopping=False):
        self.B, self.K, self.n_max, self.pad = B, K, n_max, pad
        self.eos = -1 if eos is None else eos
        self.lp, self.early = float(length_penalty), bool(early_stopping)
        self.tok = np.full((B, K), pad, dtype=np.int64)
        self.scores = np.zeros((B, K))
        self.hist = np.zeros((n_max, B, K, 2), dtype=np.int64)
        self.ind = np.zeros((B, K, n_max), dtype=np.int64)
        self.pool = [[] for _ in range(B)]          # entries [score, column of the eos, parent beam, insertion number]
        self.seq = [0] * B
        self.done = [False] * B
        self.col = 0

    def insert(self, b, score, col, parent):
        pool, K = self.pool[b], self.K
        entry = [score, col, parent, self.seq[b]]
        self.seq[b] += 1
        if len(pool) < K:
            pool.append(entry)
            return
        w = 0
        for e in range(1, K):
            if pool[e][0] < pool[w][0] or (pool[e][0] == pool[w][0] and pool[e][3] > pool[w][3]):
                w = e
        if score > pool[w][0]:
            pool[w] = entry

    def step(self, logits):
        """logits [B, K_in, V] (anything numpy converts; their float64 values are the inputs)"""
        K, col = self.K, self.col
        L = col + 1
        pen = float(L) ** self.lp
        for b in range(self.B):
            if self.done[b]:
                self.tok[b] = self.pad
                self.hist[col, b, :, 0] = self.pad
                self.hist[col, b, :, 1] = np.arange(K)
                self.ind[b, :, col] = np.arange(K)
                continue
            x = np.asarray(logits[b], dtype=np.float64)
            V = x.shape[1]
            cand = candidates(self.scores[b], x)
            flat = cand.reshape(-1)
            parent, tok, sc = [], [], []
            for r, f in enumerate(ranked(cand, 2 * K)):
                k, c = int(f) // V, int(f) % V
                if c == self.eos:
                    if r < K:
                        self.insert(b, flat[f] / pen, col, k)
                    continue
                parent.append(k), tok.append(c), sc.append(flat[f])
                if len(parent) == K:
                    break
            while len(parent) < K:
                parent.append(0), tok.append(self.pad), sc.append(-np.inf)
            self.scores[b] = sc
            self.tok[b] = tok
            self.hist[col, b, :, 0] = tok
            self.hist[col, b, :, 1] = parent
            self.ind[b, :, :col] = self.ind[b, parent, :col]
            self.ind[b, :, col] = np.arange(K)
            if len(self.pool[b]) == K:
                worst = min(e[0] for e in self.pool[b])
                self.done[b] = self.early or sc[0] / pen <= worst
        self.col += 1

    def sequence(self, b, col, k):
        """the tokens of beam k of sample b at output column col"""
        seq = []
        for i in range(col, -1, -1):
            t, k = self.hist[i, b, k]
            seq.append(int(t))
        return seq[::-1]

    def finalize(self, num_return_sequences=1):
        """after the last step -> (rows: B * nret lists of ids, scores): unfinished samples add their finite running
        beams in beam order; the pool by score descending, ties to the earlier insertion"""
        rows, scores = [], []
        pen = float(self.col) ** self.lp
        for b in range(self.B):
            if not self.done[b]:
                for k in range(self.K):
                    if np.isfinite(self.scores[b, k]):
                        self.insert(b, self.scores[b, k] / pen, -1, k)       # column -1: a running beam, no eos
            for e in sorted(self.pool[b], key=lambda e: (-e[0], e[3]))[:num_return_sequences]:
                rows.append(self.sequence(b, self.col - 1, e[2]) if e[1] < 0 else
                            self.sequence(b, e[1] - 1, e[2]) + [self.eos])
                scores.append(e[0])
        return rows, scores


def padded(rows, pad):
    width = max(1, max(len(r) for r in rows))
    return [r + [pad] * (width - len(r)) for r in rows]


# ----------------------------------------------------------------- the inputs of the GPU selection test --
# (B, K, K_in, V, pitch, dtype, spiked, seed).  spiked: 2K + 4 values 2, 2.25, ... (exact in every dtype) at random
# places, two or more per row, over a bulk near -30 -- 16-bit logits drawn from a continuous distribution tie within a
# row (bf16 has 8 bits), and a tie among the best 2K + 1 candidates is what the precondition below excludes; the ties
# have a test of their own.  Unspiked cases are fp32 draws.  The seeds were chosen so that the precondition holds.
CASES = [
    (1, 1, 1, 32, 32, "float32", True, 0),
    (3, 2, 2, 32, 40, "bfloat16", True, 0),
    (3, 4, 1, 1000, 1000, "float16", True, 0),
    (3, 4, 4, 1000, 1000, "bfloat16", True, 0),
    (1, 16, 16, 1000, 1008, "float32", True, 0),
    (3, 16, 1, 32, 32, "bfloat16", True, 0),
    (1, 4, 4, 32007, 32064, "bfloat16", True, 0),
    (3, 16, 16, 32007, 32064, "bfloat16", True, 0),
    (3, 2, 2, 32007, 32064, "float16", True, 0),
    (1, 16, 16, 32007, 32064, "float32", False, 0),
    (3, 4, 4, 1000, 1000, "float32", False, 0),
    (1, 1, 1, 32007, 32064, "bfloat16", True, 0),
]
EOS_COL = 5
MIN_GAP = 1e-4


def case_id(case):
    B, K, K_in, V, ld, dtype, spiked, seed = case
    return f"B{B}-K{K}-Kin{K_in}-V{V}-{dtype}-{'spiked' if spiked else 'plain'}"


def beam_inputs(case):
    """-> (logits float32 numpy [B * K_in, ld] BEFORE rounding to the case's dtype, columns [V, ld) = 1e4 which no kernel
    may read; scores float32 [B, K], zero for K_in = 1).  A few spikes of every sample sit in column EOS_COL."""
    B, K, K_in, V, ld, dtype, spiked, seed = case
    g = np.random.default_rng(1000 * seed + 7 * V + 31 * K + B + K_in)
    x = np.full((B * K_in, ld), 1e4, dtype=np.float32)
    if spiked:
        x[:, :V] = g.standard_normal((B * K_in, V)).astype(np.float32) * 0.5 - 30.0
        n_sp = min(V, 2 * K + 4)
        for b in range(B):
            vals = 2.0 + 0.25 * g.permutation(n_sp)
            for j in range(n_sp):
                row = b * K_in + j % K_in
                if j < min(3, K_in):
                    c = EOS_COL
                else:
                    c = int(g.integers(0, V))
                    while x[row, c] > -10 or c == EOS_COL:
                        c = (c + 1) % V
                x[row, c] = vals[j]
    else:
        x[:, :V] = g.standard_normal((B * K_in, V)).astype(np.float32) * 3.0
    scores = np.zeros((B, K), dtype=np.float32)
    if K_in == K and K > 1:
        scores = (-3.0 * g.random((B, K))).astype(np.float32)
    return x, scores


def top_gaps(case, quantise):
    """the precondition: for every sample the gaps between consecutive entries of the best 2K + 1 float64 candidates
    of the QUANTISED logits (quantise: float32 array -> the case dtype's values as float64).  -> the smallest gap"""
    B, K, K_in, V, ld, dtype, spiked, seed = case
    x, scores = beam_inputs(case)
    xq = quantise(x)[:, :V]
    worst = np.inf
    for b in range(B):
        cand = candidates(scores[b].astype(np.float64), xq[b * K_in:(b + 1) * K_in])
        top = cand.reshape(-1)[ranked(cand, 2 * K + 1)]
        assert len(top) >= min(2 * K + 1, K_in * V)
        worst = min(worst, float(np.min(top[:-1] - top[1:])))
    return worst
