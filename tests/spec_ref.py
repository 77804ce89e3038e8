"""Prompt-lookup speculative decoding, restated in numpy (no torch, no GPU): the rule of include/macaw_hip.h ("Prompt-lookup
speculative decoding") that mk_spec_lookup, mk_spec_verify_emit (csrc/spec.hip) and generate(prompt_lookup_num_tokens=G)
are pinned to.

  lookup    the draft of one sample: transformers' PromptLookupCandidateGenerator.get_candidates without a logits processor
  argmax    the first argmax of a row with mk_argmax_rows' treatment of NaN (the first NaN wins) and -inf
  verify    one verify-and-emit step of one sample's books
  simulate  the whole loop of one sample, with a given emitted sequence itself as the model"""
import numpy as np


def lookup(history, G, max_ngram, eos=-1, V=None):
    """history: the ids of prompt ++ emitted tokens.  Returns the draft (a list of at most G ids)."""
    h = [int(x) for x in history]
    L = len(h)
    ok = (lambda x: 0 <= x < V) if V is not None else (lambda x: True)
    for n in range(min(max_ngram, L - 1), 0, -1):
        tail = h[L - n:]
        if not all(ok(x) for x in tail):            # an id outside the vocabulary equals nothing
            continue
        for i in range(L - n):                      # i + n < L: the trailing window itself is never a match
            if h[i:i + n] == tail:
                draft = h[i + n:min(i + n + G, L)]
                for j, x in enumerate(draft):       # cut BEFORE the first eos (or id outside the vocabulary)
                    if x == eos or not ok(x):
                        draft = draft[:j]
                        break
                return draft                        # the first n with a match decides, even when nothing is left
    return []


def argmax(row):
    """row: a 1-D float array -> the column torch.argmax / mk_argmax_rows selects"""
    row = np.asarray(row, dtype=np.float64)
    nan = np.isnan(row)
    if nan.any():
        return int(np.argmax(nan))
    return int(np.argmax(row))                      # the first maximum; a row of -inf gives column 0


class Books:
    """the per-sample state of the rule for ONE sample (plain Python values)"""

    def __init__(self, G, max_new, pad, pos=0):
        self.G, self.max_new, self.pad = G, max_new, pad
        self.pos, self.n_out, self.done, self.steps = pos, 0, False, 0
        self.out = [pad] * max_new
        self.tok = [pad] * (G + 1)
        self.n_draft = 0

    def fields(self):
        return dict(pos=self.pos, n_out=self.n_out, done=self.done, steps=self.steps, out=list(self.out),
                    tok=list(self.tok), n_draft=self.n_draft)


def draft_into(bk, prompt, max_ngram, eos=-1, V=None):
    """mk_spec_lookup for one sample: writes tok[1:] and n_draft"""
    d = [] if bk.done else lookup(list(prompt) + bk.out[:bk.n_out], bk.G, max_ngram, eos, V)
    bk.n_draft = len(d)
    bk.tok[1:] = d + [bk.pad] * (bk.G - len(d))


def verify(bk, a, eos=-1):
    """mk_spec_verify_emit for one sample: a = the argmax of each of its rows (G + 1 for a step, 1 for token 0, where
    the draft is not read).  Returns the number of tokens emitted."""
    if bk.done:
        return 0
    nd = bk.n_draft if len(a) > 1 else 0
    A = 0
    while A < nd and bk.tok[1 + A] == a[A]:
        A += 1
    emit = [int(x) for x in a[:A + 1]]
    if eos in emit:
        emit = emit[:emit.index(eos) + 1]           # cut after the first eos, inclusive
    emit = emit[:bk.max_new - bk.n_out]
    m = len(emit)
    bk.out[bk.n_out:bk.n_out + m] = emit
    bk.n_out += m
    bk.pos += m
    bk.steps += 1
    if m:
        bk.tok[0] = emit[-1]
    if (m and emit[-1] == eos) or bk.n_out == bk.max_new:
        bk.done = True
    return m


def simulate(history, emitted, G, n, eos, max_new):
    """The whole loop of one sample with `emitted` itself as the model: at every row the model's argmax is the next id of
    `emitted` (ids past its end never equal a draft token).  history: the prompt ids; emitted: what the model emits under
    greedy decoding, up to and including its eos if it has one.  Returns (tokens emitted per step, steps); token 0 is a
    step without a draft."""
    emitted = [int(x) for x in emitted]
    bk = Books(G, max_new, pad=-7)

    def model(k):                                   # the argmax of the row that follows k emitted tokens
        return emitted[k] if k < len(emitted) else -1

    counts = [verify(bk, [model(0)], eos)]
    while not bk.done and bk.n_out < len(emitted):
        draft_into(bk, history, n, eos)
        # row g sees the emitted tokens and the draft up to g: its argmax is the model's only while the draft was right
        a, k = [], bk.n_out
        for g in range(G + 1):
            a.append(model(k + g))
            if g < bk.n_draft and bk.tok[1 + g] != a[g]:
                a += [-2] * (G - g)                 # rows behind a wrong draft token are never used
                break
        counts.append(verify(bk, a, eos))
    return counts, bk.steps
