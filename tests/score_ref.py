"""The rule of LlamaForCausalLM.score() (include/macaw_hip.h, "Scoring"), restated in plain Python, shared by
tests/test_score_cpu.py, tests/test_score_attn_gpu.py and tests/test_score_gpu.py.

There are B prompts.  Prompt b has L_b valid tokens and n_b <= n options.  Option (b, j) is a token list c[0 ... len - 1],
len >= 1.  Its result is, for g = 0 ... len - 1:

    lp[b, j, g] = log_softmax(logits of the model at position L_b + g - 1, given prompt b followed by c[0 ... g - 1])[c[g]]

- Positions are 0 ... L_b + len - 1: exactly what a fresh call on the concatenation alone computes, and what
  generate(return_logprobs=True) reports for a token it emitted itself.
- Token 0 of every option of prompt b is predicted by the prompt's last valid hidden row; it is computed once per prompt.
- Token g >= 1 is predicted by the hidden row of fed token g - 1, so an option FEEDS its first len - 1 tokens: the pass has
  F = (longest option) - 1 rows per option, and with F = 0 no pass runs at all.
- The arithmetic of a value is mk_token_logprobs' (fp64 log-sum-exp, one rounding).

The layout of the pass: row (b * n + j) * F + g carries fed token g of option (b, j); lens[b * n + j] = max(len - 1, 0) of
them are live; a dead row feeds id 0.  mk_score_attn runs live row g of option (b, j) at position L_b + g over prompt rows
0 ... L_b - 1 and tail rows 0 ... g of the option.
"""


def layout(continuations):
    """continuations: B lists of token-id lists -> dict(n, F, Lc, fed [B * n * F], lens [B * n], targets [B][n][Lc],
    lengths [B][n]), plain lists; absent options (j >= n_b) have length 0"""
    B = len(continuations)
    n = max(len(p) for p in continuations)
    Lc = max(len(o) for p in continuations for o in p)
    F = Lc - 1
    fed, lens = [], []
    targets = [[[0] * Lc for _ in range(n)] for _ in range(B)]
    lengths = [[0] * n for _ in range(B)]
    for b in range(B):
        for j in range(n):
            o = list(continuations[b][j]) if j < len(continuations[b]) else []
            lengths[b][j] = len(o)
            lens.append(max(len(o) - 1, 0))
            for g in range(F):
                fed.append(o[g] if g < len(o) - 1 else 0)
            for g, t in enumerate(o):
                targets[b][j][g] = t
    return dict(n=n, F=F, Lc=Lc, fed=fed, lens=lens, targets=targets, lengths=lengths)


def fed_rows(lens, F):
    """f of the kernel: clamp(len, 0, F) per option"""
    return [min(max(x, 0), F) for x in lens]


def prompt_len(S0, off):
    """L_b of mk_score_attn (off = t_off[b], 0 without a t_off)"""
    return min(max(S0 + off, 0), S0)


def live_rows(lens, F):
    """[(option, g)] of the live rows of a pass, in row order"""
    return [(r, g) for r, f in enumerate(fed_rows(lens, F)) for g in range(f)]


def scored_context(prompt, option, g):
    """the ids the model has seen when it predicts token g of the option, and the position of the predicting row"""
    ctx = list(prompt) + list(option[:g])
    return ctx, len(ctx) - 1


def log_softmax_pick(row, t):
    """log_softmax(row)[t] in Python floats (fp64): the value of one scored token from its logits row"""
    import math
    mx = max(row)
    return row[t] - mx - math.log(sum(math.exp(x - mx) for x in row))
