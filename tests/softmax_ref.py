"""float64 reference of csrc/softmax.hip -- the eager attention softmax (forward and backward), the attention dropout
and the shifted cross-entropy -- shared by tests/test_softmax_ce_gpu.py and tests/test_softmax_ref_cpu.py, together with
the elementwise error bounds the kernels are held to, a float32 restatement of every kernel (what the CPU test holds
to the same bounds), and the shapes, masks and seeded inputs both files use.  Nothing here needs a GPU.

Mask rule (softmax.hip `masked`): the score of key k for query q of sample b becomes finfo(dtype).min where
k > q + (Lk - Lq) (causal) or kmask[b, k] == 0 -- what `scores + mask` followed by `max(., finfo.min)` gives in the model
(oracle/restate.py decoder_mask).  A row WITHOUT an allowed key is therefore uniform, 1 / Lk, never NaN.
(fp16 only: the model's own sum rounds -65504 + s back to -65504 while |s| < 16; the inputs of the comparison with
decoder_mask stay below that.)

Dropout rule (common.h mk_hash32 / mk_keep, softmax.hip keep_thr): element (row, k) is kept iff
hash32(seed mod 2^64, row * Lk + k) < min(int((1 - p) * 2^32), 0xFFFFFFFF); the index runs over the Lk real keys of a row,
not over its pitch; p is the fp32 number the kernel receives.  Kept values are multiplied by the fp32 1 / (1 - p).

Bounds.  u_T is the half-ulp of the output type (0 for fp32, 2^-8 for bf16, 2^-11 for fp16), C = 2e-5 the project's fp32
rtol (header of tests/test_kernels_gpu.py), a_T one fp16 subnormal step (2^-24) or 1e-30:
    probabilities   |got - ref| <= ref (u_T + C) + a_T
    dS              |got - ref| <= scale P (|g| + sum |g P|) (u_T + C) + a_T
    row_lse         2e-5 + 2e-5 |lse|                       row_loss   2e-5 + 2e-5 max|logit| of the row
    sum_cnt[0, 2]   2e-5 + 2e-5 |ref|                       sum_cnt[1] exact
    dlogits         (gs / n) (p_c + [c == label]) (u_T + 2e-5 (1 + max|logit| of the row)) + a_T
They are derived -- the final rounding plus fp32 arithmetic (an fp32 `logit - lse` carries an absolute error of the
size of 2e-5 (1 + max|logit|)) -- not fitted to the kernels; tests/test_softmax_ref_cpu.py shows that the float32
restatements below stay inside them at every case listed here.
"""
import numpy as np
import torch

MASK64 = 0xFFFFFFFFFFFFFFFF
C_F32 = 2e-5
DTYPE_TAG = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}


# ------------------------------------------------------------------------------------------------- dropout hash
def hash32(seed, idx):
    """numpy copy of mk_hash32 (csrc/common.h)"""
    with np.errstate(over="ignore"):
        z = idx.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(seed)
        z ^= z >> np.uint64(30)
        z *= np.uint64(0xBF58476D1CE4E5B9)
        z ^= z >> np.uint64(27)
        z *= np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
    return (z >> np.uint64(16)).astype(np.uint32)


def keep_threshold(p):
    """keep_thr (softmax.hip): p arrives as an fp32 kernel argument"""
    return min(int((1.0 - float(np.float32(p))) * 4294967296.0), 0xFFFFFFFF)


def drop_scale(p):
    """the fp32 factor of the kept values: 1.f / (1.f - p), 1 without dropout"""
    p32 = np.float32(p)
    return np.float32(1.0) / (np.float32(1.0) - p32) if p32 > 0 else np.float32(1.0)


def softmax_keep(seed, nrows, Lk, p):
    """[nrows, Lk] bool keep mask of mk_softmax_fwd / mk_softmax_bwd (see the module docstring)"""
    idx = np.arange(nrows * Lk, dtype=np.uint64)
    keep = hash32(seed & MASK64, idx) < np.uint32(keep_threshold(p))
    return torch.from_numpy(keep.reshape(nrows, Lk))


# ------------------------------------------------------------------------------------------------- bounds
def u_of(dtype):
    return {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}[dtype]


def a_of(dtype):
    return 2.0 ** -24 if dtype == torch.float16 else 1e-30


def probs_bound(ref, dtype):
    return ref * (u_of(dtype) + C_F32) + a_of(dtype)


def check_inside(got, ref, bound, what):
    """asserts |got - ref| <= bound elementwise (float64) and returns the worst ratio"""
    got = got.detach().double().cpu()
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    ratio = ((got - ref).abs() / bound).max().item()
    assert ratio <= 1.0, f"{what}: |got - ref| reaches {ratio:.3f} of its bound"
    return ratio


# ------------------------------------------------------------------------------------------------- softmax
def allowed(kmask, causal, B, Lq, Lk):
    """[B, 1, Lq, Lk] bool: key k allowed for query q of sample b"""
    ok = torch.ones(B, 1, Lq, Lk, dtype=torch.bool)
    if causal:
        q = torch.arange(Lq)[:, None]
        k = torch.arange(Lk)[None, :]
        ok = ok & (k <= q + (Lk - Lq))[None, None]
    if kmask is not None:
        ok = ok & (kmask != 0)[:, None, None, :]
    return ok


def masked_scores(s, kmask, causal, Lq, Lk, dtype):
    """s [B, H, Lq, Lk] -> float64 scores with finfo(dtype).min at every key that is not allowed"""
    ok = allowed(kmask, causal, s.shape[0], Lq, Lk)
    return torch.where(ok, s.double(), torch.tensor(torch.finfo(dtype).min, dtype=torch.float64))


def softmax_ref(s, kmask, causal, Lq, Lk, dtype):
    return torch.softmax(masked_scores(s, kmask, causal, Lq, Lk, dtype), -1)


def softmax_bwd_ref(P, dP, keep, p, scale):
    """float64 dS from the kernel's own rounded P: g = dP keep / (1 - p), dS = P (g - sum g P) scale.
    Returns (dS, bound / (u_T + C)) -- see dS_bound."""
    P = P.double()
    g = dP.double() * float(drop_scale(p))
    if keep is not None:
        g = g * keep.view(P.shape).double()
    dS = P * (g - (g * P).sum(-1, keepdim=True)) * scale
    mag = abs(scale) * P * (g.abs() + (g * P).abs().sum(-1, keepdim=True))
    return dS, mag


def dS_bound(mag, dtype):
    return mag * (u_of(dtype) + C_F32) + a_of(dtype)


def softmax_f32(s, kmask, causal, Lq, Lk, dtype):
    """the forward kernels restated in float32 torch, rounded to `dtype`"""
    ok = allowed(kmask, causal, s.shape[0], Lq, Lk)
    x = torch.where(ok, s.float(), torch.tensor(torch.finfo(dtype).min, dtype=torch.float32))
    e = torch.exp(x - x.max(-1, keepdim=True).values)
    return (e * (1.0 / e.sum(-1, keepdim=True))).to(dtype)


def dropped_f32(P, keep, p):
    """probs_dropped from the rounded probabilities: one fp32 multiply, one rounding"""
    scaled = (P.float() * torch.tensor(float(drop_scale(p)), dtype=torch.float32)).to(P.dtype)
    return torch.where(keep.view(P.shape), scaled, torch.zeros((), dtype=P.dtype))


def softmax_bwd_f32(P, dP, keep, p, scale):
    """the backward kernels restated in float32 torch, rounded to P's dtype"""
    Pf = P.float()
    g = dP.float()
    if keep is not None:
        g = torch.where(keep.view(P.shape), g * torch.tensor(float(drop_scale(p)), dtype=torch.float32),
                        torch.zeros((), dtype=torch.float32))
    return (Pf * (g - (g * Pf).sum(-1, keepdim=True)) * scale).to(P.dtype)


# Which kernel mk_softmax_fwd / mk_softmax_bwd select (softmax_fwd_t / softmax_bwd_t), by nch = ld / N with N = 8
# elements per 16 bytes for bf16 / fp16 and 4 for fp32:
#   forward   wave MAXC 1 | 2 | 4 | 8 for nch <= 64 | 128 | 256 | 512, the block kernel above
#             16-bit: ld <= 512 | 1024 | 2048 | 4096 | above       fp32: ld <= 256 | 512 | 1024 | 2048 | above
#   backward  wave MAXC 1 | 2 | 4 for nch <= 64 | 128 | 256, the block kernel above
#             16-bit: ld <= 512 | 1024 | 2048 | above              fp32: ld <= 256 | 512 | 1024 | above
# If the thresholds of softmax.hip move, PITCHES and DROPOUT_PITCHES move with them (test_softmax_ref_cpu.py checks
# that every branch is selected, on both sides of every threshold).
def branch(dtype, ld, backward=False):
    nch = ld // (4 if dtype == torch.float32 else 8)
    for maxc in (1, 2, 4) if backward else (1, 2, 4, 8):
        if nch <= 64 * maxc:
            return f"wave{maxc}"
    return "block"


B, H, LQ = 2, 3, 5             # 30 rows: no multiple of the wave kernels' 4 rows per block
NROWS = B * H * LQ
BWD_SCALE = 0.125
PITCHES = [8, 256, 264, 512, 520, 1024, 1032, 2048, 2056, 4096, 4104]
# (Lk, ld): the tail inside the last vector at every pitch; a full last vector at the first pitch and at the pitches that
# are a threshold; one pad64 pitch with whole pad chunks per kernel family
SWEEP_SHAPES = ([(ld - 3, ld) for ld in PITCHES] + [(8, 8)] + [(ld, ld) for ld in PITCHES[1::2]]
                + [(4099, 4160), (2051, 2112)])
MASK_MODES = ["none", "kmask", "causal_left"]
# (Lk, ld, mask mode, score scale): a sample masked everywhere, and scores ~N(0, 8^2), in a wave and in a block kernel
EXTRA_CASES = [(261, 264, "full1", 2.0), (4101, 4104, "full1", 2.0),
               (1029, 1032, "kmask", 8.0), (4101, 4104, "causal_left", 8.0)]
# one pitch per forward and per backward branch of every dtype (Lk = ld - 3)
DROPOUT_PITCHES = [256, 264, 520, 1032, 2056, 4104]
DROPOUT_P = 0.1
DROPOUT_SEED = 2 ** 40 + 12345
SAME_LK_PITCHES = [(2051, 2056, 2112), (4099, 4104, 4160)]      # (Lk, pad8, pad64)


def kmask_mode(mode, Lk, Lq=LQ):
    """-> ([B, Lk] int32 key mask or None, causal)"""
    if mode == "none":
        return None, False
    km = torch.ones(B, Lk, dtype=torch.int32)
    if mode == "kmask":                 # sample 0 right-padded by 4, sample 1 with holes
        km[0, Lk - 4:] = 0
        km[1, 1::7] = 0
        km[1, Lk // 2:Lk // 2 + 9] = 0
        return km, False
    if mode == "causal_left":           # left padding on sample 1: its query rows 0 and 1 have no allowed key
        km[1, :Lk - Lq + 2] = 0
        return km, True
    if mode == "full1":                 # sample 1 masked everywhere
        km[1] = 0
        return km, False
    raise ValueError(mode)


def make_scores(dtype, Lk, ld, scale=2.0):
    """seeded scores ~N(0, scale^2) and gradient ~N(0, 1), [B, H, LQ, Lk], rounded to `dtype`"""
    g = torch.Generator().manual_seed(Lk * 8191 + ld * 3 + DTYPE_TAG[dtype])
    s = (torch.randn((B, H, LQ, Lk), generator=g) * scale).to(dtype)
    dP = torch.randn((B, H, LQ, Lk), generator=g).to(dtype)
    return s, dP


def uniform_value(Lk, dtype):
    """a row without an allowed key: exp(0) = 1, the sum Lk and 1 / Lk are exact in fp32, one rounding to `dtype`"""
    return (torch.ones((), dtype=torch.float32) / Lk).to(dtype)


# ------------------------------------------------------------------------------------------------- cross-entropy
CE_GS = 1.0                    # the gradient scale of every case: grad_scale 2.0 x device 0.5 == host-only 1.0
CE_CASES = {                   # name: (rows, V, logits)
    "reduce": (700, 1000, "normal"),       # crosses ce_reduce_kernel's 256-row stride twice; ignored and >= V labels
    "vocab": (12, 32003, "normal"),        # V % 256 != 0, 126 strides per thread
    "small": (12, 107, "normal"),          # threads without a column
    "extreme": (12, 32003, "extreme"),     # logits past +-88: no finite result without the max subtraction
    "ignored": (12, 107, "none_valid"),    # n = 0
}


def pad64(n):
    return (n + 63) // 64 * 64


def make_ce(name, dtype):
    """-> (logits [rows, V] rounded to `dtype`, labels int64 [rows], V)"""
    rows, V, kind = CE_CASES[name]
    g = torch.Generator().manual_seed(rows * 131 + V + DTYPE_TAG[dtype])
    x = torch.randn((rows, V), generator=g)
    x = (x * 30).clamp(-200, 200) if kind == "extreme" else x * 2
    labels = torch.randint(0, V, (rows,), generator=g)
    if kind == "none_valid":
        labels[:] = -100
        labels[3], labels[7] = V, V + 7
    else:
        labels[::5] = -100
        if name == "reduce":
            labels[[1, 257, 258, 699]] = V
            labels[[2, 511, 513]] = V + 7
    return x.to(dtype), labels, V


def ce_ref(logits, labels, V, dtype, gs=CE_GS):
    """float64 reference and bounds of mk_cross_entropy / mk_cross_entropy_bwd on the rounded logits"""
    x = logits.double()
    rows = x.shape[0]
    valid = (labels >= 0) & (labels < V)
    lab = torch.where(valid, labels, torch.zeros_like(labels))
    lse = torch.logsumexp(x, -1)
    picked = x.gather(1, lab[:, None])[:, 0]
    zero = torch.zeros((), dtype=torch.float64)
    row_lse = torch.where(valid, lse, zero)
    row_loss = torch.where(valid, lse - picked, zero)
    n = int(valid.sum())
    total = row_loss.sum().item()
    mean = total / n if n else 0.0
    xmax = x.abs().max(-1).values
    onehot = torch.zeros(rows, V, dtype=torch.float64)
    onehot[torch.arange(rows)[valid], lab[valid]] = 1.0
    per_row = torch.where(valid, torch.full((), gs / max(n, 1), dtype=torch.float64), zero)[:, None]
    p = torch.softmax(x, -1)
    return {
        "valid": valid, "n": n, "row_lse": row_lse, "row_loss": row_loss, "sum": total, "mean": mean,
        "row_lse_bound": 2e-5 + 2e-5 * row_lse.abs(),
        "row_loss_bound": 2e-5 + 2e-5 * xmax,
        "sum_bound": 2e-5 + 2e-5 * abs(total), "mean_bound": 2e-5 + 2e-5 * abs(mean),
        "dlogits": (p - onehot) * per_row,
        "dlogits_bound": per_row * (p + onehot) * (u_of(dtype) + 2e-5 * (1.0 + xmax[:, None])) + a_of(dtype),
    }


def ce_f32(logits, labels, V, gs=CE_GS):
    """the cross-entropy kernels restated in float32 torch: (row_loss, row_lse, [sum, n, mean], dlogits in the dtype)"""
    x = logits.float()
    valid = (labels >= 0) & (labels < V)
    lab = torch.where(valid, labels, torch.zeros_like(labels))
    mx = x.max(-1).values
    lse = mx + torch.log(torch.exp(x - mx[:, None]).sum(-1))
    zero = torch.zeros((), dtype=torch.float32)
    row_lse = torch.where(valid, lse, zero)
    row_loss = torch.where(valid, lse - x.gather(1, lab[:, None])[:, 0], zero)
    n = valid.sum().float()
    total = row_loss.sum()
    mean = total / n if n > 0 else zero
    onehot = torch.zeros_like(x)
    onehot[torch.arange(x.shape[0])[valid], lab[valid]] = 1.0
    per_row = torch.where(valid & (n > 0), torch.tensor(gs, dtype=torch.float32) / n.clamp(min=1), zero)[:, None]
    dl = ((torch.exp(x - lse[:, None]) - onehot) * per_row).to(logits.dtype)
    return row_loss, row_lse, torch.stack([total, n, mean]), dl
