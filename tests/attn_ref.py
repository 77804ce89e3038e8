"""fp32 reference of the fused attention kernels (mk_flash_attn_fwd / _bwd), shared by tests/test_attention_edges_gpu.py
and tests/test_attn_ref_cpu.py:  o = softmax(scale Q K^T + mask) V  on the 16-bit inputs, in fp32, with lse and, through
autograd, dq, dk, dv.

Mask rule (the kernels'): key j is visible to query i of sample b iff  kmask[b, j] != 0  and, causal,
j <= i + (Lk - Lq).  A row WITHOUT a visible key gives o = 0, lse = -inf and zero gradients -- and nothing here is ever
NaN: a plain softmax of an all -inf row is NaN, and a torch.where behind it still sends NaN * 0 through autograd.  Such a
row therefore never reaches the softmax: its scores are replaced by constant zeros before it, its probabilities by
constant zeros behind it, so both selects hand its (finite) gradient a zero.

Tensors are token-major as the kernels see them: q, o, dout, dq [B, Lq, H * hd]; k, v, dk, dv [B, Lk, H * hd];
lse [B, H, Lq]; kmask [B, Lk] int32 or None.

The module also holds the shapes, masks and seeded inputs that the GPU tests and the CPU test of this reference share.
"""
import torch

# ---- shapes of the mask census (q = 0), chosen to cross every edge of the kernels: the 64-key tile, the 32-key
# sub-block, the 32-row wave slice, the 128 / 256-row block, the 160-row limit of the short-sequence kernels
CENSUS_SHAPES = [  # (Lq, Lk, causal)
    (1, 1, True), (64, 64, True), (65, 129, True), (129, 65, True), (160, 160, True), (161, 161, True),
    (300, 520, True), (520, 300, True),
    (31, 33, False), (257, 257, False), (520, 520, False),
]
# right padding of 1, 31, 32, 33 and 64 keys needs five samples; with B = 3 it is spread over two patterns
CENSUS_MASKS = ["none", "padA", "padB", "hole"]

# ---- backward edges on random data: (Lq, Lk, causal, kmask pattern)
BWD_EDGE_CASES = [
    (200, 200, True, "pad37"),      # the LLaMA layer beyond the short-kernel limit: causal + key padding
    (130, 300, True, "none"),       # Lk > Lq: every row sees a prefix of 170 extra keys
    (300, 130, True, "none"),       # Lq > Lk: rows 0 .. 169 see nothing (dq exactly 0)
    (5, 333, True, "none"),         # a handful of rows over six key tiles
    (257, 257, False, "full1"),     # one sample with every key padded (its dq, dk, dv exactly 0)
    (520, 520, False, "pad77"),     # five query blocks, padding, B H = 9
]


def kmask_pattern(name, B, Lk):
    """[B, Lk] int32 key-validity mask, or None for "none" """
    if name == "none":
        return None
    km = torch.ones(B, Lk, dtype=torch.int32)
    if name in ("padA", "padB"):
        pads = {"padA": (1, 31, 32), "padB": (33, 64, 0)}[name]
        for b in range(B):
            p = min(pads[b % 3], Lk)                # (a sequence shorter than the padding: fully padded)
            if p:
                km[b, Lk - p:] = 0
    elif name == "hole":                            # a hole [40, 70) on sample 0, sample 1 fully padded
        km[0, 40:70] = 0
        km[1 % B] = 0
    elif name == "pad37":
        km[1 % B, Lk - 37:] = 0
        km[2 % B, Lk - 64:] = 0
    elif name == "pad77":
        km[1 % B, Lk - 77:] = 0
        km[2 % B, Lk - 130:] = 0
    elif name == "full1":
        km[1 % B] = 0
    elif name == "pad11":                           # (what the short-sequence tests of test_kernels_gpu.py pad)
        p = min(11, Lk - 1)
        if p:
            km[1 % B, Lk - p:] = 0
    else:
        raise ValueError(name)
    return km


def visible(B, Lq, Lk, causal, kmask):
    """[B, Lq, Lk] bool: key j visible to query i of sample b"""
    vis = torch.ones(B, Lq, Lk, dtype=torch.bool)
    if causal:
        i = torch.arange(Lq)[:, None]
        j = torch.arange(Lk)[None, :]
        vis = vis & (j <= i + (Lk - Lq))[None]
    if kmask is not None:
        vis = vis & (kmask != 0)[:, None, :]
    return vis


def make_inputs(seed, dtype, B, H, Lq, Lk, hd, qk_scale=0.7, zero_q=False):
    """seeded q, k, v (N(0, qk_scale^2)) and dout (N(0, 1)) rounded to `dtype`, token-major"""
    g = torch.Generator().manual_seed(seed)
    D = H * hd
    q, k, v = ((torch.randn((B, L, D), generator=g) * qk_scale).to(dtype) for L in (Lq, Lk, Lk))
    do = torch.randn((B, Lq, D), generator=g).to(dtype)
    if zero_q:
        q = torch.zeros_like(q)
    return q, k, v, do


def attention_ref(q, k, v, H, scale, causal=False, kmask=None, dout=None):
    """dict(o, lse) and, with dout, dict(o, lse, dq, dk, dv): fp32, token-major (see the module docstring)"""
    B, Lq, D = q.shape
    Lk = k.shape[1]
    hd = D // H
    need_grad = dout is not None
    qf = q.float().view(B, Lq, H, hd).transpose(1, 2).detach().clone().requires_grad_(need_grad)
    kf = k.float().view(B, Lk, H, hd).transpose(1, 2).detach().clone().requires_grad_(need_grad)
    vf = v.float().view(B, Lk, H, hd).transpose(1, 2).detach().clone().requires_grad_(need_grad)
    vis = visible(B, Lq, Lk, causal, kmask)[:, None]              # [B, 1, Lq, Lk]
    alive = vis.any(-1, keepdim=True)                             # [B, 1, Lq, 1]: the row has a visible key
    s = (qf @ kf.transpose(-1, -2)) * scale
    s = s.masked_fill(~vis, float("-inf"))
    s = torch.where(alive, s, torch.zeros((), dtype=s.dtype))     # a dead row enters the softmax as constant zeros
    p = torch.softmax(s, -1)
    p = torch.where(alive, p, torch.zeros((), dtype=p.dtype))     # ... and leaves it as constant zeros
    o = p @ vf
    with torch.no_grad():
        lse = torch.where(alive[..., 0], torch.logsumexp(s, -1), torch.full((), float("-inf")))
    out = {"o": o.detach().transpose(1, 2).reshape(B, Lq, D), "lse": lse.expand(B, H, Lq).contiguous()}
    if need_grad:
        o.backward(dout.float().view(B, Lq, H, hd).transpose(1, 2))
        out["dq"] = qf.grad.transpose(1, 2).reshape(B, Lq, D)
        out["dk"] = kf.grad.transpose(1, 2).reshape(B, Lk, D)
        out["dv"] = vf.grad.transpose(1, 2).reshape(B, Lk, D)
    return out


def census_expect(v, H, Lq, causal, kmask):
    """q = 0: every visible score is exactly 0, so lse[b, h, i] = log(n_visible(b, i)) and o is the mean of the visible
    v rows.  Returns (n [B, Lq] int64, lse [B, H, Lq] float64 with -inf at n = 0, o [B, Lq, D] float64)."""
    B, Lk, D = v.shape
    vis = visible(B, Lq, Lk, causal, kmask)
    n = vis.sum(-1)
    lse = torch.where(n > 0, torch.log(n.double().clamp(min=1)), torch.full((), float("-inf"), dtype=torch.float64))
    o = (vis.double() @ v.double()) / n.clamp(min=1)[..., None].double()
    return n, lse[:, None, :].expand(B, H, Lq).contiguous(), o
