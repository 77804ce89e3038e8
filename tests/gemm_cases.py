"""Case table and float64 reference of tests/test_gemm_plans_gpu.py (checked on the CPU by tests/test_gemm_cases_cpu.py).

A case is a Problem: CPU buffers exactly as the kernel will see them on the device (pitches, batch strides, element offsets),
the descriptor fields, and a reference that is computed from those same buffers by explicit index arithmetic -- a Python loop
over (z1, z2) that forms `offset + z1 s1 + z2 s2 + row ld + col` itself and gathers, in float64.  It shares nothing with the
kernels' addressing and uses no view / transpose of the buffers.

The plan rules of the launcher (csrc/gemm.hip, mk_gemm) restated, n = planned CUs:
  256 x 256 kernels (cfg 11, cfg 15): T = ceil(M/256) ceil(N/256) per batch, R = T mod n
    eighths  iff R > 0 and 8R <= n and A is K-major;  else quarters iff R > 0 and 4R <= 2n;  else no tail
    dp_tiles = T - R with a tail, T without;  cfg 11 walks iff nbatch == 1, n % 8 == 0, dp_tiles > n, dp_tiles % n == 0
    cfg 15 runs the whole tiles iff dp_tiles >= n (tail = a second launch on v7), walks only with its register epilogue;
    with dp_tiles < n it runs on v7 and the profile says 11
  128 x 128 kernels: cfg 5 slots = 2n, K-tile 64;  both operands reduction-major = cfg 7: slots = 4n, K-tile 32
    Tb = tiles nbatch, R = Tb mod slots, sp = min(slots / R, nkt / 2, 64);  split iff R > 0 and sp >= 2,
    kt_per_piece = ceil(nkt / sp), dp_tiles = Tb - R, workspace need = 4096 + R sp 65536 bytes
"""
import math

import torch

SLAB_BYTES = 64 * 256 * 4          # one K-piece's fp32 accumulators of a 128 x 128 tile
COUNTER_BYTES = 4096               # arrival counters at the head of the workspace


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------ the rules --
def plan256(n, M, N, a_red, nbatch=1):
    """(dp_tiles, tail, tiles per walking workgroup or 0) of the 256 x 256 kernels"""
    T = cdiv(M, 256) * cdiv(N, 256)
    R = T % n
    if R > 0 and 8 * R <= n and not a_red:
        tail = "eighths"
    elif R > 0 and 4 * R <= 2 * n:
        tail = "quarters"
    else:
        tail = None
    dp = T - R if tail else T
    walk = dp // n if (nbatch == 1 and n % 8 == 0 and dp > n and dp % n == 0) else 0
    return dp, tail, walk


def label256(n, M, N, a_red, nbatch=1):
    dp, tail, walk = plan256(n, M, N, a_red, nbatch)
    return (f"walk×{walk}" if walk else f"{dp} whole") + (f"+{tail}" if tail else "")


def plan128(n, M, N, K, a_red, b_red, nbatch=1):
    both = a_red and b_red
    slots, bk = n * (4 if both else 2), (32 if both else 64)
    per = cdiv(M, 128) * cdiv(N, 128)
    Tb, nkt = per * nbatch, cdiv(K, bk)
    R = Tb % slots
    sp = min(slots // R, nkt // 2, 64) if R else 1
    split = R > 0 and sp >= 2
    return dict(cfg=7 if both else 5, per=per, Tb=Tb, nkt=nkt, R=R, sp=sp if split else 1, dp=Tb - R if split else Tb,
                kpp=cdiv(nkt, sp) if split else 0, need=COUNTER_BYTES + R * sp * SLAB_BYTES if split else 0)


def label128(n, M, N, K, a_red, b_red, nbatch=1):
    p = plan128(n, M, N, K, a_red, b_red, nbatch)
    if p["sp"] < 2:
        return "no split, tail tile" if p["R"] else "no split"
    pieces = [max(0, min(p["nkt"], (i + 1) * p["kpp"]) - i * p["kpp"]) for i in range(p["sp"])]
    kind = "empty piece" if 0 in pieces else "short last piece" if pieces[-1] < p["kpp"] else "even"
    return f"split sp={p['sp']} {kind}"


# --------------------------------------------------------------- the table: A --
LAYOUTS = [(False, False), (False, True), (True, False), (True, True)]     # (a_red, b_red)

# n, M, N, K, C pitch, plan with A K-major, plan with A reduction-major, also on cfg 15 (whole tiles only)
A_ROWS = [
    (8, 512, 1024, 128, 1032, "8 whole", "8 whole", True),
    (8, 768, 768, 192, 776, "8 whole+eighths", "8 whole+quarters", True),
    (8, 700, 760, 448, 763, "8 whole+eighths", "8 whole+quarters", False),
    (8, 768, 1024, 128, 1032, "8 whole+quarters", "8 whole+quarters", True),
    (8, 768, 1280, 192, 1288, "15 whole", "15 whole", True),
    (8, 1024, 1024, 448, 1032, "walk×2", "walk×2", True),
    (8, 1024, 1536, 128, 1544, "walk×3", "walk×3", True),
    (8, 4352, 256, 192, 264, "walk×2+eighths", "walk×2+quarters", True),
    (8, 1536, 768, 448, 776, "walk×2+quarters", "walk×2+quarters", True),
    (12, 1024, 1536, 128, 1544, "24 whole", "24 whole", True),
    (12, 3328, 256, 192, 264, "12 whole+eighths", "12 whole+quarters", True),
    (16, 1536, 768, 448, 776, "16 whole+eighths", "16 whole+quarters", True),
]
A_IDS = [f"n{r[0]}-{r[1]}x{r[2]}x{r[3]}" for r in A_ROWS]
A_PLANS = ["8 whole", "8 whole+eighths", "8 whole+quarters", "15 whole", "walk×2", "walk×3", "walk×2+eighths",
           "walk×2+quarters", "24 whole", "12 whole+eighths", "12 whole+quarters", "16 whole+eighths", "16 whole+quarters"]
# the shapes of the automatic-choice test (9, 16 and 17 tiles under 8 planned CUs)
AUTO_SHAPES = [(768, 768, 192), (1024, 1024, 448), (4352, 256, 192)]

# --------------------------------------------------------------- the table: B --
# cfg, n, M, N, K, plan.  cfg 5: 17 tiles against 16 slots; cfg 7 (both operands reduction-major): 33 against 32, the
# K list of cfg 5 (all even splits at a K-tile of 32) and three more K for the other piece shapes.
B_ROWS = [
    (5, 8, 2176, 128, 1152, "split sp=9 even"),
    (5, 8, 2176, 128, 448, "split sp=3 short last piece"),
    (5, 8, 2176, 128, 576, "split sp=4 empty piece"),
    (5, 8, 2176, 128, 128, "no split, tail tile"),
    (7, 8, 4224, 128, 1152, "split sp=18 even"),
    (7, 8, 4224, 128, 448, "split sp=7 even"),
    (7, 8, 4224, 128, 576, "split sp=9 even"),
    (7, 8, 4224, 128, 128, "split sp=2 even"),
    (7, 8, 4224, 128, 224, "split sp=3 short last piece"),
    (7, 8, 4224, 128, 288, "split sp=4 empty piece"),
    (7, 8, 4224, 128, 64, "no split, tail tile"),
]
B_IDS = [f"cfg{r[0]}-K{r[4]}" for r in B_ROWS]
B_PLANS = {5: ["split sp=9 even", "split sp=3 short last piece", "split sp=4 empty piece", "no split, tail tile"],
           7: ["split sp=18 even", "split sp=3 short last piece", "split sp=4 empty piece", "no split, tail tile"]}


def b_layouts(cfg):
    return [(True, True)] if cfg == 7 else LAYOUTS[:3]


# ------------------------------------------------------------------- problems --
def rounded(shape, dtype, g, scale=1.0):
    """seeded normal values rounded to the element type on the CPU"""
    return (torch.randn(shape, generator=g) * scale).to(dtype)


def _nan(shape, dtype):
    return torch.full(shape, float("nan"), dtype=dtype)


def act64(v, act):
    if act == 1:
        return 0.5 * v * (1.0 + torch.special.erf(v / math.sqrt(2.0)))
    if act == 2:
        return v * torch.sigmoid(1.702 * v)
    return v


class Problem:
    """one mk_gemm call: CPU buffers (any shape, contiguous; addressed flat) + descriptor fields"""

    def __init__(self, name, dtype, M, N, K, A, B, C, lda, ldb, ldc, *, a_red=False, b_red=False, nb1=1, nb2=1,
                 sA=(0, 0), sB=(0, 0), sC=(0, 0), sR=(0, 0), a_off=0, b_off=0, c_off=0, r_off=0, R=None, ldr=0,
                 bias=None, act=0, alpha=1.0, accumulate=False, added=0.0):
        self.name, self.dtype, self.M, self.N, self.K = name, dtype, M, N, K
        self.A, self.B, self.C, self.R, self.bias = A, B, C, R, bias
        self.lda, self.ldb, self.ldc, self.ldr = lda, ldb, ldc, ldr
        self.a_red, self.b_red, self.nb1, self.nb2 = a_red, b_red, nb1, nb2
        self.sA, self.sB, self.sC, self.sR = sA, sB, sC, sR
        self.a_off, self.b_off, self.c_off, self.r_off = a_off, b_off, c_off, r_off
        self.act, self.alpha, self.accumulate = act, alpha, accumulate
        # bound of tests/test_kernels_gpu.py::_close: scale = 0.1 sqrt(K) + the magnitude of the added terms
        self.scale = 0.1 * math.sqrt(K) + added
        self._ref = None

    @property
    def nbatch(self):
        return self.nb1 * self.nb2

    def gemm_args(self):
        """keyword arguments of ops.gemm_raw besides the tensors"""
        return dict(a_red=self.a_red, b_red=self.b_red, ldr=self.ldr, bias_mode=1 if self.bias is not None else 0,
                    act=self.act, accumulate=self.accumulate, alpha=self.alpha, nb1=self.nb1, nb2=self.nb2, sA=self.sA,
                    sB=self.sB, sC=self.sC, sR=self.sR, a_off=self.a_off, b_off=self.b_off, c_off=self.c_off,
                    r_off=self.r_off)

    def reference(self):
        """(index of every logical output element in the flat C buffer, its float64 reference value), batches concatenated"""
        if self._ref is not None:
            return self._ref
        M, N, K = self.M, self.N, self.K
        m, n, k = torch.arange(M)[:, None], torch.arange(N)[None, :], torch.arange(K)
        A64, B64, C64 = (t.reshape(-1).double() for t in (self.A, self.B, self.C))
        R64 = self.R.reshape(-1).double() if self.R is not None else None
        idx, val = [], []
        for z1 in range(self.nb1):
            for z2 in range(self.nb2):
                a0 = self.a_off + z1 * self.sA[0] + z2 * self.sA[1]
                b0 = self.b_off + z1 * self.sB[0] + z2 * self.sB[1]
                c0 = self.c_off + z1 * self.sC[0] + z2 * self.sC[1]
                Al = A64[a0 + (k[None, :] * self.lda + m if self.a_red else m * self.lda + k[None, :])]        # [M, K]
                Bl = B64[b0 + (k[:, None] * self.ldb + n if self.b_red else n * self.ldb + k[:, None])]        # [K, N]
                v = self.alpha * (Al @ Bl)
                if self.bias is not None:
                    v = v + self.bias.double()[None, :]
                v = act64(v, self.act)
                if R64 is not None:
                    v = v + R64[self.r_off + z1 * self.sR[0] + z2 * self.sR[1] + m * self.ldr + n]
                ci = c0 + m * self.ldc + n
                if self.accumulate:
                    v = v + C64[ci]
                idx.append(ci.reshape(-1))
                val.append(v.reshape(-1))
        self._ref = (torch.cat(idx), torch.cat(val))
        return self._ref


EPILOGUES = {
    # name: (alpha, bias, act, residual, accumulate)
    "plain": (1.0, False, 0, False, False),
    "alpha+bias+residual+accumulate": (0.5, True, 0, True, True),      # tests/test_kernels_gpu.py, walkers and eighth tail
    "alpha+residual": (0.5, False, 0, True, False),                   # gemm_v9's register epilogue
    "bias": (1.0, True, 0, False, False),
    "bias+gelu+residual+accumulate": (1.0, True, 1, True, True),
}


def single(dtype, M, N, K, a_red, b_red, epilogue="plain", ldc=None, seed=0):
    """one product, C (and R) pitched wider than N, pad columns NaN"""
    alpha, has_bias, act, has_r, acc = EPILOGUES[epilogue]
    g = torch.Generator().manual_seed(seed + M + 3 * N + K)
    # (a reduction-major operand's pitch is padded to 16 bytes with zeros, as the MFMA kernels require)
    lda, ldb = ((M + 7) // 8 * 8 if a_red else K), ((N + 7) // 8 * 8 if b_red else K)
    A = torch.zeros((K, lda) if a_red else (M, K), dtype=dtype)
    B = torch.zeros((K, ldb) if b_red else (N, K), dtype=dtype)
    A[:, :M if a_red else K] = rounded((K, M) if a_red else (M, K), dtype, g)
    B[:, :N if b_red else K] = rounded((K, N) if b_red else (N, K), dtype, g, 0.1)
    ldc = ldc or N + 8
    C = _nan((M, ldc), dtype)
    if acc:
        C[:, :N] = rounded((M, N), dtype, g)
    R = None
    if has_r:
        R = _nan((M, ldc), dtype)
        R[:, :N] = rounded((M, N), dtype, g)
    bias = rounded((N,), dtype, g) if has_bias else None
    return Problem(f"{M}x{N}x{K} a_red={a_red} b_red={b_red} {dtype} {epilogue}", dtype, M, N, K, A, B, C,
                   lda, ldb, ldc, a_red=a_red, b_red=b_red, R=R, ldr=ldc if has_r else 0,
                   bias=bias, act=act, alpha=alpha, accumulate=acc, added=float(has_bias + has_r + acc))


# ------------------------------------------------------- the table: C (batches) --
NB1, NB2 = 2, 3     # batch x heads of the attention patterns


def _guarded(nb, rows, guard, ld, dtype):
    return _nan((nb, rows + guard, ld), dtype)


def batched(pattern, dtype, S=136, hd=64, Lq=320, Lk=648, G=264, E=192, seed=0):
    """the engine's batched products (macaw_llm_amd/engine.py) at a reduced geometry, same stride structure"""
    g = torch.Generator().manual_seed(seed + 17)
    Bn, H = NB1, NB2
    D = H * hd
    if pattern == "scores":
        # q k^T out of [B S, H hd] projection buffers into a pitched [B, H, S + guard rows, Lp] buffer
        q, k = rounded((Bn * S, D), dtype, g), rounded((Bn * S, D), dtype, g, 0.1)
        Lp, Sg = (S + 8) // 8 * 8, S + 3
        C = _nan((Bn, H, Sg, Lp), dtype)
        return Problem(f"scores S={S} hd={hd} {dtype}", dtype, S, S, hd, q, k, C, D, D, Lp, nb1=Bn, nb2=H,
                       sA=(S * D, hd), sB=(S * D, hd), sC=(H * Sg * Lp, Sg * Lp), alpha=1.0 / math.sqrt(hd))
    if pattern in ("pv", "dsk"):
        # P V / dS k: B reduction-major out of a projection buffer, K = Lk padded to a multiple of 64 with ZERO rows;
        # dsk: k and dq are the middle / first third of fused [.., 3 H hd] buffers (element offsets, wider pitch)
        Lkv = S - 56
        Kred = cdiv(Lkv, 64) * 64
        wide = 3 * D if pattern == "dsk" else D
        P = rounded((Bn, H, S, Kred), dtype, g)
        V = torch.zeros((Bn, Kred, wide), dtype=dtype)
        V[:, :Lkv] = rounded((Bn, Lkv, wide), dtype, g, 0.1)
        Sg = S + 3
        C = _nan((Bn, Sg, wide), dtype)
        return Problem(f"{pattern} S={S} Kred={Kred} hd={hd} {dtype}", dtype, S, hd, Kred, P, V, C, Kred, wide, wide,
                       b_red=True, nb1=Bn, nb2=H, sA=(H * S * Kred, S * Kred), sB=(Kred * wide, hd), sC=(Sg * wide, hd),
                       b_off=D if pattern == "dsk" else 0)
    if pattern in ("ptdo", "dstq"):
        # dv = P^T do / dk = dS^T q: both operands reduction-major, K = Lq; hd output columns at batch stride hd inside a
        # [B Lk, H hd] buffer; dstq: q and dk are the first / middle third of fused [.., 3 H hd] buffers
        wide = 3 * D if pattern == "dstq" else D
        Lp = (Lk + 7) // 8 * 8
        P = rounded((Bn, H, Lq, Lp), dtype, g)
        X = rounded((Bn, Lq, wide), dtype, g, 0.1)
        Lg = Lk + 3
        C = _nan((Bn, Lg, wide), dtype)
        return Problem(f"{pattern} Lk={Lk} Lq={Lq} hd={hd} {dtype}", dtype, Lk, hd, Lq, P, X, C, Lp, wide, wide, a_red=True,
                       b_red=True, nb1=Bn, nb2=H, sA=(H * Lq * Lp, Lq * Lp), sB=(Lq * wide, hd), sC=(Lg * wide, hd),
                       c_off=D if pattern == "dstq" else 0)
    if pattern == "shared":
        # CLIP patch embedding / Whisper conv2 / k|v projection / modality projection in one: rows 1 .. G of every sample
        # (a_off), the second half of a stacked weight shared by all samples (b_off, sB = 0), bias + GELU, a broadcast
        # residual from its row 1 on (r_off, sR = 0), written from row 1 of every [T, E] output slice on (c_off)
        nb, K = 3, 256
        A = rounded((nb, G + 1, K), dtype, g)
        W = rounded((2 * E, K), dtype, g, 0.1)
        ldc, T = E + 8, G + 1
        C = _nan((nb, T + 2, ldc), dtype)
        R = rounded((T, E), dtype, g)
        return Problem(f"shared G={G} E={E} {dtype}", dtype, G, E, K, A, W, C, K, K, ldc, nb1=nb, nb2=1,
                       sA=((G + 1) * K, 0), sB=(0, 0), sC=((T + 2) * ldc, 0), sR=(0, 0), a_off=K, b_off=E * K, c_off=ldc,
                       r_off=E, R=R, ldr=E, bias=rounded((E,), dtype, g), act=1, added=2.0)
    raise KeyError(pattern)


# pattern -> sizes on the 128 x 128 kernels: the default CU count takes the whole problem into the K-split (where K allows
# one), 8 planned CUs leave 0 < dp_tiles < Tb with the tail tiles in the LAST batch
C_PATTERNS = {
    "scores": dict(S=136, hd=64),               # nkt = 1: never split, batch through blockIdx.z
    "scores128": dict(S=136, hd=128),           # nkt = 2: no split either
    "pv": dict(S=264, hd=64),                   # 3 tiles x 6 batches, K = 256
    "dsk": dict(S=264, hd=64),
    "ptdo": dict(Lk=648, Lq=320, hd=64),        # cfg 7: 6 tiles x 6 batches, nkt = 10
    "dstq": dict(Lk=648, Lq=320, hd=64),
    "shared": dict(G=264, E=192),               # 6 tiles x 3 batches, K = 256
}
# the same patterns where the 256 x 256 kernel is legal (M, N > 128, K >= 128), planned CUs: whole tiles + a tail per batch
C_V7 = {
    "scores": (dict(S=264, hd=192), 3),         # 4 tiles: 3 whole + quarters
    "scores128": (dict(S=264, hd=128), 0),      # all CUs: 4 tiles, all eighths
    "pv": (dict(S=520, hd=192), 2),             # 3 tiles: 2 whole + quarters
    "dsk": (dict(S=520, hd=192), 2),
    "ptdo": (dict(Lk=648, Lq=320, hd=192), 2),
    "dstq": (dict(Lk=648, Lq=320, hd=192), 2),
    "shared": (dict(G=520, E=192), 2),
}


def c_problem(name, dtype, sizes=None):
    return batched("scores" if name == "scores128" else name, dtype, **(sizes or C_PATTERNS[name]))
