"""Tensor-level wrappers over the C ABI (ctypes).  PyTorch is used only for
device memory and the current HIP stream; every arithmetic op below runs in a
hand-written gfx950 kernel from csrc/.

All wrappers require CUDA(HIP) tensors and raise MacawHipError otherwise —
there is no eager / CPU fallback on the product path.
"""
from __future__ import annotations

import ctypes as C
import itertools
import math
import numbers
import os
import struct
from typing import Optional

import torch

from . import lib as _L
from .lib import GemmDesc, MacawHipError, MK_BF16, MK_F16, MK_F32, MK_FP8

_DT = {torch.float32: MK_F32, torch.bfloat16: MK_BF16, torch.float16: MK_F16}
_null = None


def dt(t: torch.Tensor) -> int:
    try:
        return _DT[t.dtype]
    except KeyError:
        raise MacawHipError(f"unsupported dtype {t.dtype}")


def _p(t: Optional[torch.Tensor]):
    if t is None:
        return None
    if not t.is_cuda:
        raise MacawHipError("macaw_llm_amd ops need device tensors (HIP); no CPU fallback exists")
    return t.data_ptr()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _rowmajor(t: torch.Tensor) -> int:
    """leading dimension of a 2-D row-major (possibly pitched) tensor"""
    if t.dim() != 2 or (t.size(1) > 1 and t.stride(1) != 1):
        raise MacawHipError(f"expected row-major 2-D tensor, got {tuple(t.shape)} {t.stride()}")
    return t.stride(0) if t.size(0) > 1 else max(t.stride(0), t.size(1))


# ------------------------------------------------------------------- GEMM --
_WS = {}
WS_BYTES = 72 << 20


def _workspace(device):
    """per-(device, stream) scratch for the GEMM stream-K tail (partials + counters)"""
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    ws = _WS.get(key)
    if ws is None and torch.cuda.is_current_stream_capturing():
        # a graph capture runs on its own stream: use the device's existing scratch (the captured
        # kernels are serialised) instead of allocating + zero-filling one inside the graph
        for (dev_i, _), w in _WS.items():
            if dev_i == device.index:
                return w
    if ws is None:
        ws = _WS[key] = torch.empty(WS_BYTES, dtype=torch.uint8, device=device)
        # the first 4 KiB are the stream-K arrival counters: zero once, the kernels leave them zero
        fill_(ws[:4096].view(torch.float32), 0.0)
    return ws


def gemm_raw(A, B, Cc, M, N, K, lda, ldb, ldc, *, a_red=False, b_red=False, R=None, ldr=0,
             bias=None, bias_mode=0, act=0, accumulate=False, alpha=1.0, nb1=1, nb2=1,
             sA=(0, 0), sB=(0, 0), sC=(0, 0), sR=(0, 0), a_off=0, b_off=0, c_off=0, r_off=0,
             flags=0):
    """Direct struct fill. *_off are element offsets added to the base pointers.
    flags: MK_GEMM_A_KPAD_ZERO (1) / MK_GEMM_B_KPAD_ZERO (2), see include/macaw_hip.h."""
    d = gemm_desc(A, B, Cc, M, N, K, lda, ldb, ldc, a_red=a_red, b_red=b_red, R=R, ldr=ldr, bias=bias, bias_mode=bias_mode,
                  act=act, accumulate=accumulate, alpha=alpha, nb1=nb1, nb2=nb2, sA=sA, sB=sB, sC=sC, sR=sR, a_off=a_off,
                  b_off=b_off, c_off=c_off, r_off=r_off, flags=flags)
    _L.check(_L.load().mk_gemm(C.byref(d), _st()), "mk_gemm")
    return Cc


def gemm_desc(A, B, Cc, M, N, K, lda, ldb, ldc, *, a_red=False, b_red=False, R=None, ldr=0,
              bias=None, bias_mode=0, act=0, accumulate=False, alpha=1.0, nb1=1, nb2=1,
              sA=(0, 0), sB=(0, 0), sC=(0, 0), sR=(0, 0), a_off=0, b_off=0, c_off=0, r_off=0,
              flags=0):
    """the mk_gemm_desc of gemm_raw's arguments (the caller keeps the tensors alive until the launch)"""
    es = A.element_size()
    d = GemmDesc()
    d.A = _p(A) + a_off * es
    d.B = _p(B) + b_off * es
    d.C = _p(Cc) + c_off * es
    d.R = (_p(R) + r_off * es) if R is not None else None
    d.bias = _p(bias) if bias is not None else None
    d.M, d.N, d.K = M, N, K
    d.lda, d.ldb, d.ldc, d.ldr = lda, ldb, ldc, ldr
    d.a_red_major, d.b_red_major = int(a_red), int(b_red)
    d.nb1, d.nb2 = nb1, nb2
    d.sA1, d.sA2 = sA
    d.sB1, d.sB2 = sB
    d.sC1, d.sC2 = sC
    d.sR1, d.sR2 = sR
    d.alpha = alpha
    d.bias_mode = bias_mode if bias is not None else 0
    d.act = act
    d.accumulate = int(accumulate)
    d.dtype = dt(A)
    d.flags = flags
    ws = _workspace(A.device)
    d.ws, d.ws_bytes = ws.data_ptr(), ws.numel()
    if B.dtype != A.dtype or Cc.dtype != A.dtype:
        raise MacawHipError("gemm: mixed dtypes")
    return d


class DwQueue:
    """Grad-weight GEMMs waiting to fill the idle CUs of grad-input launches (mk_gemm_grouped, include/macaw_hip.h).

    push() queues dW = dy^T x; dx() launches a grad-input GEMM together with as many queued tiles as balance it (all of
    them with drain).  dy, x and the destination of a queued product stay referenced until its last tile has been
    launched; everything runs on the current stream.  A member that the grouped kernel cannot take makes the launch fall
    back to mk_gemm for the whole queue and the grad-input GEMM (same results: every tile is computed the same way)."""

    def __init__(self):
        self.items = []          # [desc, tiles done, tiles, (dy, x, out)]
        self.grouped = 0         # launches that went through mk_gemm_grouped

    def push(self, dy, x, out):
        M, N = dy.shape
        K = x.shape[1]
        d = gemm_desc(dy, x, out, N, K, M, _rowmajor(dy), _rowmajor(x), _rowmajor(out), a_red=True, b_red=True)
        self.items.append([d, 0, ((N + 255) // 256) * ((K + 255) // 256), (dy, x, out)])
        return out

    def _launch(self, main, drain, limit=_L.GROUP_MAX_FILL):
        lib = _L.load()
        live = self.items[:limit]
        arr = (_L.GroupFill * max(len(live), 1))()
        for f, it in zip(arr, live):
            f.d, f.first_tile = it[0], it[1]
        rc = lib.mk_gemm_grouped(C.byref(main) if main is not None else None, arr, len(live), int(drain), _st())
        if rc == _L.NOT_GROUPED:
            return False
        _L.check(rc, "mk_gemm_grouped")
        for f, it in zip(arr, live):
            it[1] += f.taken
        self.items = [it for it in self.items if it[1] < it[2]]
        self.grouped += 1
        return True

    def flush(self):
        """run everything that is queued.  One grouped launch if it is accepted; else problem by problem, so that a partly
        computed (hence legal) one still finishes grouped and only a problem outside the grouped domain goes to mk_gemm"""
        while self.items and self._launch(None, True):
            pass
        while self.items:
            head = self.items[0]
            if self._launch(None, True, limit=1):
                continue
            if head[1]:      # (cannot happen: the launch that computed its first tiles accepted this descriptor)
                raise MacawHipError("mk_gemm_grouped refused a partly computed grad-weight GEMM")
            _L.check(_L.load().mk_gemm(C.byref(head[0]), _st()), "mk_gemm")
            self.items.pop(0)

    def dx(self, dy, W, drain=False):
        """dx[M, K] = dy[M, N] @ W[N, K] (linear_dx) with queued grad-weight tiles in the same launch.  drain: False = what
        balances the launch, True = everything, lib.GROUP_CARRY = the level of least idle time (the queue lives on)"""
        M, N = dy.shape
        K = W.shape[1]
        out = torch.empty((M, K), dtype=dy.dtype, device=dy.device)
        d = gemm_desc(dy, W, out, M, K, N, _rowmajor(dy), _rowmajor(W), _rowmajor(out), b_red=True)
        if len(self.items) >= _L.GROUP_MAX_FILL:
            drain = True
        if not self._launch(d, drain):
            self.flush()
            _L.check(_L.load().mk_gemm(C.byref(d), _st()), "mk_gemm")
        elif drain == 1:
            self.flush()         # (only if more problems were queued than one launch takes)
        return out


# One DwQueue for all groupable layers of a backward pass (engine._DwFill, profiles/dw_carry_cfg3.txt).  A step runtime opens
# the window (bucketed.BucketedStep.begin); inside it a layer whose grad-weight GEMMs all store straight into their gradient-
# bucket slots does not drain the queue in its last grad-input launch: every launch takes the level of least idle time
# (lib.GROUP_CARRY) and what stays queued fills the launches of the layer processed next.  Whoever reads a carried gradient
# calls dw_flush() first -- BucketedStep.finish() and its bucket launches, and the end-of-backward callback that the first
# carrying layer of a backward pass queues.  Everything runs on the stream of the window's first carrying layer.
DW_WINDOW = {"q": None, "stream": None, "callback": False, "carried": 0, "flushed": 0}


def dw_carry_open():
    """open the window (a window left open is dropped with what it holds: nobody will read those gradients)"""
    DW_WINDOW.update(q=DwQueue(), stream=None, callback=False)


def dw_carry_close():
    """launch what is queued and close the window"""
    dw_flush()
    DW_WINDOW.update(q=None, stream=None, callback=False)


def dw_carry_drop():
    """close the window without launching anything (the backward raised: its gradients are not read)"""
    DW_WINDOW.update(q=None, stream=None, callback=False)


def dw_flush():
    """launch every carried grad-weight tile (filler-only grouped launches) on the window's stream, in front of a reader of the
    gradients; a no-op without a window or with nothing queued"""
    q = DW_WINDOW["q"]
    if q is None or not q.items:
        return
    DW_WINDOW["flushed"] += sum(it[2] - it[1] for it in q.items)
    st, cur = DW_WINDOW["stream"], torch.cuda.current_stream()
    if st is None or st == cur:
        q.flush()
        return
    with torch.cuda.stream(st):
        q.flush()
    cur.wait_stream(st)      # (a reader on another stream than the backward's: order it behind the flush)


# --------------------------------------------------------------------- fp8 --
def quantize_fp8(x):
    """per-tensor scaled OCP e4m3: returns (q uint8 tensor of x's shape, dequant scale f32[1] on
    the device).  x bf16 / f32, contiguous, numel % 8 == 0."""
    lib = _L.load()
    xc = x if x.is_contiguous() else x.contiguous()
    q = torch.empty(xc.shape, dtype=torch.uint8, device=x.device)
    ws = torch.empty(2, dtype=torch.float32, device=x.device)
    _L.check(lib.mk_fp8_quantize(_p(xc), xc.numel(), dt(xc), _p(q), _p(ws), _p(ws) + 4, _st()),
             "mk_fp8_quantize")
    return q, ws[1:2]


def quantize_fp8_rows(x, out=None):
    """per-ROW scaled OCP e4m3 of a row-major bf16 matrix [rows, cols] (pitched rows allowed):
    returns (q uint8 [rows, cols], scales f32 [rows]); q[r] = e4m3(x[r] * 448 / amax_r), scales[r] =
    amax_r / 448.  One scale per token (activations, gradients) / per output channel (weights)."""
    lib = _L.load()
    rows, cols = x.shape
    q = out if out is not None else torch.empty((rows, cols), dtype=torch.uint8, device=x.device)
    sc = torch.empty(rows, dtype=torch.float32, device=x.device)
    _L.check(lib.mk_fp8_quantize_rows(_p(x), rows, cols, _rowmajor(x), dt(x), _p(q), _rowmajor(q), _p(sc), _st()),
             "mk_fp8_quantize_rows")
    return q, sc


def quantize_fp8_cols_t(W):
    """per-COLUMN scaled e4m3 of W [rows, cols], written TRANSPOSED: returns (qt uint8 [cols, rows],
    scales f32 [cols]) -- W^T K-major for the fp8 grad-input GEMM dx = dy W (one scale per input
    channel)."""
    lib = _L.load()
    rows, cols = W.shape
    qt = torch.empty((cols, rows), dtype=torch.uint8, device=W.device)
    sc = torch.empty(cols, dtype=torch.float32, device=W.device)
    ws = torch.empty(cols, dtype=torch.float32, device=W.device)
    _L.check(lib.mk_fp8_quantize_cols_t(_p(W), rows, cols, _rowmajor(W), dt(W), _p(qt), rows, _p(sc), _p(ws), _st()),
             "mk_fp8_quantize_cols_t")
    return qt, sc


# fp8 copies of weights are made ONCE per optimizer step, not per call: (data_ptr, shape, kind) ->
# (weight version, torch version counter, q, scales).  The optimizer runtimes bump WEIGHT_VERSION after
# every update (bucketed.BucketedStep.finish, optim.FusedAdamW.step*); torch-side in-place edits
# (load_state_dict, manual .copy_) move the tensor's own version counter.
WEIGHT_VERSION = [0]
_W8 = {}
_W4 = {}       # the MXFP4 copies (mxfp4_weight), keyed and versioned the same way


def bump_weight_version():
    WEIGHT_VERSION[0] += 1


def fp8_weight(W, transposed=False):
    """cached e4m3 copy of weight W [N, K]: rows scaled (q [N, K], scales [N]) for y = x W^T, or
    transposed / column scaled (qt [K, N], scales [K]) for dx = dy W"""
    key = (W.data_ptr(), tuple(W.shape), W.stride(0), transposed)
    ver = (WEIGHT_VERSION[0], W._version)
    ent = _W8.get(key)
    if ent is None or ent[0] != ver:
        q, sc = quantize_fp8_cols_t(W) if transposed else quantize_fp8_rows(W)
        ent = _W8[key] = (ver, q, sc)
    return ent[1], ent[2]


def clear_fp8_cache():
    _W8.clear()
    _W4.clear()


def quantize_mxfp4_rows(x):
    """OCP MXFP4 (round to nearest, the format of include/macaw_hip.h) of a row-major bf16 / fp16 matrix [rows, cols]
    (pitched rows allowed, cols % 32 == 0): returns (q uint8 [rows, cols / 2], two e2m1 codes per byte, low nibble
    first; e uint8 [rows, cols / 32], one E8M0 exponent per block of 32 along the row, scale 2^(e - 127))"""
    lib = _L.load()
    rows, cols = x.shape
    q = torch.empty((rows, cols // 2), dtype=torch.uint8, device=x.device)
    e = torch.empty((rows, cols // 32), dtype=torch.uint8, device=x.device)
    _L.check(lib.mk_mxfp4_quantize_rows(_p(x), rows, cols, _rowmajor(x), dt(x), _p(q), max(cols // 2, 1), _p(e),
                                        max(cols // 32, 1), _st()), "mk_mxfp4_quantize_rows")
    return q, e


def mxfp4_weight(W):
    """cached MXFP4 copy (q [N, K / 2], e [N, K / 32]: quantize_mxfp4_rows) of weight W [N, K] for y = x W^T; made
    once, re-made when the weight version moves (the rule of fp8_weight)"""
    key = (W.data_ptr(), tuple(W.shape), W.stride(0))
    ver = (WEIGHT_VERSION[0], W._version)
    ent = _W4.get(key)
    if ent is None or ent[0] != ver:
        q, e = quantize_mxfp4_rows(W)
        ent = _W4[key] = (ver, q, e)
    return ent[1], ent[2]


def linear_fp8(xq, sx, wq, sw, bias=None, act=0, residual=None, out=None, accumulate=False):
    """out[M, N] (bf16) = act((xq . wq^T) * sx * sw + bias) + residual (+ out) with fp8 operands xq
    [M, K], wq [N, K] (uint8 e4m3 bytes, K-major) and their device de-quantisation scales: f32[1]
    per-tensor scalars, or f32[M] / f32[N] per-row vectors (quantize_fp8_rows / fp8_weight)."""
    lib = _L.load()
    M, K = xq.shape
    N = wq.shape[0]
    if out is None:
        out = torch.empty((M, N), dtype=torch.bfloat16, device=xq.device)
    vec = sx.numel() > 1 or sw.numel() > 1
    if vec and (sx.numel() != M or sw.numel() != N):
        raise MacawHipError(f"linear_fp8: scale vectors {sx.numel()} / {sw.numel()} for a {M} x {N} output")
    d = GemmDesc()
    d.A, d.B, d.C = _p(xq), _p(wq), _p(out)
    d.R = _p(residual) if residual is not None else None
    d.bias = _p(bias) if bias is not None else None
    d.M, d.N, d.K = M, N, K
    d.lda, d.ldb, d.ldc = _rowmajor(xq), _rowmajor(wq), _rowmajor(out)
    d.ldr = _rowmajor(residual) if residual is not None else 0
    d.nb1 = d.nb2 = 1
    d.alpha = 1.0
    d.bias_mode = 1 if bias is not None else 0
    d.act = act
    d.accumulate = int(accumulate)
    d.dtype = MK_FP8
    d.flags = 4 if vec else 0            # MK_GEMM_SCALE_VEC
    ws = _workspace(xq.device)
    d.ws, d.ws_bytes = ws.data_ptr(), ws.numel()
    d.scale_a, d.scale_b = _p(sx), _p(sw)
    _L.check(lib.mk_gemm(C.byref(d), _st()), "mk_gemm(fp8)")
    return out


def linear_fwd(x, W, bias=None, act=0, residual=None, out=None, alpha=1.0):
    """y[M,N] = act(alpha * x[M,K] @ W[N,K]^T + bias) + residual"""
    M, K = x.shape
    N = W.shape[0]
    if out is None:
        out = torch.empty((M, N), dtype=x.dtype, device=x.device)
    gemm_raw(x, W, out, M, N, K, _rowmajor(x), _rowmajor(W), _rowmajor(out), bias=bias,
             bias_mode=1, act=act, R=residual, ldr=_rowmajor(residual) if residual is not None else 0,
             alpha=alpha)
    return out


def linear_dx(dy, W, out=None, accumulate=False, residual=None, dy_pad_zero=False):
    """dx[M,K] = dy[M,N] @ W[N,K]  (W consumed red-major: no transpose pass).
    dy_pad_zero: dy is a column view of a pitched buffer whose columns [N, pad64(N)) are zero
    (d(logits) for V = 32007): the reduction may then run over the padded width on the MFMA tile
    kernels instead of the generic edge kernel."""
    M, N = dy.shape
    K = W.shape[1]
    if out is None:
        out = torch.empty((M, K), dtype=dy.dtype, device=dy.device)
    gemm_raw(dy, W, out, M, K, N, _rowmajor(dy), _rowmajor(W), _rowmajor(out), b_red=True,
             accumulate=accumulate, R=residual,
             ldr=_rowmajor(residual) if residual is not None else 0,
             flags=1 if dy_pad_zero else 0)
    return out


# Weight-gradient destinations (bucketed.BucketedStep): (data_ptr, numel) of a weight (or of a fused
# q|k|v / gate|up view) -> the view of the flat gradient bucket its dW is written to, so that
# the grad-weight GEMM stores straight into the buffer the collective reads (no copy, no per-step
# gradient allocation).  Empty = every dW gets a fresh tensor (the default).
GRAD_DST = {}
GRAD_DST_OWNER = [None]     # the BucketedStep whose table is installed (begin() ... finish())
GRAD_DST_TAKEN = set()      # keys handed out in the current backward: a direct store OVERWRITES its slot, so a
                            # parameter whose gradient is produced twice (tied / shared weights, a module called
                            # twice) gets the slot once and a fresh tensor afterwards (autograd sums the two)

# data_ptr of every storage that a BucketedStep owns (parameter buckets).  Parameters living there
# must never be re-homed by the lazy q|k|v / gate|up fusion of modeling.py: the optimizer and the
# collectives keep working on the bucket, the model would compute with the moved copy.
PINNED_STORAGE = set()


def is_pinned(t) -> bool:
    """True if tensor `t` views a storage owned by a BucketedStep"""
    return bool(PINNED_STORAGE) and t.untyped_storage().data_ptr() in PINNED_STORAGE


def grad_dst(w):
    """registered destination for the gradient of parameter `w` (same shape), else None"""
    if not GRAD_DST or w is None:
        return None
    key = (w.data_ptr(), w.numel())
    d = GRAD_DST.get(key)
    if d is not None and key in GRAD_DST_TAKEN:
        return None
    if d is not None and d.dtype == w.dtype and d.numel() == w.numel() and (d.shape == w.shape or w.is_contiguous()):
        # a FRESH view object every time: autograd's AccumulateGrad takes a returned gradient as p.grad
        # without copying only if nobody else references that tensor object -- handing out the
        # dictionary's own tensor made it clone every such gradient (and the hook copy it back):
        # ~150 hidden device copies + ~150 copy-backs per step in round 2's "direct" path
        GRAD_DST_TAKEN.add(key)
        return d.view(w.shape)
    return None


def linear_dw(dy, x, out=None, accumulate=False, w=None):
    """dW[N,K] = dy[M,N]^T @ x[M,K]  (both operands red-major); `w` = the weight this is the
    gradient of (looked up in GRAD_DST when no explicit `out` is given)"""
    M, N = dy.shape
    K = x.shape[1]
    if out is None and not accumulate:
        out = grad_dst(w)
    if out is None:
        out = torch.empty((N, K), dtype=dy.dtype, device=dy.device)
    gemm_raw(dy, x, out, N, K, M, _rowmajor(dy), _rowmajor(x), _rowmajor(out), a_red=True,
             b_red=True, accumulate=accumulate)
    return out


def transpose(x, out=None):
    """out[c, r] = x[r, c] for a 2-D row-major tensor (batched form: 3-D contiguous)."""
    lib = _L.load()
    if x.dim() == 2:
        rows, cols = x.shape
        if out is None:
            out = torch.empty((cols, rows), dtype=x.dtype, device=x.device)
        _L.check(lib.mk_transpose(_p(x), _p(out), rows, cols, _rowmajor(x), _rowmajor(out), 1, 0, 0,
                                  x.element_size(), _st()), "mk_transpose")
        return out
    b, rows, cols = x.shape
    x = x.contiguous()
    if out is None:
        out = torch.empty((b, cols, rows), dtype=x.dtype, device=x.device)
    _L.check(lib.mk_transpose(_p(x), _p(out), rows, cols, cols, rows, b, rows * cols, rows * cols,
                              x.element_size(), _st()), "mk_transpose")
    return out


# ------------------------------------------------------------------ norms --
NORM_BLOCKS = 512  # row-slab blocks for the weight-gradient partial sums
# RMSNorm backward prefetches its next row (csrc/norm.hip): ONE block per CU keeps more rows in flight than two
# did without it, and halves the partial sums the reduction has to read (scripts/bench_norm.py, 4608 x 4096:
# 37.6 us at 256 blocks against 45.4 at 512; the round-2 kernel: 55.4 / 49.9)
RMSNORM_BLOCKS = 256


def rmsnorm_fwd(x, w, eps, res=None):
    """returns (h, y, rstd); h = x (+ res) — h is x itself when res is None"""
    lib = _L.load()
    rows, cols = x.shape
    y = torch.empty_like(x)
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
    h = torch.empty_like(x) if res is not None else x
    _L.check(lib.mk_rmsnorm_fwd(_p(x), _p(res), _p(w), _p(h) if res is not None else None, _p(y),
                                _p(rstd), rows, cols, eps, dt(x), _st()), "mk_rmsnorm_fwd")
    return h, y, rstd


def rmsnorm_fwd_fp8(x, w, eps, res=None):
    """rmsnorm_fwd + quantize_fp8_rows(y) in one pass over the row: returns (h, y, rstd, q uint8 [rows, cols],
    scales f32 [rows]) -- bit-identical to the two calls"""
    lib = _L.load()
    rows, cols = x.shape
    y = torch.empty_like(x)
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
    h = torch.empty_like(x) if res is not None else x
    q = torch.empty((rows, cols), dtype=torch.uint8, device=x.device)
    sc = torch.empty(rows, dtype=torch.float32, device=x.device)
    _L.check(lib.mk_rmsnorm_fwd_fp8(_p(x), _p(res), _p(w), _p(h) if res is not None else None, _p(y), _p(rstd),
                                    _p(q), cols, _p(sc), rows, cols, eps, dt(x), _st()), "mk_rmsnorm_fwd_fp8")
    return h, y, rstd, q, sc


def rmsnorm_bwd(dy, h, w, rstd, dres=None, dw_out=None, dw_accumulate=False):
    """returns (dx, dw); dx = dres + d/dh, dw in w.dtype"""
    lib = _L.load()
    rows, cols = h.shape
    nblk = min(RMSNORM_BLOCKS, rows)
    dx = torch.empty_like(h)
    part = torch.empty((nblk, cols), dtype=torch.float32, device=h.device)
    _L.check(lib.mk_rmsnorm_bwd(_p(dy), _p(h), _p(w), _p(rstd), _p(dres), _p(dx), _p(part), nblk,
                                rows, cols, dt(h), _st()), "mk_rmsnorm_bwd")
    if dw_out is None:
        dw_out = torch.empty_like(w)
        dw_accumulate = False
    _L.check(lib.mk_colsum_partials(_p(part), _p(dw_out), nblk, cols, int(dw_accumulate),
                                    dt(w), _st()), "mk_colsum_partials")
    return dx, dw_out


def layernorm_fwd(x, w, b, eps):
    lib = _L.load()
    rows, cols = x.shape
    y = torch.empty_like(x)
    mean = torch.empty(rows, dtype=torch.float32, device=x.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
    _L.check(lib.mk_layernorm_fwd(_p(x), _p(w), _p(b), _p(y), _p(mean), _p(rstd), rows, cols, eps,
                                  dt(x), _st()), "mk_layernorm_fwd")
    return y, mean, rstd


def layernorm_bwd(dy, x, w, mean, rstd, dres=None):
    """returns (dx, dw, db)"""
    lib = _L.load()
    rows, cols = x.shape
    nblk = min(NORM_BLOCKS, rows)
    dx = torch.empty_like(x)
    pw = torch.empty((nblk, cols), dtype=torch.float32, device=x.device)
    pb = torch.empty((nblk, cols), dtype=torch.float32, device=x.device)
    _L.check(lib.mk_layernorm_bwd(_p(dy), _p(x), _p(w), _p(mean), _p(rstd), _p(dres), _p(dx),
                                  _p(pw), _p(pb), nblk, rows, cols, dt(x), _st()),
             "mk_layernorm_bwd")
    dw = torch.empty_like(w)
    db = torch.empty_like(w)
    _L.check(lib.mk_colsum_partials(_p(pw), _p(dw), nblk, cols, 0, dt(w), _st()), "colsum")
    _L.check(lib.mk_colsum_partials(_p(pb), _p(db), nblk, cols, 0, dt(w), _st()), "colsum")
    return dx, dw, db


def colsum(x, out=None, accumulate=False):
    """out[c] (+)= sum_r x[r, c]  (bias gradient)"""
    lib = _L.load()
    rows, cols = x.shape
    nblk = max(1, min(256, rows // 16))
    ws = torch.empty((nblk, cols), dtype=torch.float32, device=x.device)
    if out is None:
        out = torch.empty(cols, dtype=x.dtype, device=x.device)
        accumulate = False
    _L.check(lib.mk_colsum(_p(x), _rowmajor(x), _p(out), _p(ws), nblk, rows, cols, int(accumulate),
                           dt(x), _st()), "mk_colsum")
    return out


# -------------------------------------------------------------- pointwise --
def rope_(x, cos_t, sin_t, pos, heads, hd, inverse=False):
    """in-place RoPE on x [tokens, heads*hd] (pitched rows allowed)"""
    lib = _L.load()
    tokens = x.shape[0]
    _L.check(lib.mk_rope(_p(x), _p(cos_t), _p(sin_t), _p(pos), tokens, heads, hd, _rowmajor(x),
                         int(inverse), dt(x), _st()), "mk_rope")
    return x


def swiglu_fwd(g, u):
    lib = _L.load()
    a = torch.empty_like(g)
    _L.check(lib.mk_swiglu_fwd(_p(g), _p(u), _p(a), g.numel(), dt(g), _st()), "mk_swiglu_fwd")
    return a


def swiglu_bwd(g, u, da):
    lib = _L.load()
    dg, du = torch.empty_like(g), torch.empty_like(u)
    _L.check(lib.mk_swiglu_bwd(_p(g), _p(u), _p(da), _p(dg), _p(du), g.numel(), dt(g), _st()),
             "mk_swiglu_bwd")
    return dg, du


def swiglu2d_fwd(gu, cols):
    """gu [rows, 2*cols] = [gate | up]; returns a [rows, cols] = silu(gate) * up"""
    lib = _L.load()
    rows = gu.shape[0]
    a = torch.empty((rows, cols), dtype=gu.dtype, device=gu.device)
    es = gu.element_size()
    _L.check(lib.mk_swiglu2d_fwd(_p(gu), _p(gu) + cols * es, _p(a), rows, cols, gu.stride(0), cols,
                                 dt(gu), _st()), "mk_swiglu2d_fwd")
    return a


def swiglu2d_bwd(gu, da, cols):
    """returns dgu [rows, 2*cols] = [dgate | dup]"""
    lib = _L.load()
    rows = gu.shape[0]
    dgu = torch.empty_like(gu)
    es = gu.element_size()
    _L.check(lib.mk_swiglu2d_bwd(_p(gu), _p(gu) + cols * es, _p(da), _p(dgu), _p(dgu) + cols * es,
                                 rows, cols, gu.stride(0), da.stride(0), dt(gu), _st()),
             "mk_swiglu2d_bwd")
    return dgu


def act_fwd(x, act):
    lib = _L.load()
    y = torch.empty_like(x)
    _L.check(lib.mk_act_fwd(_p(x), _p(y), x.numel(), act, dt(x), _st()), "mk_act_fwd")
    return y


def act_bwd(x_pre, dy, act):
    lib = _L.load()
    dx = torch.empty_like(dy)
    _L.check(lib.mk_act_bwd(_p(x_pre), _p(dy), _p(dx), dy.numel(), act, dt(dy), _st()), "mk_act_bwd")
    return dx


def add(a, b, out=None, period=0):
    lib = _L.load()
    if out is None:
        out = torch.empty_like(a)
    _L.check(lib.mk_add(_p(a), _p(b), _p(out), a.numel(), period, dt(a), _st()), "mk_add")
    return out


def cast(x, dtype):
    if x.dtype == dtype:
        return x
    lib = _L.load()
    x = x.contiguous()
    out = torch.empty(x.shape, dtype=dtype, device=x.device)
    _L.check(lib.mk_cast(_p(x), dt(x), _p(out), _DT[dtype], x.numel(), _st()), "mk_cast")
    return out


def fill_(x, v):
    lib = _L.load()
    _L.check(lib.mk_fill(_p(x), float(v), x.numel(), dt(x), _st()), "mk_fill")
    return x


_SUMSQ_WS = {}


def sumsq(x, out=None, accumulate=False):
    """out[0] (+)= sum x^2 (fp32, deterministic); x contiguous / 16-byte aligned"""
    lib = _L.load()
    ws = _SUMSQ_WS.get(x.device)
    if ws is None:
        ws = _SUMSQ_WS[x.device] = torch.empty(1024, dtype=torch.float32, device=x.device)
    if out is None:
        out = torch.empty(1, dtype=torch.float32, device=x.device)
        accumulate = False
    _L.check(lib.mk_sumsq(_p(x), x.numel(), _p(ws), _p(out), int(accumulate), dt(x), _st()), "mk_sumsq")
    return out


def copy2d(src, dst, rows, cols, ld_src, ld_dst, batch=1, s_src=0, s_dst=0, src_off=0, dst_off=0):
    """strided 2-D (batched) copy; offsets/strides in elements"""
    lib = _L.load()
    es = src.element_size()
    _L.check(lib.mk_copy2d(_p(src) + src_off * es, _p(dst) + dst_off * es, rows, cols, ld_src, ld_dst,
                           batch, s_src, s_dst, es, _st()), "mk_copy2d")
    return dst


def set_dropout_seed_offset(t):
    """register (or, with None, clear) a device int64[1] whose value every dropout kernel adds to
    its seed at execution time (mk_set_dropout_seed_offset)"""
    lib = _L.load()
    _L.check(lib.mk_set_dropout_seed_offset(_p(t) if t is not None else None), "mk_set_dropout_seed_offset")


def kv_append(src, cache, cols, batch, s_src, s_cache, ld_cache, t_dev, t_max, src_off=0, dst_off=0):
    """cache[b, *t_dev, dst_off : dst_off + cols] = src[b, src_off : src_off + cols]; the row index is
    read from the DEVICE int32 t_dev at execution time (graph-capturable decode step)"""
    lib = _L.load()
    es = src.element_size()
    _L.check(lib.mk_kv_append(_p(src) + src_off * es, _p(cache) + dst_off * es, cols, batch, s_src, s_cache,
                              ld_cache, _p(t_dev), t_max, es, _st()), "mk_kv_append")
    return cache


def decode_attn(q, k, v, out, t_dev, t_add, t_max, B, H, hd, q_bs, k_ld, k_bs, v_ld, v_bs, o_bs, scale,
                k_off=0, v_off=0):
    """one query row per (sample, head) against the first *t_dev + t_add cached keys (device int32)"""
    lib = _L.load()
    es = q.element_size()
    _L.check(lib.mk_decode_attn(_p(q), _p(k) + k_off * es, _p(v) + v_off * es, _p(out), _p(t_dev), t_add,
                                t_max, B, H, hd, q_bs, k_ld, k_bs, v_ld, v_bs, o_bs, scale, dt(q), _st()),
             "mk_decode_attn")
    return out


def decode_linear(x, W, prologue=0, norm_w=None, eps=0.0, residual=None, out=None):
    """y[M <= 16, N] = prologue(x) W^T (+ residual) in one launch: prologue 1 = RMSNorm(x; norm_w, eps),
    2 = SwiGLU of x = [gate | up] ([M, 2K]); W [N, K] row-major"""
    lib = _L.load()
    M = x.shape[0]
    N, K = W.shape
    if out is None:
        out = torch.empty((M, N), dtype=x.dtype, device=x.device)
    _L.check(lib.mk_decode_linear(_p(x), _rowmajor(x), _p(W), _rowmajor(W), _p(out), _rowmajor(out),
                                  _p(residual), _rowmajor(residual) if residual is not None else 0, M, N, K,
                                  prologue, _p(norm_w), eps, dt(x), _st()), "mk_decode_linear")
    return out


def _decode_linear_ok(x, W, K, kmult, prologue):
    """the domain the three weight-streaming entry points share (mk_decode_linear_plan in csrc/common.h): kmult is
    the K-block of the weight format's kernel; with a prologue the prepared token rows must fit 40 KiB of LDS"""
    M = x.shape[0]
    return (x.dtype in (torch.bfloat16, torch.float16) and M <= (16 if prologue else 32) and K % kmult == 0 and W.is_contiguous()
            and (prologue == 0 or M * (K + 8) * 2 <= 40 * 1024))


def decode_linear_ok(x, W, prologue=0):
    """mk_decode_linear's domain; with a prologue the prepared token rows must fit 40 KiB of LDS"""
    return _decode_linear_ok(x, W, W.shape[1], 64, prologue)


def decode_linear_fp8(x, Wq, s, prologue=0, norm_w=None, eps=0.0, residual=None, out=None):
    """decode_linear with the weight streamed as e4m3 bytes (W8A16): y[M <= 16, N] = prologue(x) (s * Wq)^T
    (+ residual); Wq uint8 [N, K] row-major, s f32 [N] (the pair fp8_weight(W) returns); x, residual, y bf16
    or fp16, tokens not quantised, fp32 accumulation, the scale applied before the residual add"""
    lib = _L.load()
    M = x.shape[0]
    N, K = Wq.shape
    if Wq.dtype != torch.uint8 or s.dtype != torch.float32 or s.numel() != N or not s.is_contiguous():
        raise MacawHipError(f"decode_linear_fp8: weight {Wq.dtype} {tuple(Wq.shape)}, scales {s.dtype} {tuple(s.shape)}")
    if out is None:
        out = torch.empty((M, N), dtype=x.dtype, device=x.device)
    _L.check(lib.mk_decode_linear_fp8(_p(x), _rowmajor(x), _p(Wq), _rowmajor(Wq), _p(s), _p(out), _rowmajor(out),
                                      _p(residual), _rowmajor(residual) if residual is not None else 0, M, N, K,
                                      prologue, _p(norm_w), eps, dt(x), _st()), "mk_decode_linear_fp8")
    return out


def decode_linear_fp8_ok(x, Wq, prologue=0):
    """mk_decode_linear_fp8's domain (Wq: the e4m3 copy, or the [N, K] 16-bit weight it will be made from); with
    a prologue the prepared token rows must fit 40 KiB of LDS"""
    return decode_linear_ok(x, Wq, prologue)       # one kernel skeleton, one domain: only the weight bytes differ


def decode_linear_mxfp4(x, Wq, e, prologue=0, norm_w=None, eps=0.0, residual=None, out=None):
    """decode_linear with the weight streamed as MXFP4 (W4A16): y[M <= 16, N] = prologue(x) dequant(Wq, e)^T
    (+ residual); Wq uint8 [N, K / 2] row-major, e uint8 [N, K / 32] (the pair mxfp4_weight(W) returns); x, residual,
    y bf16 or fp16, tokens not quantised, fp32 accumulation, the block scales applied while widening (exact)"""
    lib = _L.load()
    M = x.shape[0]
    N, K = Wq.shape[0], 2 * Wq.shape[1]
    if Wq.dtype != torch.uint8 or e.dtype != torch.uint8 or tuple(e.shape) != (N, K // 32):
        raise MacawHipError(f"decode_linear_mxfp4: codes {Wq.dtype} {tuple(Wq.shape)}, exponents {e.dtype} {tuple(e.shape)}")
    if out is None:
        out = torch.empty((M, N), dtype=x.dtype, device=x.device)
    _L.check(lib.mk_decode_linear_mxfp4(_p(x), _rowmajor(x), _p(Wq), _rowmajor(Wq), _p(e), _rowmajor(e), _p(out),
                                        _rowmajor(out), _p(residual),
                                        _rowmajor(residual) if residual is not None else 0, M, N, K, prologue,
                                        _p(norm_w), eps, dt(x), _st()), "mk_decode_linear_mxfp4")
    return out


def decode_linear_mxfp4_ok(x, W, prologue=0):
    """mk_decode_linear_mxfp4's domain (W: the uint8 codes [N, K / 2], or the [N, K] 16-bit weight they will be made
    from): decode_linear_ok's rule with K % 128 == 0 (a K-block is four MX blocks and one dword of exponents)"""
    return _decode_linear_ok(x, W, 2 * W.shape[1] if W.dtype == torch.uint8 else W.shape[1], 128, prologue)


def decode_emit(logits, V, pad, eos, tok, done, out, state):
    """greedy selection + step bookkeeping in one launch (see mk_decode_emit): logits [B, >= V]
    row-major, tok int64 [B], done bool [B], out int64 [B, n], state int32 [>= 3] = (position, output
    column, 0)"""
    lib = _L.load()
    B = logits.shape[0]
    _L.check(lib.mk_decode_emit(_p(logits), _rowmajor(logits), V, B, pad, eos, _p(tok), _p(done), _p(out),
                                out.stride(0), _p(state), dt(logits), _st()), "mk_decode_emit")


def decode_emit_sample(logits, V, pad, eos, tok, done, out, state, temperature=1.0, top_k=0, top_p=1.0, seed=0):
    """decode_emit with the argmax replaced by a draw (see mk_decode_emit_sample): temperature, top-k (0 = off),
    top-p, and the counter hash of (seed, state[1], sample) as the random number -- the same ids as
    sample_rows(step=state[1]) on the same logits"""
    lib = _L.load()
    B = logits.shape[0]
    _L.check(lib.mk_decode_emit_sample(_p(logits), _rowmajor(logits), V, B, pad, eos, _p(tok), _p(done), _p(out),
                                       out.stride(0), _p(state), float(temperature), int(top_k), float(top_p),
                                       int(seed) & 0xFFFFFFFFFFFFFFFF, dt(logits), _st()), "mk_decode_emit_sample")


def _warpers_on(min_p, typical_p, epsilon_cutoff, eta_cutoff):
    """whether any of the four warpers behind top-p is on (their off values: 0, 1, 0, 0)"""
    return not (min_p == 0 and typical_p == 1 and epsilon_cutoff == 0 and eta_cutoff == 0)


def decode_emit_sample_warp(logits, V, pad, eos, tok, done, out, state, temperature=1.0, top_k=0, top_p=1.0, seed=0,
                            min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0):
    """decode_emit_sample with the four warpers behind top-p (rule 6 of the header; see mk_decode_emit_sample_warp): min_p,
    typical_p, epsilon_cutoff, eta_cutoff, off at 0, 1, 0, 0 -- the same ids as sample_rows_warp(step=state[1]) on the
    same logits.  With all four off this IS the decode_emit_sample call."""
    if not _warpers_on(min_p, typical_p, epsilon_cutoff, eta_cutoff):
        return decode_emit_sample(logits, V, pad, eos, tok, done, out, state, temperature, top_k, top_p, seed)
    lib = _L.load()
    B = logits.shape[0]
    _L.check(lib.mk_decode_emit_sample_warp(_p(logits), _rowmajor(logits), V, B, pad, eos, _p(tok), _p(done), _p(out),
                                            out.stride(0), _p(state), float(temperature), int(top_k), float(top_p),
                                            float(min_p), float(typical_p), float(epsilon_cutoff), float(eta_cutoff),
                                            int(seed) & 0xFFFFFFFFFFFFFFFF, dt(logits), _st()),
             "mk_decode_emit_sample_warp")


def decode_emit_sample_table(logits, V, pad, eos, tok, done, out, state, table):
    """decode_emit with the selection of sample b read from record b of `table`, an ops.SampleTable (see
    mk_decode_emit_sample_table): greedy and sampled rows, temperatures, filters and seeds mixed in one launch -- the same
    ids as sample_rows_table(step=state[1]) on the same logits"""
    lib = _L.load()
    B = logits.shape[0]
    _sample_table_check("decode_emit_sample_table", logits, table)
    _L.check(lib.mk_decode_emit_sample_table(_p(logits), _rowmajor(logits), V, B, pad, eos, _p(tok), _p(done), _p(out),
                                             out.stride(0), _p(state), _p(table.records), dt(logits), _st()),
             "mk_decode_emit_sample_table")


def logits_process(logits, V, out, n_dev=None, n_add=0, prompt=None, prompt_len=None, repetition_penalty=1.0,
                   no_repeat_ngram_size=0, min_new_tokens=0, eos=None):
    """the logits processors in one launch, in place, in front of an emit (see mk_logits_process): logits [B, >= V]
    row-major; the history of row b is prompt[b, :prompt_len[b]] (int64 [B, P] and int32 [B], or None) followed by
    out[b, :n] (int64 [B, n_max], the emit's output matrix), n = (n_dev[0] if n_dev is not None else 0) + n_add with
    n_dev an int32 device tensor (the graph loop's state[1:2]).  repetition_penalty (1.0 = off), then
    no_repeat_ngram_size (0 = off), then min_new_tokens (0 = off; eos None or negative = off).  Everything off: no
    launch.  Returns logits"""
    lib = _L.load()
    B = logits.shape[0]
    if out.dtype != torch.int64 or out.dim() != 2 or out.shape[0] != B or (out.shape[1] > 1 and out.stride(1) != 1):
        raise MacawHipError(f"logits_process: out {out.dtype} {tuple(out.shape)} {out.stride()}; expected row-major int64 "
                            f"[{B}, n]")
    if n_dev is not None and (n_dev.dtype != torch.int32 or n_dev.numel() < 1):
        raise MacawHipError(f"logits_process: n_dev {n_dev.dtype} {tuple(n_dev.shape)}; expected int32 [>= 1]")
    P = p_ld = 0
    if prompt is not None:
        if (prompt.dtype != torch.int64 or prompt.dim() != 2 or prompt.shape[0] != B
                or (prompt.shape[1] > 1 and prompt.stride(1) != 1)):
            raise MacawHipError(f"logits_process: prompt {prompt.dtype} {tuple(prompt.shape)} {prompt.stride()}; expected "
                                f"row-major int64 [{B}, P]")
        if (prompt_len is None or prompt_len.dtype != torch.int32 or prompt_len.numel() != B
                or not prompt_len.is_contiguous()):
            raise MacawHipError(f"logits_process: prompt_len must be a contiguous int32 [{B}] next to a prompt")
        P, p_ld = prompt.shape[1], max(prompt.stride(0), prompt.shape[1])
    _L.check(lib.mk_logits_process(_p(logits), _rowmajor(logits), V, B, _p(prompt), p_ld, P,
                                   _p(prompt_len) if prompt is not None else None, _p(out),
                                   max(out.stride(0), out.shape[1]), out.shape[1], _p(n_dev), int(n_add),
                                   float(repetition_penalty), int(no_repeat_ngram_size), int(min_new_tokens),
                                   -1 if eos is None else int(eos), dt(logits), _st()), "mk_logits_process")
    return logits


MAX_BIAS = 1024


class BiasTable:
    """the logit_bias lists of a batch on the device (include/macaw_hip.h, "Per-request penalties"), built once per call,
    in CSR form: off int32 [B + 1], ids int32 [nnz] ascending and distinct within a row, val float32 [nnz].  rows: None,
    one dict {token id: bias} for every row, or a list with one dict | None per row; ids are integers in [0, V), values
    finite numbers, at most MAX_BIAS entries per row.  Without one entry the table is off: `on` is False, off / ids / val
    are None and nothing is allocated"""

    def __init__(self, rows, B, V, dev):
        if rows is None or isinstance(rows, dict):
            rows = [rows] * B
        rows = list(rows)
        if len(rows) != B:
            raise MacawHipError(f"BiasTable: {len(rows)} rows for a batch of {B}")
        ids, val, off = [], [], [0]
        for b, r in enumerate(rows):
            r = {} if r is None else r
            if not isinstance(r, dict) or len(r) > MAX_BIAS:
                raise MacawHipError(f"BiasTable: row {b} must be None or a dict of at most {MAX_BIAS} entries, got "
                                    f"{type(r).__name__}" + (f" of {len(r)}" if isinstance(r, dict) else ""))
            for c, v in r.items():
                if (isinstance(c, bool) or not isinstance(c, numbers.Integral) or not 0 <= c < V
                        or isinstance(v, bool) or not isinstance(v, numbers.Real) or not math.isfinite(v)):
                    raise MacawHipError(f"BiasTable: row {b}: entry {c!r}: {v!r}; expected an integer id in [0, {V}) and a "
                                        "finite bias")
            r = sorted((int(c), float(v)) for c, v in r.items())      # (a dict's keys are distinct)
            ids += [c for c, _ in r]
            val += [v for _, v in r]
            off.append(len(ids))
        self.B, self.on = B, bool(ids)
        self.off = self.ids = self.val = None
        if self.on:
            self.off = torch.tensor(off, dtype=torch.int32).to(dev)
            self.ids = torch.tensor(ids, dtype=torch.int32).to(dev)
            self.val = torch.tensor(val, dtype=torch.float32).to(dev)


def logits_penalize(logits, V, out, n_dev=None, n_add=0, frequency=None, presence=None, bias=None):
    """frequency_penalty, presence_penalty and logit_bias in one launch, in place, behind logits_process and in front of
    seq_ban, grammar_mask and every selection (see mk_logits_penalize): logits [B, >= V] row-major; the generated ids of
    row b are out[b, :n] (int64 [B, n_max], the emit's output matrix), n = (n_dev[0] if n_dev is not None else 0) + n_add
    as logits_process takes them.  frequency, presence: contiguous float32 [B] device tensors or None (all zeros); bias:
    a BiasTable of B rows or None.  Column c of row b gets + bias - frequency[b] * count - presence[b] (the last two
    where count > 0), one rounding.  All three None (or the table off): no launch.  Returns logits"""
    lib = _L.load()
    B = logits.shape[0]
    _gen_args("logits_penalize", B, out, n_dev)
    for name, t in (("frequency", frequency), ("presence", presence)):
        if t is not None and (t.dtype != torch.float32 or t.numel() != B or not t.is_contiguous()
                              or t.device != logits.device):
            raise MacawHipError(f"logits_penalize: {name} {t.dtype} {tuple(t.shape)} on {t.device}; expected a contiguous "
                                f"float32 [{B}] on {logits.device}")
    if bias is not None and bias.B != B:
        raise MacawHipError(f"logits_penalize: a BiasTable of {bias.B} rows for logits of {B}")
    on = bias is not None and bias.on
    _L.check(lib.mk_logits_penalize(_p(logits), _rowmajor(logits), V, B, _p(out), max(out.stride(0), out.shape[1]),
                                    out.shape[1], _p(n_dev), int(n_add), _p(frequency), _p(presence),
                                    _p(bias.off) if on else None, _p(bias.ids) if on else None,
                                    _p(bias.val) if on else None, dt(logits), _st()), "mk_logits_penalize")
    return logits


MAX_SEQS, MAX_SEQ_LEN = 1 << 16, 64


class SeqTable:
    """a table of token sequences on the device (include/macaw_hip.h, "Token-sequence matching"), built once per call:
    ids int64 [total], the sequences back to back, and off int32 [n + 1].  seqs: a non-empty list of non-empty lists of
    ints, at most MAX_SEQS of at most MAX_SEQ_LEN ids"""

    def __init__(self, seqs, dev):
        seqs = [list(q) for q in seqs]
        if not 1 <= len(seqs) <= MAX_SEQS or not all(1 <= len(q) <= MAX_SEQ_LEN for q in seqs):
            raise MacawHipError(f"SeqTable: {len(seqs)} sequences of {min(map(len, seqs), default=0)} to "
                                f"{max(map(len, seqs), default=0)} ids; expected 1 to {MAX_SEQS} of 1 to {MAX_SEQ_LEN}")
        self.n = len(seqs)
        self.ids = torch.tensor([c for q in seqs for c in q], dtype=torch.long).to(dev)
        self.off = torch.tensor(list(itertools.accumulate(map(len, seqs), initial=0)), dtype=torch.int32).to(dev)


def _gen_args(op, B, out, n_dev):
    """the generated ids of the sequence matchers: out row-major int64 [B, n_max], n_dev int32 [>= 1] or None"""
    if out.dtype != torch.int64 or out.dim() != 2 or out.shape[0] != B or (out.shape[1] > 1 and out.stride(1) != 1):
        raise MacawHipError(f"{op}: out {out.dtype} {tuple(out.shape)} {out.stride()}; expected row-major int64 [{B}, n]")
    if n_dev is not None and (n_dev.dtype != torch.int32 or n_dev.numel() < 1):
        raise MacawHipError(f"{op}: n_dev {n_dev.dtype} {tuple(n_dev.shape)}; expected int32 [>= 1]")


def seq_ban(logits, V, out, table: SeqTable, n_dev=None, n_add=0, prompt=None, prompt_len=None):
    """bad_words_ids in one launch, in place, behind logits_process and in front of a selection (see mk_seq_ban): the
    last id of every sequence of `table` whose other ids are the tail of row b's history gets -inf.  logits [B, >= V]
    row-major; the history is prompt[b, :prompt_len[b]] ++ out[b, :n], n = (n_dev[0] if n_dev is not None else 0) +
    n_add, all as logits_process takes them.  Returns logits"""
    lib = _L.load()
    B = logits.shape[0]
    _gen_args("seq_ban", B, out, n_dev)
    P = p_ld = 0
    if prompt is not None:
        if (prompt.dtype != torch.int64 or prompt.dim() != 2 or prompt.shape[0] != B
                or (prompt.shape[1] > 1 and prompt.stride(1) != 1)):
            raise MacawHipError(f"seq_ban: prompt {prompt.dtype} {tuple(prompt.shape)} {prompt.stride()}; expected "
                                f"row-major int64 [{B}, P]")
        if (prompt_len is None or prompt_len.dtype != torch.int32 or prompt_len.numel() != B
                or not prompt_len.is_contiguous()):
            raise MacawHipError(f"seq_ban: prompt_len must be a contiguous int32 [{B}] next to a prompt")
        P, p_ld = prompt.shape[1], max(prompt.stride(0), prompt.shape[1])
    _L.check(lib.mk_seq_ban(_p(logits), _rowmajor(logits), V, B, _p(prompt), p_ld, P,
                            _p(prompt_len) if prompt is not None else None, _p(out), max(out.stride(0), out.shape[1]),
                            out.shape[1], _p(n_dev), int(n_add), _p(table.ids), _p(table.off), table.n, dt(logits), _st()),
             "mk_seq_ban")
    return logits


def stop_match(out, table: SeqTable, done, n_dev=None, n_add=0):
    """stop_sequences in one launch, right behind an emit (see mk_stop_match): done[b] (bool or uint8 [B], in place) is set
    where row b has not finished and out[b, :n] ends with a sequence of `table`, n = (n_dev[0] if n_dev is not None else
    0) + n_add -- the graph loop passes state[1:2], which the emit has advanced, a host loop its count"""
    lib = _L.load()
    B = out.shape[0]
    _gen_args("stop_match", B, out, n_dev)
    if done.dtype not in (torch.bool, torch.uint8) or done.numel() != B or not done.is_contiguous():
        raise MacawHipError(f"stop_match: done {done.dtype} {tuple(done.shape)}; expected contiguous bool / uint8 [{B}]")
    _L.check(lib.mk_stop_match(_p(out), max(out.stride(0), out.shape[1]), out.shape[1], B, _p(n_dev), int(n_add),
                               _p(table.ids), _p(table.off), table.n, _p(done), _st()), "mk_stop_match")


class GrammarTable:
    """the device table of a grammar (include/macaw_hip.h, "Grammar-constrained decoding"): next int32 [n_states, V]
    row-major at a pitch >= V whose rows are whole in its storage, flags uint8 [n_states] (bit 0 accepting, bit 1
    terminal).  Taken as it stands: grammar.TokenDFA.table makes a trimmed one"""

    def __init__(self, next, flags):
        if next.dtype != torch.int32 or next.dim() != 2 or (next.shape[1] > 1 and next.stride(1) != 1) or next.numel() == 0:
            raise MacawHipError(f"GrammarTable: next {next.dtype} {tuple(next.shape)} {next.stride()}; expected row-major "
                                "int32 [n_states, V]")
        self.n_states, self.V = next.shape
        self.ld = max(next.stride(0), self.V)
        if next.storage_offset() + self.n_states * self.ld > next.untyped_storage().nbytes() // 4:
            raise MacawHipError("GrammarTable: the last row of next is shorter than the row pitch")
        if flags.dtype != torch.uint8 or flags.numel() != self.n_states or not flags.is_contiguous():
            raise MacawHipError(f"GrammarTable: flags {flags.dtype} {tuple(flags.shape)}; expected contiguous uint8 "
                                f"[{self.n_states}]")
        self.next, self.flags = next, flags


def _grammar_rows(op, B, state, done):
    if state.dtype != torch.int32 or state.numel() != B or not state.is_contiguous():
        raise MacawHipError(f"{op}: state {state.dtype} {tuple(state.shape)}; expected contiguous int32 [{B}]")
    if done.dtype not in (torch.bool, torch.uint8) or done.numel() != B or not done.is_contiguous():
        raise MacawHipError(f"{op}: done {done.dtype} {tuple(done.shape)}; expected contiguous bool / uint8 [{B}]")


def grammar_mask(logits, V, table: GrammarTable, state, done, eos=None):
    """the grammar's mask in one launch, in place, behind logits_process and seq_ban and in front of a selection (see
    mk_grammar_mask): in row b of logits [B, >= V] row-major every column that table.next[state[b]] does not allow gets
    -inf, and so does eos unless the state is accepting; rows whose done flag is set or whose state is no state of the
    table (-1: unconstrained) are not written.  Returns logits"""
    lib = _L.load()
    B = logits.shape[0]
    _grammar_rows("grammar_mask", B, state, done)
    if V != table.V:
        raise MacawHipError(f"grammar_mask: {V} columns, but the table holds {table.V} tokens")
    _L.check(lib.mk_grammar_mask(_p(logits), _rowmajor(logits), V, B, _p(table.next), table.ld, table.n_states,
                                 _p(table.flags), _p(state), _p(done), -1 if eos is None else int(eos), dt(logits), _st()),
             "mk_grammar_mask")
    return logits


def grammar_advance(out, table: GrammarTable, state, done, end, n_dev=None, n_add=0):
    """the grammar's step in one launch, right behind an emit and in front of stop_match (see mk_grammar_advance): row b
    that has not finished and has a state >= 0 moves along out[b, n - 1], n = (n_dev[0] if n_dev is not None else 0) +
    n_add; a terminal state (or a token the table does not allow: state -2) sets done[b] and end[b] = n.  state int32
    [B], done bool / uint8 [B] and end int32 [B] are updated in place.  Run it exactly once per step"""
    lib = _L.load()
    B = out.shape[0]
    _gen_args("grammar_advance", B, out, n_dev)
    _grammar_rows("grammar_advance", B, state, done)
    if end.dtype != torch.int32 or end.numel() != B or not end.is_contiguous():
        raise MacawHipError(f"grammar_advance: end {end.dtype} {tuple(end.shape)}; expected contiguous int32 [{B}]")
    _L.check(lib.mk_grammar_advance(_p(out), max(out.stride(0), out.shape[1]), out.shape[1], B, table.V, _p(n_dev),
                                    int(n_add), _p(table.next), table.ld, table.n_states, _p(table.flags), _p(state),
                                    _p(done), _p(end), _st()), "mk_grammar_advance")


def grammar_build(char_next, tok_bytes, tok_off, dev=None, ld_next=None):
    """the token table of a byte automaton in one launch (see mk_grammar_build): char_next int32 [S, 256], tok_bytes uint8
    [total] and tok_off int32 [V + 1], the vocabulary's bytes back to back -- host or device tensors; the offsets are
    checked on the host (ascending from 0, the last one the total) before they are uploaded.  Returns next int32 [S, V] on
    dev (default: char_next's device) at pitch ld_next (default: V rounded up to a multiple of 4, which lets the mask
    load 16 bytes at a time)"""
    lib = _L.load()
    if char_next.dtype != torch.int32 or char_next.dim() != 2 or char_next.shape[1] != 256 or char_next.shape[0] < 1:
        raise MacawHipError(f"grammar_build: char_next {char_next.dtype} {tuple(char_next.shape)}; expected int32 [S, 256]")
    if tok_off.dtype != torch.int32 or tok_off.dim() != 1 or tok_off.numel() < 2 or tok_bytes.dtype != torch.uint8:
        raise MacawHipError(f"grammar_build: tok_off {tok_off.dtype} {tuple(tok_off.shape)}, tok_bytes {tok_bytes.dtype}; "
                            "expected int32 [V + 1] and uint8 [total]")
    off = tok_off.cpu()
    if int(off[0]) != 0 or bool((off[1:] < off[:-1]).any()) or int(off[-1]) != tok_bytes.numel():
        raise MacawHipError("grammar_build: tok_off must ascend from 0 to the number of bytes")
    dev = torch.device(char_next.device if dev is None else dev)
    if dev.type != "cuda":
        raise MacawHipError(f"grammar_build: the table is made by a HIP kernel and needs a GPU device, got {dev}")
    S, V = char_next.shape[0], tok_off.numel() - 1
    ld = (V + 3) // 4 * 4 if ld_next is None else int(ld_next)
    if ld < V:
        raise MacawHipError(f"grammar_build: ld_next {ld} < V {V}")
    nxt = torch.full((S, ld), -1, dtype=torch.int32, device=dev)
    cn, tb, to = char_next.to(dev).contiguous(), tok_bytes.to(dev).contiguous(), tok_off.to(dev).contiguous()
    if tb.numel() == 0:          # a vocabulary of empty tokens: nothing to read, and no null pointer to pass
        tb = torch.zeros(1, dtype=torch.uint8, device=dev)
    _L.check(lib.mk_grammar_build(_p(cn), _p(tb), _p(to), S, V, _p(nxt), ld, _st()), "mk_grammar_build")
    return nxt[:, :V]


MAX_TOP_LOGPROBS = 20


def token_logprobs(logits, V, ids, top_n=0):
    """the log-softmax value of ids[r] in row r of logits [rows, >= V] row-major, and with top_n > 0 the top_n most
    likely columns of every row with theirs, in one launch (see mk_token_logprobs: fp64 log-sum-exp, one rounding, exact
    selection, ties to the lower column; an id outside [0, V) gives NaN).  ids int64 [rows].  Returns (lp f32 [rows],
    top_ids int64 [rows, top_n] | None, top_lp f32 [rows, top_n] | None); the stand-alone twin of argmax_rows"""
    lib = _L.load()
    rows, top_n = logits.shape[0], int(top_n)
    if ids.dtype != torch.int64 or ids.numel() != rows or not ids.is_contiguous():
        raise MacawHipError(f"token_logprobs: ids {ids.dtype} {tuple(ids.shape)}; expected contiguous int64 [{rows}]")
    lp = torch.empty(rows, dtype=torch.float32, device=logits.device)
    top_ids = top_lp = None
    if top_n > 0:
        top_ids = torch.empty((rows, top_n), dtype=torch.long, device=logits.device)
        top_lp = torch.empty((rows, top_n), dtype=torch.float32, device=logits.device)
    _L.check(lib.mk_token_logprobs(_p(logits), _rowmajor(logits), rows, V, _p(ids), top_n, _p(lp), _p(top_ids),
                                   _p(top_lp), dt(logits), _st()), "mk_token_logprobs")
    return lp, top_ids, top_lp


class LogprobState:
    """the device books of generate(return_logprobs=True) on the step path (include/macaw_hip.h, "Token
    log-probabilities"): B samples, n_max output columns, n_top top columns per token (0: none).  lp starts as zeros,
    top_ids as pad, top_lp as zeros: what a column behind a sample's end holds; fin is the kernel's own latch"""

    def __init__(self, B, n_max, n_top, pad, dev):
        self.B, self.n_max, self.n_top, self.pad = B, n_max, int(n_top), pad
        self.lp = torch.zeros((B, n_max), dtype=torch.float32, device=dev)
        self.top_ids = torch.full((B, n_max, self.n_top), pad, dtype=torch.long, device=dev) if self.n_top else None
        self.top_lp = torch.zeros((B, n_max, self.n_top), dtype=torch.float32, device=dev) if self.n_top else None
        self.fin = torch.zeros(B, dtype=torch.uint8, device=dev)


def decode_emit_logprobs(logits, V, tok, done, state, ls: LogprobState):
    """the log-probability of the token an emit just stored, launched right behind decode_emit / decode_emit_sample on
    the same logits (see mk_decode_emit_logprobs): fills column state[1] - 1 of ls.lp (and of ls.top_ids / ls.top_lp),
    the column read on the device, so a captured step replays; a sample finished before this step gets 0.0 / pad / 0.0"""
    lib = _L.load()
    B = logits.shape[0]
    if B != ls.B or tok.numel() != B or done.numel() != B:
        raise MacawHipError(f"decode_emit_logprobs: {B} rows of logits, {tok.numel()} tokens and {done.numel()} flags for "
                            f"B = {ls.B}")
    _L.check(lib.mk_decode_emit_logprobs(_p(logits), _rowmajor(logits), V, B, ls.pad, _p(tok), _p(done), _p(state),
                                         _p(ls.fin), ls.n_max, ls.n_top, _p(ls.lp), ls.n_max, _p(ls.top_ids),
                                         _p(ls.top_lp), dt(logits), _st()), "mk_decode_emit_logprobs")


def cfg_combine(logits, V, B, scale):
    """classifier-free guidance in one launch, in place, behind the lm_head of a guided step (see mk_cfg_combine): logits
    [2B, >= V] row-major, rows [0, B) scored on the prompt and rows [B, 2B) on the negative prompt; row b becomes
    lu + scale * (lc - lu) of the two rows' log-probabilities (fp64, one rounding), rows [B, 2B) stay as they are.
    Returns the view logits[:B] -- the same pitch, so the processors, the emits and the log-probabilities take it as
    they take a step's logits"""
    lib = _L.load()
    if logits.dim() != 2 or logits.shape[0] != 2 * B:
        raise MacawHipError(f"cfg_combine: logits {tuple(logits.shape)}; expected [2 B = {2 * B}, >= V]")
    _L.check(lib.mk_cfg_combine(_p(logits), _rowmajor(logits), V, B, float(scale), dt(logits), _st()), "mk_cfg_combine")
    return logits[:B]


def decode_step_attn(q, k_new, v_new, in_bs, cos_t, sin_t, cache, t_dev, t_max, B, H, hd, out, scale,
                     q_off=0, k_off=0, v_off=0):
    """RoPE(q, k_new) at position *t_dev + append [k_new | v_new] to cache [B, t_max, 2 * H * hd] row
    *t_dev + attention of q over keys 0 ... *t_dev, one launch (q / k_new / v_new may be slices of one
    fused [B, 3D] buffer: element offsets q_off / k_off / v_off)"""
    lib = _L.load()
    es = q.element_size()
    D = H * hd
    _L.check(lib.mk_decode_step_attn(_p(q) + q_off * es, _p(k_new) + k_off * es, _p(v_new) + v_off * es,
                                     in_bs, _p(cos_t), _p(sin_t), _p(cache), _p(cache) + D * es, 2 * D,
                                     t_max * 2 * D, _p(out), D, _p(t_dev), t_max, B, H, hd, scale, dt(q),
                                     _st()), "mk_decode_step_attn")
    return out


def decode_step_attn_beam(q, k_new, v_new, in_bs, cos_t, sin_t, cache, t_dev, ind, S0, t_max, B, K, H, hd, out, scale,
                          q_off=0, k_off=0, v_off=0):
    """decode_step_attn for the B * K (sample, beam) rows of a beam step over cache [B, K, t_max, 2 * H * hd], read
    through the indirection table ind int32 [B * K, n]: key t < S0 from slot 0 of the row's sample (the shared prompt),
    key S0 <= t < *t_dev from slot ind[row, t - S0], the new key appended to row *t_dev of the row's own slot.  No cache
    row is copied; bit-identical per row to decode_step_attn on a physically gathered [B * K, t_max, 2D] cache"""
    lib = _L.load()
    es = q.element_size()
    D = H * hd
    if cache.dtype != q.dtype or tuple(cache.shape) != (B, K, t_max, 2 * D) or not cache.is_contiguous():
        raise MacawHipError(f"decode_step_attn_beam: cache {cache.dtype} {tuple(cache.shape)}; expected {q.dtype} "
                            f"{(B, K, t_max, 2 * D)}, contiguous")
    if ind.dtype != torch.int32 or ind.dim() != 2 or ind.shape[0] != B * K or not ind.is_contiguous():
        raise MacawHipError(f"decode_step_attn_beam: ind {ind.dtype} {tuple(ind.shape)}; expected contiguous int32 "
                            f"[{B * K}, n]")
    _L.check(lib.mk_decode_step_attn_beam(_p(q) + q_off * es, _p(k_new) + k_off * es, _p(v_new) + v_off * es, in_bs,
                                          _p(cos_t), _p(sin_t), _p(cache), _p(cache) + D * es, 2 * D, t_max * 2 * D,
                                          _p(out), D, _p(t_dev), _p(ind), ind.shape[1], S0, t_max, B, K, H, hd, scale,
                                          dt(q), _st()), "mk_decode_step_attn_beam")
    return out


SHARED_MAX_N = 32


def shared_attn_ok(dtype, hd, n):
    """mk_decode_step_attn_shared's domain: bf16 / fp16, hd in {16, 32, 64, 128}, 1 <= n <= 32 rows per sample.  The
    kernel keeps no per-key buffer in LDS, so neither the prompt's nor the tail's length bounds it"""
    return dtype in (torch.bfloat16, torch.float16) and hd in (16, 32, 64, 128) and 1 <= n <= SHARED_MAX_N


def decode_step_attn_shared(q, k_new, v_new, in_bs, cos_t, sin_t, prompt, tail, t_dev, t_off, S0, B, n, H, hd, out, scale,
                            q_off=0, k_off=0, v_off=0):
    """decode_step_attn for the B * n rows of a parallel-sampling step (see mk_decode_step_attn_shared): row b * n + j is
    sample j of prompt b.  prompt [B, S0, 2 * H * hd] holds each prompt's keys and values ONCE (read only; a padded
    batch's compacted rows, t_off int32 [B] on the device = engine.Ragged.t_off, or None), tail [B * n, Tn, 2 * H * hd]
    the rows' own tokens.  With i = clamp(*t_dev - S0, 0, Tn - 1) and L_b = clamp(S0 + t_off[b], 0, S0): RoPE at
    position L_b + i, append to tail row i of the row, attention over prompt rows 0 ... L_b - 1 of sample b and tail
    rows 0 ... i of the row.  out [B * n, H * hd].  Bit-identical per row to decode_step_attn on a physically gathered
    cache; one launch, the rows of a tile run in one workgroup and find the prompt's keys in cache behind its first row"""
    lib = _L.load()
    es = q.element_size()
    D = H * hd
    if prompt.dtype != q.dtype or tuple(prompt.shape) != (B, S0, 2 * D) or not prompt.is_contiguous():
        raise MacawHipError(f"decode_step_attn_shared: prompt {prompt.dtype} {tuple(prompt.shape)}; expected {q.dtype} "
                            f"{(B, S0, 2 * D)}, contiguous")
    if (tail.dtype != q.dtype or tail.dim() != 3 or tail.shape[0] != B * n or tail.shape[1] < 1 or tail.shape[2] != 2 * D
            or not tail.is_contiguous()):
        raise MacawHipError(f"decode_step_attn_shared: tail {tail.dtype} {tuple(tail.shape)}; expected {q.dtype} "
                            f"[{B * n}, Tn >= 1, {2 * D}], contiguous")
    Tn = tail.shape[1]
    if t_off is not None:
        _i32_check("decode_step_attn_shared", "t_off", t_off, B)
    if out.shape[0] != B * n or q.shape[0] != B * n:
        raise MacawHipError(f"decode_step_attn_shared: {q.shape[0]} input and {out.shape[0]} output rows for B * n = {B * n}")
    if cos_t.shape[0] < S0 + Tn or sin_t.shape[0] < S0 + Tn:
        raise MacawHipError(f"decode_step_attn_shared: {cos_t.shape[0]} table rows for positions up to {S0 + Tn - 1}")
    _L.check(lib.mk_decode_step_attn_shared(_p(q) + q_off * es, _p(k_new) + k_off * es, _p(v_new) + v_off * es, in_bs,
                                            _p(cos_t), _p(sin_t), _p(prompt) if S0 else None,
                                            _p(prompt) + D * es if S0 else None, 2 * D, S0 * 2 * D, _p(tail),
                                            _p(tail) + D * es, 2 * D, Tn * 2 * D, _p(out), _rowmajor(out), _p(t_dev),
                                            _p(t_off), S0, Tn, B, n, H, hd, scale, dt(q), _st()),
             "mk_decode_step_attn_shared")
    return out


def score_attn_ok(dtype, hd, H=1):
    """mk_score_attn's domain: bf16 / fp16, hd in {16, 32, 64, 128}, at most 65535 heads.  The kernel keeps no per-key
    buffer in LDS and splits its rows over as many launches as they need, so neither the prompt's length, the options'
    length nor their number bounds it"""
    return dtype in (torch.bfloat16, torch.float16) and hd in (16, 32, 64, 128) and 1 <= H <= 65535


def score_attn(q, k_new, v_new, in_bs, cos_t, sin_t, prompt, tail, lens, t_off, S0, B, n, H, hd, out, scale,
               q_off=0, k_off=0, v_off=0):
    """the attention of a scoring pass (see mk_score_attn): row (b * n + j) * F + g is fed token g of option j of prompt
    b, F = tail.shape[1].  prompt [B, S0, 2 * H * hd] holds each prompt's keys and values once (read only; t_off int32
    [B] on the device = engine.Ragged.t_off, or None), tail [B * n, F, 2 * H * hd] receives the options' own rows, lens
    int32 [B * n] on the device the fed rows of each option.  With L_b = clamp(S0 + t_off[b], 0, S0) a live row
    (g < clamp(lens, 0, F)) runs at position L_b + g: RoPE, tail row g, attention over prompt rows 0 ... L_b - 1 and tail
    rows 0 ... g; a dead row's output is zeros and nothing of it is read or stored.  out [B * n * F, H * hd].
    Bit-identical per live row to decode_step_attn on a physically gathered cache"""
    lib = _L.load()
    es = q.element_size()
    D = H * hd
    if prompt.dtype != q.dtype or tuple(prompt.shape) != (B, S0, 2 * D) or not prompt.is_contiguous():
        raise MacawHipError(f"score_attn: prompt {prompt.dtype} {tuple(prompt.shape)}; expected {q.dtype} "
                            f"{(B, S0, 2 * D)}, contiguous")
    if (tail.dtype != q.dtype or tail.dim() != 3 or tail.shape[0] != B * n or tail.shape[1] < 1 or tail.shape[2] != 2 * D
            or not tail.is_contiguous()):
        raise MacawHipError(f"score_attn: tail {tail.dtype} {tuple(tail.shape)}; expected {q.dtype} "
                            f"[{B * n}, F >= 1, {2 * D}], contiguous")
    F = tail.shape[1]
    _i32_check("score_attn", "lens", lens, B * n)
    if t_off is not None:
        _i32_check("score_attn", "t_off", t_off, B)
    if out.shape[0] != B * n * F or q.shape[0] != B * n * F:
        raise MacawHipError(f"score_attn: {q.shape[0]} input and {out.shape[0]} output rows for B * n * F = {B * n * F}")
    if cos_t.shape[0] < S0 + F or sin_t.shape[0] < S0 + F:
        raise MacawHipError(f"score_attn: {cos_t.shape[0]} table rows for positions up to {S0 + F - 1}")
    _L.check(lib.mk_score_attn(_p(q) + q_off * es, _p(k_new) + k_off * es, _p(v_new) + v_off * es, in_bs, _p(cos_t),
                               _p(sin_t), _p(prompt) if S0 else None, _p(prompt) + D * es if S0 else None, 2 * D,
                               S0 * 2 * D, _p(tail), _p(tail) + D * es, 2 * D, F * 2 * D, _p(out), _rowmajor(out), _p(lens),
                               _p(t_off), S0, F, B, n, H, hd, scale, dt(q), _st()), "mk_score_attn")
    return out


class BeamState:
    """the device state of a beam search (include/macaw_hip.h, "State layout"): B samples, K beams, n_max columns"""

    def __init__(self, B, K, n_max, pad, device):
        self.B, self.K, self.n_max = B, K, n_max
        self.tok = torch.full((B * K,), pad, dtype=torch.long, device=device)
        self.scores = torch.zeros(B * K, dtype=torch.float32, device=device)
        self.hist = torch.zeros((n_max, B, K, 2), dtype=torch.int32, device=device)
        self.ind = torch.zeros((B * K, n_max), dtype=torch.int32, device=device)
        self.pool_score = torch.zeros((B, K), dtype=torch.float32, device=device)
        self.pool_info = torch.zeros((B, K + 1, 4), dtype=torch.int32, device=device)
        self.done = torch.zeros(B, dtype=torch.bool, device=device)


def beam_emit(logits, V, K_in, pad, eos, length_penalty, early_stopping, bs: BeamState, state):
    """one beam-search step for every sample in one launch (see mk_beam_emit): logits [B * K_in, >= V] row-major, K_in
    = 1 (the prefill's row) or K; eos None or negative never matches; state int32 [>= 3] = (position, output column,
    0) as decode_emit's.  Updates bs (tok, scores, hist, ind, pool, done) in place"""
    lib = _L.load()
    B, K = bs.B, bs.K
    if logits.shape[0] != B * K_in:
        raise MacawHipError(f"beam_emit: {logits.shape[0]} rows of logits for B = {B}, K_in = {K_in}")
    _L.check(lib.mk_beam_emit(_p(logits), _rowmajor(logits), V, B, K, K_in, pad, -1 if eos is None else eos,
                              float(length_penalty), int(bool(early_stopping)), _p(bs.tok), _p(bs.scores), _p(bs.hist),
                              _p(bs.ind), bs.n_max, _p(bs.pool_score), _p(bs.pool_info), _p(bs.done), _p(state),
                              dt(logits), _st()), "mk_beam_emit")


SPEC_MAX_Q = 16


def spec_attn_ok(dtype, hd, t_max, Q):
    """mk_decode_step_attn_multi's domain: bf16 / fp16, hd in {16, 32, 64, 128}, 1 <= Q <= 16 rows per sample.  The
    kernel keeps no per-key buffer in LDS, so any t_max >= 1 is inside"""
    return dtype in (torch.bfloat16, torch.float16) and hd in (16, 32, 64, 128) and 1 <= Q <= SPEC_MAX_Q and t_max >= 1


def decode_step_attn_multi(q, k_new, v_new, in_bs, cos_t, sin_t, cache, pos, t_max, B, Q, H, hd, out, scale,
                           q_off=0, k_off=0, v_off=0):
    """decode_step_attn for the B * Q rows of a prompt-lookup verify step (see mk_decode_step_attn_multi): row b * Q + g
    of q / k_new / v_new (row stride in_bs; slices of one fused [B * Q, 3D] buffer through the element offsets) runs at
    position pos[b] + g (pos int32 [B] on the device): RoPE, append to row pos[b] + g of cache [B, t_max, 2 * H * hd],
    attention over keys 0 ... pos[b] + g.  out [B * Q, H * hd].  Bit-identical per row to decode_step_attn at that
    position; one launch, one workgroup per (head, sample, row)"""
    lib = _L.load()
    es = q.element_size()
    D = H * hd
    if cache.dtype != q.dtype or tuple(cache.shape) != (B, t_max, 2 * D) or not cache.is_contiguous():
        raise MacawHipError(f"decode_step_attn_multi: cache {cache.dtype} {tuple(cache.shape)}; expected {q.dtype} "
                            f"{(B, t_max, 2 * D)}, contiguous")
    if pos.dtype != torch.int32 or pos.numel() != B or not pos.is_contiguous():
        raise MacawHipError(f"decode_step_attn_multi: pos {pos.dtype} {tuple(pos.shape)}; expected contiguous int32 [{B}]")
    if out.shape[0] != B * Q or q.shape[0] != B * Q:
        raise MacawHipError(f"decode_step_attn_multi: {q.shape[0]} input and {out.shape[0]} output rows for B * Q = {B * Q}")
    _L.check(lib.mk_decode_step_attn_multi(_p(q) + q_off * es, _p(k_new) + k_off * es, _p(v_new) + v_off * es, in_bs,
                                           _p(cos_t), _p(sin_t), _p(cache), _p(cache) + D * es, 2 * D, t_max * 2 * D,
                                           _p(out), _rowmajor(out), _p(pos), t_max, B, Q, H, hd, scale, dt(q), _st()),
             "mk_decode_step_attn_multi")
    return out


class SpecState:
    """the per-sample device state of prompt-lookup decoding (include/macaw_hip.h, "Per-sample state"): B samples, G
    draft tokens (Q = G + 1 rows per sample and step), n_max = max_new_tokens output columns.  pos starts at 0: the loop
    sets it to S0 - 1 in front of token 0"""

    def __init__(self, B, G, n_max, pad, device):
        self.B, self.G, self.Q, self.n_max, self.pad = B, G, G + 1, n_max, pad
        self.pos = torch.zeros(B, dtype=torch.int32, device=device)
        self.n_out = torch.zeros(B, dtype=torch.int32, device=device)
        self.done = torch.zeros(B, dtype=torch.bool, device=device)
        self.out = torch.full((B, n_max), pad, dtype=torch.long, device=device)
        self.tok = torch.full((B, G + 1), pad, dtype=torch.long, device=device)
        self.n_draft = torch.zeros(B, dtype=torch.int32, device=device)
        self.steps = torch.zeros(B, dtype=torch.int32, device=device)


def spec_lookup(ss: SpecState, V, max_matching_ngram_size, eos, prompt=None, prompt_len=None):
    """the draft of a prompt-lookup step for every sample in one launch (see mk_spec_lookup): the history of sample b is
    prompt[b, :prompt_len[b]] (int64 [B, P] and int32 [B], or None) followed by ss.out[b, :ss.n_out[b]].  Writes
    ss.tok[:, 1:] (pad behind the draft) and ss.n_draft; eos None or negative never matches"""
    lib = _L.load()
    B = ss.B
    P = p_ld = 0
    if prompt is not None:
        if (prompt.dtype != torch.int64 or prompt.dim() != 2 or prompt.shape[0] != B
                or (prompt.shape[1] > 1 and prompt.stride(1) != 1)):
            raise MacawHipError(f"spec_lookup: prompt {prompt.dtype} {tuple(prompt.shape)} {prompt.stride()}; expected "
                                f"row-major int64 [{B}, P]")
        if (prompt_len is None or prompt_len.dtype != torch.int32 or prompt_len.numel() != B
                or not prompt_len.is_contiguous()):
            raise MacawHipError(f"spec_lookup: prompt_len must be a contiguous int32 [{B}] next to a prompt")
        P, p_ld = prompt.shape[1], max(prompt.stride(0), prompt.shape[1])
    _L.check(lib.mk_spec_lookup(_p(prompt), p_ld, P, _p(prompt_len) if prompt is not None else None, _p(ss.out),
                                max(ss.out.stride(0), ss.n_max), ss.n_max, _p(ss.n_out), _p(ss.done), _p(ss.tok),
                                _p(ss.n_draft), B, ss.G, min(int(max_matching_ngram_size), 2 ** 31 - 1), V, ss.pad,
                                -1 if eos is None else int(eos), _st()), "mk_spec_lookup")


def spec_verify_emit(logits, V, eos, ss: SpecState):
    """verify the draft against the step's logits and emit, for every sample in one launch (see mk_spec_verify_emit):
    logits [B * R, >= V] row-major with R = ss.Q rows per sample, or R = 1 for token 0 (the prefill's rows, no draft).
    Updates ss (out, n_out, pos, steps, done, tok[:, 0]) in place"""
    lib = _L.load()
    B = ss.B
    R = logits.shape[0] // B
    if logits.shape[0] != B * R or R not in (1, ss.Q):
        raise MacawHipError(f"spec_verify_emit: {logits.shape[0]} rows of logits for B = {B}, Q = {ss.Q}")
    _L.check(lib.mk_spec_verify_emit(_p(logits), _rowmajor(logits), V, B, R, ss.Q, -1 if eos is None else int(eos),
                                     _p(ss.tok), _p(ss.n_draft), _p(ss.pos), _p(ss.n_out), _p(ss.done), _p(ss.out),
                                     max(ss.out.stride(0), ss.n_max), ss.n_max, _p(ss.steps), dt(logits), _st()),
             "mk_spec_verify_emit")


def kv8_cache(B, t_max, H, hd, device):
    """an empty e4m3 KV cache in the one format of include/macaw_hip.h: (bytes uint8 [B, t_max, 2 * H * hd] =
    [keys of all heads | values of all heads] per position, scales f32 [B, t_max, 2 * H])"""
    return (torch.empty((B, t_max, 2 * H * hd), dtype=torch.uint8, device=device),
            torch.empty((B, t_max, 2 * H), dtype=torch.float32, device=device))


def _kv8_check(op, cache, scales, t_max, B, H, hd):
    if (cache.dtype != torch.uint8 or scales.dtype != torch.float32 or tuple(cache.shape) != (B, t_max, 2 * H * hd)
            or tuple(scales.shape) != (B, t_max, 2 * H) or not cache.is_contiguous() or not scales.is_contiguous()):
        raise MacawHipError(f"{op}: cache {cache.dtype} {tuple(cache.shape)}, scales {scales.dtype} "
                            f"{tuple(scales.shape)}; expected uint8 {(B, t_max, 2 * H * hd)} and float32 "
                            f"{(B, t_max, 2 * H)}, contiguous")


def kv_quant_append(k, v, ld, in_bs, cache, scales, t0, Sn, t_max, B, H, hd):
    """the prefill's write of an e4m3 KV cache (kv8_cache): Sn rows per sample of the ROTATED keys k and of the values
    v (16-bit; row pitch ld, sample stride in_bs in elements; k / v may be slices of one fused [M, 3D] buffer) are
    quantised per head (scale = amax / 448 over hd) into cache rows [t0, t0 + Sn); no other row is touched"""
    lib = _L.load()
    _kv8_check("kv_quant_append", cache, scales, t_max, B, H, hd)
    _L.check(lib.mk_kv_quant_append(_p(k), _p(v), ld, in_bs, _p(cache), _p(scales), t0, Sn, t_max, B, H, hd, dt(k),
                                    _st()), "mk_kv_quant_append")
    return cache, scales


def decode_step_attn_kv8(q, k_new, v_new, in_bs, cos_t, sin_t, cache, scales, t_dev, t_max, B, H, hd, out, scale,
                         q_off=0, k_off=0, v_off=0):
    """decode_step_attn over an e4m3 KV cache (kv8_cache): RoPE(q, k_new) at position *t_dev + per-head quantisation
    of the rotated key and of v_new + append of their bytes and scales at cache row *t_dev + attention of the 16-bit
    q over rows 0 ... *t_dev of the cache as stored after the append (fp32 de-quantisation), one launch"""
    lib = _L.load()
    es = q.element_size()
    _kv8_check("decode_step_attn_kv8", cache, scales, t_max, B, H, hd)
    _L.check(lib.mk_decode_step_attn_kv8(_p(q) + q_off * es, _p(k_new) + k_off * es, _p(v_new) + v_off * es, in_bs,
                                         _p(cos_t), _p(sin_t), _p(cache), _p(scales), _p(out), H * hd, _p(t_dev),
                                         t_max, B, H, hd, scale, dt(q), _st()), "mk_decode_step_attn_kv8")
    return out


def _i32_check(op, name, t, n):
    if t.dtype != torch.int32 or t.numel() != n or not t.is_contiguous():
        raise MacawHipError(f"{op}: {name} {t.dtype} {tuple(t.shape)}; expected {n} contiguous int32")


def decode_step_attn_var(q, k_new, v_new, in_bs, cos_t, sin_t, cache, t_dev, t_off, t_max, B, H, hd, out, scale,
                         q_off=0, k_off=0, v_off=0):
    """decode_step_attn at a position per sample, p_b = *t_dev + t_off[b] (t_off int32 [B] on the device): RoPE at
    table row p_b, append at cache row p_b, attention over rows 0 ... p_b of sample b's cache -- the step of a padded
    batch over its compacted cache (kv_append_rows).  Bit-identical per sample to decode_step_attn at *t_dev = p_b"""
    lib = _L.load()
    es = q.element_size()
    D = H * hd
    _i32_check("decode_step_attn_var", "t_off", t_off, B)
    if cache.dtype != q.dtype:
        raise MacawHipError(f"decode_step_attn_var: cache {cache.dtype}, tokens {q.dtype}")
    _L.check(lib.mk_decode_step_attn_var(_p(q) + q_off * es, _p(k_new) + k_off * es, _p(v_new) + v_off * es,
                                         in_bs, _p(cos_t), _p(sin_t), _p(cache), _p(cache) + D * es, 2 * D,
                                         t_max * 2 * D, _p(out), D, _p(t_dev), _p(t_off), t_max, B, H, hd, scale,
                                         dt(q), _st()), "mk_decode_step_attn_var")
    return out


def decode_step_attn_kv8_var(q, k_new, v_new, in_bs, cos_t, sin_t, cache, scales, t_dev, t_off, t_max, B, H, hd, out,
                             scale, q_off=0, k_off=0, v_off=0):
    """decode_step_attn_kv8 at a position per sample, p_b = *t_dev + t_off[b] (see decode_step_attn_var)"""
    lib = _L.load()
    es = q.element_size()
    _kv8_check("decode_step_attn_kv8_var", cache, scales, t_max, B, H, hd)
    _i32_check("decode_step_attn_kv8_var", "t_off", t_off, B)
    _L.check(lib.mk_decode_step_attn_kv8_var(_p(q) + q_off * es, _p(k_new) + k_off * es, _p(v_new) + v_off * es,
                                             in_bs, _p(cos_t), _p(sin_t), _p(cache), _p(scales), _p(out), H * hd,
                                             _p(t_dev), _p(t_off), t_max, B, H, hd, scale, dt(q), _st()),
             "mk_decode_step_attn_kv8_var")
    return out


def kv_append_rows(k, v, ld, in_bs, cache, slot, Sn, t_max, B, H, hd):
    """the compacting prefill write of a 16-bit KV cache [B, t_max, 2 * H * hd]: source row j of sample b of the
    ROTATED keys k and of the values v (row pitch ld, sample stride in_bs in elements; k / v may be slices of one
    fused [M, 3D] buffer) goes to cache row slot[b, j] (int32 [B, Sn]); slot < 0 skips the row, and no other cache
    byte is touched"""
    lib = _L.load()
    if (cache.dtype != k.dtype or tuple(cache.shape) != (B, t_max, 2 * H * hd) or not cache.is_contiguous()):
        raise MacawHipError(f"kv_append_rows: cache {cache.dtype} {tuple(cache.shape)}; expected {k.dtype} "
                            f"{(B, t_max, 2 * H * hd)}, contiguous")
    _i32_check("kv_append_rows", "slot", slot, B * Sn)
    _L.check(lib.mk_kv_append_rows(_p(k), _p(v), ld, in_bs, _p(cache), _p(slot), Sn, t_max, B, H, hd, dt(k), _st()),
             "mk_kv_append_rows")
    return cache


def kv_quant_append_rows(k, v, ld, in_bs, cache, scales, slot, Sn, t_max, B, H, hd):
    """kv_append_rows into an e4m3 KV cache (kv8_cache) with kv_quant_append's quantisation: the bytes and scales of
    a written row are what kv_quant_append writes for that source row"""
    lib = _L.load()
    _kv8_check("kv_quant_append_rows", cache, scales, t_max, B, H, hd)
    _i32_check("kv_quant_append_rows", "slot", slot, B * Sn)
    _L.check(lib.mk_kv_quant_append_rows(_p(k), _p(v), ld, in_bs, _p(cache), _p(scales), _p(slot), Sn, t_max, B, H,
                                         hd, dt(k), _st()), "mk_kv_quant_append_rows")
    return cache, scales


def decode_attn_ok(dtype, hd, t_max):
    return dtype in (torch.bfloat16, torch.float16) and hd in (16, 32, 64, 128) and t_max * 4 <= 60 * 1024


def embedding_fwd(table, ids, out=None):
    """out[t, :] = table[ids[t], :]; ids int64 1-D"""
    lib = _L.load()
    tokens = ids.numel()
    vocab, dim = table.shape
    if out is None:
        out = torch.empty((tokens, dim), dtype=table.dtype, device=table.device)
    _L.check(lib.mk_embedding_fwd(_p(table), _p(ids), _p(out), tokens, dim, _rowmajor(out), vocab,
                                  dt(table), _st()), "mk_embedding_fwd")
    return out


def embedding_bwd_(dtable, dout, ids, padding_idx=-1):
    """dtable[ids[t]] += dout[t] (deterministic)"""
    lib = _L.load()
    vocab, dim = dtable.shape
    _L.check(lib.mk_embedding_bwd(_p(dout), _rowmajor(dout), _p(ids), _p(dtable), ids.numel(), dim,
                                  vocab, -1 if padding_idx is None else padding_idx, dt(dtable),
                                  _st()), "mk_embedding_bwd")
    return dtable


def pad8(n: int) -> int:
    return (n + 7) // 8 * 8


def im2col1d(x, B, C_, T, kw, stride, pad, sb, sc, st, ld_out=None):
    lib = _L.load()
    Lout = (T + 2 * pad - kw) // stride + 1
    K = C_ * kw
    if ld_out is None:
        ld_out = pad8(K)
    out = torch.empty((B * Lout, ld_out), dtype=x.dtype, device=x.device)
    _L.check(lib.mk_im2col1d(_p(x), _p(out), B, C_, T, kw, stride, pad, Lout, sb, sc, st, ld_out,
                             dt(x), _st()), "mk_im2col1d")
    return out, Lout


def col2im1d(dcols, B, C_, T, kw, stride, pad, Lout, sb, sc, st, out_shape):
    lib = _L.load()
    dx = torch.empty(out_shape, dtype=dcols.dtype, device=dcols.device)
    _L.check(lib.mk_col2im1d(_p(dcols), _p(dx), B, C_, T, kw, stride, pad, Lout, sb, sc, st,
                             _rowmajor(dcols), dt(dcols), _st()), "mk_col2im1d")
    return dx


def patchify(img, P):
    lib = _L.load()
    B, C_, H, W = img.shape
    img = img.contiguous()
    K = C_ * P * P
    ld = pad8(K)
    out = torch.empty((B * (H // P) * (W // P), ld), dtype=img.dtype, device=img.device)
    _L.check(lib.mk_patchify(_p(img), _p(out), B, C_, H, W, P, ld, dt(img), _st()), "mk_patchify")
    return out


def unpatchify(dcols, B, C_, H, W, P):
    lib = _L.load()
    dimg = torch.empty((B, C_, H, W), dtype=dcols.dtype, device=dcols.device)
    _L.check(lib.mk_unpatchify(_p(dcols), _p(dimg), B, C_, H, W, P, _rowmajor(dcols), dt(dcols),
                               _st()), "mk_unpatchify")
    return dimg


# ---------------------------------------------------------------- softmax --
def softmax_fwd(scores, nz, heads, Lq, Lk, ld, kmask=None, causal=False, dropout_p=0.0, seed=0,
                probs=None, want_dropped=False):
    """scores: buffer of nz*Lq rows with pitch ld.  Returns (probs, probs_dropped|None)."""
    lib = _L.load()
    if probs is None:
        probs = torch.empty_like(scores)
    pd = torch.empty_like(scores) if (dropout_p > 0.0 and want_dropped) else None
    _L.check(lib.mk_softmax_fwd(_p(scores), _p(probs), _p(pd), _p(kmask), nz, heads, Lq, Lk, ld,
                                int(causal), float(dropout_p), int(seed), dt(scores), _st()),
             "mk_softmax_fwd")
    return probs, pd


def softmax_bwd_(probs, dprobs, nz, Lq, Lk, ld, scale=1.0, dropout_p=0.0, seed=0):
    lib = _L.load()
    _L.check(lib.mk_softmax_bwd(_p(probs), _p(dprobs), nz, Lq, Lk, ld, float(scale),
                                float(dropout_p), int(seed), dt(probs), _st()), "mk_softmax_bwd")
    return dprobs


def flash_rope_ok(hd, Lq, Lk, cos_t, x) -> bool:
    """RoPE can ride inside the fused attention kernels (mk_flash_attn_rope_*): the one-workgroup-per-(b, h)
    short-sequence kernels, tables in the activations' dtype."""
    return (hd == 128 and Lq == Lk and Lk <= 160 and cos_t.dtype == x.dtype and cos_t.shape[-1] == hd
            and cos_t.is_contiguous())


def rope_fuse_mode() -> str:
    """how LlamaLayerFn folds RoPE into the short-sequence attention kernels (MACAW_ROPE_FUSE, read per layer call).
    "off" (default): mk_rope before the forward, mk_rope(inverse) behind the backward -- three launches;
    "bwd": the rotation of dq / dk back inside the backward kernel's stores; "full": q, k stay unrotated in HBM and
    are rotated on every load (three rotations per element in the backward).  All three are bit-identical
    (tests/test_kernels_gpu.py); measured in the cfg-3 step the fused forms save the 1.9 ms of the two in-place
    launches and spend 0.9 (bwd) / 1.8 ms (full) more inside the attention kernels, whose tails wait for the table
    rows and round six times per output pair: 215.1-215.6 / 214.6-215.2 / 215.0-215.5 ms -- no gain, so the plain
    form stays the default (profiles/r06_rope_fuse.txt)."""
    m = os.environ.get("MACAW_ROPE_FUSE", "off")
    if m not in ("bwd", "full", "off"):
        raise MacawHipError(f"MACAW_ROPE_FUSE={m!r}: expected bwd, full or off")
    return m


def flash_attn_fwd(q, k, v, o, B, H, Lq, Lk, hd, q_ld, q_bs, k_ld, k_bs, v_ld, v_bs, o_ld, o_bs,
                   scale, kmask=None, causal=False, lse=None, q_off=0, k_off=0, v_off=0, o_off=0,
                   rope=None):
    """fused attention forward on strided bf16 buffers (element offsets/strides).
    rope = (cos_t, sin_t, pos): q and k are the unrotated projections (see flash_rope_ok)"""
    lib = _L.load()
    es = q.element_size()
    if rope is not None:
        cos_t, sin_t, pos = rope
        _L.check(lib.mk_flash_attn_rope_fwd(_p(q) + q_off * es, _p(k) + k_off * es, _p(v) + v_off * es,
                                            _p(o) + o_off * es, _p(lse), _p(kmask), _p(cos_t), _p(sin_t),
                                            _p(pos), B, H, Lq, Lk, hd, q_ld, q_bs, k_ld, k_bs, v_ld, v_bs,
                                            o_ld, o_bs, float(scale), int(causal), dt(q), _st()),
                 "mk_flash_attn_rope_fwd")
        return o
    _L.check(lib.mk_flash_attn_fwd(_p(q) + q_off * es, _p(k) + k_off * es, _p(v) + v_off * es,
                                   _p(o) + o_off * es, _p(lse), _p(kmask), B, H, Lq, Lk, hd, q_ld,
                                   q_bs, k_ld, k_bs, v_ld, v_bs, o_ld, o_bs, float(scale),
                                   int(causal), dt(q), _st()), "mk_flash_attn_fwd")
    return o


def flash_varlen_ok(dtype, hd) -> bool:
    """the domain of flash_attn_varlen_fwd (besides the 16-byte alignment and the strides % 8 of flash_attn_fwd)"""
    return dtype in (torch.bfloat16, torch.float16) and hd in (64, 128)


def flash_attn_varlen_fwd(q, k, v, o, q_len, k_len, B, H, Lq, Lk, hd, q_ld, q_bs, k_ld, k_bs, v_ld, v_bs, o_ld, o_bs,
                          scale, lse=None, q_off=0, k_off=0, v_off=0, o_off=0):
    """the causal fused forward with per-sample lengths on the device (q_len / k_len int32 [B]; Lq / Lk host upper
    bounds): row i < q_len[b] of sample b sees key j iff j < k_len[b] and j <= i + (k_len[b] - q_len[b]); every other
    row gets o = 0 and lse = -inf; k / v rows >= k_len[b] are never read (macaw_hip.h: mk_flash_attn_varlen_fwd).
    k and v may be the two halves of a [B, t_max, 2D] cache (k_ld = v_ld = 2D, v_off = D)"""
    lib = _L.load()
    es = q.element_size()
    _i32_check("flash_attn_varlen_fwd", "q_len", q_len, B)
    _i32_check("flash_attn_varlen_fwd", "k_len", k_len, B)
    _L.check(lib.mk_flash_attn_varlen_fwd(_p(q) + q_off * es, _p(k) + k_off * es, _p(v) + v_off * es,
                                          _p(o) + o_off * es, _p(lse), _p(q_len), _p(k_len), B, H, Lq, Lk, hd, q_ld,
                                          q_bs, k_ld, k_bs, v_ld, v_bs, o_ld, o_bs, float(scale), dt(q), _st()),
             "mk_flash_attn_varlen_fwd")
    return o


def flash_attn_bwd(q, k, v, o, dout, lse, dq, dk, dv, B, H, Lq, Lk, hd, q_ld, q_bs, k_ld, k_bs, v_ld,
                   v_bs, o_ld, o_bs, scale, kmask=None, causal=False, rope=None, qk_rotated=False):
    """rope = (cos_t, sin_t, pos): dq / dk come back as gradients of the UNROTATED q, k; q and k themselves are
    the unrotated tensors, or with qk_rotated the rotated ones (mk_rope ran before the forward)"""
    lib = _L.load()
    dvec = torch.empty(B * H * Lq, dtype=torch.float32, device=q.device)
    if rope is not None:
        cos_t, sin_t, pos = rope
        _L.check(lib.mk_flash_attn_rope_bwd(_p(q), _p(k), _p(v), _p(o), _p(dout), _p(lse), _p(dvec), _p(dq),
                                            _p(dk), _p(dv), _p(kmask), _p(cos_t), _p(sin_t), _p(pos), B, H,
                                            Lq, Lk, hd, q_ld, q_bs, k_ld, k_bs, v_ld, v_bs, o_ld, o_bs,
                                            float(scale), int(causal), int(qk_rotated), dt(q), _st()),
                 "mk_flash_attn_rope_bwd")
        return
    _L.check(lib.mk_flash_attn_bwd(_p(q), _p(k), _p(v), _p(o), _p(dout), _p(lse), _p(dvec), _p(dq),
                                   _p(dk), _p(dv), _p(kmask), B, H, Lq, Lk, hd, q_ld, q_bs, k_ld,
                                   k_bs, v_ld, v_bs, o_ld, o_bs, float(scale), int(causal), dt(q),
                                   _st()), "mk_flash_attn_bwd")


def cross_entropy(logits, labels, V):
    """logits [rows, ld>=V] row-major; labels int64 [rows] already shifted.
    returns (row_loss, row_lse, sum_cnt[2])"""
    lib = _L.load()
    rows = logits.shape[0]
    row_loss = torch.empty(rows, dtype=torch.float32, device=logits.device)
    row_lse = torch.empty(rows, dtype=torch.float32, device=logits.device)
    sum_cnt = torch.empty(4, dtype=torch.float32, device=logits.device)
    _L.check(lib.mk_cross_entropy(_p(logits), _p(labels), _p(row_loss), _p(row_lse), _p(sum_cnt),
                                  rows, V, _rowmajor(logits), dt(logits), _st()),
             "mk_cross_entropy")
    return row_loss, row_lse, sum_cnt


def cross_entropy_bwd(logits, labels, row_lse, sum_cnt, V, grad_scale=1.0, out=None,
                      grad_scale_dev=None):
    lib = _L.load()
    rows = logits.shape[0]
    if out is None:
        out = torch.empty_like(logits)
    _L.check(lib.mk_cross_entropy_bwd(_p(logits), _p(out), _p(labels), _p(row_lse), _p(sum_cnt),
                                      float(grad_scale), _p(grad_scale_dev), rows, V,
                                      _rowmajor(logits), dt(logits),
                                      _st()), "mk_cross_entropy_bwd")
    return out


def argmax_rows(x, cols=None):
    """first-max index of every row of a 2-D row-major (pitched) tensor -> int64 [rows]"""
    lib = _L.load()
    rows = x.shape[0]
    cols = x.shape[1] if cols is None else cols
    out = torch.empty(rows, dtype=torch.int64, device=x.device)
    _L.check(lib.mk_argmax_rows(_p(x), _rowmajor(x), rows, cols, _p(out), dt(x), _st()),
             "mk_argmax_rows")
    return out


def sample_rows(x, cols=None, temperature=1.0, top_k=0, top_p=1.0, seed=0, step=0):
    """one sampled column per row of a 2-D row-major (pitched) tensor -> int64 [rows] (see mk_sample_rows): temperature,
    then top-k (0 = off; exactly k columns, ties to the lower column), then top-p, then the draw with the counter hash
    of (seed, step, row); the sampled twin of argmax_rows"""
    lib = _L.load()
    rows = x.shape[0]
    cols = x.shape[1] if cols is None else cols
    out = torch.empty(rows, dtype=torch.int64, device=x.device)
    _L.check(lib.mk_sample_rows(_p(x), _rowmajor(x), rows, cols, float(temperature), int(top_k), float(top_p),
                                int(seed) & 0xFFFFFFFFFFFFFFFF, int(step), _p(out), dt(x), _st()), "mk_sample_rows")
    return out


def sample_rows_warp(x, cols=None, temperature=1.0, top_k=0, top_p=1.0, seed=0, min_p=0.0, typical_p=1.0,
                     epsilon_cutoff=0.0, eta_cutoff=0.0, step=0):
    """sample_rows with the four warpers behind top-p, in front of the draw (rule 6 of the header; see
    mk_sample_rows_warp): min_p, typical_p, epsilon_cutoff, eta_cutoff, off at 0, 1, 0, 0.  With all four off this IS the
    sample_rows call."""
    if not _warpers_on(min_p, typical_p, epsilon_cutoff, eta_cutoff):
        return sample_rows(x, cols, temperature, top_k, top_p, seed, step)
    lib = _L.load()
    rows = x.shape[0]
    cols = x.shape[1] if cols is None else cols
    out = torch.empty(rows, dtype=torch.int64, device=x.device)
    _L.check(lib.mk_sample_rows_warp(_p(x), _rowmajor(x), rows, cols, float(temperature), int(top_k), float(top_p),
                                     float(min_p), float(typical_p), float(epsilon_cutoff), float(eta_cutoff),
                                     int(seed) & 0xFFFFFFFFFFFFFFFF, int(step), _p(out), dt(x), _st()),
             "mk_sample_rows_warp")
    return out


def sample_keep_rows(x, cols=None, temperature=1.0, top_k=0, top_p=1.0, min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0,
                     eta_cutoff=0.0):
    """the kept mask of sample_rows_warp's filter -> bool [rows, cols]: True where a draw with these arguments can land (HF's
    "which tokens survive the warpers"; see mk_sample_keep_rows).  A row without a finite logit is all False."""
    lib = _L.load()
    rows = x.shape[0]
    cols = x.shape[1] if cols is None else cols
    keep = torch.empty((rows, cols), dtype=torch.uint8, device=x.device)
    _L.check(lib.mk_sample_keep_rows(_p(x), _rowmajor(x), rows, cols, float(temperature), int(top_k), float(top_p),
                                     float(min_p), float(typical_p), float(epsilon_cutoff), float(eta_cutoff), _p(keep),
                                     cols, dt(x), _st()), "mk_sample_keep_rows")
    return keep.bool()


class SampleTable:
    """the per-row sampling records of a batch on the device (include/macaw_hip.h, "Per-row sampling table"), built once
    per call from validated host values.  rows: one entry per row of logits, None for a greedy row or a dict with the
    keys temperature (1.0), top_k (0 = off), top_p (1.0), min_p (0.0), typical_p (1.0), epsilon_cutoff (0.0), eta_cutoff
    (0.0), seed (0) and stream (0), every one optional.  A value outside the scalar entries' domain is refused here: the
    kernel would decode such a row greedily.  records: uint8 [rows, 48] on `device`; sampled: bool per row on the host"""
    RECORD = struct.Struct("<fifffffIQii")      # 48 bytes: the header's layout
    KEYS = ("temperature", "top_k", "top_p", "min_p", "typical_p", "epsilon_cutoff", "eta_cutoff", "seed", "stream")

    def __init__(self, rows, device):
        rows = list(rows)
        if not rows:
            raise MacawHipError("SampleTable: no rows")
        buf, self.sampled = bytearray(), []
        for b, r in enumerate(rows):
            if r is not None and (not isinstance(r, dict) or set(r) - set(self.KEYS)):
                raise MacawHipError(f"SampleTable: row {b} must be None or a dict with keys out of {self.KEYS}, got {r!r}")
            self.sampled.append(r is not None)
            r = r or {}
            t, k, p = r.get("temperature", 1.0), r.get("top_k", 0), r.get("top_p", 1.0)
            w = (r.get("min_p", 0.0), r.get("typical_p", 1.0), r.get("epsilon_cutoff", 0.0), r.get("eta_cutoff", 0.0))
            seed, stream = r.get("seed", 0), r.get("stream", 0)
            ok = (all(isinstance(v, numbers.Real) and not isinstance(v, bool) for v in (t, p, *w))
                  and all(isinstance(v, numbers.Integral) and not isinstance(v, bool) for v in (k, seed, stream))
                  and math.isfinite(t) and t > 0 and 0 < p <= 1 and 0 <= k < 2 ** 31 and 0 <= w[0] <= 1 and 0 < w[1] <= 1
                  and 0 <= w[2] < 1 and 0 <= w[3] < 1 and 0 <= stream < 2 ** 32)
            if not ok:
                raise MacawHipError(f"SampleTable: row {b}: {r!r} lies outside the domain of sample_rows / sample_rows_warp")
            buf += self.RECORD.pack(float(t), int(k), float(p), *map(float, w), int(stream),
                                    int(seed) & 0xFFFFFFFFFFFFFFFF, int(self.sampled[-1]), 0)
        self.rows = len(rows)
        self.records = torch.frombuffer(buf, dtype=torch.uint8).view(self.rows, self.RECORD.size).to(device)


def _sample_table_check(op, x, table):
    if not isinstance(table, SampleTable):
        raise MacawHipError(f"{op}: table must be an ops.SampleTable, got {type(table).__name__}")
    if x.dim() != 2 or table.rows != x.shape[0]:
        raise MacawHipError(f"{op}: a SampleTable of {table.rows} rows for logits {tuple(x.shape)}")
    if table.records.device != x.device:
        raise MacawHipError(f"{op}: the table lives on {table.records.device}, the logits on {x.device}")


def sample_rows_table(x, cols, table: SampleTable, step=0):
    """one column per row of a 2-D row-major (pitched) tensor -> int64 [rows], every row by its own record of `table` (see
    mk_sample_rows_table): a greedy row what argmax_rows returns, a sampled row what sample_rows / sample_rows_warp return
    with the record's values and seed for the same logits at row index record.stream, whatever its place in the batch"""
    lib = _L.load()
    rows = x.shape[0]
    cols = x.shape[1] if cols is None else cols
    _sample_table_check("sample_rows_table", x, table)
    out = torch.empty(rows, dtype=torch.int64, device=x.device)
    _L.check(lib.mk_sample_rows_table(_p(x), _rowmajor(x), rows, cols, _p(table.records), int(step), _p(out), dt(x),
                                      _st()), "mk_sample_rows_table")
    return out


def adamw_(param, master, m, v, grad, lr, beta1, beta2, eps, wd, step, grad_scale=1.0):
    lib = _L.load()
    _L.check(lib.mk_adamw(_p(param), _p(master), _p(m), _p(v), _p(grad), param.numel(), lr, beta1,
                          beta2, eps, wd, step, grad_scale, dt(param), _st()), "mk_adamw")


def prof_begin():
    _L.check(_L.load().mk_prof_begin(), "mk_prof_begin")


def prof_report(path: str):
    _L.check(_L.load().mk_prof_report(path.encode()), "mk_prof_report")


def prof_sum(kind: int):
    """(total_ms, total_flops, launches) of one launch kind since prof_begin: 0 GEMM, 1 fused
    attention forward, 2 fused attention backward.  Call before prof_end."""
    ms, fl, n = C.c_double(0), C.c_double(0), C.c_int64(0)
    _L.check(_L.load().mk_prof_sum(kind, C.byref(ms), C.byref(fl), C.byref(n)), "mk_prof_sum")
    return ms.value, fl.value, n.value


def prof_end():
    """returns (total_ms, total_flops, launches) of the mk_gemm launches since prof_begin"""
    ms, fl, n = C.c_double(0), C.c_double(0), C.c_int64(0)
    _L.check(_L.load().mk_prof_end(C.byref(ms), C.byref(fl), C.byref(n)), "mk_prof_end")
    return ms.value, fl.value, n.value


# ------------------------------------------------------------------- LoRA --
# csrc/lora.hip: the rank-r products of the adapters (macaw_llm_amd/lora.py).  A GROUP is 1-3 modules sharing
# one input (q|k|v, gate|up); U / dU are [M, G r] in the activation dtype, Ut / dUt their transposes with a
# pitch of pad8(M).  Launch kind 4 of the in-library profiler.
PROF_LORA = 4


def _ptrs3(ts):
    return [_p(t) for t in ts] + [None] * (3 - len(ts))


def _tags(tags, G):
    return (C.c_uint64 * 3)(*(list(tags or []) + [0] * (3 - len(tags or []))))


def lora_workspace(M, N, G, r, device):
    b = C.c_int64(0)
    _L.check(_L.load().mk_lora_workspace(M, N, G, r, C.byref(b)), "mk_lora_workspace")
    return torch.empty(b.value, dtype=torch.uint8, device=device)


def lora_down(x, As, p=0.0, seed=0, tags=None):
    """U[:, i r:(i+1) r] = drop_i(x) A_i^T for the group As ([r, K] each); returns (U, Ut)"""
    M, K = x.shape
    G, r = len(As), As[0].shape[0]
    U = torch.empty((M, G * r), dtype=x.dtype, device=x.device)
    Ut = torch.empty((G * r, pad8(M)), dtype=x.dtype, device=x.device)
    _L.check(_L.load().mk_lora_down(_p(x), _rowmajor(x), M, K, *_ptrs3(As), G, r, _p(U), _p(Ut), Ut.shape[1],
                                    float(p), int(seed) & 0xFFFFFFFFFFFFFFFF, _tags(tags, G), dt(x), _st()),
             "mk_lora_down")
    return U, Ut


def lora_up_add_(U, Bs, Ys, s):
    """Y_i += s U_i B_i^T in place (Ys: [M, N] views sharing one pitch)"""
    M, N = Ys[0].shape
    G, r = len(Bs), Bs[0].shape[1]
    _L.check(_L.load().mk_lora_up_add(_p(U), M, r, G, *_ptrs3(Bs), *_ptrs3(Ys), _rowmajor(Ys[0]), N, float(s), dt(U),
                                      _st()), "mk_lora_up_add")


def lora_bwd_dy(dYs, Bs, Ut, s):
    """(dU, dUt, [dB_i]) with dU = s dY_i B_i, dB_i = s dY_i^T U_i"""
    M, N = dYs[0].shape
    G, r = len(Bs), Bs[0].shape[1]
    dev, dtype = dYs[0].device, dYs[0].dtype
    dU = torch.empty((M, G * r), dtype=dtype, device=dev)
    dUt = torch.empty((G * r, pad8(M)), dtype=dtype, device=dev)
    dB = [torch.empty((N, r), dtype=dtype, device=dev) for _ in range(G)]
    ws = lora_workspace(M, N, G, r, dev)
    _L.check(_L.load().mk_lora_bwd_dy(*_ptrs3(dYs), _rowmajor(dYs[0]), M, N, *_ptrs3(Bs), _p(Ut), Ut.shape[1], G, r,
                                      float(s), _p(dU), _p(dUt), *_ptrs3(dB), _p(ws), ws.numel(), dt(dU), _st()),
             "mk_lora_bwd_dy")
    return dU, dUt, dB


def lora_bwd_x_(x, dU, dUt, As, dx, p=0.0, seed=0, tags=None):
    """dx += sum_i drop'_i(dU_i A_i) in place; returns [dA_i] with dA_i = dU_i^T drop_i(x)"""
    M, K = x.shape
    G, r = len(As), As[0].shape[0]
    dA = [torch.empty((r, K), dtype=x.dtype, device=x.device) for _ in range(G)]
    ws = lora_workspace(M, K, G, r, x.device)
    _L.check(_L.load().mk_lora_bwd_x(_p(x), _rowmajor(x), M, K, _p(dU), _p(dUt), dUt.shape[1], *_ptrs3(As), G, r,
                                     float(p), int(seed) & 0xFFFFFFFFFFFFFFFF, _tags(tags, G), _p(dx), _rowmajor(dx),
                                     *_ptrs3(dA), _p(ws), ws.numel(), dt(x), _st()), "mk_lora_bwd_x")
    return dA


def lora_merge_(W, A, B, s):
    """W += s B A (fp32 product, one rounding) in place"""
    N, K = W.shape
    r = A.shape[0]
    ws = lora_workspace(1, K, 1, r, W.device)
    _L.check(_L.load().mk_lora_merge(_p(W), _rowmajor(W), N, K, _p(A), _p(B), r, float(s), _p(ws), ws.numel(), dt(W),
                                     _st()), "mk_lora_merge")
    return W


# csrc/lora_bgmv.hip: mixed-adapter LoRA of a decode step.  Row m of the batch uses adapter idx[m] of the bank's
# stacks A [n, G r, K] / B [n, G N, r] / s [n]; an idx outside [0, n) is a base row (zero row of U, Y untouched).
def lora_bgmv_ok(x, A, prologue=0):
    """mk_lora_bgmv_shrink / _expand's domain on the token side: 16-bit rows, M <= 32, 16-byte rows of K <= 30712"""
    K = A.shape[2]
    return (x.dtype in (torch.bfloat16, torch.float16) and x.dim() == 2 and x.shape[0] <= 32 and K % 8 == 0 and
            K <= 30712 and x.shape[1] == (2 * K if prologue == 2 else K) and x.stride(1) == 1 and x.stride(0) % 8 == 0 and
            x.data_ptr() % 16 == 0)


def lora_bgmv_shrink(x, A, idx, G, prologue=0, norm_w=None, eps=0.0, out=None):
    """U[m] = rnd16(prologue(x)[m] A[idx[m]]^T) [M, G r] (out: a [M, G r] view, pitched rows allowed); prologue as
    decode_linear (1 = RMSNorm(x; norm_w, eps), 2 = SwiGLU of x = [gate | up] [M, 2 K]) with the same rounding points"""
    M = x.shape[0]
    n, GR, K = A.shape
    if GR % G or not A.is_contiguous() or idx.dtype != torch.int32 or idx.numel() != M or not idx.is_contiguous():
        raise MacawHipError(f"lora_bgmv_shrink: stack {tuple(A.shape)} for G = {G}, idx {idx.dtype} {tuple(idx.shape)}")
    if out is None:
        out = torch.empty((M, GR), dtype=x.dtype, device=x.device)
    _L.check(_L.load().mk_lora_bgmv_shrink(_p(x), _rowmajor(x), M, K, _p(A), n, G, GR // G, _p(idx), prologue,
                                           _p(norm_w), eps, _p(out), _rowmajor(out), dt(x), _st()), "mk_lora_bgmv_shrink")
    return out


def lora_bgmv_expand_(U, B, s, idx, Y, G):
    """Y[m, :G N] = rnd16(Y[m, :G N] + s[idx[m]] U[m] (x) B[idx[m]]) in place, module i of the group on columns
    [i N, (i + 1) N) with its r columns of U; Y [M, >= G N] (pitched rows allowed)"""
    M = U.shape[0]
    n, GN, r = B.shape
    if (GN % G or U.shape[1] != G * r or not B.is_contiguous() or s.dtype != torch.float32 or s.numel() != n or
            not s.is_contiguous() or idx.dtype != torch.int32 or idx.numel() != M or not idx.is_contiguous() or
            Y.shape[0] != M or Y.shape[1] < GN):
        raise MacawHipError(f"lora_bgmv_expand_: U {tuple(U.shape)}, stack {tuple(B.shape)} for G = {G}, s {s.dtype} "
                            f"{tuple(s.shape)}, idx {idx.dtype} {tuple(idx.shape)}, Y {tuple(Y.shape)}")
    _L.check(_L.load().mk_lora_bgmv_expand(_p(U), _rowmajor(U), M, G, r, _p(B), _p(s), n, _p(idx), _p(Y), _rowmajor(Y),
                                           GN // G, dt(U), _st()), "mk_lora_bgmv_expand")
    return Y
