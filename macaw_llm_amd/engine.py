"""Layer-level forward/backward engine for the Macaw-LLM hot path.

Each autograd.Function here is one *block* of the reference graph (a LLaMA decoder layer,
a CLIP/Whisper encoder layer, an nn.MultiheadAttention, the lm_head+loss, the multimodal
prefix assembly) whose forward AND backward are hand-orchestrated sequences of the gfx950
kernels in csrc/ (through ops.py).  PyTorch autograd only chains these blocks; it never
differentiates an eager op on the hot path, and residual / fan-out gradient sums are fused
into our kernels (rmsnorm/layernorm `dres`, GEMM `accumulate`).

Attention is formulated as batched MFMA GEMMs + the softmax kernel (scores are written in
the activation dtype, softmax runs in fp32: the reference's rounding points,
modeling.py:197-215).  At the sequence lengths of BASELINE cfg 2/3 (S = 136/144) the score
tensor is ~42 MB per layer; a fused flash kernel for S = 2048 (cfg 4) is a later row.
"""
from __future__ import annotations

import math
import os
from typing import NamedTuple, Optional

import torch

from . import lib as _L
from . import ops

pad8 = ops.pad8


# =========================================================================
# attention core on strided buffers
# =========================================================================
class TDesc:
    """A [rows, heads*hd]-style operand inside a bigger buffer: element offset of
    (batch b, head h) = off + b*bs + h*hd; row pitch ld."""
    __slots__ = ("t", "ld", "bs", "off")

    def __init__(self, t, ld, bs, off=0):
        self.t, self.ld, self.bs, self.off = t, ld, bs, off


def _pad64(n):
    return (n + 63) // 64 * 64


def attention_fwd(q: TDesc, k: TDesc, v: TDesc, o: TDesc, B, H, Lq, Lk, hd, scale, kmask=None,
                  causal=False, p=0.0, seed=0, Lk_pad=None):
    """o[b,h] = dropout(softmax(scale * q[b,h] k[b,h]^T + mask)) v[b,h].
    Returns (probs, probs_dropped|None) with rows [B*H*Lq, Lp].

    Lk_pad (multiple of 64, optional): the caller guarantees that rows [Lk, Lk_pad) of the K/V
    buffers exist and are ZERO; the key reduction then runs over Lk_pad so the long-K products
    take the aligned LDS-DMA GEMM with a batched stream-K split of the long reduction."""
    Lp = Lk_pad if Lk_pad is not None else pad8(Lk)
    Kred = Lk_pad if Lk_pad is not None else Lk
    dev, dtype = q.t.device, q.t.dtype
    scores = torch.empty((B * H * Lq, Lp), dtype=dtype, device=dev)
    ops.gemm_raw(q.t, k.t, scores, Lq, Lk, hd, q.ld, k.ld, Lp, nb1=B, nb2=H, sA=(q.bs, hd),
                 sB=(k.bs, hd), sC=(H * Lq * Lp, Lq * Lp), a_off=q.off, b_off=k.off, alpha=scale)
    probs, pd = ops.softmax_fwd(scores, B * H, H, Lq, Lk, Lp, kmask=kmask, causal=causal,
                                dropout_p=p, seed=seed, probs=scores, want_dropped=p > 0.0)
    pa = pd if pd is not None else probs
    ops.gemm_raw(pa, v.t, o.t, Lq, hd, Kred, Lp, v.ld, o.ld, b_red=True, nb1=B, nb2=H,
                 sA=(H * Lq * Lp, Lq * Lp), sB=(v.bs, hd), sC=(o.bs, hd), b_off=v.off, c_off=o.off)
    return probs, pd


def attention_bwd(do: TDesc, q: TDesc, k: TDesc, v: TDesc, probs, pd, dq: TDesc, dk: TDesc,
                  dv: TDesc, B, H, Lq, Lk, hd, scale, p=0.0, seed=0, Lk_pad=None):
    """Given do = dL/do, writes dq, dk, dv (same layouts as q, k, v)."""
    Lp = Lk_pad if Lk_pad is not None else pad8(Lk)
    Kred = Lk_pad if Lk_pad is not None else Lk
    dP = torch.empty_like(probs)
    sP = (H * Lq * Lp, Lq * Lp)
    # dP = do v^T
    ops.gemm_raw(do.t, v.t, dP, Lq, Lk, hd, do.ld, v.ld, Lp, nb1=B, nb2=H, sA=(do.bs, hd),
                 sB=(v.bs, hd), sC=sP, a_off=do.off, b_off=v.off)
    # dv = P_dropped^T do      (both operands reduction-major: no transposes)
    pa = pd if pd is not None else probs
    ops.gemm_raw(pa, do.t, dv.t, Lk, hd, Lq, Lp, do.ld, dv.ld, a_red=True, b_red=True, nb1=B, nb2=H,
                 sA=sP, sB=(do.bs, hd), sC=(dv.bs, hd), b_off=do.off, c_off=dv.off)
    # dS = softmax'(P, dP) * scale   (in place; pad columns come out as zeros)
    ops.softmax_bwd_(probs, dP, B * H, Lq, Lk, Lp, scale=scale, dropout_p=p, seed=seed)
    # dq = dS k ; dk = dS^T q
    ops.gemm_raw(dP, k.t, dq.t, Lq, hd, Kred, Lp, k.ld, dq.ld, b_red=True, nb1=B, nb2=H, sA=sP,
                 sB=(k.bs, hd), sC=(dq.bs, hd), b_off=k.off, c_off=dq.off)
    ops.gemm_raw(dP, q.t, dk.t, Lk, hd, Lq, Lp, q.ld, dk.ld, a_red=True, b_red=True, nb1=B, nb2=H,
                 sA=sP, sB=(q.bs, hd), sC=(dk.bs, hd), b_off=q.off, c_off=dk.off)


# BASELINE cfg 5: "fp8 MFMA for alignment-attn and QKV GEMMs".  Opt-in (MM_LLMs.set_fp8): the FORWARD
# and the GRAD-INPUT GEMMs of the fused q|k|v projection (modeling.py:159-162) and of the alignment
# K/V projection of the token table (:882-910) run on the f8f6f4 MFMA at twice the bf16 rate:
#   * activations / gradients: e4m3 with ONE SCALE PER ROW (token), quantised where they are produced;
#   * weights: e4m3 with one scale per output channel (forward) and, as a transposed copy, one scale
#     per input channel (grad-input), made ONCE per optimizer step (ops.fp8_weight) and reused by the
#     checkpoint recompute;
#   * grad-weight GEMMs stay bf16 (they reduce over tokens: both operands would need transposed 8-bit
#     copies per step for a GEMM that is a third of the projection's work).
# "mlp" extends the same treatment to gate|up and down (beyond BASELINE cfg 5's wording; off unless asked).
FP8 = {"qkv": False, "align": False, "mlp": False}

# Grad-weight GEMMs of a decoder layer on a SECOND stream beside the grad-input GEMMs of the first.  dx = dy W and
# dW = dy^T x of a projection are independent, and a grad-input GEMM with fewer 256 x 256 tiles than the chip has CUs
# (M = 2176 at BASELINE cfg 2: 9 x 16 = 144 tiles on 256 CUs, one round at 56 % occupancy) leaves CUs idle that the
# grad-weight GEMM's workgroups can take.  The grad-input launch is submitted FIRST (it gets its CUs), the grad-weight
# launch waits only for the event recorded when dy was complete; the layer's backward joins the side stream before it
# returns, so gradient hooks, bucket collectives and the optimizer see finished gradients exactly as before.  Same
# kernels on the same operands (the GEMM scratch is per stream, ops._workspace): results are bit-identical.
# Measured (profiles/r06_dw_side_stream.txt): cfg 2 136.0 / 135.4 -> 131.0 / 130.1 ms per step (+3.9 %), cfg 3 (M = 4608:
# 288 tiles, whose 32-tile tail already fills the chip as eighths) +-0, cfg 5 (360 tiles) +0.7 % -- so "auto" (default) turns it
# on where the [M, D] grad-input GEMMs are less than one round or end in a round between 1/8 and full -- on ONE rank (see
# _DwSide: beside collectives it stays off unless forced).  MACAW_DW_STREAM = 0 | 1 | auto; DW_SIDE["on"] at run time
# (bench.py switches it off for its instrumented last step: per-launch durations need serial launches).
DW_SIDE = {"on": {"0": False, "1": True}.get(os.environ.get("MACAW_DW_STREAM", "auto"), "auto"), "streams": {},
           # which projections' pairs go out on two streams when it is on (A/B switch: MACAW_DW_PAIRS=o,qkv ...)
           "pairs": set((os.environ.get("MACAW_DW_PAIRS") or "down,gu,o,qkv,lm").split(","))}


# Frozen audio tower on a second stream beside the image / video tower (MACAW_ENC_STREAMS = 1; off by default): the towers are
# independent until the prefix is assembled, and their short-K GEMMs / 4-wave attention leave CUs idle between rounds.
# cfg 3, alternated in fresh processes: one box 218.4 / 218.4 -> 217.6 / 217.3 ms per step (+0.4-0.5 %), another 207.5 / 207.8 ->
# 207.6 / 207.5 (+-0) (profiles/r06_dw_side_stream.txt "towers"): inside the noise, so the default keeps one stream.
# Outputs bit-identical (tests/test_model_gpu.py); bench.py switches it off for its instrumented last step.
ENC_SIDE = {"on": os.environ.get("MACAW_ENC_STREAMS", "0") == "1", "streams": {}}


def tower_side_stream(x, tower, other=True):
    """the stream a FROZEN modality tower may run on beside the other towers, or None (experiment: ENC_SIDE)"""
    if not (ENC_SIDE["on"] and other and x.is_cuda) or torch.cuda.is_current_stream_capturing():
        return None
    if torch.is_grad_enabled() and any(p.requires_grad for p in tower.parameters()):
        return None
    if not getattr(tower, "_macaw_side_warm", False):
        # the FIRST forward of a tower re-homes its q / k / v parameters into fused storage (modeling.fused_encoder_qkv):
        # that must happen on the stream everybody else reads the parameters on (found by the NaN-poisoned allocator of
        # tests/conftest.py: re-homed on the side stream, the weights read as NaN in the next test's oracle)
        tower._macaw_side_warm = True
        return None
    st = ENC_SIDE["streams"].get(x.device)
    if st is None:
        st = ENC_SIDE["streams"][x.device] = torch.cuda.Stream(device=x.device)
    ENC_SIDE["launches"] = ENC_SIDE.get("launches", 0) + 1
    return st


def dw_side_auto(M: int, D: int, cus: int) -> bool:
    """the "auto" rule of DW_SIDE: do the [M, D] grad-input GEMMs of a layer leave CUs idle?  Less than one round of
    256 x 256 tiles (cfg 2: 9 x 16 = 144 on 256 CUs, +3.9 %), or a last round between 1/8 and full (cfg 5: 18 x 20 = 360 =
    256 + 104, +0.7 %); tails of <= 1/8 of the CUs already run as eighth-tiles on the whole chip (cfg 3: 288 = 256 + 32,
    measured +-0 / -0.3 %), whole rounds have nothing idle (cfg 4: 512); fewer than 256 rows take the skinny kernels"""
    if M < 256:
        return False
    tiles = ((M + 255) // 256) * ((D + 255) // 256)
    return tiles < cus or tiles % cus > cus // 8


class _DwSide:
    """fork / launch / join of one layer's grad-weight GEMMs (no-op object when off)"""

    def __init__(self, dev, M=0, D=0):
        self.side = None
        on = DW_SIDE["on"]
        if on == "auto":
            # one rank only: with the stream FORCED on, the world-2 test of the retired per-tensor runtime (tests/legacy_steps.py)
            # came out with ONE deviating weight in 2 of 5 full-suite runs (never stand-alone: 0 of 12; the bucket runtime's own
            # world-2 test 11 of 11 green) -- cause not found, so beside collectives the default stays one stream
            # (profiles/r06_dw_side_stream.txt "world 2")
            multi = torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1
            on = (dev.type == "cuda" and not multi
                  and dw_side_auto(M, D, torch.cuda.get_device_properties(dev).multi_processor_count))
        # (inside a hipGraph capture every stream shares the device's ONE GEMM scratch: stay on the capture stream)
        if on and dev.type == "cuda" and not torch.cuda.is_current_stream_capturing():
            st = DW_SIDE["streams"].get(dev)
            if st is None:
                st = DW_SIDE["streams"][dev] = torch.cuda.Stream(device=dev)
            self.side, self.main, self.used = st, torch.cuda.current_stream(dev), False

    def fork(self):
        """call when dy is complete on the main stream, BEFORE the grad-input launch"""
        return self.main.record_event() if self.side is not None else None

    def dw(self, ev, dy, x, w, pair=None):
        if self.side is None or (pair is not None and pair not in DW_SIDE["pairs"]):
            return ops.linear_dw(dy, x, w=w)
        # the destination comes from the COMPUTE stream's pool (a bucket slot, or a fresh tensor allocated here, outside the
        # side-stream context): everything that reads the gradient later lives on that stream or synchronises with it
        out = ops.grad_dst(w)
        if out is None:
            out = torch.empty((dy.shape[1], x.shape[1]), dtype=dy.dtype, device=dy.device)
        self.side.wait_event(ev)
        with torch.cuda.stream(self.side):
            ops.linear_dw(dy, x, out=out)
        for t in (dy, x, out):
            t.record_stream(self.side)       # (the allocator must not hand these blocks out before the side GEMM ran)
        self.used = True
        DW_SIDE["launches"] = DW_SIDE.get("launches", 0) + 1      # (for the tests: did anything go through the side stream?)
        return out

    def pair(self, dy, W, x, name, want_dw, fp8=False, drain=False):
        """(dx = dy W, dW = dy^T x or None) of one projection: the grad-input launch first, its partner beside it"""
        ev = self.fork()
        dx = _fp8_dx(dy, W) if fp8 else ops.linear_dx(dy, W)
        return dx, (self.dw(ev, dy, x, W, name) if want_dw else None)

    def join(self):
        if self.side is not None and self.used:
            # More than one rank (the stream is then on only if FORCED): a HOST wait in front of the stream-ordered one.  With the
            # event join alone the retired per-tensor runtime's world-2 test deviated in 2 of 5 full-suite runs, with the host wait
            # in 0 of 5 (profiles/r06_dw_side_stream.txt "World 2") -- which consumer is not ordered by the event is not known yet.
            # MACAW_DW_JOIN_SYNC = 1 / 0 overrides.
            hs = os.environ.get("MACAW_DW_JOIN_SYNC")
            if hs == "1" or (hs is None and torch.distributed.is_available() and torch.distributed.is_initialized()
                             and torch.distributed.get_world_size() > 1):
                self.side.synchronize()
            self.main.wait_stream(self.side)


# Grad-weight tiles inside the grad-input launches of a decoder layer (ops.DwQueue / mk_gemm_grouped): the layer's four
# grad-input GEMMs run whole 256 x 256 tiles only, and the CUs that a partial last round leaves idle compute tiles of the
# layer's grad-weight GEMMs in the same launch -- dW(down) queued before dx(down), dW(gate|up) before dx(gate|up), dW(o)
# before dx(o), dW(q|k|v) before dx(q|k|v), whose launch drains the queue.  One stream, no events: every gradient of the
# layer is complete on the compute stream when its backward returns, under graph capture and planned CU counts alike.
# Every tile is computed as mk_gemm computes a whole tile, so results are bit-identical.  A layer takes this path only
# when all four projections are groupable (16-bit, fused q|k|v and gate|up storage, whole tiles, no fp8 grad-input, no
# LoRA, every weight gradient wanted); other layers keep _DwSide.  Both are the projection backend of the ONE backward body.
# MACAW_DW_FILL = 0 | 1 | auto; DW_FILL["on"] at run time.  Measured: profiles/dw_fill_cfg3.txt.
DW_FILL = {"on": {"0": False, "1": True}.get(os.environ.get("MACAW_DW_FILL", "auto"), "auto"), "layers": 0}
DW_FILL_AUTO = True        # what "auto" means


def _dw_fill_ok(M, D, FF, x2, need, lo, gu, wqkv, wgu, fp8_any) -> bool:
    """may this layer's backward run its grad-weight GEMMs as fillers of its grad-input launches?"""
    on = DW_FILL["on"]
    if on == "auto":
        on = DW_FILL_AUTO
    if not on or lo is not None or gu is None or wqkv is None or wgu is None or fp8_any or not x2.is_cuda:
        return False
    if x2.dtype not in (torch.bfloat16, torch.float16) or not all(need[7:14]):
        return False
    # whole 256 x 256 x 64 tiles in all eight products (M is an output extent of dx and the reduction of dW)
    return M % 256 == 0 and D % 256 == 0 and FF % 256 == 0


class _DwFill:
    """the projections' backward of a groupable layer (DW_FILL): _DwSide's interface over an ops.DwQueue"""

    def __init__(self):
        DW_FILL["layers"] += 1
        # inside a carry window the layers of a backward pass share one queue, and a layer leaves it un-drained as long as
        # every one of its gradients goes straight into its bucket slot (`slots`): nothing reads a slot before ops.dw_flush()
        self.shared = DW_CARRY["on"] and _dw_window_join()
        self.slots = True
        self.q = ops.DW_WINDOW["q"] if self.shared else ops.DwQueue()

    def pair(self, dy, W, x, name, want_dw, fp8=False, drain=False):
        """dW is queued BEFORE the grad-input launch, which takes its tiles as fillers (all that is queued with drain, the
        least-idle level while the layer carries); its destination is the weight's gradient-bucket slot, else a fresh tensor"""
        out = ops.grad_dst(W)
        if out is None:
            # (a fresh tensor is read by the gradient hook as soon as the layer returns: the layer drains as without a window)
            self.slots = False
            out = torch.empty((dy.shape[1], x.shape[1]), dtype=dy.dtype, device=dy.device)
        dw = self.q.push(dy, x, out)
        return self.q.dx(dy, W, drain=_L.GROUP_CARRY if self.shared and self.slots else drain), dw

    def join(self):
        if self.shared and self.slots:
            ops.DW_WINDOW["carried"] += sum(it[2] - it[1] for it in self.q.items)     # (tiles left to the next layer's launches)
        else:
            self.q.flush()       # (nothing is left behind a draining launch)


# One queue per backward pass instead of one per layer (ops.DW_WINDOW; opened by bucketed.BucketedStep.begin): the dx(q|k|v)
# launch of a layer no longer has to use the queue up, so each of the four launches ends at the level of least idle time and
# the tiles left over fill the launches of the layer processed next (csrc/gemm_group_plan.h plan_carry).  The same tiles,
# the same instruction stream: bit-identical results.  MACAW_DW_CARRY = 0 | 1; DW_CARRY["on"] at run time.
# Measured: profiles/dw_carry_cfg3.txt.
DW_CARRY = {"on": os.environ.get("MACAW_DW_CARRY", "1") != "0"}


def _dw_window_flush():
    """end of a backward pass that carried: code that reads .grad without the runtime's finish() sees complete gradients"""
    ops.DW_WINDOW["callback"] = False
    ops.dw_flush()


def _dw_window_join() -> bool:
    """may this layer use the open window's queue?  The window lives on ONE stream, and the first carrying layer of a
    backward pass queues the end-of-backward flush on the autograd engine (no engine running: no carry)"""
    win = ops.DW_WINDOW
    if win["q"] is None:
        return False
    cur = torch.cuda.current_stream()
    if win["stream"] is None:
        win["stream"] = cur
    elif win["stream"] != cur:
        return False
    if not win["callback"]:
        try:
            torch.autograd.Variable._execution_engine.queue_callback(_dw_window_flush)
        except RuntimeError:
            return False
        win["callback"] = True
    return True


def _fp8_ok(x, W) -> bool:
    """x [M, K] bf16 rows, W [N, K]: fp8 needs K % 128 (MFMA k-slots) and 16-byte aligned pitches"""
    return (x.dim() == 2 and x.dtype == torch.bfloat16 and W.dtype == torch.bfloat16 and x.shape[1] % 128 == 0
            and x.stride(1) == 1 and x.stride(0) % 8 == 0 and W.is_contiguous() and W.shape[0] % 8 == 0)


def _fp8_linear(x, W, bias=None, residual=None, out=None):
    """y = x W^T (+ bias, + residual) with e4m3 operands: per-token scales for x, per-output-channel
    scales for W (cached per optimizer step)"""
    xq, sx = ops.quantize_fp8_rows(x)
    wq, sw = ops.fp8_weight(W)
    return ops.linear_fp8(xq, sx, wq, sw, bias=bias, residual=residual, out=out)


def _fp8_dx_ok(dy, W) -> bool:
    """dy [M, N] bf16 rows, W [N, K]: the reduction runs over N"""
    return (dy.dim() == 2 and dy.dtype == torch.bfloat16 and W.dtype == torch.bfloat16 and dy.shape[1] % 128 == 0
            and dy.stride(1) == 1 and dy.stride(0) % 8 == 0 and W.is_contiguous() and W.shape[1] % 8 == 0)


def _fp8_dx(dy, W, out=None, accumulate=False):
    """dx = dy W with e4m3 operands: per-token scales for dy, W^T K-major with per-input-channel scales"""
    dq, sd = ops.quantize_fp8_rows(dy)
    wt, st = ops.fp8_weight(W, transposed=True)
    return ops.linear_fp8(dq, sd, wt, st, out=out, accumulate=accumulate)


def flash_ok(dtype, hd) -> bool:
    """the fused attention kernels cover the 16-bit dtypes (bf16, fp16) with head_dim 64 / 128"""
    return dtype in (torch.bfloat16, torch.float16) and hd in (64, 128)


def _c2(x: torch.Tensor, rows: int, cols: int) -> torch.Tensor:
    """view as contiguous [rows, cols] (copy through our kernel when needed)"""
    if x.is_contiguous():
        return x.view(rows, cols)
    src = x.reshape(rows, cols) if x.dim() != 2 else x
    if src.stride(1) == 1:
        out = torch.empty((rows, cols), dtype=x.dtype, device=x.device)
        return ops.copy2d(src, out, rows, cols, src.stride(0), cols)
    raise ops.MacawHipError(f"unsupported layout {tuple(x.shape)} {x.stride()}")


# =========================================================================
# LoRA adapters of a decoder layer (macaw_llm_amd/lora.py, csrc/lora.hip)
# =========================================================================
LORA_MODULES = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")
# the four groups of projections that share an input: name, members (indices into LORA_MODULES)
LORA_GROUPS = (("qkv", (0, 1, 2)), ("o", (3,)), ("gu", (4, 5)), ("down", (6,)))


class LoraSpec:
    """what LlamaLayerFn needs to know about one layer's adapters: `mods` = the targeted indices into
    LORA_MODULES (their (A, B) tensors follow as trailing arguments, in this order), the scaling
    s = lora_alpha / r, the dropout probability of this call (0 outside training), the step's seed and the
    layer index (the high bits of the mask's hash index: tag = 8 * layer + module)"""
    __slots__ = ("mods", "s", "p", "seed", "layer")

    def __init__(self, mods, s, p, seed, layer):
        self.mods, self.s, self.p, self.seed, self.layer = tuple(mods), float(s), float(p), int(seed), int(layer)

    def groups(self, ab):
        """[(group name, [(module index, A, B)])] for the groups with at least one adapter"""
        at = {m: (ab[2 * i], ab[2 * i + 1]) for i, m in enumerate(self.mods)}
        out = []
        for name, members in LORA_GROUPS:
            g = [(m, *at[m]) for m in members if m in at]
            if g:
                out.append((name, g))
        return out

    def tags(self, g):
        return [8 * self.layer + m for m, _, _ in g]


def _lora_fwd(spec, g, x, ys):
    """U = drop(x) A^T for the group, then ys_i += s U_i B_i^T; returns Ut (saved for the backward)"""
    U, Ut = ops.lora_down(x, [A for _, A, _ in g], spec.p, spec.seed, spec.tags(g))
    ops.lora_up_add_(U, [B for _, _, B in g], ys, spec.s)
    return Ut


def _lora_bwd(spec, g, x, Ut, dys, dx, grads):
    """dB_i, dA_i of the group into grads[module], dx += the adapters' grad-input"""
    dU, dUt, dB = ops.lora_bwd_dy(dys, [B for _, _, B in g], Ut, spec.s)
    dA = ops.lora_bwd_x_(x, dU, dUt, [A for _, A, _ in g], dx, spec.p, spec.seed, spec.tags(g))
    for (m, _, _), a, b in zip(g, dA, dB):
        grads[m] = (a, b)


# =========================================================================
# LLaMA decoder layer  (modeling.py:234-299)
# =========================================================================
class LlamaLayerFn(torch.autograd.Function):
    """wqkv / wgu (optional, not differentiated) are [3D, D] / [2FF, D] tensors that ALIAS the
    storage of (wq, wk, wv) / (wg, wu) when LlamaDecoderLayer.fuse_projections() has laid the
    parameters out contiguously: the three (two) projections then run as ONE GEMM in forward,
    grad-input and grad-weight (better tile quantisation, 7 fewer launches per layer and pass);
    the weight gradients are returned as row slices of the fused gradient."""

    @staticmethod
    def _fwd(x2, B, S, kmask, pos, cos, sin, n_heads, eps, wq, wk, wv, wo, wg, wu, wd, ln1, ln2, wqkv,
             wgu, grad_mode, lora=None, ab=()):
        """the layer's forward on [M, D] rows; returns (out, intermediates the backward needs).
        Deterministic (fixed reduction orders everywhere), so calling it again in the backward
        of a checkpointed layer reproduces the intermediates bit for bit."""
        M, D = x2.shape
        H, hd = n_heads, D // n_heads
        FF = wg.shape[0]
        lg = dict(lora.groups(ab)) if lora is not None else {}
        lut = {}       # group -> Ut of its adapters (the backward's dB needs it)
        if lg and any(FP8.values()):
            raise NotImplementedError("LoRA adapters cannot be combined with the fp8 switches (MM_LLMs.set_fp8)")
        fp8_qkv = (wqkv is not None and FP8["qkv"] and x2.is_contiguous() and x2.shape[1] <= 16384 and _fp8_ok(x2, wqkv))
        if fp8_qkv:      # (y1's e4m3 image and row scales leave the RMSNorm kernel with it: one pass over the row)
            _, y1, rstd1, y1q, y1s = ops.rmsnorm_fwd_fp8(x2, ln1, eps)
        else:
            _, y1, rstd1 = ops.rmsnorm_fwd(x2, ln1, eps)
        use_flash = flash_ok(x2.dtype, hd)
        # short sequences (ops.rope_fuse_mode): "bwd" -- q, k rotated by mk_rope as ever, only the backward kernel folds
        # the rotation of dq / dk back into its stores; "full" -- q, k stay UNROTATED in HBM, also as the tensors saved
        # for the backward, and every kernel rotates them on the way in
        fuse = ops.rope_fuse_mode() if use_flash and ops.flash_rope_ok(hd, S, S, cos, x2) else "off"
        rope_in = (cos, sin, pos) if fuse == "full" else None
        if wqkv is not None:
            if fp8_qkv:
                wq8, ws8 = ops.fp8_weight(wqkv)
                qkv = ops.linear_fp8(y1q, y1s, wq8, ws8)      # e4m3 x e4m3 -> bf16 (cfg 5)
            else:
                qkv = ops.linear_fwd(y1, wqkv)                # [M, 3D]
            q, k, v = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
            ldq = 3 * D
            if "qkv" in lg:        # (the adapters see q, k before the rotation, as in peft)
                lut["qkv"] = _lora_fwd(lora, lg["qkv"], y1, [(q, k, v)[m] for m, _, _ in lg["qkv"]])
            if rope_in is None:
                ops.rope_(qkv[:, :2 * D], cos, sin, pos, 2 * H, hd)   # q and k heads in one launch
        else:
            q, k, v = ops.linear_fwd(y1, wq), ops.linear_fwd(y1, wk), ops.linear_fwd(y1, wv)
            ldq = D
            if "qkv" in lg:
                lut["qkv"] = _lora_fwd(lora, lg["qkv"], y1, [(q, k, v)[m] for m, _, _ in lg["qkv"]])
            if rope_in is None:
                ops.rope_(q, cos, sin, pos, H, hd)
                ops.rope_(k, cos, sin, pos, H, hd)
        att = torch.empty((M, D), dtype=x2.dtype, device=x2.device)
        if use_flash:
            # fused attention: the S x S scores never reach HBM; training keeps only the
            # per-row log-sum-exp and recomputes P in the fused backward
            lse = torch.empty((B, H, S), dtype=torch.float32, device=x2.device) if grad_mode else None
            ops.flash_attn_fwd(q, k, v, att, B, H, S, S, hd, ldq, S * ldq, ldq, S * ldq, ldq, S * ldq,
                               D, S * D, 1.0 / math.sqrt(hd), kmask=kmask, causal=True, lse=lse, rope=rope_in)
            probs = lse
        else:
            probs, _ = attention_fwd(TDesc(q, ldq, S * ldq), TDesc(k, ldq, S * ldq),
                                     TDesc(v, ldq, S * ldq), TDesc(att, D, S * D), B, H, S, S, hd,
                                     1.0 / math.sqrt(hd), kmask=kmask, causal=True)
        h1 = ops.linear_fwd(att, wo, residual=x2)
        if "o" in lg:
            lut["o"] = _lora_fwd(lora, lg["o"], att, [h1])
        _, y2, rstd2 = ops.rmsnorm_fwd(h1, ln2, eps)
        fp8_mlp = FP8["mlp"] and wgu is not None and _fp8_ok(y2, wgu) and _fp8_dx_ok(y2, wd)
        if wgu is not None:
            gu = _fp8_linear(y2, wgu) if fp8_mlp else ops.linear_fwd(y2, wgu)     # [M, 2FF] = [gate | up]
            if "gu" in lg:
                lut["gu"] = _lora_fwd(lora, lg["gu"], y2, [(gu[:, :FF], gu[:, FF:])[m - 4] for m, _, _ in lg["gu"]])
            a = ops.swiglu2d_fwd(gu, FF)
            g = u = None
        else:
            g, u = ops.linear_fwd(y2, wg), ops.linear_fwd(y2, wu)
            if "gu" in lg:
                lut["gu"] = _lora_fwd(lora, lg["gu"], y2, [(g, u)[m - 4] for m, _, _ in lg["gu"]])
            a = ops.swiglu_fwd(g, u)
            gu = None
        if wgu is not None and fp8_mlp and _fp8_ok(a, wd):
            out = _fp8_linear(a, wd, residual=h1)
        else:
            out = ops.linear_fwd(a, wd, residual=h1)
        if "down" in lg:
            lut["down"] = _lora_fwd(lora, lg["down"], a, [out])
        if lora is not None:
            return out, (rstd1, y1, q, k, v, probs, att, h1, rstd2, y2, g, u, gu, a,
                         *(lut.get(n) for n, _ in LORA_GROUPS)), ({"full": 2, "bwd": 3, "off": 1}[fuse] if use_flash else 0)
        # (the third value tells the backward what its fused kernel has to do: 1 = nothing, 2 = q, k unrotated, RoPE
        # inside the kernels; 3 = q, k rotated, dq / dk rotated back at the store)
        return out, (rstd1, y1, q, k, v, probs, att, h1, rstd2, y2, g, u, gu, a), \
            ({"full": 2, "bwd": 3, "off": 1}[fuse] if use_flash else 0)

    @staticmethod
    def forward(ctx, x, kmask, pos, cos, sin, n_heads, eps, wq, wk, wv, wo, wg, wu, wd, ln1, ln2,
                wqkv=None, wgu=None, recompute=False, lora=None, *ab):
        """recompute=True is activation checkpointing (modeling.py:474-489): only the layer
        input is kept and the backward re-runs `_fwd` first (identical results, ~13 fewer saved
        [M, *] tensors per layer).  lora (LoraSpec) with ab = (A, B) of every targeted projection:
        LoRA adapters (y += s drop(x) A^T B^T), whose gradients the backward returns."""
        B, S, D = x.shape
        M, H, hd = B * S, n_heads, D // n_heads
        x2 = _c2(x, M, D)
        grad_mode = any(ctx.needs_input_grad)
        out, inter, use_flash = LlamaLayerFn._fwd(x2, B, S, kmask, pos, cos, sin, n_heads, eps, wq, wk,
                                                  wv, wo, wg, wu, wd, ln1, ln2, wqkv, wgu,
                                                  grad_mode and not recompute, lora, ab)
        if grad_mode:
            ctx.recompute = bool(recompute)
            ctx.n_heads, ctx.eps = n_heads, eps
            ctx.lora = lora
            if recompute:
                inter = (None,) * len(inter)
            ctx.save_for_backward(x2, *inter, pos, cos, sin, wq, wk, wv, wo, wg, wu, wd, ln1, ln2,
                                  kmask, wqkv, wgu, *ab)
            ctx.dims = (B, S, D, H, hd, use_flash, wg.shape[0])
        return out.view(B, S, D)

    @staticmethod
    def backward(ctx, dout):
        lora = ctx.lora
        if lora is not None:
            return LlamaLayerFn._backward_lora(ctx, dout)
        (x2, rstd1, y1, q, k, v, probs, att, h1, rstd2, y2, g, u, gu, a, pos, cos, sin, wq, wk, wv,
         wo, wg, wu, wd, ln1, ln2, kmask, wqkv, wgu) = ctx.saved_tensors
        B, S, D, H, hd, use_flash, FF = ctx.dims
        M = B * S
        if ctx.recompute:
            _, (rstd1, y1, q, k, v, probs, att, h1, rstd2, y2, g, u, gu, a), use_flash = LlamaLayerFn._fwd(
                x2, B, S, kmask, pos, cos, sin, ctx.n_heads, ctx.eps, wq, wk, wv, wo, wg, wu, wd, ln1,
                ln2, wqkv, wgu, True)
        return LlamaLayerFn._backward_body(ctx, dout, x2, rstd1, y1, q, k, v, probs, att, h1, rstd2, y2, g, u, gu, a,
                                           pos, cos, sin, wq, wk, wv, wo, wg, wu, wd, ln1, ln2, kmask, wqkv, wgu,
                                           B, S, D, H, hd, use_flash, FF, M)

    @staticmethod
    def _backward_lora(ctx, dout):
        n_ab = 2 * len(ctx.lora.mods)
        saved = ctx.saved_tensors
        ab = saved[len(saved) - n_ab:]
        (x2, rstd1, y1, q, k, v, probs, att, h1, rstd2, y2, g, u, gu, a, ut_qkv, ut_o, ut_gu, ut_down, pos, cos, sin,
         wq, wk, wv, wo, wg, wu, wd, ln1, ln2, kmask, wqkv, wgu) = saved[:len(saved) - n_ab]
        B, S, D, H, hd, use_flash, FF = ctx.dims
        M = B * S
        if ctx.recompute:       # (same seed, same masks: U and the dropout are reproduced bit for bit)
            _, (rstd1, y1, q, k, v, probs, att, h1, rstd2, y2, g, u, gu, a, ut_qkv, ut_o, ut_gu, ut_down), use_flash = \
                LlamaLayerFn._fwd(x2, B, S, kmask, pos, cos, sin, ctx.n_heads, ctx.eps, wq, wk, wv, wo, wg, wu, wd, ln1,
                                  ln2, wqkv, wgu, True, ctx.lora, ab)
        lut = {"qkv": ut_qkv, "o": ut_o, "gu": ut_gu, "down": ut_down}
        grads = {}
        res = LlamaLayerFn._backward_body(ctx, dout, x2, rstd1, y1, q, k, v, probs, att, h1, rstd2, y2, g, u, gu, a,
                                          pos, cos, sin, wq, wk, wv, wo, wg, wu, wd, ln1, ln2, kmask, wqkv, wgu,
                                          B, S, D, H, hd, use_flash, FF, M, (ctx.lora, ab, lut, grads))
        need = ctx.needs_input_grad
        extra = []
        for i, m in enumerate(ctx.lora.mods):
            dA, dB = grads[m]
            extra += [dA if need[20 + 2 * i] else None, dB if need[21 + 2 * i] else None]
        return (*res, None, *extra)

    @staticmethod
    def _backward_body(ctx, dout, x2, rstd1, y1, q, k, v, probs, att, h1, rstd2, y2, g, u, gu, a, pos, cos, sin, wq, wk,
                       wv, wo, wg, wu, wd, ln1, ln2, kmask, wqkv, wgu, B, S, D, H, hd, use_flash, FF, M, lo=None):
        if lo is not None:
            lora, ab, lut, grads = lo
            lg = dict(lora.groups(ab))
        else:
            lg = {}
        need = ctx.needs_input_grad
        dout2 = _c2(dout, M, D)
        # ---- MLP
        fp8_mlp = FP8["mlp"] and gu is not None and _fp8_dx_ok(dout2, wd) and _fp8_ok(y2, wgu)
        # the projections' backward: grad-weight tiles inside the grad-input launches (DW_FILL), else launch by launch
        # with the grad-weight GEMMs on a second stream where that pays (DW_SIDE)
        if _dw_fill_ok(M, D, FF, x2, need, lo, gu, wqkv, wgu, fp8_mlp or FP8["qkv"]):
            sd = _DwFill()
        else:
            sd = _DwSide(x2.device, M, D)
        da, dwd = sd.pair(dout2, wd, a, "down", need[13], fp8=fp8_mlp)
        if "down" in lg:
            _lora_bwd(lora, lg["down"], a, lut["down"], [dout2], da, grads)
        dwg = dwu = None
        if gu is not None:
            dgu = ops.swiglu2d_bwd(gu, da, FF)
            del da
            dy2, dwgu = sd.pair(dgu, wgu, y2, "gu", need[11] or need[12], fp8=fp8_mlp and _fp8_dx_ok(dgu, wgu))   # [2FF, D]
            if "gu" in lg:
                _lora_bwd(lora, lg["gu"], y2, lut["gu"], [(dgu[:, :FF], dgu[:, FF:])[m - 4] for m, _, _ in lg["gu"]],
                          dy2, grads)
            if dwgu is not None:
                dwg, dwu = dwgu[:FF], dwgu[FF:]
            del dgu
        else:
            dg, du = ops.swiglu_bwd(g, u, da)
            del da
            dy2 = ops.linear_dx(dg, wg)
            ops.linear_dx(du, wu, out=dy2, accumulate=True)
            if "gu" in lg:
                _lora_bwd(lora, lg["gu"], y2, lut["gu"], [(dg, du)[m - 4] for m, _, _ in lg["gu"]], dy2, grads)
            dwg = ops.linear_dw(dg, y2) if need[11] else None
            dwu = ops.linear_dw(du, y2) if need[12] else None
            del dg, du
        dh1, dln2 = ops.rmsnorm_bwd(dy2, h1, ln2, rstd2, dres=dout2, dw_out=ops.grad_dst(ln2) if need[15] else None)
        # ---- attention
        datt, dwo = sd.pair(dh1, wo, att, "o", need[10])
        if "o" in lg:
            _lora_bwd(lora, lg["o"], att, lut["o"], [dh1], datt, grads)
        ldq = q.stride(0)
        if wqkv is not None:
            dqkv = torch.empty((M, 3 * D), dtype=q.dtype, device=q.device)
            dq, dk, dv = dqkv[:, :D], dqkv[:, D:2 * D], dqkv[:, 2 * D:]
        else:
            dqkv = None
            dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        rope_in = (cos, sin, pos) if use_flash >= 2 else None
        if use_flash:
            ops.flash_attn_bwd(q, k, v, att, datt, probs, dq, dk, dv, B, H, S, S, hd, ldq, S * ldq,
                               ldq, S * ldq, ldq, S * ldq, D, S * D, 1.0 / math.sqrt(hd),
                               kmask=kmask, causal=True, rope=rope_in, qk_rotated=use_flash == 3)
        else:
            d = lambda t: TDesc(t, ldq, S * ldq)  # noqa: E731
            attention_bwd(TDesc(datt, D, S * D), d(q), d(k), d(v), probs, None, d(dq), d(dk), d(dv),
                          B, H, S, S, hd, 1.0 / math.sqrt(hd))
        if rope_in is not None:
            pass                                               # dq, dk already are gradients of the unrotated q, k
        elif dqkv is not None:
            ops.rope_(dqkv[:, :2 * D], cos, sin, pos, 2 * H, hd, inverse=True)
        else:
            ops.rope_(dq, cos, sin, pos, H, hd, inverse=True)
            ops.rope_(dk, cos, sin, pos, H, hd, inverse=True)
        dwq = dwk = dwv = None
        lora_qkv = lg.get("qkv")
        if wqkv is not None:
            # (fp8: e4m3 dy x e4m3 W^T, cfg 5)    the layer's last projection: a fill queue is drained here
            dy1, dwqkv = sd.pair(dqkv, wqkv, y1, "qkv", need[7] or need[8] or need[9],
                                 fp8=FP8["qkv"] and _fp8_dx_ok(dqkv, wqkv) and _fp8_ok(y1, wqkv), drain=True)   # [3D, D]
            if lora_qkv:
                _lora_bwd(lora, lora_qkv, y1, lut["qkv"], [(dq, dk, dv)[m] for m, _, _ in lora_qkv], dy1, grads)
            if dwqkv is not None:
                dwq, dwk, dwv = dwqkv[:D], dwqkv[D:2 * D], dwqkv[2 * D:]
        else:
            dy1 = ops.linear_dx(dq, wq)
            ops.linear_dx(dk, wk, out=dy1, accumulate=True)
            ops.linear_dx(dv, wv, out=dy1, accumulate=True)
            if lora_qkv:
                _lora_bwd(lora, lora_qkv, y1, lut["qkv"], [(dq, dk, dv)[m] for m, _, _ in lora_qkv], dy1, grads)
            dwq = ops.linear_dw(dq, y1) if need[7] else None
            dwk = ops.linear_dw(dk, y1) if need[8] else None
            dwv = ops.linear_dw(dv, y1) if need[9] else None
        dx, dln1 = ops.rmsnorm_bwd(dy1, x2, ln1, rstd1, dres=dh1, dw_out=ops.grad_dst(ln1) if need[14] else None)
        sd.join()
        return (dx.view(B, S, D), None, None, None, None, None, None, dwq, dwk, dwv, dwo, dwg, dwu,
                dwd, dln1 if need[14] else None, dln2 if need[15] else None, None, None, None)


class LayerWeights(NamedTuple):
    """the projection weights of one decoder layer, in llama_layer_cached's order (its two norm weights go between wd
    and wqkv): the seven [out, in] matrices, and the fused q|k|v [3D, D] / gate|up [2 FF, D] buffers that wq, wk, wv /
    wg, wu are row slices of where the storage is fused (else None)"""
    wq: torch.Tensor
    wk: torch.Tensor
    wv: torch.Tensor
    wo: torch.Tensor
    wg: torch.Tensor
    wu: torch.Tensor
    wd: torch.Tensor
    wqkv: Optional[torch.Tensor]
    wgu: Optional[torch.Tensor]


class Ragged(NamedTuple):
    """a padded batch for llama_layer_cached (ragged_from_mask): the prompt's key mask, where each prompt row goes in
    the COMPACTED cache, and where each sample's decode steps run relative to the common step counter"""
    kmask: torch.Tensor      # int32 [B, S0], non-zero = valid: the prefill attention's key mask
    slot: torch.Tensor       # int32 [B, S0]: cache row of prompt row (b, j) = its position; -1 for a masked row
    t_off: torch.Tensor      # int32 [B]: n_b - S0; the step of sample b runs at position / cache row *t_dev + t_off[b]


class Beam(NamedTuple):
    """a beam step for llama_layer_cached (generate(num_beams=K)): the rows are (sample, beam) pairs and the cache is
    [B, K, Tmax, 2D], read through the indirection table that ops.beam_emit keeps"""
    ind: torch.Tensor        # int32 [B * K, n]: the slot of sample b that holds the key of position S0 + i for row (b, k)
    K: int                   # beams per sample
    S0: int                  # prompt length: keys below it are read from slot 0 of the sample


class Spec(NamedTuple):
    """a prompt-lookup verify step for llama_layer_cached (generate(prompt_lookup_num_tokens=G)): Q = G + 1 token rows per
    sample, row (b, g) at position pos[b] + g, the positions kept per sample on the device by ops.spec_verify_emit"""
    pos: torch.Tensor        # int32 [B]: position and cache row of each sample's row 0
    Q: int                   # rows per sample


class SharedPrompt(NamedTuple):
    """a parallel-sampling step for llama_layer_cached (generate(num_samples=n)), passed IN PLACE of the cache tensor kvc:
    the prompt's keys once per prompt and the rows' own tokens per row.  Row b * n + j is sample j of prompt b"""
    prompt: torch.Tensor     # [B, S0, 2D]: the cache the prefill wrote at B rows (Tmax = S0); a padded batch's compacted rows
    tail: torch.Tensor       # [B * n, Tn, 2D]: tail row i holds the row's token of step i
    n: int                   # samples per prompt
    S0: int                  # prompt rows per sample of `prompt`


class AdapterGroup(NamedTuple):
    """the stacks of one LORA_GROUPS entry of one layer in a lora.AdapterBank, one slab per adapter: the group's G
    modules row-concatenated, ranks below r (the bank's largest) and untargeted modules zero-filled"""
    A: torch.Tensor          # [n, G r, K]
    B: torch.Tensor          # [n, G N, r]
    s: torch.Tensor          # f32 [n]: lora_alpha / r of each adapter
    G: int


class Adapters(NamedTuple):
    """mixed-adapter LoRA for llama_layer_cached (generate(adapter_names=)), passed IN PLACE of w8, whose copies it carries,
    so that the signature every other caller binds to stays what it is.  A decode step reads idx on the device (the
    mk_lora_bgmv kernels around each streamed linear: _stream_linear); the prefill walks `runs` on the host"""
    idx: torch.Tensor        # int32 [rows of a step]: the adapter of each row, -1 = the base model
    runs: tuple              # ((b0, b1, a), ...): the maximal runs of consecutive samples [b0, b1) with the same adapter a >= 0
    s_host: tuple            # lora_alpha / r per adapter, once more on the host for the prefill's launches
    qkv: Optional[AdapterGroup]      # this layer's stacks, in LORA_GROUPS order (None: no adapter targets the group here)
    o: Optional[AdapterGroup]
    gu: Optional[AdapterGroup]
    down: Optional[AdapterGroup]
    w8: Optional[tuple] = None       # what w8 would have carried


class Adapted(NamedTuple):
    """_stream_linear's q8 argument for a group that carries adapters: the rows' adapters, the group's stacks and the
    quantised copy (or None) that q8 would have been"""
    idx: torch.Tensor
    group: AdapterGroup
    q8: Optional[tuple]


def _adapted(ad, group, q8):
    return Adapted(ad.idx, group, q8) if ad is not None and group is not None else q8


def _lora_runs(ad, name, x, ys, Sn):
    """the prefill's adapters of the group `name` (ad: an Adapters or None): per run of samples with one adapter,
    ys_i[rows] += s U_i B_i^T on the run's contiguous row slice with the MFMA kernels of csrc/lora.hip (p = 0); base
    runs are skipped"""
    group = getattr(ad, name) if ad is not None else None
    if group is None:
        return
    G = group.G
    r, N = group.A.shape[1] // G, group.B.shape[1] // G
    for b0, b1, a in ad.runs:
        r0, r1 = b0 * Sn, b1 * Sn
        U, _ = ops.lora_down(x[r0:r1], [group.A[a, i * r:(i + 1) * r] for i in range(G)])
        ops.lora_up_add_(U, [group.B[a, i * N:(i + 1) * N] for i in range(G)], [y[r0:r1] for y in ys], ad.s_host[a])


def ragged_from_mask(mask, B, S0):
    """The host side of generate(attention_mask=): mask [B, S0], any integer or bool dtype, non-zero = valid.
    Returns None for a mask without a zero (the unpadded path), else (Ragged, pos, last):
      pos  int32 [B * S0]  RoPE positions, max(cumsum(mask) - 1, 0) (the reference's prepare_inputs_for_generation rule)
      last int64 [B]       flat row b * S0 + (last valid index of sample b): the hidden row that predicts token 0
    ValueError for a shape other than (B, S0) and for a sample without a valid token."""
    if mask.dim() != 2 or tuple(mask.shape) != (B, S0):
        raise ValueError(f"attention_mask should be of size {(B, S0)}, but is {tuple(mask.shape)}")
    valid = mask != 0
    if bool(valid.all()):
        return None
    n = valid.sum(1)
    if bool((n == 0).any()):
        raise ValueError(f"attention_mask: sample(s) {torch.nonzero(n == 0).flatten().tolist()} have no valid token")
    cs = valid.long().cumsum(1)
    pos = (cs - 1).clamp_(min=0)
    slot = torch.where(valid, pos, torch.full_like(pos, -1))
    idx = torch.arange(S0, device=mask.device).expand(B, S0)
    last = torch.where(valid, idx, torch.full_like(idx, -1)).max(1).values
    last = last + torch.arange(B, device=mask.device) * S0
    rg = Ragged(valid.to(torch.int32).contiguous(), slot.to(torch.int32).contiguous(),
                (n - S0).to(torch.int32).contiguous())
    return rg, pos.to(torch.int32).reshape(-1).contiguous(), last.contiguous()


class Chunk(NamedTuple):
    """the prefill of a CONTINUED call for llama_layer_cached (chunk_layout): q_len[b] new rows of sample b, left-compacted
    in its Sc rows, behind the k_len[b] - q_len[b] rows its compacted cache already holds"""
    q_len: torch.Tensor      # int32 [B]: n_b, the new rows of sample b (its pending token, then its valid new tokens)
    k_len: torch.Tensor      # int32 [B]: C_b + n_b, the rows of sample b's cache once the new ones are appended
    slot: torch.Tensor       # int32 [B, Sc]: cache row of new row (b, j) = C_b + j; -1 for a filler row (j >= n_b)
    Lk: int                  # max k_len: the host bound of the key loop
    q_host: tuple            # q_len and k_len once more on the host, for the per-sample attention where the
    k_host: tuple            # variable-length kernel does not take the head size


def chunk_layout(cached, n_valid, device=None):
    """The host side of generate(session=): cached[b] = C_b rows in sample b's compacted cache, n_valid[b] = v_b >= 1 valid
    tokens in its new prompt (sequences of int).  The new rows of a sample are LEFT-COMPACTED: row 0 is the session's
    pending token (emitted by the last turn, never fed), rows 1 ... v_b its valid new tokens in order, n_b = 1 + v_b,
    Sc = max n_b; the rows behind n_b are filler that repeats the sample's last row and is never appended or attended.
    Returns (Chunk, pos, last, S0n, t_off), tensors on `device` (None: the CPU):
      pos   int32 [B * Sc]  RoPE position of row (b, j): C_b + min(j, n_b - 1)
      last  int64 [B]       flat row b * Sc + n_b - 1: the hidden row that predicts token 0
      S0n   int             max_b k_len[b]: where the decode steps' common counter starts
      t_off int32 [B]       k_len[b] - S0n: Ragged.t_off, the step of sample b runs at row *t_dev + t_off[b]
    ValueError for lists of different lengths, a negative C_b and a sample without a valid token."""
    cached, n_valid = [int(c) for c in cached], [int(v) for v in n_valid]
    if len(cached) != len(n_valid) or not cached:
        raise ValueError(f"chunk_layout: {len(cached)} cached counts for {len(n_valid)} samples")
    if min(cached) < 0:
        raise ValueError(f"chunk_layout: negative cached row count in {cached}")
    if min(n_valid) < 1:
        raise ValueError(f"sample(s) {[b for b, v in enumerate(n_valid) if v < 1]} have no valid token")
    B = len(cached)
    n = torch.tensor(n_valid, dtype=torch.int64) + 1
    C = torch.tensor(cached, dtype=torch.int64)
    Sc = int(n.max())
    j = torch.arange(Sc, dtype=torch.int64).expand(B, Sc)
    pos = C[:, None] + torch.minimum(j, n[:, None] - 1)
    slot = torch.where(j < n[:, None], C[:, None] + j, torch.full_like(j, -1))
    k_len = C + n
    S0n = int(k_len.max())
    i32 = lambda t: t.to(torch.int32).contiguous().to(device) if device is not None else t.to(torch.int32).contiguous()  # noqa: E731
    last = torch.arange(B, dtype=torch.int64) * Sc + n - 1
    chunk = Chunk(i32(n), i32(k_len), i32(slot), S0n, tuple(n.tolist()), tuple(k_len.tolist()))
    return chunk, i32(pos.reshape(-1)), (last.to(device) if device is not None else last), S0n, i32(k_len - S0n)


def _step_attn(q, k, v, in_bs, cos, sin, kvc, kv8, t_dev, Tmax, B, H, hd, att, scale, ragged=None, beam=None, spec=None,
               **off):
    """the attention block of a decode step: ops.decode_step_attn on the 16-bit cache, or (kv8 = the scales of an
    e4m3 cache, kvc its bytes) ops.decode_step_attn_kv8; with ragged (a padded batch) their per-sample-position forms;
    with beam (a Beam; B samples of beam.K rows each) ops.decode_step_attn_beam over the [B, K, Tmax, 2D] cache; with
    spec (a Spec; B samples of spec.Q rows each) ops.decode_step_attn_multi at the per-sample positions spec.pos; with kvc
    a SharedPrompt (B prompts of kvc.n rows each) ops.decode_step_attn_shared over its two buffers, ragged.t_off passed
    through for a padded batch"""
    if isinstance(kvc, SharedPrompt):
        return ops.decode_step_attn_shared(q, k, v, in_bs, cos, sin, kvc.prompt, kvc.tail, t_dev,
                                           ragged.t_off if ragged is not None else None, kvc.S0, B, kvc.n, H, hd, att, scale,
                                           **off)
    if spec is not None:
        return ops.decode_step_attn_multi(q, k, v, in_bs, cos, sin, kvc, spec.pos, Tmax, B, spec.Q, H, hd, att, scale, **off)
    if beam is not None:
        return ops.decode_step_attn_beam(q, k, v, in_bs, cos, sin, kvc, t_dev, beam.ind, beam.S0, Tmax, B, beam.K, H, hd,
                                         att, scale, **off)
    if ragged is not None:
        if kv8 is not None:
            return ops.decode_step_attn_kv8_var(q, k, v, in_bs, cos, sin, kvc, kv8, t_dev, ragged.t_off, Tmax, B, H, hd,
                                                att, scale, **off)
        return ops.decode_step_attn_var(q, k, v, in_bs, cos, sin, kvc, t_dev, ragged.t_off, Tmax, B, H, hd, att, scale,
                                        **off)
    if kv8 is not None:
        return ops.decode_step_attn_kv8(q, k, v, in_bs, cos, sin, kvc, kv8, t_dev, Tmax, B, H, hd, att, scale, **off)
    return ops.decode_step_attn(q, k, v, in_bs, cos, sin, kvc, t_dev, Tmax, B, H, hd, att, scale, **off)


def _stream_linear(x, W, q8, pro, w_ln, eps, residual, FF):
    """y = pro(x) W^T (+ residual) for the few token rows of a decode step, the weight streamed once: W 16-bit, or
    q8 = its e4m3 copy (q uint8 [N, K], scales f32 [N]) where that is not None.  The prologue pro (1 = RMSNorm(x;
    w_ln, eps), 2 = SwiGLU of x = [gate | up] [M, 2 FF], 0 = none) is folded into the weight stream where the
    prepared token rows fit the kernel's LDS budget (ops.decode_linear_ok: not for M > 4 at K = 4096); otherwise the
    separate RMSNorm / SwiGLU kernel runs first and the PLAIN launch follows, so every batch size up to 32 streams
    the bytes it was given.  A 16-bit weight outside ops.decode_linear's domain goes through ops.linear_fwd.
    A copy whose second member is uint8 is an MXFP4 copy (codes uint8 [N, K / 2], block exponents uint8 [N, K / 32]:
    ops.mxfp4_weight) and streams through ops.decode_linear_mxfp4 under the same rule.
    q8 an Adapted (the rows' adapters and the group's stacks around the copy, or None, that q8 would have been): the
    16-bit adapters go on top of whichever base launch runs.  ops.lora_bgmv_shrink takes the (x, prologue) the base
    launch takes, or the prepared x of the fallback branch -- the same bits either way --, the base launch is unchanged,
    and ops.lora_bgmv_expand_ adds into its output (behind the residual, where LlamaLayerFn adds the adapter)."""
    ad = None
    if isinstance(q8, Adapted):
        ad, q8 = q8, q8.q8

    def around(base, xs, p):    # shrink, the base launch, expand
        if ad is None:
            return base()
        U = ops.lora_bgmv_shrink(xs, ad.group.A, ad.idx, ad.group.G, p, w_ln if p == 1 else None, eps)
        return ops.lora_bgmv_expand_(U, ad.group.B, ad.group.s, ad.idx, base(), ad.group.G)

    if q8 is not None:      # the kind of a copy, per entry: uint8 block exponents = MXFP4, f32 channel scales = e4m3
        mx = q8[1].dtype == torch.uint8
        lin, ok = (ops.decode_linear_mxfp4, ops.decode_linear_mxfp4_ok) if mx else (ops.decode_linear_fp8, ops.decode_linear_fp8_ok)
        if ok(x, q8[0], pro):
            return around(lambda: lin(x, q8[0], q8[1], pro, w_ln, eps, residual), x, pro)
    elif ops.decode_linear_ok(x, W, pro):
        return around(lambda: ops.decode_linear(x, W, pro, w_ln, eps, residual), x, pro)
    if pro == 1:
        x = ops.rmsnorm_fwd(x, w_ln, eps)[1]
    elif pro == 2:
        x = ops.swiglu2d_fwd(x, FF)
    if q8 is not None:
        return around(lambda: lin(x, q8[0], q8[1], residual=residual), x, 0)
    return around(lambda: ops.linear_fwd(x, W, residual=residual), x, 0)


def llama_layer_cached(x2, B, Sn, t0, kvc, Tmax, pos, cos, sin, n_heads, eps, wq, wk, wv, wo, wg, wu,
                       wd, ln1, ln2, wqkv=None, wgu=None, t_dev=None, w8=None, kv8=None, ragged=None, beam=None,
                       spec=None):
    """No-grad decoder layer over `Sn` NEW positions per sample (rows of x2 are (b, s)) that
    start at position t0, with a preallocated KV cache kvc [B, Tmax, 2D] = [keys | values] per
    position (post-RoPE keys, modeling.py:183-195 semantics without the torch.cat per step).
    Sn = prompt length for the prefill (t0 = 0, causal), Sn = 1 for a decode step (attends to
    the t0 + 1 cached keys).  No attention mask (the reference's generate passes none,
    modeling.py:959 / SURVEY Q7).  With fused q|k|v storage a step is one GEMM, ONE RoPE launch
    over the q and k heads and ONE strided copy of [k | v] into the cache.

    t_dev (int32[1] on the device, Sn = 1 only): the position is read from device memory by the
    cache append and the attention kernel (`pos` already is a device tensor) and t0 is ignored, so
    the launch sequence does not depend on the step and can be replayed from a hipGraph.

    w8 (with t_dev and fused storage only): the e4m3 copies (q uint8 [N, K], scales f32 [N]: ops.fp8_weight) of
    the four streamed weights, in the order fused q|k|v, o, fused gate|up, down.  The same five launches then
    stream e4m3 bytes (ops.decode_linear_fp8: W8A16, tokens / KV cache / accumulation unchanged).  An entry
    may be None for a projection outside the plain fp8 domain: that one keeps its 16-bit launch.  Each entry may
    instead be an MXFP4 copy (codes uint8 [N, K / 2], exponents uint8 [N, K / 32]: ops.mxfp4_weight), streamed by
    ops.decode_linear_mxfp4 (W4A16); the kind is decided per entry (_stream_linear).

    kv8 (the f32 [B, Tmax, 2H] scales of an e4m3 KV cache; kvc then is its uint8 [B, Tmax, 2D] bytes:
    ops.kv8_cache): every decode step (t_dev) runs ops.decode_step_attn_kv8 in place of ops.decode_step_attn, with
    or without w8.  The prefill (t0 = 0) attends over the fresh 16-bit q, k, v of the prompt -- the data a 16-bit
    cache would have held -- and then writes the cache through ops.kv_quant_append; there is no quantised
    attention over several new positions, so t0 > 0 without t_dev raises ValueError.

    ragged (a Ragged: ragged_from_mask): a padded batch.  The prefill (t0 = 0, `pos` the caller's cumsum positions)
    attends causally over the prompt's own fresh k, v with ragged.kmask and writes the cache COMPACTED through
    ops.kv_append_rows / ops.kv_quant_append_rows: the valid token at position i of a sample goes to cache row i,
    masked rows are not written.  Every decode step (t_dev) runs the per-sample-position step attention at
    *t_dev + ragged.t_off[b] and never reads past that row, so the cache's unwritten tail may stay uninitialised.
    There is no masked attention over a cache: anything else (t0 > 0 without t_dev) raises ValueError.

    beam (a Beam; decode steps with t_dev only): a beam-search step.  B stays the number of SAMPLES, x2 holds the
    B * beam.K (sample, beam) rows and kvc is [B, K, Tmax, 2D]; the step attention reads it through beam.ind
    (ops.decode_step_attn_beam), every other launch sees B * K token rows and is unchanged.  The prefill of such a
    cache is a plain call at B rows on kvc.view(B, K * Tmax, 2D) with Tmax = K * Tmax: it writes slot 0 of every
    sample.  Not with kv8 or ragged.

    spec (a Spec; decode steps with t_dev only, Sn = spec.Q): a prompt-lookup verify step.  x2 holds the B * spec.Q rows
    (b, g), row g of sample b at position spec.pos[b] + g; the step attention is ops.decode_step_attn_multi, which
    appends the Q new rows of a sample and lets row g attend over the cache up to its own position; every other launch
    sees B * Q token rows and is unchanged.  Not with kv8, ragged or beam, and not with a host position.

    kvc a SharedPrompt (decode steps with t_dev only): a parallel-sampling step.  B stays the number of PROMPTS and x2
    holds the B * kvc.n rows; the step attention is ops.decode_step_attn_shared over kvc.prompt (stored once per prompt)
    and kvc.tail (per row), every other launch sees B * n token rows and is unchanged.  Tmax is not read.  The prefill
    of such a cache is an ordinary call at B rows on kvc.prompt with Tmax = S0 (with ragged: the compacting write, and
    the steps then pass ragged.t_off on).  Not with kv8, beam or spec, and not with a host position.

    ragged a Chunk (chunk_layout; passed IN PLACE of a Ragged, as a SharedPrompt is of the cache, so that the signature
    every other caller binds to stays what it is; Sn = its Sc, t0 is ignored, `pos` its positions): the prefill of a
    continued call,
    chunk.q_len[b] new positions of sample b over the chunk.k_len[b] - chunk.q_len[b] rows its compacted cache holds.
    The new keys / values go into the cache first (ops.kv_append_rows at chunk.slot), then ops.flash_attn_varlen_fwd
    attends over the cache's two halves with the lengths read on the device; where that kernel does not take the head
    size (ops.flash_varlen_ok), the samples run one by one through attention_fwd at their host lengths.  Filler rows
    come out as zeros.  The decode steps that follow are the ragged batch's (Ragged.t_off = chunk_layout's t_off).  Not
    with kv8, beam, spec, a SharedPrompt or t_dev.

    w8 an Adapters (passed IN PLACE of the copies, which it carries in its own w8 field): mixed-adapter LoRA, row m of a
    step using adapter ad.idx[m] of the layer's stacks (-1: the base model).  A step must be the five-launch one (t_dev,
    fused storage, 16-bit, at most 32 rows: ValueError otherwise) and wraps each streamed linear in the mk_lora_bgmv pair
    (_stream_linear); the prefill adds the adapters per run of samples with the MFMA kernels (_lora_runs) at the four
    points where LlamaLayerFn adds them, fused storage or not.  Not with beam, spec, a SharedPrompt or a Chunk."""
    M, D = x2.shape
    dyn = t_dev is not None
    ad = None
    if isinstance(w8, Adapters):
        ad, w8 = w8, w8.w8
        if beam is not None or spec is not None or isinstance(kvc, SharedPrompt) or isinstance(ragged, Chunk):
            raise ValueError("llama_layer_cached: Adapters map rows to samples one to one: not with beam, spec, a "
                             "SharedPrompt or a Chunk")
    chunk = None
    if isinstance(ragged, Chunk):
        chunk, ragged = ragged, None
        if (kv8 is not None or beam is not None or spec is not None or dyn or
                isinstance(kvc, SharedPrompt) or M != B * Sn or tuple(chunk.slot.shape) != (B, Sn)):
            raise ValueError("llama_layer_cached: a Chunk takes the B * Sc new rows of a continued prefill on the 16-bit "
                             "compacted cache, not kv8, beam, spec, a SharedPrompt or t_dev")
        t0 = 0
    if isinstance(kvc, SharedPrompt) and (not dyn or kv8 is not None or beam is not None or spec is not None or
                                          M != B * kvc.n):
        raise ValueError("llama_layer_cached: a SharedPrompt cache takes single-position decode steps (t_dev) of B * n rows "
                         "on the 16-bit cache, not kv8, beam, spec or a host position")
    if spec is not None:
        if not dyn or kv8 is not None or ragged is not None or beam is not None or Sn != spec.Q or M != B * spec.Q:
            raise ValueError("llama_layer_cached: spec takes decode steps at device positions (t_dev) of B * Q rows "
                             "(Sn = Q) on the 16-bit unpadded cache, not kv8, ragged, beam or a host position")
        Sn = 1                  # per row it is a single-position step
    if beam is not None and (not dyn or kv8 is not None or ragged is not None or M != B * beam.K):
        raise ValueError("llama_layer_cached: beam takes single-position decode steps (t_dev) of B * K rows on the 16-bit "
                         "unpadded cache, not kv8 or ragged")
    if ragged is not None and not dyn and t0 != 0:
        raise ValueError("llama_layer_cached: ragged takes a prefill from position 0 (t0 = 0) or single-position "
                         f"decode steps (t_dev), not {Sn} new positions at t0 = {t0}")
    if kv8 is not None and not dyn and t0 != 0:
        raise ValueError("llama_layer_cached: kv8 takes a prefill from position 0 (t0 = 0) or single-position decode "
                         f"steps (t_dev), not {Sn} new positions at t0 = {t0}")
    if dyn and Sn != 1:
        raise ValueError("llama_layer_cached: t_dev is for single-position decode steps")
    step = dyn and wqkv is not None and wgu is not None and ops.decode_linear_ok(x2, wqkv)
    if w8 is not None and not step:
        raise ValueError("llama_layer_cached: w8 is for the five-launch decode step (t_dev, fused q|k|v and "
                         "gate|up storage, at most 32 rows)")
    if ad is not None and dyn and not (step and ad.idx.numel() == M):
        raise ValueError("llama_layer_cached: a decode step with Adapters is the five-launch one (t_dev, fused q|k|v and "
                         "gate|up storage, bf16 / fp16, at most 32 rows, one adapter index per row)")
    H, hd = n_heads, D // n_heads
    FF = wg.shape[0]
    att = torch.empty((M, D), dtype=x2.dtype, device=x2.device)
    scale = 1.0 / math.sqrt(hd)
    if step:
        # five launches: RMSNorm folded into the q|k|v and gate|up weight streams, SwiGLU into down's, each weight
        # 16-bit or (w8) its e4m3 copy: _stream_linear.  o asks ops.decode_linear_ok like the other three, with or
        # without w8; under the gate above that matters only for a non-contiguous wo, which takes ops.linear_fwd.
        q_qkv, q_o, q_gu, q_d = w8 if w8 is not None else (None,) * 4
        if ad is not None:      # each group's adapters ride in front of its copy (Adapted)
            q_qkv, q_o = _adapted(ad, ad.qkv, q_qkv), _adapted(ad, ad.o, q_o)
            q_gu, q_d = _adapted(ad, ad.gu, q_gu), _adapted(ad, ad.down, q_d)
        qkv = _stream_linear(x2, wqkv, q_qkv, 1, ln1, eps, None, FF)
        _step_attn(qkv, qkv, qkv, 3 * D, cos, sin, kvc, kv8, t_dev, Tmax, B, H, hd, att, scale, ragged, beam, spec, k_off=D,
                   v_off=2 * D)
        h1 = _stream_linear(att, wo, q_o, 0, None, eps, x2, FF)
        gu = _stream_linear(h1, wgu, q_gu, 1, ln2, eps, None, FF)
        return _stream_linear(gu, wd, q_d, 2, None, eps, h1, FF)
    _, y1, _ = ops.rmsnorm_fwd(x2, ln1, eps)
    ldc = 2 * D
    # the layout of the new q, k, v, decided once: what the step kernel reads, what RoPE rotates (tensor, heads) and
    # what the cache append copies (source, columns, source offset, cache column)
    if wqkv is not None:        # fused: column blocks of ONE [M, 3D] buffer, one RoPE launch, one copy of [k | v]
        qkv = ops.linear_fwd(y1, wqkv)
        ldq = 3 * D
        q, k, v = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
        new, off = (qkv, qkv, qkv), {"k_off": D, "v_off": 2 * D}
        ropes, appends = ((qkv[:, :2 * D], 2 * H),), ((qkv, 2 * D, D, 0),)
    else:
        q, k, v = ops.linear_fwd(y1, wq), ops.linear_fwd(y1, wk), ops.linear_fwd(y1, wv)
        ldq = D
        new, off = (q, k, v), {}
        ropes, appends = ((q, H), (k, H)), ((k, D, 0, 0), (v, D, 0, D))
    _lora_runs(ad, "qkv", y1, (q, k, v), Sn)
    if dyn:     # RoPE + cache append + attention of the new position: one launch
        _step_attn(*new, ldq, cos, sin, kvc, kv8, t_dev, Tmax, B, H, hd, att, scale, ragged, beam, spec, **off)
    elif chunk is not None:
        # a continued prefill: the new rows join the compacted cache, then every row attends over its sample's cache
        for t, heads in ropes:
            ops.rope_(t, cos, sin, pos, heads, hd)
        ops.kv_append_rows(k, v, ldq, Sn * ldq, kvc, chunk.slot, Sn, Tmax, B, H, hd)
        if ops.flash_varlen_ok(x2.dtype, hd):
            ops.flash_attn_varlen_fwd(q, kvc, kvc, att, chunk.q_len, chunk.k_len, B, H, Sn, chunk.Lk, hd, ldq, Sn * ldq,
                                      ldc, Tmax * ldc, ldc, Tmax * ldc, D, Sn * D, scale, v_off=D)
        else:           # (a head size outside the kernel: sample by sample at the host lengths; the filler rows zeroed)
            ops.fill_(att, 0.0)
            for b, (nq, nk) in enumerate(zip(chunk.q_host, chunk.k_host)):
                attention_fwd(TDesc(q, ldq, Sn * ldq, b * Sn * ldq), TDesc(kvc, ldc, Tmax * ldc, b * Tmax * ldc),
                              TDesc(kvc, ldc, Tmax * ldc, b * Tmax * ldc + D), TDesc(att, D, Sn * D, b * Sn * D),
                              1, H, nq, nk, hd, scale, causal=True)
    else:
        for t, heads in ropes:
            ops.rope_(t, cos, sin, pos, heads, hd)
        kmask = ragged.kmask if ragged is not None else None
        if kv8 is None and ragged is None:
            # append the new keys / values to the cache rows [t0, t0 + Sn) of every sample, attend over rows [0, t0 + Sn)
            for src, cols, src_off, col in appends:
                ops.copy2d(src, kvc, Sn, cols, ldq, ldc, batch=B, s_src=Sn * ldq, s_dst=Tmax * ldc, src_off=src_off,
                           dst_off=t0 * ldc + col)
            kd, vd, Lk = TDesc(kvc, ldc, Tmax * ldc, 0), TDesc(kvc, ldc, Tmax * ldc, D), t0 + Sn
        else:
            # e4m3 cache or padded batch, prefill: causal attention over the prompt's own 16-bit k, v (read at the ldq
            # pitch), then the quantising / compacting cache write
            kd, vd, Lk = TDesc(k, ldq, Sn * ldq), TDesc(v, ldq, Sn * ldq), Sn
        if flash_ok(x2.dtype, hd):      # (takes views: the D columns at the operand's offset)
            ops.flash_attn_fwd(q, kd.t[..., kd.off:kd.off + D], vd.t[..., vd.off:vd.off + D], att, B, H, Sn, Lk, hd,
                               ldq, Sn * ldq, kd.ld, kd.bs, vd.ld, vd.bs, D, Sn * D, scale, kmask=kmask, causal=True)
        else:
            attention_fwd(TDesc(q, ldq, Sn * ldq), kd, vd, TDesc(att, D, Sn * D), B, H, Sn, Lk, hd, scale, kmask=kmask,
                          causal=True)
        if ragged is not None and kv8 is not None:
            ops.kv_quant_append_rows(k, v, ldq, Sn * ldq, kvc, kv8, ragged.slot, Sn, Tmax, B, H, hd)
        elif ragged is not None:
            ops.kv_append_rows(k, v, ldq, Sn * ldq, kvc, ragged.slot, Sn, Tmax, B, H, hd)
        elif kv8 is not None:
            ops.kv_quant_append(k, v, ldq, Sn * ldq, kvc, kv8, 0, Sn, Tmax, B, H, hd)
    h1 = ops.linear_fwd(att, wo, residual=x2)
    _lora_runs(ad, "o", att, (h1,), Sn)
    _, y2, _ = ops.rmsnorm_fwd(h1, ln2, eps)
    if wgu is not None:
        gu = ops.linear_fwd(y2, wgu)
        _lora_runs(ad, "gu", y2, (gu[:, :FF], gu[:, FF:]), Sn)
        a = ops.swiglu2d_fwd(gu, FF)
    else:
        g, u = ops.linear_fwd(y2, wg), ops.linear_fwd(y2, wu)
        _lora_runs(ad, "gu", y2, (g, u), Sn)
        a = ops.swiglu_fwd(g, u)
    out = ops.linear_fwd(a, wd, residual=h1)
    _lora_runs(ad, "down", a, (out,), Sn)
    return out


class ScoreLayout(NamedTuple):
    """the options of LlamaForCausalLM.score() as the scoring pass takes them (score_layout): B prompts, n options each,
    Lc = the longest option, F = Lc - 1 fed rows per option"""
    fed: torch.Tensor        # int64 [B * n * F]: row (b * n + j) * F + g feeds token g of option (b, j); a dead row feeds id 0
    lens: torch.Tensor       # int32 [B * n]: the fed rows of each option, max(length - 1, 0): mk_score_attn's len
    targets: torch.Tensor    # int64 [B, n, Lc]: the scored ids, 0 behind each option's end
    lengths: torch.Tensor    # int64 [B, n]: tokens per option, 0 = absent
    n: int
    F: int
    Lc: int


SCORE_MAX_N = 32


def score_layout(continuations=None, continuation_ids=None, continuation_lengths=None, B=None, V=None):
    """The host side of LlamaForCausalLM.score(): pure, and for the list form on the CPU.
    continuations: a list of B lists of token-id lists (prompt b's options; prompts may have different counts, absent ones
    are padded to n = the largest count; options may have different lengths >= 1), or continuation_ids int64 [B, n, Lc]
    with continuation_lengths [B, n] (0 = absent; any device, no value of either is read on the host: lengths are clamped
    into [0, Lc] and, with V, the ids fed into [0, V - 1] by tensor operations).  Exactly one form.  Option (b, j) feeds
    its first length - 1 tokens: F = Lc - 1 rows per option, the rows behind an option's own feed id 0.
    ValueError: both or neither form, a batch other than B (where B is given), n > 32, and in list form a prompt without
    options, an empty option and (with V) an id outside [0, V)."""
    if (continuations is None) == (continuation_ids is None):
        raise ValueError("score: pass exactly one of continuations (lists) and continuation_ids (a tensor), got "
                         f"{'both' if continuations is not None else 'neither'}")
    if continuations is not None:
        if continuation_lengths is not None:
            raise ValueError("score: continuation_lengths goes with continuation_ids, not with continuations")
        opts = [[[int(t) for t in o] for o in p] for p in continuations]
        if B is not None and len(opts) != B:
            raise ValueError(f"score: {len(opts)} lists of continuations for a batch of {B} prompts")
        if not opts or any(len(p) == 0 for p in opts):
            raise ValueError("score: every prompt needs at least one continuation")
        empty = [(b, j) for b, p in enumerate(opts) for j, o in enumerate(p) if len(o) == 0]
        if empty:
            raise ValueError(f"score: empty continuation(s) at (prompt, option) {empty}: an option has at least one token")
        if V is not None:
            bad = sorted({t for p in opts for o in p for t in o if not 0 <= t < V})
            if bad:
                raise ValueError(f"score: token id(s) {bad[:8]} outside [0, {V})")
        n, Lc = max(len(p) for p in opts), max(len(o) for p in opts for o in p)
        if n > SCORE_MAX_N:
            raise ValueError(f"score: {n} continuations for one prompt; at most {SCORE_MAX_N}")
        ids = torch.zeros((len(opts), n, Lc), dtype=torch.int64)
        lengths = torch.zeros((len(opts), n), dtype=torch.int64)
        for b, p in enumerate(opts):
            for j, o in enumerate(p):
                ids[b, j, :len(o)] = torch.tensor(o, dtype=torch.int64)
                lengths[b, j] = len(o)
    else:
        ids, lengths = continuation_ids, continuation_lengths
        if lengths is None:
            raise ValueError("score: continuation_ids needs continuation_lengths [B, n]")
        if ids.dim() != 3 or ids.dtype != torch.int64 or ids.shape[2] < 1:
            raise ValueError(f"score: continuation_ids should be int64 [B, n, Lc >= 1], but is {ids.dtype} {tuple(ids.shape)}")
        if tuple(lengths.shape) != tuple(ids.shape[:2]) or lengths.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"score: continuation_lengths should be an integer tensor {tuple(ids.shape[:2])}, but is "
                             f"{lengths.dtype} {tuple(lengths.shape)}")
        if B is not None and ids.shape[0] != B:
            raise ValueError(f"score: continuation_ids for {ids.shape[0]} prompts and a batch of {B}")
        if ids.shape[1] < 1 or ids.shape[1] > SCORE_MAX_N:
            raise ValueError(f"score: {ids.shape[1]} continuations per prompt; between 1 and {SCORE_MAX_N}")
        n, Lc = ids.shape[1], ids.shape[2]
        lengths = lengths.to(device=ids.device, dtype=torch.int64).clamp(0, Lc)
    F = Lc - 1
    col = torch.arange(Lc, device=ids.device)
    targets = torch.where(col < lengths[..., None], ids, torch.zeros_like(ids)).contiguous()
    fed = torch.where(col[:F] < lengths[..., None] - 1, ids[..., :F], torch.zeros_like(ids[..., :F]))
    if V is not None:
        fed = fed.clamp(0, V - 1)
    lens = (lengths - 1).clamp(0, F).to(torch.int32).reshape(-1).contiguous()
    return ScoreLayout(fed.reshape(-1).contiguous(), lens, targets, lengths.contiguous(), n, F, Lc)


def llama_layer_score(x2, B, sp, lens, t_off, cos, sin, n_heads, eps, ws, ln1, ln2):
    """No-grad decoder layer over the B * sp.n * F FED rows of a scoring pass (score_layout; F = sp.tail.shape[1]): row
    (b * n + j) * F + g is fed token g of option j of prompt b.  A GEMM pass, not a weight stream: the four linears go
    through ops.linear_fwd, RMSNorm and SwiGLU are the prefill's, and the attention is ops.score_attn over sp (a
    SharedPrompt: the prompt cache the prefill wrote at B rows, and the layer's tail cache, which this call fills).  lens
    int32 [B * n] on the device: the fed rows of each option; t_off: Ragged.t_off of a padded batch or None.  ws: the
    layer's LayerWeights (the merged copies under a live adapter).  The rows of dead positions carry zeros out of the
    attention and whatever the linears make of them; nothing reads them."""
    M, D = x2.shape
    H, hd = n_heads, D // n_heads
    F = sp.tail.shape[1]
    if M != B * sp.n * F:
        raise ValueError(f"llama_layer_score: {M} rows for B * n * F = {B} * {sp.n} * {F}")
    FF = ws.wg.shape[0]
    att = torch.empty((M, D), dtype=x2.dtype, device=x2.device)
    _, y1, _ = ops.rmsnorm_fwd(x2, ln1, eps)
    if ws.wqkv is not None:
        qkv = ops.linear_fwd(y1, ws.wqkv)
        ops.score_attn(qkv, qkv, qkv, 3 * D, cos, sin, sp.prompt, sp.tail, lens, t_off, sp.S0, B, sp.n, H, hd, att,
                       1.0 / math.sqrt(hd), k_off=D, v_off=2 * D)
    else:
        q, k, v = ops.linear_fwd(y1, ws.wq), ops.linear_fwd(y1, ws.wk), ops.linear_fwd(y1, ws.wv)
        ops.score_attn(q, k, v, D, cos, sin, sp.prompt, sp.tail, lens, t_off, sp.S0, B, sp.n, H, hd, att, 1.0 / math.sqrt(hd))
    h1 = ops.linear_fwd(att, ws.wo, residual=x2)
    _, y2, _ = ops.rmsnorm_fwd(h1, ln2, eps)
    if ws.wgu is not None:
        a = ops.swiglu2d_fwd(ops.linear_fwd(y2, ws.wgu), FF)
    else:
        a = ops.swiglu_fwd(ops.linear_fwd(y2, ws.wg), ops.linear_fwd(y2, ws.wu))
    return ops.linear_fwd(a, ws.wd, residual=h1)


# =========================================================================
# final norm + lm_head + shifted cross-entropy  (modeling.py:508,597-610)
# =========================================================================
class LMHeadLossFn(torch.autograd.Function):
    """returns (loss[1] f32, logits view [B,S,V] on a pitched buffer)."""

    @staticmethod
    def forward(ctx, h, norm_w, lm_w, shift_labels, eps):
        B, S, D = h.shape
        M, V = B * S, lm_w.shape[0]
        h2 = _c2(h, M, D)
        _, y, rstd = ops.rmsnorm_fwd(h2, norm_w, eps)
        ldv = (V + 63) // 64 * 64
        buf = torch.empty((M, ldv), dtype=h.dtype, device=h.device)
        ops.gemm_raw(y, lm_w, buf, M, V, D, D, D, ldv)
        logits = buf.view(B, S, ldv)[:, :, :V]
        if shift_labels is None:
            ctx.has_loss = False
            ctx.save_for_backward(h2, rstd, y, norm_w, lm_w)
            ctx.dims = (B, S, D, V, ldv)
            loss = torch.zeros(1, dtype=torch.float32, device=h.device)
            ctx.mark_non_differentiable(loss)
            return loss, logits
        _, row_lse, sum_cnt = ops.cross_entropy(buf, shift_labels, V)
        ctx.has_loss = True
        ctx.save_for_backward(h2, rstd, y, norm_w, lm_w, buf, shift_labels, row_lse, sum_cnt)
        ctx.dims = (B, S, D, V, ldv)
        ctx.set_materialize_grads(False)
        return sum_cnt[2:3], logits

    @staticmethod
    def backward(ctx, dloss, dlogits_ext):
        B, S, D, V, ldv = ctx.dims
        M = B * S
        need = ctx.needs_input_grad
        if ctx.has_loss:
            h2, rstd, y, norm_w, lm_w, buf, labels, row_lse, sum_cnt = ctx.saved_tensors
        else:
            h2, rstd, y, norm_w, lm_w = ctx.saved_tensors
        dl = None
        if ctx.has_loss and dloss is not None:
            gs = _c2(dloss.to(torch.float32), 1, 1) if dloss.dtype != torch.float32 else dloss
            dl = ops.cross_entropy_bwd(buf, labels, row_lse, sum_cnt, V, grad_scale=1.0,
                                       grad_scale_dev=gs.contiguous())
        if dlogits_ext is not None:
            ext = torch.empty((M, ldv), dtype=h2.dtype, device=h2.device)
            ops.fill_(ext, 0.0)
            src = dlogits_ext.reshape(M, V)
            ops.copy2d(src, ext, M, V, src.stride(0), ldv)
            dl = ext if dl is None else ops.add(dl, ext, out=dl)
        if dl is None:
            return None, None, None, None, None
        dlv = dl[:, :V]
        # the pad columns [V, ldv) of dl are zero (ce_bwd writes the whole pitch, `ext` is
        # zero-filled): the K = V reduction of dx runs on the tile kernels over the padded width
        sd = _DwSide(h2.device, M, D)                    # (see DW_SIDE: the [M, D] grad-input GEMM beside the grad-weight GEMM)
        ev = sd.fork()
        dy = ops.linear_dx(dlv, lm_w, dy_pad_zero=True)
        dlm = sd.dw(ev, dlv, y, lm_w, "lm") if need[2] else None
        dh, dnw = ops.rmsnorm_bwd(dy, h2, norm_w, rstd, dw_out=ops.grad_dst(norm_w) if need[1] else None)
        sd.join()
        return dh.view(B, S, D), (dnw if need[1] else None), dlm, None, None


# =========================================================================
# pre-LN transformer encoder layer (HF CLIPEncoderLayer / WhisperEncoderLayer)
# =========================================================================
ACT_CODE = {"gelu": 1, "quick_gelu": 2}


class EncoderLayerFn(torch.autograd.Function):
    """x + attn(LN1(x)) ; h + fc2(act(fc1(LN2(h)))).  k_proj bias may be None (Whisper).
    w3 / b3: the [3E, E] / [3E] views ALIASING wq|wk|wv and their biases when the module keeps
    them back to back (modeling.fused_encoder_qkv), else None."""

    @staticmethod
    def forward(ctx, x, n_heads, eps, act, ln1w, ln1b, wq, bq, wk, bk, wv, bv, wo, bo, ln2w, ln2b,
                w1, b1, w2, b2, w3=None, b3=None):
        B, T, E = x.shape
        M, H, hd = B * T, n_heads, E // n_heads
        x2 = _c2(x, M, E)
        y1, mean1, rstd1 = ops.layernorm_fwd(x2, ln1w, ln1b, eps)
        grad_mode = any(ctx.needs_input_grad)
        if grad_mode or w3 is None:
            q = ops.linear_fwd(y1, wq, bias=bq)
            k = ops.linear_fwd(y1, wk, bias=bk)
            v = ops.linear_fwd(y1, wv, bias=bv)
            ldq = E
        else:   # frozen tower / inference: one q|k|v GEMM on the module's fused storage
            qkv = ops.linear_fwd(y1, w3, bias=b3)
            q, k, v = qkv[:, :E], qkv[:, E:2 * E], qkv[:, 2 * E:]
            ldq = 3 * E
        att = torch.empty((M, E), dtype=x.dtype, device=x.device)
        d = lambda t: TDesc(t, ldq, T * ldq)  # noqa: E731
        use_flash = flash_ok(x.dtype, hd)
        if use_flash:   # fused attention, the T x T scores never reach HBM
            lse = torch.empty((B, H, T), dtype=torch.float32, device=x.device) if grad_mode else None
            ops.flash_attn_fwd(q, k, v, att, B, H, T, T, hd, ldq, T * ldq, ldq, T * ldq, ldq, T * ldq,
                               E, T * E, hd ** -0.5, lse=lse)
            probs = lse
        else:
            probs, _ = attention_fwd(d(q), d(k), d(v), TDesc(att, E, T * E), B, H, T, T, hd, hd ** -0.5)
        h1 = ops.linear_fwd(att, wo, bias=bo, residual=x2)
        y2, mean2, rstd2 = ops.layernorm_fwd(h1, ln2w, ln2b, eps)
        if grad_mode:
            f1 = ops.linear_fwd(y2, w1, bias=b1)
            a = ops.act_fwd(f1, act)
        else:  # inference / frozen tower: activation fused into the GEMM epilogue
            f1 = None
            a = ops.linear_fwd(y2, w1, bias=b1, act=act)
        out = ops.linear_fwd(a, w2, bias=b2, residual=h1)
        if grad_mode:
            ctx.save_for_backward(x2, mean1, rstd1, y1, q, k, v, probs, att, h1, mean2, rstd2, y2,
                                  f1, a, ln1w, wq, wk, wv, wo, ln2w, w1, w2)
            ctx.dims = (B, T, E, H, hd, act, bk is not None, use_flash)
        return out.view(B, T, E)

    @staticmethod
    def backward(ctx, dout):
        (x2, mean1, rstd1, y1, q, k, v, probs, att, h1, mean2, rstd2, y2, f1, a, ln1w, wq, wk, wv,
         wo, ln2w, w1, w2) = ctx.saved_tensors
        B, T, E, H, hd, act, has_bk, use_flash = ctx.dims
        M = B * T
        dout2 = _c2(dout, M, E)
        da = ops.linear_dx(dout2, w2)
        dw2, db2 = ops.linear_dw(dout2, a), ops.colsum(dout2)
        df1 = ops.act_bwd(f1, da, act)
        dy2 = ops.linear_dx(df1, w1)
        dw1, db1 = ops.linear_dw(df1, y2), ops.colsum(df1)
        dh1, dln2w, dln2b = ops.layernorm_bwd(dy2, h1, ln2w, mean2, rstd2, dres=dout2)
        datt = ops.linear_dx(dh1, wo)
        dwo, dbo = ops.linear_dw(dh1, att), ops.colsum(dh1)
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        d = lambda t: TDesc(t, E, T * E)  # noqa: E731
        if use_flash:
            ops.flash_attn_bwd(q, k, v, att, datt, probs, dq, dk, dv, B, H, T, T, hd, E, T * E, E,
                               T * E, E, T * E, E, T * E, hd ** -0.5)
        else:
            attention_bwd(d(datt), d(q), d(k), d(v), probs, None, d(dq), d(dk), d(dv), B, H, T, T,
                          hd, hd ** -0.5)
        dy1 = ops.linear_dx(dq, wq)
        ops.linear_dx(dk, wk, out=dy1, accumulate=True)
        ops.linear_dx(dv, wv, out=dy1, accumulate=True)
        dwq, dbq = ops.linear_dw(dq, y1), ops.colsum(dq)
        dwk, dbk = ops.linear_dw(dk, y1), (ops.colsum(dk) if has_bk else None)
        dwv, dbv = ops.linear_dw(dv, y1), ops.colsum(dv)
        dx, dln1w, dln1b = ops.layernorm_bwd(dy1, x2, ln1w, mean1, rstd1, dres=dh1)
        return (dx.view(B, T, E), None, None, None, dln1w, dln1b, dwq, dbq, dwk, dbk, dwv, dbv, dwo,
                dbo, dln2w, dln2b, dw1, db1, dw2, db2, None, None)


class LayerNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, eps):
        shp = x.shape
        x2 = _c2(x, x.numel() // shp[-1], shp[-1])
        y, mean, rstd = ops.layernorm_fwd(x2, w, b, eps)
        ctx.save_for_backward(x2, w, mean, rstd)
        return y.view(shp)

    @staticmethod
    def backward(ctx, dy):
        x2, w, mean, rstd = ctx.saved_tensors
        dx, dw, db = ops.layernorm_bwd(_c2(dy, x2.shape[0], x2.shape[1]), x2, w, mean, rstd)
        return dx.view(dy.shape), dw, db, None


class RMSNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, eps):
        shp = x.shape
        x2 = _c2(x, x.numel() // shp[-1], shp[-1])
        _, y, rstd = ops.rmsnorm_fwd(x2, w, eps)
        ctx.save_for_backward(x2, w, rstd)
        return y.view(shp)

    @staticmethod
    def backward(ctx, dy):
        x2, w, rstd = ctx.saved_tensors
        dx, dw = ops.rmsnorm_bwd(_c2(dy, x2.shape[0], x2.shape[1]), x2, w, rstd)
        return dx.view(dy.shape), dw, None


class LinearFn(torch.autograd.Function):
    """y = act(x W^T + b): nn.Linear call sites outside the fused blocks."""

    @staticmethod
    def forward(ctx, x, w, b, act):
        shp = x.shape
        x2 = _c2(x, x.numel() // shp[-1], shp[-1])
        if act:
            pre = ops.linear_fwd(x2, w, bias=b)
            y = ops.act_fwd(pre, act)
        else:
            pre = None
            y = ops.linear_fwd(x2, w, bias=b)
        ctx.save_for_backward(x2, w, pre)
        ctx.act, ctx.has_b = act, b is not None
        return y.view(*shp[:-1], w.shape[0])

    @staticmethod
    def backward(ctx, dy):
        x2, w, pre = ctx.saved_tensors
        dy2 = _c2(dy, x2.shape[0], w.shape[0])
        if ctx.act:
            dy2 = ops.act_bwd(pre, dy2, ctx.act)
        need = ctx.needs_input_grad
        dx = ops.linear_dx(dy2, w).view(*dy.shape[:-1], w.shape[1]) if need[0] else None
        dw = ops.linear_dw(dy2, x2) if need[1] else None
        db = ops.colsum(dy2) if (ctx.has_b and need[2]) else None
        return dx, dw, db, None


# =========================================================================
# nn.MultiheadAttention(add_bias_kv, add_zero_attn, dropout) as SELF attention
# (video_long_self_attention, modeling.py:906-910,1078); batch-first inside.
# =========================================================================
class MHASelfFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, n_heads, p, seed, in_w, in_b, bias_k, bias_v, out_w, out_b):
        B, L, E = x.shape
        H, hd, Lk = n_heads, E // n_heads, L + 2
        x2 = _c2(x, B * L, E)
        q = ops.linear_fwd(x2, in_w[:E], bias=in_b[:E])
        # K|V rows per sample: [L projected rows, bias_k|bias_v row, zero row]
        kv = torch.empty((B, Lk, 2 * E), dtype=x.dtype, device=x.device)
        ops.fill_(kv, 0.0)
        ops.gemm_raw(x2, in_w, kv, L, 2 * E, E, E, E, 2 * E, bias=in_b[E:], bias_mode=1, nb1=B,
                     sA=(L * E, 0), sC=(Lk * 2 * E, 0), b_off=E * E)
        ops.copy2d(bias_k, kv, 1, E, E, 2 * E, batch=B, s_src=0, s_dst=Lk * 2 * E, dst_off=L * 2 * E)
        ops.copy2d(bias_v, kv, 1, E, E, 2 * E, batch=B, s_src=0, s_dst=Lk * 2 * E,
                   dst_off=L * 2 * E + E)
        att = torch.empty((B * L, E), dtype=x.dtype, device=x.device)
        kd, vd = TDesc(kv, 2 * E, Lk * 2 * E, 0), TDesc(kv, 2 * E, Lk * 2 * E, E)
        probs, pd = attention_fwd(TDesc(q, E, L * E), kd, vd, TDesc(att, E, L * E), B, H, L, Lk, hd,
                                  math.sqrt(1.0 / hd), p=p, seed=seed)
        out = ops.linear_fwd(att, out_w, bias=out_b)
        ctx.save_for_backward(x2, q, kv, probs, pd, att, in_w, out_w)
        ctx.dims = (B, L, E, H, hd, p, seed)
        ctx.in_b_ref, ctx.out_b_ref = in_b, out_b        # (only their addresses are used: gradient-bucket lookup)
        return out.view(B, L, E)

    @staticmethod
    def backward(ctx, dout):
        x2, q, kv, probs, pd, att, in_w, out_w = ctx.saved_tensors
        B, L, E, H, hd, p, seed = ctx.dims
        Lk = L + 2
        need = ctx.needs_input_grad
        dout2 = _c2(dout, B * L, E)
        datt = ops.linear_dx(dout2, out_w)
        dwo, dbo = ops.linear_dw(dout2, att, w=out_w), ops.colsum(dout2, out=ops.grad_dst(ctx.out_b_ref))
        dq = torch.empty_like(q)
        dkv = torch.empty_like(kv)
        kd, vd = TDesc(kv, 2 * E, Lk * 2 * E, 0), TDesc(kv, 2 * E, Lk * 2 * E, E)
        dkd, dvd = TDesc(dkv, 2 * E, Lk * 2 * E, 0), TDesc(dkv, 2 * E, Lk * 2 * E, E)
        attention_bwd(TDesc(datt, E, L * E), TDesc(q, E, L * E), kd, vd, probs, pd,
                      TDesc(dq, E, L * E), dkd, dvd, B, H, L, Lk, hd, math.sqrt(1.0 / hd), p=p,
                      seed=seed)
        # bias_k / bias_v grads: sum over batch of row L
        rows = dkv.view(B * Lk, 2 * E)
        brow = torch.empty((B, 2 * E), dtype=x2.dtype, device=x2.device)
        ops.copy2d(rows, brow, 1, 2 * E, 2 * E, 2 * E, batch=B, s_src=Lk * 2 * E, s_dst=2 * E,
                   src_off=L * 2 * E)
        bsum = ops.colsum(brow)
        dbk, dbv = bsum[:E].view(1, 1, E), bsum[E:].view(1, 1, E)
        # compact the projected rows [B, L, 2E] (drop the 2 extra rows per sample)
        dkvc = torch.empty((B * L, 2 * E), dtype=x2.dtype, device=x2.device)
        ops.copy2d(rows, dkvc, L, 2 * E, 2 * E, 2 * E, batch=B, s_src=Lk * 2 * E, s_dst=L * 2 * E)
        din_w = ops.grad_dst(in_w)
        if din_w is None:
            din_w = torch.empty_like(in_w)
        din_b = ops.grad_dst(ctx.in_b_ref)
        if din_b is None:
            din_b = torch.empty((3 * E,), dtype=x2.dtype, device=x2.device)
        ops.linear_dw(dq, x2, out=din_w[:E])
        ops.linear_dw(dkvc, x2, out=din_w[E:])
        ops.colsum(dq, out=din_b[:E])
        ops.colsum(dkvc, out=din_b[E:])
        dx = None
        if need[0]:
            dx = ops.linear_dx(dq, in_w[:E])
            ops.linear_dx(dkvc, in_w[E:], out=dx, accumulate=True)
            dx = dx.view(B, L, E)
        return dx, None, None, None, din_w, din_b, dbk, dbv, dwo, dbo


# =========================================================================
# Multimodal prefix: Conv1d -> Linear -> alignment attention -> splice
# (modeling.py:965-1048) as ONE block, K/V of the embedding table projected once per
# step and shared by the whole batch, dE accumulated in place.
# =========================================================================
MODALITIES = ("image", "audio", "video")  # final prefix order after BOS
N_ALIGN_PARAMS = 10  # conv_w, conv_b, lin_w, lin_b, in_w, in_b, bias_k, bias_v, out_w, out_b


def _align_fwd(feats, E, prm, heads, kw, stride, p, seed):
    conv_w, conv_b, lin_w, lin_b, in_w, in_b, bias_k, bias_v, out_w, out_b = prm
    B, T, C = feats.shape
    V, D = E.shape
    H, hd = heads, D // heads
    f2 = _c2(feats, B * T, C)
    cols, Lout = ops.im2col1d(f2, B, C, T, kw, stride, 0, T * C, 1, C)
    K = C * kw
    cw = conv_w.view(conv_w.shape[0], K)
    pj = torch.empty((B * Lout, cw.shape[0]), dtype=feats.dtype, device=feats.device)
    ops.gemm_raw(cols, cw, pj, B * Lout, cw.shape[0], K, cols.stride(0), K, cw.shape[0], bias=conv_b,
                 bias_mode=1)
    t = ops.linear_fwd(pj, lin_w, bias=lin_b)
    Lq = B * Lout
    q = ops.linear_fwd(t, in_w[:D], bias=in_b[:D])
    Lk = V + 2
    Lkp = _pad64(Lk)   # rows [V+1, Lkp) are zero: the add_zero_attn row + alignment padding
    kv = torch.empty((Lkp, 2 * D), dtype=feats.dtype, device=feats.device)
    if FP8["align"] and _fp8_ok(E, in_w[D:]):
        _fp8_linear(E, in_w[D:], bias=in_b[D:], out=kv[:V])
    else:
        ops.gemm_raw(E, in_w, kv, V, 2 * D, D, D, D, 2 * D, bias=in_b[D:], bias_mode=1, b_off=D * D)
    ops.copy2d(bias_k, kv, 1, D, D, 2 * D, dst_off=V * 2 * D)
    ops.copy2d(bias_v, kv, 1, D, D, 2 * D, dst_off=V * 2 * D + D)
    ops.fill_(kv[V + 1:], 0.0)
    o = torch.empty((Lq, D), dtype=feats.dtype, device=feats.device)
    kd, vd = TDesc(kv, 2 * D, 0, 0), TDesc(kv, 2 * D, 0, D)
    probs, pd = attention_fwd(TDesc(q, D, 0), kd, vd, TDesc(o, D, 0), 1, H, Lq, Lk, hd,
                              math.sqrt(1.0 / hd), p=p, seed=seed, Lk_pad=Lkp)
    aligned = ops.linear_fwd(o, out_w, bias=out_b)  # rows are (b, j): [B, Lout, D]
    saved = (f2, cols, pj, t, q, kv, probs, pd, o)
    return aligned, Lout, saved


def _align_bwd(da, E, dE, dE_init, prm, saved, dims, need_feats):
    """da [B*Lout, D]. Accumulates the table gradient into dE (initialised iff dE_init)."""
    conv_w, conv_b, lin_w, lin_b, in_w, in_b, bias_k, bias_v, out_w, out_b = prm
    f2, cols, pj, t, q, kv, probs, pd, o = saved
    B, T, C, Lout, H, kw, stride, p, seed = dims
    V, D = E.shape
    hd, Lq, Lk = D // H, B * Lout, V + 2
    g = {}
    g["out_w"], g["out_b"] = ops.linear_dw(da, o, w=out_w), ops.colsum(da, out=ops.grad_dst(out_b))
    do = ops.linear_dx(da, out_w)
    dq = torch.empty_like(q)
    dkv = torch.empty_like(kv)
    kd, vd = TDesc(kv, 2 * D, 0, 0), TDesc(kv, 2 * D, 0, D)
    attention_bwd(TDesc(do, D, 0), TDesc(q, D, 0), kd, vd, probs, pd, TDesc(dq, D, 0),
                  TDesc(dkv, 2 * D, 0, 0), TDesc(dkv, 2 * D, 0, D), 1, H, Lq, Lk, hd,
                  math.sqrt(1.0 / hd), p=p, seed=seed, Lk_pad=kv.shape[0])
    brow = torch.empty((1, 2 * D), dtype=da.dtype, device=da.device)
    ops.copy2d(dkv, brow, 1, 2 * D, 2 * D, 2 * D, src_off=V * 2 * D)
    g["bias_k"], g["bias_v"] = brow[0, :D].reshape(1, 1, D), brow[0, D:].reshape(1, 1, D)
    dkvt = dkv[:V]
    # table gradient: dE (+)= dKV W_kv
    if FP8["align"] and _fp8_dx_ok(dkvt, in_w[D:]) and _fp8_ok(E, in_w[D:]):
        _fp8_dx(dkvt, in_w[D:], out=dE, accumulate=not dE_init)
    else:
        ops.linear_dx(dkvt, in_w[D:], out=dE, accumulate=not dE_init)
    din_w = ops.grad_dst(in_w)              # (a registered gradient-bucket slot, else a fresh tensor)
    if din_w is None:
        din_w = torch.empty_like(in_w)
    din_b = ops.grad_dst(in_b)
    if din_b is None:
        din_b = torch.empty((3 * D,), dtype=da.dtype, device=da.device)
    ops.linear_dw(dq, t, out=din_w[:D])
    ops.linear_dw(dkvt, E, out=din_w[D:])
    ops.colsum(dq, out=din_b[:D])
    ops.colsum(dkvt, out=din_b[D:])
    g["in_w"], g["in_b"] = din_w, din_b
    dt = ops.linear_dx(dq, in_w[:D])
    g["lin_w"], g["lin_b"] = ops.linear_dw(dt, pj, w=lin_w), ops.colsum(dt, out=ops.grad_dst(lin_b))
    dpj = ops.linear_dx(dt, lin_w)
    K = C * kw
    cw = conv_w.view(conv_w.shape[0], K)
    dcw = ops.grad_dst(cw)
    if dcw is None:
        dcw = torch.empty_like(cw)
    ops.gemm_raw(dpj, cols, dcw, cw.shape[0], K, Lq, dpj.stride(0), cols.stride(0), K, a_red=True,
                 b_red=True)
    g["conv_w"], g["conv_b"] = dcw.view_as(conv_w), ops.colsum(dpj, out=ops.grad_dst(conv_b))
    dfeats = None
    if need_feats:
        dcols = torch.empty((Lq, cols.shape[1]), dtype=da.dtype, device=da.device)
        ops.gemm_raw(dpj, cw, dcols, Lq, K, cw.shape[0], dpj.stride(0), K, cols.shape[1], b_red=True)
        dfeats = ops.col2im1d(dcols, B, C, T, kw, stride, 0, Lout, T * C, 1, C, (B, T, C))
    return g, dfeats


class PrefixAssembleFn(torch.autograd.Function):
    """inputs_embeds = [BOS][<image> a_img </image>][<audio> a_aud </audio>][<video> a_vid
    </video>][text 1:]  (modeling.py:977-1034; order verified in SURVEY A8).

    meta: dict(ids_full [B,S] int64 with -1 at feature slots, slots {name: (start, Lq)},
               heads, geom {name: (kernel, stride)}, p, seeds {name: seed}, padding_idx)."""

    @staticmethod
    def forward(ctx, E, meta, image_f, audio_f, video_f, *params):
        feats = dict(image=image_f, audio=audio_f, video=video_f)
        ids_full = meta["ids_full"]
        B, S = ids_full.shape
        V, D = E.shape
        out = torch.empty((B, S, D), dtype=E.dtype, device=E.device)
        ops.embedding_fwd(E, ids_full.view(-1), out=out.view(B * S, D))
        saved, dims = {}, {}
        for i, name in enumerate(MODALITIES):
            f = feats[name]
            if f is None:
                continue
            prm = params[i * N_ALIGN_PARAMS:(i + 1) * N_ALIGN_PARAMS]
            kw, stride = meta["geom"][name]
            aligned, Lout, sv = _align_fwd(f, E, prm, meta["heads"], kw, stride, meta["p"],
                                           meta["seeds"][name])
            start, Lq = meta["slots"][name]
            assert Lq == Lout, (name, Lq, Lout)
            ops.copy2d(aligned, out, Lout, D, D, D, batch=B, s_src=Lout * D, s_dst=S * D,
                       dst_off=start * D)
            saved[name] = sv
            dims[name] = (f.shape[0], f.shape[1], f.shape[2], Lout, meta["heads"], kw, stride,
                          meta["p"], meta["seeds"][name])
        ctx.meta, ctx.dims_, ctx.saved_ = meta, dims, saved
        ctx.params = params
        ctx.E = E
        return out

    @staticmethod
    def backward(ctx, dout):
        meta, E, params = ctx.meta, ctx.E, ctx.params
        ids_full = meta["ids_full"]
        B, S = ids_full.shape
        V, D = E.shape
        need = ctx.needs_input_grad
        dout2 = _c2(dout, B * S, D)
        dE = ops.grad_dst(E) if need[0] else None     # straight into the gradient bucket when one is registered
        if dE is None:
            dE = torch.empty_like(E)
        dE_init = True
        grads = [None] * (len(MODALITIES) * N_ALIGN_PARAMS)
        dfeats = dict(image=None, audio=None, video=None)
        order = ("conv_w", "conv_b", "lin_w", "lin_b", "in_w", "in_b", "bias_k", "bias_v", "out_w",
                 "out_b")
        for i, name in enumerate(MODALITIES):
            if name not in ctx.saved_:
                continue
            prm = params[i * N_ALIGN_PARAMS:(i + 1) * N_ALIGN_PARAMS]
            start, Lq = meta["slots"][name]
            da = torch.empty((B * Lq, D), dtype=dout.dtype, device=dout.device)
            ops.copy2d(dout2, da, Lq, D, D, D, batch=B, s_src=S * D, s_dst=Lq * D, src_off=start * D)
            g, df = _align_bwd(da, E, dE, dE_init, prm, ctx.saved_[name], ctx.dims_[name],
                               need[2 + i])
            dE_init = False
            for j, key in enumerate(order):
                grads[i * N_ALIGN_PARAMS + j] = g[key]
            dfeats[name] = df
        if dE_init:
            ops.fill_(dE, 0.0)
        ops.embedding_bwd_(dE, dout2, ids_full.view(-1), padding_idx=meta.get("padding_idx", -1))
        ctx.saved_ = None
        return (dE, None, dfeats["image"], dfeats["audio"], dfeats["video"], *grads)


# =========================================================================
# encoder stems / heads (HF CLIPVisionEmbeddings, visual_projection, Whisper conv stem)
# =========================================================================
class ClipEmbedFn(torch.autograd.Function):
    """[CLS + pos[0] ; patch_embed(x) + pos[1:]] — Conv2d(k=P, s=P, no bias) as patchify + GEMM
    written straight into rows 1.. of the [B, T, E] buffer with the position rows as the
    GEMM residual."""

    @staticmethod
    def forward(ctx, x, patch_w, cls, pos, P):
        B, C, Hh, Ww = x.shape
        E = patch_w.shape[0]
        G = (Hh // P) * (Ww // P)
        T = G + 1
        K = C * P * P
        cols = ops.patchify(x, P)
        ldk = cols.shape[1]
        wp = torch.empty((E, ldk), dtype=x.dtype, device=x.device)
        if ldk != K:
            ops.fill_(wp, 0.0)
        ops.copy2d(patch_w.view(E, K), wp, E, K, K, ldk)
        out = torch.empty((B, T, E), dtype=x.dtype, device=x.device)
        ops.gemm_raw(cols, wp, out, G, E, ldk, ldk, ldk, E, R=pos, ldr=E, nb1=B, sA=(G * ldk, 0),
                     sC=(T * E, 0), sR=(0, 0), c_off=E, r_off=E)
        clsrow = ops.add(cls.view(-1), pos[0].contiguous().view(-1))
        ops.copy2d(clsrow, out, 1, E, E, E, batch=B, s_src=0, s_dst=T * E)
        if any(ctx.needs_input_grad):
            ctx.save_for_backward(cols, wp)
            ctx.dims = (B, C, Hh, Ww, P, E, G, T, K, ldk)
        return out

    @staticmethod
    def backward(ctx, dout):
        cols, wp = ctx.saved_tensors
        B, C, Hh, Ww, P, E, G, T, K, ldk = ctx.dims
        need = ctx.needs_input_grad
        d2 = _c2(dout, B, T * E)
        dpos = ops.colsum(d2).view(T, E) if need[3] else None
        dcls = None
        if need[2]:
            first = torch.empty((B, E), dtype=dout.dtype, device=dout.device)
            ops.copy2d(d2, first, 1, E, E, E, batch=B, s_src=T * E, s_dst=E)
            dcls = ops.colsum(first)
        dy = torch.empty((B * G, E), dtype=dout.dtype, device=dout.device)
        ops.copy2d(d2, dy, G, E, E, E, batch=B, s_src=T * E, s_dst=G * E, src_off=E)
        dw = None
        if need[1]:
            dwp = ops.linear_dw(dy, cols)            # [E, ldk]
            dw = torch.empty((E, K), dtype=dout.dtype, device=dout.device)
            ops.copy2d(dwp, dw, E, K, ldk, K)
            dw = dw.view(E, C, P, P)
        dx = None
        if need[0]:
            dcols = ops.linear_dx(dy, wp)            # [B*G, ldk]
            dx = ops.unpatchify(dcols, B, C, Hh, Ww, P)
        return dx, dw, dcls, dpos, None


class DropClsProjectFn(torch.autograd.Function):
    """visual_projection(h)[:, 1:, :] without computing the CLS row (bias-free Linear)."""

    @staticmethod
    def forward(ctx, h, w):
        B, T, E = h.shape
        Pd = w.shape[0]
        hc = _c2(h, B * T, E)
        out = torch.empty((B, T - 1, Pd), dtype=h.dtype, device=h.device)
        ops.gemm_raw(hc, w, out, T - 1, Pd, E, E, E, Pd, nb1=B, sA=(T * E, 0), sC=((T - 1) * Pd, 0),
                     a_off=E)
        ctx.save_for_backward(hc, w)
        ctx.dims = (B, T, E, Pd)
        return out

    @staticmethod
    def backward(ctx, dout):
        hc, w = ctx.saved_tensors
        B, T, E, Pd = ctx.dims
        need = ctx.needs_input_grad
        dy = _c2(dout, B * (T - 1), Pd)
        dh = dw = None
        if need[0]:
            dh = torch.empty((B, T, E), dtype=dout.dtype, device=dout.device)
            zero = torch.empty((E,), dtype=dout.dtype, device=dout.device)
            ops.fill_(zero, 0.0)
            ops.copy2d(zero, dh, 1, E, E, E, batch=B, s_src=0, s_dst=T * E)
            ops.gemm_raw(dy, w, dh, T - 1, E, Pd, Pd, E, E, b_red=True, nb1=B,
                         sA=((T - 1) * Pd, 0), sC=(T * E, 0), c_off=E)
        if need[1]:
            hs = torch.empty((B * (T - 1), E), dtype=dout.dtype, device=dout.device)
            ops.copy2d(hc, hs, T - 1, E, E, E, batch=B, s_src=T * E, s_dst=(T - 1) * E, src_off=E)
            dw = ops.linear_dw(dy, hs)
        return dh, dw


class WhisperStemFn(torch.autograd.Function):
    """gelu(conv2(gelu(conv1(mel)))) + embed_positions, channels-last output [B, T2, d]:
    Conv1d(k3,p1) and Conv1d(k3,s2,p1) as window-gather + MFMA GEMM with fused bias/GELU."""

    @staticmethod
    def forward(ctx, mel, w1, b1, w2, b2, pos):
        B, Cm, Tm = mel.shape
        d = w1.shape[0]
        grad_mode = any(ctx.needs_input_grad)
        mel = mel.contiguous()
        cols1, L1 = ops.im2col1d(mel, B, Cm, Tm, 3, 1, 1, Cm * Tm, Tm, 1)
        w1v = w1.view(d, Cm * 3)
        if grad_mode:
            pre1 = ops.linear_fwd(cols1, w1v, bias=b1)
            h1 = ops.act_fwd(pre1, 1)
        else:
            pre1 = None
            h1 = ops.linear_fwd(cols1, w1v, bias=b1, act=1)
        cols2, T2 = ops.im2col1d(h1, B, d, L1, 3, 2, 1, L1 * d, 1, d)
        w2v = w2.view(d, d * 3)
        ld2 = cols2.shape[1]
        out = torch.empty((B, T2, d), dtype=mel.dtype, device=mel.device)
        if grad_mode:
            pre2 = ops.linear_fwd(cols2, w2v, bias=b2)
            a2 = ops.act_fwd(pre2, 1)
            ops.add(a2, pos.contiguous().view(-1), out=out, period=T2 * d)
        else:
            pre2 = None
            ops.gemm_raw(cols2, w2v, out, T2, d, d * 3, ld2, d * 3, d, bias=b2, bias_mode=1, act=1,
                         R=pos, ldr=d, nb1=B, sA=(T2 * ld2, 0), sC=(T2 * d, 0), sR=(0, 0))
        if grad_mode:
            ctx.save_for_backward(cols1, pre1, cols2, pre2, w1v, w2v)
            ctx.dims = (B, Cm, Tm, d, L1, T2)
        return out

    @staticmethod
    def backward(ctx, dout):
        cols1, pre1, cols2, pre2, w1v, w2v = ctx.saved_tensors
        B, Cm, Tm, d, L1, T2 = ctx.dims
        need = ctx.needs_input_grad
        d2 = _c2(dout, B * T2, d)
        dpos = ops.colsum(_c2(dout, B, T2 * d)).view(T2, d) if need[5] else None
        dpre2 = ops.act_bwd(pre2, d2, 1)
        dw2 = ops.linear_dw(dpre2, cols2)[:, : d * 3].contiguous().view(d, d, 3) if need[3] else None
        db2 = ops.colsum(dpre2) if need[4] else None
        dcols2 = ops.linear_dx(dpre2, w2v)
        dh1 = ops.col2im1d(dcols2, B, d, L1, 3, 2, 1, T2, L1 * d, 1, d, (B * L1, d))
        dpre1 = ops.act_bwd(pre1, dh1, 1)
        dw1 = ops.linear_dw(dpre1, cols1)[:, : Cm * 3].contiguous().view(d, Cm, 3) if need[1] else None
        db1 = ops.colsum(dpre1) if need[2] else None
        dmel = None
        if need[0]:
            dcols1 = ops.linear_dx(dpre1, w1v)
            dmel = ops.col2im1d(dcols1, B, Cm, Tm, 3, 1, 1, L1, Cm * Tm, Tm, 1, (B, Cm, Tm))
        return dmel, dw1, db1, dw2, db2, dpos


class AddBroadcastFn(torch.autograd.Function):
    """x[B, L, h] + pe[L, h]  (add_positional_encoding, modeling.py:1108-1118)."""

    @staticmethod
    def forward(ctx, x, pe):
        B = x.shape[0]
        xc = _c2(x, B, x.numel() // B)
        out = ops.add(xc, pe.contiguous().view(-1), period=pe.numel())
        return out.view(x.shape)

    @staticmethod
    def backward(ctx, dout):
        return dout, None
