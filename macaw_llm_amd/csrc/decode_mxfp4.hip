// W4A16 decode linear: y[M <= 32][N] = prologue(x) dequant(Wq, e)^T (+ residual) with the weight streamed as OCP MXFP4
// (e2m1 codes, two per byte, one E8M0 power-of-two scale per 32 elements along K: the pair mk_mxfp4_quantize_rows
// writes) and widened to the 16-bit token type in registers by v_cvt_scalef32_pk_{bf16,f16}_fp4, which applies the
// block scale in the same instruction.  The next halving of the weight stream after mk_decode_linear_fp8
// (decode_fp8.hip), whose kernel this one follows line by line; tokens, KV cache and the fp32 accumulation are unchanged.
//
// Replaces: the nn.Linear call sites of a decode step (modeling.py:127-135,165-200) when generate() is asked
// for decode_weights="mxfp4".
#include "common.h"
#include "../../include/macaw_hip.h"

namespace {
struct DecodeMxfp4Args {
  const void* x; const uint8_t* Wq; const uint8_t* e; void* y; const void* residual;
  int M, N, K;
  long ldx, ldw, lde, ldy, ldr;
  const void* pro_w; float pro_eps;   // prologue 1: RMSNorm weight / eps
};
bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
}  // namespace

#define MK_E16_T bf16
#define MK_E16_NS e_bf16
#include "decode_mxfp4_impl.inc"
#undef MK_E16_T
#undef MK_E16_NS
#define MK_E16_T _Float16
#define MK_E16_NS e_f16
#include "decode_mxfp4_impl.inc"
#undef MK_E16_T
#undef MK_E16_NS

extern "C" int mk_mxfp4_quantize_rows(const void* x, int32_t rows, int32_t cols, int64_t ld, int32_t dtype, void* q,
                                      int64_t ldq, void* e, int64_t lde, void* stream) {
  if (!x || !q || !e || rows <= 0 || cols <= 0) return MK_ERR_BAD_ARG;
  // one thread per block of 32: four 16-byte loads, one 16-byte store of codes, one exponent byte
  if ((dtype != MK_BF16 && dtype != MK_F16) || (cols % 32) || (ld % 8) || ld < cols || (ldq % 16) || ldq < cols / 2 ||
      lde < cols / 32 || !aligned16(x) || !aligned16(q))
    return MK_ERR_UNSUPPORTED;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  uint8_t* qp = reinterpret_cast<uint8_t*>(q);
  uint8_t* ep = reinterpret_cast<uint8_t*>(e);
  if (dtype == MK_F16) e_f16::launch_mxfp4_quantize_rows(x, rows, cols, ld, qp, ldq, ep, lde, st);
  else e_bf16::launch_mxfp4_quantize_rows(x, rows, cols, ld, qp, ldq, ep, lde, st);
  return mk_check_launch();
}

extern "C" int mk_decode_linear_mxfp4(const void* x, int64_t ldx, const void* Wq, int64_t ldw, const void* e,
                                      int64_t lde, void* y, int64_t ldy, const void* residual, int64_t ldr, int32_t M,
                                      int32_t N, int32_t K, int32_t prologue, const void* norm_w, float eps,
                                      int32_t dtype, void* stream) {
  if (!x || !Wq || !e || !y || M <= 0 || N <= 0 || K <= 0) return MK_ERR_BAD_ARG;
  if (prologue < 0 || prologue > 2 || (prologue == 1 && !norm_w)) return MK_ERR_BAD_ARG;
  // 16-byte loads of both operands: a K-block is 64 weight bytes / 128 token elements and one dword of exponents; the
  // x rows of the SwiGLU form are [gate | up], 2 K elements
  if ((dtype != MK_BF16 && dtype != MK_F16) || M > (prologue ? 16 : 32) || (K % 128) || (ldx % 8) || (ldw % 16) ||
      ldw < K / 2 || (lde % 4) || lde < K / 32 || ldx < (prologue == 2 ? 2 * (int64_t)K : (int64_t)K) || ldy < N ||
      (residual && ldr < N) || !aligned16(x) || !aligned16(Wq) || (reinterpret_cast<uintptr_t>(e) & 3) ||
      (prologue == 1 && !aligned16(norm_w)))
    return MK_ERR_UNSUPPORTED;
  const size_t lds = prologue ? (size_t)M * (K + 8) * 2 : 0;   // prepared token rows
  if (lds > 40 * 1024) return MK_ERR_UNSUPPORTED;   // (two workgroups per CU must still fit)
  DecodeMxfp4Args g{};
  g.x = x; g.Wq = reinterpret_cast<const uint8_t*>(Wq); g.e = reinterpret_cast<const uint8_t*>(e); g.y = y;
  g.residual = residual;
  g.M = M; g.N = N; g.K = K;
  g.ldx = ldx; g.ldw = ldw; g.lde = lde; g.ldy = ldy; g.ldr = ldr;
  g.pro_w = norm_w; g.pro_eps = eps;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const bool wide = N <= 16 * 256 && K <= 4096;     // as mk_decode_linear: 16 waves where N / 16 workgroups are few
  if (dtype == MK_F16) e_f16::launch_decode_linear_mxfp4(g, prologue, wide, lds, st);
  else e_bf16::launch_decode_linear_mxfp4(g, prologue, wide, lds, st);
  return mk_check_launch();
}
