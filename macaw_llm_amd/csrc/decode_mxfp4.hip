// W4A16 decode linear: y[M <= 32][N] = prologue(x) dequant(Wq, e)^T (+ residual) with the weight streamed as OCP MXFP4
// (e2m1 codes, two per byte, one E8M0 power-of-two scale per 32 elements along K: the pair mk_mxfp4_quantize_rows
// writes) and widened to the 16-bit token type in registers by v_cvt_scalef32_pk_{bf16,f16}_fp4, which applies the
// block scale in the same instruction.  The next halving of the weight stream after mk_decode_linear_fp8
// (decode_fp8.hip); tokens, KV cache and the fp32 accumulation are unchanged: the token prologue and the cross-wave
// reduction are the same code (skinny16_parts.inc), the argument checks the same rule (common.h mk_decode_linear_plan).
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
  if (!e) return MK_ERR_BAD_ARG;
  bool wide;
  size_t lds;
  // a K-block is 64 weight bytes / 128 token elements and one dword of exponents
  if (const int rc = mk_decode_linear_plan(x, ldx, Wq, y, M, N, K, 128, prologue, norm_w, dtype, &wide, &lds)) return rc;
  // one 16-byte load of a weight row per K-block; the x rows of the SwiGLU form are [gate | up], 2 K elements
  if ((ldw % 16) || ldw < K / 2 || (lde % 4) || lde < K / 32 || ldx < (prologue == 2 ? 2 * (int64_t)K : (int64_t)K) ||
      ldy < N || (residual && ldr < N) || (reinterpret_cast<uintptr_t>(e) & 3))
    return MK_ERR_UNSUPPORTED;
  DecodeMxfp4Args g{};
  g.x = x; g.Wq = reinterpret_cast<const uint8_t*>(Wq); g.e = reinterpret_cast<const uint8_t*>(e); g.y = y;
  g.residual = residual;
  g.M = M; g.N = N; g.K = K;
  g.ldx = ldx; g.ldw = ldw; g.lde = lde; g.ldy = ldy; g.ldr = ldr;
  g.pro_w = norm_w; g.pro_eps = eps;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (dtype == MK_F16) e_f16::launch_decode_linear_mxfp4(g, prologue, wide, lds, st);
  else e_bf16::launch_decode_linear_mxfp4(g, prologue, wide, lds, st);
  return mk_check_launch();
}
