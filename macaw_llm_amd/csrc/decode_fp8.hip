// W8A16 decode linear: y[M <= 32][N] = prologue(x) (s * Wq)^T (+ residual) with the weight streamed as OCP e4m3
// bytes (one fp32 de-quantisation scale per output channel: the pair mk_fp8_quantize_rows writes) and widened to
// the 16-bit token type in registers.  A decode step reads every decoder weight once and little else, so the
// number of weight bytes is the first-order term of the token time; tokens, KV cache and the fp32 accumulation
// are those of mk_decode_linear (gemm.hip): the token prologue and the cross-wave reduction are the same code
// (skinny16_parts.inc), the argument checks the same rule (common.h mk_decode_linear_plan).
//
// Replaces: the nn.Linear call sites of a decode step (modeling.py:127-135,165-200) when generate() is asked
// for decode_weights="fp8".
#include "common.h"
#include "../../include/macaw_hip.h"

namespace {
struct DecodeFp8Args {
  const void* x; const uint8_t* Wq; const float* scale; void* y; const void* residual;
  int M, N, K;
  long ldx, ldw, ldy, ldr;
  const void* pro_w; float pro_eps;   // prologue 1: RMSNorm weight / eps
};
}  // namespace

#define MK_E16_T bf16
#define MK_E16_NS e_bf16
#include "decode_fp8_impl.inc"
#undef MK_E16_T
#undef MK_E16_NS
#define MK_E16_T _Float16
#define MK_E16_NS e_f16
#include "decode_fp8_impl.inc"
#undef MK_E16_T
#undef MK_E16_NS

extern "C" int mk_decode_linear_fp8(const void* x, int64_t ldx, const void* Wq, int64_t ldw, const float* scale,
                                    void* y, int64_t ldy, const void* residual, int64_t ldr, int32_t M,
                                    int32_t N, int32_t K, int32_t prologue, const void* norm_w, float eps,
                                    int32_t dtype, void* stream) {
  if (!scale) return MK_ERR_BAD_ARG;
  bool wide;
  size_t lds;
  // a K-block is 64 weight bytes / 64 token elements
  if (const int rc = mk_decode_linear_plan(x, ldx, Wq, y, M, N, K, 64, prologue, norm_w, dtype, &wide, &lds)) return rc;
  // one 16-byte load of a weight row per K-block; the x rows of the SwiGLU form are [gate | up], 2 K elements
  if ((ldw % 16) || ldw < K || ldx < (prologue == 2 ? 2 * (int64_t)K : (int64_t)K) || ldy < N || (residual && ldr < N) ||
      (reinterpret_cast<uintptr_t>(scale) & 3))
    return MK_ERR_UNSUPPORTED;
  DecodeFp8Args g{};
  g.x = x; g.Wq = reinterpret_cast<const uint8_t*>(Wq); g.scale = scale; g.y = y; g.residual = residual;
  g.M = M; g.N = N; g.K = K;
  g.ldx = ldx; g.ldw = ldw; g.ldy = ldy; g.ldr = ldr;
  g.pro_w = norm_w; g.pro_eps = eps;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (dtype == MK_F16) e_f16::launch_decode_linear_fp8(g, prologue, wide, lds, st);
  else e_bf16::launch_decode_linear_fp8(g, prologue, wide, lds, st);
  return mk_check_launch();
}
