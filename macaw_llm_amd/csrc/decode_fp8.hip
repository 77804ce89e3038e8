// W8A16 decode linear: y[M <= 32][N] = prologue(x) (s * Wq)^T (+ residual) with the weight streamed as OCP e4m3
// bytes (one fp32 de-quantisation scale per output channel: the pair mk_fp8_quantize_rows writes) and widened to
// the 16-bit token type in registers.  A decode step reads every decoder weight once and little else, so the
// number of weight bytes is the first-order term of the token time; tokens, KV cache and the fp32 accumulation
// are those of mk_decode_linear (gemm.hip), whose kernel this one follows line by line.
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
bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
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
  if (!x || !Wq || !scale || !y || M <= 0 || N <= 0 || K <= 0) return MK_ERR_BAD_ARG;
  if (prologue < 0 || prologue > 2 || (prologue == 1 && !norm_w)) return MK_ERR_BAD_ARG;
  // 16-byte loads of both operands: a K-block is 64 weight bytes / 64 token elements; the x rows of the SwiGLU
  // form are [gate | up], 2 K elements
  if ((dtype != MK_BF16 && dtype != MK_F16) || M > (prologue ? 16 : 32) || (K % 64) || (ldx % 8) || (ldw % 16) ||
      ldw < K || ldx < (prologue == 2 ? 2 * (int64_t)K : (int64_t)K) || ldy < N || (residual && ldr < N) ||
      !aligned16(x) || !aligned16(Wq) || (reinterpret_cast<uintptr_t>(scale) & 3) ||
      (prologue == 1 && !aligned16(norm_w)))
    return MK_ERR_UNSUPPORTED;
  const size_t lds = prologue ? (size_t)M * (K + 8) * 2 : 0;   // prepared token rows
  if (lds > 40 * 1024) return MK_ERR_UNSUPPORTED;   // (two workgroups per CU must still fit)
  DecodeFp8Args g{};
  g.x = x; g.Wq = reinterpret_cast<const uint8_t*>(Wq); g.scale = scale; g.y = y; g.residual = residual;
  g.M = M; g.N = N; g.K = K;
  g.ldx = ldx; g.ldw = ldw; g.ldy = ldy; g.ldr = ldr;
  g.pro_w = norm_w; g.pro_eps = eps;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const bool wide = N <= 16 * 256 && K <= 4096;     // as mk_decode_linear: 16 waves where N / 16 workgroups are few
  if (dtype == MK_F16) e_f16::launch_decode_linear_fp8(g, prologue, wide, lds, st);
  else e_bf16::launch_decode_linear_fp8(g, prologue, wide, lds, st);
  return mk_check_launch();
}
