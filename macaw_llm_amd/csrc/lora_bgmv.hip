// Mixed-adapter LoRA for the decode step (engine._stream_linear, lora.AdapterBank): every token row m carries its own
// adapter idx[m], so one batch serves several adapters, or an adapter next to the base model (idx outside the bank).
// Two launches per projection group (the G <= 3 modules that share an input), around the unchanged base launch:
//
//   shrink   U[m, c] = rnd16( sum_k p(x)[m, k] A[idx[m]][c, k] )                       c < G r
//   expand   Y[m, i N + n] = rnd16( Y[m, i N + n] + s[idx[m]] sum_j U[m, i r + j] B[idx[m]][i N + n, j] )
//
// A [n_adapters, G r, K] and B [n_adapters, G N, r] are the bank's stacks (the group's matrices row-concatenated, one
// slab per adapter, ranks below r and untargeted modules zero-filled), s f32 [n_adapters], idx int32 [M] on the device.
// p is the token prologue of the skinny16 stream kernels (skinny16_parts.inc, reused: 0 none, 1 RMSNorm, 2 SwiGLU), so
// that the adapter sees the tokens the base launch sees, bit for bit.
//
// Both are latency-bound streams over a few hundred KB per distinct adapter (served from L2 where rows share one); the
// rank-r products are too small for a tile of rows to share an MFMA operand when every row may name another adapter.
// So a workgroup owns ONE row: fp32 FMAs on 16-byte loads, a wave-level xor reduction in shrink, a serial j loop in
// expand.  Every sum runs in an order fixed by (K, r) alone: a row's bits do not depend on M or on the other rows, and
// there are no float atomics.
#include "common.h"
#include "../../include/macaw_hip.h"
#include "skinny16_parts.inc"

namespace {

constexpr int BGMV_NW = 4;        // waves per workgroup: the RMSNorm sum of squares then runs in rmsnorm_fwd_kernel's order
constexpr int BGMV_CW = 2;        // shrink: columns of U a wave computes at a time
constexpr int BGMV_CB = BGMV_NW * BGMV_CW;   // shrink: columns of U per workgroup
constexpr int BGMV_MAX_M = 32;

template <typename T> using x8_t = typename E16<T>::x8;

// grid (ceil(G r / BGMV_CB), M).  The row p(x)[m, :] is prepared into LDS ([K + 8] T) by skinny16_stage_tokens at
// M = 1, or copied there (PRO 0); wave w then owns columns c0 + BGMV_CW w ... of U: lane l holds elements
// k = 8 l + 512 t of every K block t, sums its own products in ascending k and the 64 lanes join in a xor tree.
template <typename T, int PRO>
__global__ __launch_bounds__(BGMV_NW * 64) void lora_bgmv_shrink_kernel(const T* X, long ldx, int K, const T* A, int n_ad,
                                                                       int GR, const int* idx, const void* pro_w,
                                                                       float pro_eps, T* U, long ldu) {
  extern __shared__ __attribute__((aligned(16))) char sk_smem[];
  __shared__ float ssq[BGMV_NW][16];
  const int l = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int m = blockIdx.y, c0 = blockIdx.x * BGMV_CB + w * BGMV_CW;
  const int ad = idx[m];
  if (ad < 0 || ad >= n_ad) {       // (uniform over the workgroup) a base row: a zero row of U, no adapter memory read
    if (threadIdx.x < BGMV_CB && blockIdx.x * BGMV_CB + threadIdx.x < GR)
      U[(long)m * ldu + blockIdx.x * BGMV_CB + threadIdx.x] = (T)0.f;
    return;
  }
  const T* xr = X + (long)m * ldx;
  T* ts = reinterpret_cast<T*>(sk_smem);
  if constexpr (PRO == 0) {
    for (int c = threadIdx.x; c < K / 8; c += BGMV_NW * 64)
      *reinterpret_cast<x8_t<T>*>(ts + c * 8) = *reinterpret_cast<const x8_t<T>*>(xr + c * 8);
    __syncthreads();
  } else {
    skinny16_stage_tokens<BGMV_NW, PRO>(xr, ldx, 1, K, pro_w, pro_eps, sk_smem, ssq, l, w);
  }
  const T* Ar = A + ((long)ad * GR + c0) * K;
  float acc[BGMV_CW];
#pragma unroll
  for (int i = 0; i < BGMV_CW; ++i) acc[i] = 0.f;
  for (int k = 8 * l; k < K; k += 512) {
    const x8_t<T> xv = *reinterpret_cast<const x8_t<T>*>(ts + k);
#pragma unroll
    for (int i = 0; i < BGMV_CW; ++i) {
      if (c0 + i < GR) {              // (uniform over the wave)
        const x8_t<T> av = *reinterpret_cast<const x8_t<T>*>(Ar + (long)i * K + k);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[i] = fmaf((float)xv[e], (float)av[e], acc[i]);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < BGMV_CW; ++i) {
    const float v = wave_sum(acc[i]);
    if (l == 0 && c0 + i < GR) U[(long)m * ldu + c0 + i] = (T)v;
  }
}

// grid (ceil(G N / 256), M): thread t owns output column col = i N + n of row m; the row of U sits in LDS as fp32 and
// the r products are summed in ascending j.  Adjacent threads read adjacent rows of B (r contiguous elements each).
template <typename T>
__global__ __launch_bounds__(256) void lora_bgmv_expand_kernel(const T* U, long ldu, int G, int r, const T* B,
                                                               const float* s, int n_ad, const int* idx, T* Y, long ldy,
                                                               int N) {
  __shared__ float us[3 * 128];
  const int m = blockIdx.y;
  const int ad = idx[m];
  if (ad < 0 || ad >= n_ad) return;     // (uniform over the workgroup) a base row keeps the base launch's bytes
  for (int c = threadIdx.x; c < G * r; c += 256) us[c] = (float)U[(long)m * ldu + c];
  __syncthreads();
  const int col = blockIdx.x * 256 + threadIdx.x;
  if (col >= G * N) return;
  const int i = col / N;
  const T* br = B + ((long)ad * G * N + col) * r;
  const float* ur = us + i * r;
  float acc = 0.f;
  for (int j = 0; j < r; j += 8) {
    const x8_t<T> bv = *reinterpret_cast<const x8_t<T>*>(br + j);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc = fmaf(ur[j + e], (float)bv[e], acc);
  }
  if (acc == 0.f) return;                // (a zero-filled module or rank: not even a -0 of the base launch changes)
  T* y = Y + (long)m * ldy + col;
  *y = (T)fmaf(s[ad], acc, (float)*y);
}

bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
bool rank_ok(int r) { return r >= 8 && r <= 128 && r % 8 == 0; }

template <typename T>
int shrink_t(const void* X, long ldx, int M, int K, const void* A, int n_ad, int GR, const int* idx, int pro,
             const void* pro_w, float eps, void* U, long ldu, hipStream_t st) {
  const dim3 grid((unsigned)((GR + BGMV_CB - 1) / BGMV_CB), (unsigned)M), block(BGMV_NW * 64);
  const size_t lds = (size_t)(K + 8) * 2;
#define BGMV_SHRINK(P)                                                                                              \
  MK_LAUNCH((lora_bgmv_shrink_kernel<T, P>), grid, block, lds, st, (const T*)X, ldx, K, (const T*)A, n_ad, GR, idx, \
            pro_w, eps, (T*)U, ldu)
  if (pro == 0) BGMV_SHRINK(0);
  else if (pro == 1) BGMV_SHRINK(1);
  else BGMV_SHRINK(2);
#undef BGMV_SHRINK
  return mk_check_launch();
}

template <typename T>
int expand_t(const void* U, long ldu, int M, int G, int r, const void* B, const float* s, int n_ad, const int* idx,
             void* Y, long ldy, int N, hipStream_t st) {
  const dim3 grid((unsigned)(((long)G * N + 255) / 256), (unsigned)M);
  MK_LAUNCH((lora_bgmv_expand_kernel<T>), grid, dim3(256), 0, st, (const T*)U, ldu, G, r, (const T*)B, s, n_ad, idx,
            (T*)Y, ldy, N);
  return mk_check_launch();
}

}  // namespace

#define MK_ST reinterpret_cast<hipStream_t>(stream)

extern "C" int mk_lora_bgmv_shrink(const void* X, int64_t ldx, int32_t M, int32_t K, const void* A, int32_t n_adapters,
                                   int32_t G, int32_t r, const int32_t* idx, int32_t prologue, const void* norm_w,
                                   float eps, void* U, int64_t ldu, int32_t dtype, void* stream) {
  if (!X || !A || !idx || !U || M <= 0 || K <= 0 || n_adapters <= 0 || G < 1 || G > 3 || !rank_ok(r) || prologue < 0 ||
      prologue > 2 || (prologue == 1 && !norm_w) || ldx < (prologue == 2 ? 2 * (int64_t)K : (int64_t)K) ||
      ldu < (int64_t)G * r)
    return MK_ERR_BAD_ARG;
  if ((dtype != MK_BF16 && dtype != MK_F16) || M > BGMV_MAX_M || K % 8 || ldx % 8 || ldu % 8 || !al16(X) || !al16(A) ||
      !al16(U) || (prologue == 1 && !al16(norm_w)) || (size_t)(K + 8) * 2 > 60 * 1024)
    return MK_ERR_UNSUPPORTED;
  const int prof = mkp::begin(MK_ST, 4, 2.0 * M * K * G * r, M, G * r, K, 1, 5, prologue);
  int rc;
  if (dtype == MK_BF16) rc = shrink_t<bf16>(X, ldx, M, K, A, n_adapters, G * r, idx, prologue, norm_w, eps, U, ldu, MK_ST);
  else rc = shrink_t<_Float16>(X, ldx, M, K, A, n_adapters, G * r, idx, prologue, norm_w, eps, U, ldu, MK_ST);
  mkp::end(prof, MK_ST);
  return rc;
}

extern "C" int mk_lora_bgmv_expand(const void* U, int64_t ldu, int32_t M, int32_t G, int32_t r, const void* B,
                                   const float* s, int32_t n_adapters, const int32_t* idx, void* Y, int64_t ldy,
                                   int32_t N, int32_t dtype, void* stream) {
  if (!U || !B || !s || !idx || !Y || M <= 0 || N <= 0 || n_adapters <= 0 || G < 1 || G > 3 || !rank_ok(r) ||
      ldu < (int64_t)G * r || ldy < (int64_t)G * N)
    return MK_ERR_BAD_ARG;
  if ((dtype != MK_BF16 && dtype != MK_F16) || M > BGMV_MAX_M || N % 8 || ldu % 8 || ldy % 8 || !al16(U) || !al16(B) ||
      !al16(Y))
    return MK_ERR_UNSUPPORTED;
  const int prof = mkp::begin(MK_ST, 4, 2.0 * M * N * G * r, M, N * G, r, 1, 6, 0);
  int rc;
  if (dtype == MK_BF16) rc = expand_t<bf16>(U, ldu, M, G, r, B, s, n_adapters, idx, Y, ldy, N, MK_ST);
  else rc = expand_t<_Float16>(U, ldu, M, G, r, B, s, n_adapters, idx, Y, ldy, N, MK_ST);
  mkp::end(prof, MK_ST);
  return rc;
}
