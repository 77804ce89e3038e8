// Classifier-free guidance for generate(guidance_scale=s): the launch that combines the two rows of logits a guided
// step scores per sample -- row b on the caller's prompt (c), row B + b on the negative prompt (u) -- into
//   g = lu + s * (lc - lu),   lc = c - lse(c),   lu = u - lse(u)
// and stores g into row b, in place, with nothing handed to the host (the rule is written down in include/macaw_hip.h
// under "Classifier-free guidance" and restated in tests/cfg_ref.py).  It stands between the lm_head and the logits
// processors / the emit of a captured step.
//
// One workgroup of 1024 threads per sample, two passes over its two rows:
//   pass 1   an online maximum and sum of both rows in one read.  A thread owns the 16-byte vectors t, t + 1024, ... of
//            a row (the columns behind the last whole vector one by one; every column one by one where the row base or
//            the pitch is not a multiple of 16 bytes).  Per vector: the fp32 maximum of its columns that are neither
//            NaN nor -inf; when it raises the thread's maximum the thread's sum is rescaled by exp(old - new) in fp64;
//            then the sum takes expf(x - max) of every such column, expf in fp32, accumulated in fp64 (logprobs.hip's
//            arithmetic).  The block's maximum is the wave_max / wave-order maximum of the threads'; every thread then
//            rescales its sum to it (fp64 exp) and the sums are added in a fixed order: lane tree, then wave order.
//            lse = (double)max + log(sum), kept in fp64.  A row with no finite logit or with +inf is degenerate.
//   pass 2   the same thread re-reads the same vectors (from L2), combines in fp64 and stores row b with ONE rounding
//            to the logits' type (g_f32).
// Rows [B, 2B), the columns [V, ld) and everything else are never written; columns [V, ld) are never read.
#include "common.h"
#include "../../include/macaw_hip.h"
#include <math.h>

namespace {

constexpr int GNT = 1024;                       // threads per sample

MK_DEV bool g_logit_ok(float v) { return !__builtin_isnan(v) && v != -INFINITY; }
MK_DEV bool g_finite(float v) { return fabsf(v) < INFINITY; }     // false for NaN

// fp64 -> the fp32 value whose conversion to T (round to nearest even, from_f32 / VecIO::store) is the SINGLE rounding of
// the fp64 value to T: for fp32 the rounding itself; for the 16-bit types fp64 -> fp32 rounded to odd (the fp32 grid is 13
// / 16 bits finer, so the second rounding sees exactly which side of a tie the fp64 value lay on)
template <typename T> MK_DEV float g_f32(double d) {
  float f = (float)d;
  if constexpr (sizeof(T) == 4) return f;
  const double back = (double)f;
  if (d == d && back != d) {                    // inexact
    uint32_t u = __float_as_uint(f);
    if (fabs(back) > fabs(d)) u -= 1;           // rounded away from zero (or to inf): one step back towards zero
    f = __uint_as_float(u | 1u);
  }
  return f;
}

// the running (maximum, sum of exp(x - maximum)) of the columns a thread has seen
struct Run {
  float m; double s;
  template <int N> MK_DEV void take(const float (&v)[N]) {
    float cm = -INFINITY;
#pragma unroll
    for (int k = 0; k < N; ++k)
      if (g_logit_ok(v[k])) cm = fmaxf(cm, v[k]);
    if (cm > m) {                               // (m == -inf: s is 0 and stays 0)
      s *= exp((double)m - (double)cm);
      m = cm;
    }
#pragma unroll
    for (int k = 0; k < N; ++k)
      if (g_logit_ok(v[k])) s += (double)expf(v[k] - m);
  }
};

struct CfgLds {
  float wmax[2][GNT / 64];
  double wsum[2][GNT / 64];
};

// rule 2 - 4 for one column: the stored values c, u and the rows' lse (ok: the row is not degenerate)
MK_DEV double g_combine(float c, float u, double lse_c, double lse_u, bool ok_c, bool ok_u, double s) {
  const double nan = __builtin_nan("");
  const double lc = ok_c ? (double)c - lse_c : nan;
  const double lu = ok_u ? (double)u - lse_u : nan;
  if (lc == -(double)INFINITY || lu == -(double)INFINITY) return lc;
  return lu + s * (lc - lu);
}

template <typename T>
__global__ __launch_bounds__(GNT) void cfg_combine_kernel(T* logits, long ld, int V, int B, float scale) {
  __shared__ CfgLds sh;
  constexpr int N = VecIO<T>::N;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  T* xc = logits + (long)b * ld;
  const T* xu = logits + ((long)B + b) * ld;
  // whole 16-byte vectors: both row bases and the pitch are multiples of 16 bytes (uniform over the grid)
  const bool vec = ((uintptr_t)logits % 16 == 0) && ((ld * (long)sizeof(T)) % 16 == 0);
  const int nvec = vec ? V / N : 0;

  // ---- pass 1: online maximum and sum of both rows
  Run rc = {-INFINITY, 0.0}, ru = {-INFINITY, 0.0};
  for (int i = tid; i < nvec; i += GNT) {
    float c[N], u[N];
    VecIO<T>::load(xc + (long)i * N, c);
    VecIO<T>::load(xu + (long)i * N, u);
    rc.take(c);
    ru.take(u);
  }
  for (int col = nvec * N + tid; col < V; col += GNT) {
    const float c[1] = {to_f32<T>(xc[col])}, u[1] = {to_f32<T>(xu[col])};
    rc.take(c);
    ru.take(u);
  }
  float mc = wave_max(rc.m), mu = wave_max(ru.m);
  if (lane == 0) { sh.wmax[0][wave] = mc; sh.wmax[1][wave] = mu; }
  __syncthreads();
  mc = sh.wmax[0][0]; mu = sh.wmax[1][0];
#pragma unroll
  for (int w = 1; w < GNT / 64; ++w) { mc = fmaxf(mc, sh.wmax[0][w]); mu = fmaxf(mu, sh.wmax[1][w]); }
  const bool ok_c = g_finite(mc), ok_u = g_finite(mu);      // false: no finite logit, or a +inf: a degenerate row
  double sc = ok_c && rc.m != -INFINITY ? rc.s * exp((double)rc.m - (double)mc) : 0.0;
  double su = ok_u && ru.m != -INFINITY ? ru.s * exp((double)ru.m - (double)mu) : 0.0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { sc += __shfl_xor(sc, o, 64); su += __shfl_xor(su, o, 64); }
  if (lane == 0) { sh.wsum[0][wave] = sc; sh.wsum[1][wave] = su; }
  __syncthreads();
  sc = sh.wsum[0][0]; su = sh.wsum[1][0];
#pragma unroll
  for (int w = 1; w < GNT / 64; ++w) { sc += sh.wsum[0][w]; su += sh.wsum[1][w]; }
  const double lse_c = ok_c ? (double)mc + log(sc) : 0.0, lse_u = ok_u ? (double)mu + log(su) : 0.0;
  const double s = (double)scale;

  // ---- pass 2: combine and store row b (every thread its own columns again: read before written)
  for (int i = tid; i < nvec; i += GNT) {
    float c[N], u[N];
    VecIO<T>::load(xc + (long)i * N, c);
    VecIO<T>::load(xu + (long)i * N, u);
    float g[N];
#pragma unroll
    for (int k = 0; k < N; ++k) g[k] = g_f32<T>(g_combine(c[k], u[k], lse_c, lse_u, ok_c, ok_u, s));
    VecIO<T>::store(xc + (long)i * N, g);
  }
  for (int col = nvec * N + tid; col < V; col += GNT)
    xc[col] = from_f32<T>(g_f32<T>(g_combine(to_f32<T>(xc[col]), to_f32<T>(xu[col]), lse_c, lse_u, ok_c, ok_u, s)));
}

}  // namespace

extern "C" int mk_cfg_combine(void* logits, int64_t ld, int32_t V, int32_t B, float scale, int32_t dtype, void* stream) {
  if (!logits || B < 1 || V < 1 || ld < V || !(fabsf(scale) < INFINITY) ||
      (dtype != MK_BF16 && dtype != MK_F16 && dtype != MK_F32))
    return MK_ERR_BAD_ARG;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (dtype == MK_BF16) MK_LAUNCH((cfg_combine_kernel<bf16>), dim3(B), dim3(GNT), 0, st, (bf16*)logits, (long)ld, V, B, scale);
  else if (dtype == MK_F16)
    MK_LAUNCH((cfg_combine_kernel<_Float16>), dim3(B), dim3(GNT), 0, st, (_Float16*)logits, (long)ld, V, B, scale);
  else MK_LAUNCH((cfg_combine_kernel<float>), dim3(B), dim3(GNT), 0, st, (float*)logits, (long)ld, V, B, scale);
  return mk_check_launch();
}
