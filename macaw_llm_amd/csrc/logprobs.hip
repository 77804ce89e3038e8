// Token log-probabilities for generate(return_logprobs=True, top_logprobs=n): the log-softmax value of the token a step
// selected, and the n most likely columns with theirs, in one launch with nothing handed to the host (the stand-alone
// twin of mk_argmax_rows, softmax.hip, and the kernel that rides behind mk_decode_emit / mk_decode_emit_sample in the
// captured step; the rule is written down in include/macaw_hip.h and restated in tests/logprobs_ref.py).
//
// One workgroup of 1024 threads per row; thread t owns the columns t, t + 1024, ... (coalesced), the row is re-read from
// L2 for every pass, and "lower column first" is decided by comparing columns, never by the order of arrival:
//   lse      fp32 maximum over the columns that are neither NaN nor -inf; the sum of expf(x - max) accumulated in fp64 in
//            a fixed order (thread, lane tree, wave order); lse = (double)max + log(sum), kept in fp64 (beam.hip's rule)
//   logprob  (float)((double)x_c - lse): one rounding.  A row without a finite logit, or with +inf in it, is degenerate:
//            every value is NaN
//   key      the order-preserving uint32 image of x_c (sample.hip's s_key, -0 folded into +0); NaN columns have no key
//   floor    every thread's best key; the n-th largest of those 1024 keys is a lower bound of the n-th largest key of the
//            row (n distinct columns reach it), so the passes below skip nearly every column
//   select   the 8-bit-per-pass radix select (256-bin LDS histogram of counts) for the n-th largest key Kt and how many
//            of its tie group are still admitted, r; when r cuts the tie group, a second select over the inverted column
//            picks its r lowest members
//   order    the <= n winners are ranked by (key descending, column ascending) in LDS and written in that order
// The select is this file's own copy of beam.hip's (their code objects stay as they are).
#include "common.h"
#include "../../include/macaw_hip.h"
#include <math.h>

namespace {

typedef uint32_t u32;
constexpr int LNT = 1024;                       // threads per row
constexpr int LTM = 20;                         // most top columns
constexpr int LCM = 32;                         // slots of the winners' lists
constexpr int LP_MAX_V = 1 << 23;

struct LpLds {
  u32 hist[256];
  int digit;
  u32 above, tie;                               // radix select: weight above the digit found / weight of the digit
  float wmax[LNT / 64];
  double wsum[LNT / 64];
  int cn;
  u32 ckey[LCM], cidx[LCM], sidx[LCM];
  int was, col;
};

MK_DEV bool l_logit_ok(float v) { return !__builtin_isnan(v) && v != -INFINITY; }
MK_DEV bool l_finite(float v) { return fabsf(v) < INFINITY; }     // false for NaN
MK_DEV u32 l_key(float x) {
  if (x == 0.f) x = 0.f;                        // -0 == +0: one key
  const u32 u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// Radix select over the keys `each` enumerates (every thread its own; all keys non-zero), each of weight 1: the key Kt
// with #(keys > Kt) < target <= #(keys >= Kt), rem = target - #(keys > Kt) and tie = #(keys == Kt).  False (uniformly)
// when fewer than target keys exist.
template <typename Each>
__device__ bool l_radix_select(Each each, u32 target, LpLds& s, u32& Kt, u32& rem, u32& tie) {
  const int tid = threadIdx.x;
  u32 prefix = 0;
  for (int shift = 24; shift >= 0; shift -= 8) {
    const u32 himask = shift == 24 ? 0u : (0xffffffffu << (shift + 8));
    __syncthreads();
    if (tid < 256) s.hist[tid] = 0;
    if (tid == 0) s.digit = -1;
    __syncthreads();
    each([&](u32 k) {
      if ((k & himask) == prefix) atomicAdd(&s.hist[(k >> shift) & 255u], 1u);
    });
    __syncthreads();
    if (tid < 64) {                             // lane l scans bins 255 - 4l ... 252 - 4l, the larger digits first
      u32 h[4], sum = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) { h[j] = s.hist[255 - 4 * tid - j]; sum += h[j]; }
      u32 inc = sum;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const u32 t = __shfl_up(inc, o, 64);
        if (tid >= o) inc += t;
      }
      u32 run = inc - sum;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (run < target && target <= run + h[j]) { s.digit = 255 - 4 * tid - j; s.above = run; s.tie = h[j]; }
        run += h[j];
      }
    }
    __syncthreads();
    const int d = s.digit;
    if (d < 0) return false;
    prefix |= (u32)d << shift;
    target -= s.above;
  }
  Kt = prefix;
  rem = target;
  tie = s.tie;                                  // the last pass fixed all 32 bits: its bin holds the keys == Kt
  return true;
}

struct LpArgs {
  const void* logits; long ld; int V, n_top;
  const int64_t* ids;                           // the selected token per row (the step form: tok)
  float* lp; int64_t* top_ids; float* top_lp;
  // the step form (state != nullptr): column state[1] - 1 of matrices of n_max columns at pitch lp_ld
  const unsigned char* done; const int32_t* state; unsigned char* fin;
  long pad, lp_ld; int n_max;
};

template <typename T>
__global__ __launch_bounds__(LNT) void token_logprobs_kernel(LpArgs a) {
  __shared__ LpLds s;
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int V = a.V, n = a.n_top;
  long at = r;                                  // the element of lp, the row of top_ids / top_lp
  if (a.state) {
    if (tid == 0) {                             // the latch: finished BEFORE this step; then it follows done
      s.was = a.fin[r];
      s.col = a.state[1] - 1;
      a.fin[r] = a.done[r];
    }
    __syncthreads();
    const int col = s.col;
    if (col < 0 || col >= a.n_max) return;
    at = (long)r * a.lp_ld + col;
    if (s.was) {
      if (tid == 0) a.lp[at] = 0.f;
      if (tid < n) { a.top_ids[at * n + tid] = a.pad; a.top_lp[at * n + tid] = 0.f; }
      return;
    }
  }
  const T* xr = (const T*)a.logits + (long)r * a.ld;

  // ---- maximum, every thread's best key
  float m = -INFINITY;
  u32 best = 0;
  for (int c = tid; c < V; c += LNT) {
    const float v = to_f32<T>(xr[c]);
    if (l_logit_ok(v)) m = fmaxf(m, v);
    if (!__builtin_isnan(v)) best = max(best, l_key(v));
  }
  m = wave_max(m);
  if (lane == 0) s.wmax[wave] = m;
  if (tid == 0) s.cn = 0;
  __syncthreads();
  m = s.wmax[0];
#pragma unroll
  for (int w = 1; w < LNT / 64; ++w) m = fmaxf(m, s.wmax[w]);
  // ---- the fp64 sum of expf(x - max): a thread's own columns, the lane tree, wave order
  const bool ok = l_finite(m);                  // false: no finite logit, or a +inf: a degenerate row
  double sum = 0.0;
  if (ok) {
    for (int c = tid; c < V; c += LNT) {
      const float v = to_f32<T>(xr[c]);
      if (l_logit_ok(v)) sum += (double)expf(v - m);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
  if (lane == 0) s.wsum[wave] = sum;
  __syncthreads();
  sum = s.wsum[0];
#pragma unroll
  for (int w = 1; w < LNT / 64; ++w) sum += s.wsum[w];
  const double lse = ok ? (double)m + log(sum) : 0.0;
  auto logprob = [&](int c) -> float {
    const float v = to_f32<T>(xr[c]);
    return ok ? (float)((double)v - lse) : __builtin_nanf("");
  };
  if (tid == 0) {
    const int64_t id = a.ids[r];
    a.lp[at] = id >= 0 && id < (int64_t)V ? logprob((int)id) : __builtin_nanf("");
  }
  if (n <= 0) return;

  // ---- the n largest keys, ties to the lower column
  auto each = [&](auto&& f) {
    for (int c = tid; c < V; c += LNT) {
      const float v = to_f32<T>(xr[c]);
      if (!__builtin_isnan(v)) f(l_key(v), (u32)c);
    }
  };
  const u32 want = (u32)n;
  u32 floor_k = 1, rem = 0, tie = 0;
  if (!l_radix_select([&](auto&& f) { if (best) f(best); }, want, s, floor_k, rem, tie)) floor_k = 1;
  u32 Kt = 0;
  const bool full = l_radix_select([&](auto&& f) { each([&](u32 k, u32) { if (k >= floor_k) f(k); }); }, want, s, Kt,
                                   rem, tie);
  u32 imax = 0xffffffffu;                       // admitted members of the tie group: column <= imax
  if (!full) {
    Kt = 0;                                     // fewer than n keys: all of them (no key is 0)
  } else if (rem < tie) {                       // the r = rem lowest columns of the tie group
    u32 It = 0, r2 = 0, t2 = 0;
    l_radix_select([&](auto&& f) { each([&](u32 k, u32 i) { if (k == Kt) f(~i); }); }, rem, s, It, r2, t2);
    imax = ~It;
  }
  // ---- gather the winners, rank them by (key descending, column ascending)
  each([&](u32 k, u32 i) {
    if (k > Kt || (full && k == Kt && i <= imax)) {
      const int p = atomicAdd(&s.cn, 1);
      if (p < LCM) { s.ckey[p] = k; s.cidx[p] = i; }
    }
  });
  __syncthreads();
  const int got = min(s.cn, n);
  if (tid < got) {
    const u32 k = s.ckey[tid], i = s.cidx[tid];
    int rank = 0;
    for (int j = 0; j < got; ++j) rank += s.ckey[j] > k || (s.ckey[j] == k && s.cidx[j] < i);
    s.sidx[rank] = i;
  }
  __syncthreads();
  if (tid < n) {
    const bool have = tid < got;
    a.top_ids[at * n + tid] = have ? (int64_t)s.sidx[tid] : (int64_t)-1;
    a.top_lp[at * n + tid] = have ? logprob((int)s.sidx[tid]) : -INFINITY;
  }
}

int launch(const LpArgs& a, int rows, int dtype, void* stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (dtype == MK_BF16) MK_LAUNCH((token_logprobs_kernel<bf16>), dim3(rows), dim3(LNT), 0, st, a);
  else if (dtype == MK_F16) MK_LAUNCH((token_logprobs_kernel<_Float16>), dim3(rows), dim3(LNT), 0, st, a);
  else MK_LAUNCH((token_logprobs_kernel<float>), dim3(rows), dim3(LNT), 0, st, a);
  return mk_check_launch();
}

}  // namespace

extern "C" int mk_token_logprobs(const void* logits, int64_t ld, int32_t rows, int32_t V, const int64_t* ids,
                                 int32_t n_top, float* lp, int64_t* top_ids, float* top_lp, int32_t dtype,
                                 void* stream) {
  if (!logits || !ids || !lp || rows <= 0 || V <= 0 || ld < V || n_top < 0 || (n_top > 0 && (!top_ids || !top_lp)))
    return MK_ERR_BAD_ARG;
  if (n_top > LTM || V > LP_MAX_V || (dtype != MK_BF16 && dtype != MK_F16 && dtype != MK_F32)) return MK_ERR_UNSUPPORTED;
  LpArgs a = {};
  a.logits = logits; a.ld = (long)ld; a.V = V; a.n_top = n_top; a.ids = ids;
  a.lp = lp; a.top_ids = top_ids; a.top_lp = top_lp;
  return launch(a, rows, dtype, stream);
}

extern "C" int mk_decode_emit_logprobs(const void* logits, int64_t ld, int32_t V, int32_t B, int64_t pad,
                                       const int64_t* tok, const void* done, const int32_t* state, void* fin,
                                       int32_t n_max, int32_t n_top, float* lp, int64_t lp_ld, int64_t* top_ids,
                                       float* top_lp, int32_t dtype, void* stream) {
  if (!logits || !tok || !done || !state || !fin || !lp || B <= 0 || V <= 0 || ld < V || n_top < 0 || n_max < 0 ||
      lp_ld < n_max || (n_top > 0 && (!top_ids || !top_lp)))
    return MK_ERR_BAD_ARG;
  if (n_top > LTM || V > LP_MAX_V || (dtype != MK_BF16 && dtype != MK_F16 && dtype != MK_F32)) return MK_ERR_UNSUPPORTED;
  LpArgs a = {};
  a.logits = logits; a.ld = (long)ld; a.V = V; a.n_top = n_top; a.ids = tok;
  a.lp = lp; a.top_ids = top_ids; a.top_lp = top_lp;
  a.done = (const unsigned char*)done; a.state = state; a.fin = (unsigned char*)fin;
  a.pad = (long)pad; a.lp_ld = (long)lp_ld; a.n_max = n_max;
  return launch(a, B, dtype, stream);
}
