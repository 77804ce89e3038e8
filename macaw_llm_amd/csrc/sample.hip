// Sampled token selection for generate(do_sample=True): temperature, top-k, top-p and the draw of one token per row
// of logits, in one launch with the randomness on the device (the sampled twins of mk_argmax_rows, softmax.hip, and
// mk_decode_emit, decode.hip; HF's TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper -> multinomial).
//
// One workgroup of 1024 threads per row; thread t owns the contiguous columns [t * ch, (t + 1) * ch), ch = ceil(V / 1024),
// so that "in column order" is "in thread order, then along the chunk".  The row is re-read from L2 for every pass.
//
// Everything is exact or integer, hence bitwise reproducible whatever the arrival order:
//   value    x_c = float(logit_c) / temperature; columns whose logit is NaN or -inf are never candidates
//   key      the order-preserving uint32 image of x_c (-0 folded into +0): larger key <=> larger value
//   mass     m_c = trunc(exp(x_c - x_max) * 2^40) as a 64-bit integer (x_max has mass 2^40 exactly): sums of masses are
//            integer sums, added with 64-bit LDS atomics or in a blocked scan, no float atomics
//   select   an 8-bit-per-pass radix select over the keys with a 256-bin LDS histogram of 64-bit integers: of counts for
//            top-k (the k-th largest key Kt and how many columns of its tie group are still admitted, r), of masses for
//            top-p (the last key whose mass strictly above it is below p * Z)
//   kept     key > Kt, or key == Kt and fewer than r columns of that key lie to the left (ties to the lower column)
//   draw     u = ((mk_hash32(seed, step << 32 | row) >> 8) + 0.5) * 2^-24; the first kept column whose inclusive
//            cumulative mass exceeds u * Z_kept, compared in integers: cum * 2^25 > (2 h + 1) * Z_kept
#include "common.h"
#include "../../include/macaw_hip.h"
#include <math.h>

namespace {

typedef unsigned long long u64;
constexpr int SNT = 1024;                       // threads per row
constexpr u64 S_ALL = ~0ull;                    // r: the whole tie group of Kt is kept
constexpr u64 S_NONE = ~0ull;                   // radix select: no digit reaches the target

struct SampleLds {
  u64 hist[256];
  u64 ws[16];
  u64 acc;            // 64-bit integer sum (LDS atomics)
  u64 digit, above;   // radix select: the digit found and the weight above it
  uint32_t kmax;      // largest candidate key (LDS atomic max)
  int ncand, nfin;    // candidates / finite logits of the row
  int sel;
  float bv[16];
  int bi[16];
};

MK_DEV bool s_cand(float v) { return !__builtin_isnan(v) && v != -INFINITY; }
MK_DEV uint32_t s_key(float x) {
  if (x == 0.f) x = 0.f;                        // -0 == +0: one key
  const uint32_t u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
MK_DEV float s_unkey(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
MK_DEV u64 s_mass(float x, float xmax) {
  return x == xmax ? (1ull << 40) : (u64)(expf(x - xmax) * 1099511627776.f);
}
MK_DEV u64 s_wave_sum(u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// exclusive prefix of v over the 1024 threads in thread order; total: the sum over all of them
MK_DEV u64 s_block_scan(u64 v, u64* ws, u64& total) {
  const int l = threadIdx.x & 63, w = threadIdx.x >> 6;
  u64 inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const u64 t = __shfl_up(inc, o, 64);
    if (l >= o) inc += t;
  }
  __syncthreads();
  if (l == 63) ws[w] = inc;
  __syncthreads();
  u64 base = 0, tot = 0;
#pragma unroll
  for (int i = 0; i < SNT / 64; ++i) {
    const u64 t = ws[i];
    if (i < w) base += t;
    tot += t;
  }
  total = tot;
  return base + inc - v;
}

// Radix select over the candidates with key > kfloor, weighted by 1 (MASS = false) or by their mass: the key Kt with
// W(keys > Kt) < target <= W(keys >= Kt), and rem = target - W(keys > Kt).  False (uniformly) when the whole weight is
// below the target.
template <typename T, bool MASS>
__device__ bool s_radix_select(const T* xr, int c0, int c1, float temp, float xmax, uint32_t kfloor, u64 target,
                               SampleLds& s, uint32_t& Kt, u64& rem) {
  const int tid = threadIdx.x;
  uint32_t prefix = 0;
  for (int shift = 24; shift >= 0; shift -= 8) {
    const uint32_t himask = shift == 24 ? 0u : (0xffffffffu << (shift + 8));
    __syncthreads();
    if (tid < 256) s.hist[tid] = 0;
    if (tid == 0) s.digit = S_NONE;
    __syncthreads();
    for (int c = c0; c < c1; ++c) {
      const float v = to_f32<T>(xr[c]);
      if (!s_cand(v)) continue;
      const float x = v / temp;
      const uint32_t k = s_key(x);
      if (k <= kfloor || (k & himask) != prefix) continue;
      atomicAdd(&s.hist[(k >> shift) & 255u], MASS ? s_mass(x, xmax) : 1ull);
    }
    __syncthreads();
    if (tid < 64) {                             // lane l scans bins 255 - 4l ... 252 - 4l, the larger digits first
      u64 h[4], sum = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) { h[j] = s.hist[255 - 4 * tid - j]; sum += h[j]; }
      u64 inc = sum;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const u64 t = __shfl_up(inc, o, 64);
        if (tid >= o) inc += t;
      }
      u64 run = inc - sum;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (run < target && target <= run + h[j]) { s.digit = (u64)(255 - 4 * tid - j); s.above = run; }
        run += h[j];
      }
    }
    __syncthreads();
    const u64 d = s.digit;
    if (d == S_NONE) return false;
    prefix |= (uint32_t)d << shift;
    target -= s.above;
  }
  Kt = prefix;
  rem = target;
  return true;
}

// the token of one row; every thread of the workgroup calls it and gets the same column
template <typename T>
__device__ int sample_row(const T* xr, int V, float temp, int top_k, float top_p, uint64_t seed, uint32_t step,
                          uint32_t row, SampleLds& s) {
  const int tid = threadIdx.x, lane = tid & 63;
  const long ch = ((long)V + SNT - 1) / SNT;
  const long lo = (long)tid * ch, hi = lo + ch;
  const int c0 = (int)(lo < V ? lo : V), c1 = (int)(hi < V ? hi : V);

  // ---- pass A: the largest candidate key, the candidate and finite counts
  if (tid == 0) { s.kmax = 0; s.ncand = 0; s.nfin = 0; s.acc = 0; }
  __syncthreads();
  {
    uint32_t km = 0;
    int nc = 0, nf = 0;
    for (int c = c0; c < c1; ++c) {
      const float v = to_f32<T>(xr[c]);
      if (!s_cand(v)) continue;
      ++nc;
      nf += v != INFINITY;
      km = max(km, s_key(v / temp));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      km = max(km, (uint32_t)__shfl_xor((int)km, o, 64));
      nc += __shfl_xor(nc, o, 64);
      nf += __shfl_xor(nf, o, 64);
    }
    if (lane == 0) { atomicMax(&s.kmax, km); atomicAdd(&s.ncand, nc); atomicAdd(&s.nfin, nf); }
  }
  __syncthreads();
  const int ncand = s.ncand;
  if (s.nfin == 0) {                            // no finite logit: what greedy emits (decode_emit_kernel's order)
    float best = -INFINITY;
    int idx = 0x7fffffff;
    for (int c = c0; c < c1; ++c) {
      const float v = to_f32<T>(xr[c]);
      if (mk_argmax_better(v, c, best, idx)) { best = v; idx = c; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(best, o, 64);
      const int oi = __shfl_xor(idx, o, 64);
      if (mk_argmax_better(ov, oi, best, idx)) { best = ov; idx = oi; }
    }
    if (lane == 0) { s.bv[tid >> 6] = best; s.bi[tid >> 6] = idx; }
    __syncthreads();
    best = s.bv[0]; idx = s.bi[0];
    for (int w = 1; w < SNT / 64; ++w)
      if (mk_argmax_better(s.bv[w], s.bi[w], best, idx)) { best = s.bv[w]; idx = s.bi[w]; }
    return idx;
  }
  const float xmax = s_unkey(s.kmax);

  // ---- top-k: exactly k columns, ties at the k-th value to the lower column
  uint32_t Kt = 0;                              // (no candidate has key 0: that is a NaN pattern)
  u64 r = S_ALL;
  const bool kon = top_k > 0 && top_k < ncand;
  if (kon) s_radix_select<T, false>(xr, c0, c1, temp, xmax, 0u, (u64)top_k, s, Kt, r);

  // ---- top-p over the survivors: keep c iff the mass strictly above x_c is below p * Z
  if (top_p < 1.f) {
    u64 m = 0;
    for (int c = c0; c < c1; ++c) {
      const float v = to_f32<T>(xr[c]);
      if (!s_cand(v)) continue;
      const float x = v / temp;
      if (s_key(x) > Kt) m += s_mass(x, xmax);
    }
    m = s_wave_sum(m);
    if (lane == 0 && m) atomicAdd(&s.acc, m);
    __syncthreads();
    const u64 above = s.acc;                    // mass above the tie group of Kt (the whole mass without top-k)
    const u64 Z = above + (kon ? r * s_mass(s_unkey(Kt), xmax) : 0ull);
    const u64 tp = (u64)ceil((double)top_p * (double)Z);
    if (above >= tp) {                          // else every survivor, the tie group included, stays
      u64 rem;
      s_radix_select<T, true>(xr, c0, c1, temp, xmax, Kt, tp, s, Kt, rem);
      r = S_ALL;
    }
  }

  // ---- the draw, in column order over the kept columns
  u64 tot;
  u64 rank0 = 0;
  if (r != S_ALL) {
    u64 nt = 0;
    for (int c = c0; c < c1; ++c) {
      const float v = to_f32<T>(xr[c]);
      nt += s_cand(v) && s_key(v / temp) == Kt;
    }
    rank0 = s_block_scan(nt, s.ws, tot);
  }
  u64 local = 0, rank = rank0;
  for (int c = c0; c < c1; ++c) {
    const float v = to_f32<T>(xr[c]);
    if (!s_cand(v)) continue;
    const float x = v / temp;
    const uint32_t k = s_key(x);
    if (k > Kt || (k == Kt && (r == S_ALL || rank++ < r))) local += s_mass(x, xmax);
  }
  const u64 excl = s_block_scan(local, s.ws, tot);
  const u64 a = 2ull * (mk_hash32(seed, ((uint64_t)step << 32) | row) >> 8) + 1ull;     // u = a * 2^-25
  const u64 thr = (__umul64hi(a, tot) << 39) | ((a * tot) >> 25);                      // floor(u * Z_kept) < Z_kept
  if (excl <= thr && thr < excl + local) {      // exactly one thread: the cumulative mass crosses u * Z_kept here
    u64 cum = excl;
    rank = rank0;
    int sel = c1 - 1;
    for (int c = c0; c < c1; ++c) {
      const float v = to_f32<T>(xr[c]);
      if (!s_cand(v)) continue;
      const float x = v / temp;
      const uint32_t k = s_key(x);
      if (k > Kt || (k == Kt && (r == S_ALL || rank++ < r))) {
        cum += s_mass(x, xmax);
        if (cum > thr) { sel = c; break; }
      }
    }
    s.sel = sel;
  }
  __syncthreads();
  return s.sel;
}

template <typename T>
__global__ __launch_bounds__(SNT) void sample_rows_kernel(const T* logits, long ld, int V, float temp, int top_k,
                                                          float top_p, uint64_t seed, uint32_t step, int64_t* out) {
  __shared__ SampleLds s;
  const int idx = sample_row<T>(logits + (long)blockIdx.x * ld, V, temp, top_k, top_p, seed, step, blockIdx.x, s);
  if (threadIdx.x == 0) out[blockIdx.x] = idx;
}

// decode_emit_kernel (decode.hip) with the argmax replaced by the draw; the RNG counter is the output column state[1]
template <typename T>
__global__ __launch_bounds__(SNT) void decode_emit_sample_kernel(const T* logits, long ld, int V, long pad, long eos,
                                                                 int64_t* tok, unsigned char* done, int64_t* out,
                                                                 long out_ld, int32_t* state, float temp, int top_k,
                                                                 float top_p, uint64_t seed) {
  __shared__ SampleLds s;
  const int b = blockIdx.x;
  const int col = state[1];                     // read by every thread before this workgroup's arrival below
  const bool fin = done[b];
  const int idx = fin ? 0 : sample_row<T>(logits + (long)b * ld, V, temp, top_k, top_p, seed, (uint32_t)col, b, s);
  if (threadIdx.x == 0) {
    const long nxt = fin ? pad : (long)idx;
    out[(long)b * out_ld + col] = nxt;
    if (nxt == eos) done[b] = 1;
    tok[b] = nxt;
    __threadfence();
    const int old = __hip_atomic_fetch_add(state + 2, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (old == (int)gridDim.x - 1) {            // every sample has read state[1]: advance the step
      state[0] += 1;
      state[1] = col + 1;
      state[2] = 0;
    }
  }
}

constexpr int SAMPLE_MAX_V = 1 << 23;          // V masses of at most 2^40 each sum inside 64 bits

bool sample_args_ok(float temperature, int32_t top_k, float top_p) {
  return isfinite(temperature) && temperature > 0.f && top_p > 0.f && top_p <= 1.f && top_k >= 0;
}

}  // namespace

extern "C" int mk_sample_rows(const void* logits, int64_t ld, int32_t rows, int32_t V, float temperature,
                              int32_t top_k, float top_p, uint64_t seed, int32_t step, int64_t* out_ids,
                              int32_t dtype, void* stream) {
  if (!logits || !out_ids || rows <= 0 || V <= 0 || ld < V || !sample_args_ok(temperature, top_k, top_p))
    return MK_ERR_BAD_ARG;
  if (V > SAMPLE_MAX_V) return MK_ERR_UNSUPPORTED;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (dtype == MK_BF16)
    MK_LAUNCH((sample_rows_kernel<bf16>), dim3(rows), dim3(SNT), 0, st, (const bf16*)logits, (long)ld, V, temperature,
              top_k, top_p, seed, (uint32_t)step, out_ids);
  else if (dtype == MK_F16)
    MK_LAUNCH((sample_rows_kernel<_Float16>), dim3(rows), dim3(SNT), 0, st, (const _Float16*)logits, (long)ld, V,
              temperature, top_k, top_p, seed, (uint32_t)step, out_ids);
  else if (dtype == MK_F32)
    MK_LAUNCH((sample_rows_kernel<float>), dim3(rows), dim3(SNT), 0, st, (const float*)logits, (long)ld, V,
              temperature, top_k, top_p, seed, (uint32_t)step, out_ids);
  else return MK_ERR_UNSUPPORTED;
  return mk_check_launch();
}

extern "C" int mk_decode_emit_sample(const void* logits, int64_t ld, int32_t V, int32_t B, int64_t pad, int64_t eos,
                                     int64_t* tok, void* done, int64_t* out, int64_t out_ld, int32_t* state,
                                     float temperature, int32_t top_k, float top_p, uint64_t seed, int32_t dtype,
                                     void* stream) {
  if (!logits || !tok || !done || !out || !state || V <= 0 || B <= 0 || ld < V ||
      !sample_args_ok(temperature, top_k, top_p))
    return MK_ERR_BAD_ARG;
  if (V > SAMPLE_MAX_V) return MK_ERR_UNSUPPORTED;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (dtype == MK_BF16)
    MK_LAUNCH((decode_emit_sample_kernel<bf16>), dim3(B), dim3(SNT), 0, st, (const bf16*)logits, (long)ld, V, (long)pad,
              (long)eos, tok, (unsigned char*)done, out, (long)out_ld, state, temperature, top_k, top_p, seed);
  else if (dtype == MK_F16)
    MK_LAUNCH((decode_emit_sample_kernel<_Float16>), dim3(B), dim3(SNT), 0, st, (const _Float16*)logits, (long)ld, V,
              (long)pad, (long)eos, tok, (unsigned char*)done, out, (long)out_ld, state, temperature, top_k, top_p, seed);
  else if (dtype == MK_F32)
    MK_LAUNCH((decode_emit_sample_kernel<float>), dim3(B), dim3(SNT), 0, st, (const float*)logits, (long)ld, V,
              (long)pad, (long)eos, tok, (unsigned char*)done, out, (long)out_ld, state, temperature, top_k, top_p, seed);
  else return MK_ERR_UNSUPPORTED;
  return mk_check_launch();
}
