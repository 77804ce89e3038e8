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
  u64 zZ, zS, zM;     // warpers: sum of m_c, sum of trunc(m_c * d_c), largest m_c over the current survivors
  u64 fl;             // warpers: the mass floor of a stage, written by thread 0
  uint32_t kmax;      // largest candidate key (LDS atomic max)
  int ncand, nfin;    // candidates / finite logits of the row
  int sel;
  float D;            // warpers: zS / zZ, written by thread 0
  float bv[16];
  int bi[16];
};

// min-p, typical-p, epsilon and eta (rule 6 of include/macaw_hip.h); all off: {0, 1, 0, 0}
struct SampleWarp { float min_p, typical_p, eps, eta; };

// The kept set of a row as uniform scalars (rank0 alone is per thread): the value prefix (Kt, r) of top-k and top-p,
// and behind the warpers a mass floor and the band t_c = |d_c - D| <= Tt of typical-p.
struct SampleKeep {
  uint32_t Kt;        // key > Kt, or key == Kt and fewer than r columns of that key to the left
  u64 r;
  u64 rank0;          // columns of key Kt to the left of this thread's chunk (r != S_ALL)
  u64 mfloor;         // m_c >= mfloor: min-p, epsilon, eta, and 1 in front of typical-p
  uint32_t Tt;        // band (typical-p on): the uint32 image of t_c is <= Tt
  float D;
  bool band;
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
MK_DEV float s_dist(float x, float xmax) { return x == xmax ? 0.f : xmax - x; }            // d_c (0 at x_max = +inf too)
MK_DEV uint32_t s_tkey(float d, float D) { return __float_as_uint(fabsf(d - D)); }         // t_c >= 0: its bits order it
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

// whether a candidate column of value x, key k stays, and its mass m; rank: the thread's running count of key Kt
template <bool WARP>
MK_DEV bool s_kept(const SampleKeep& kp, float x, uint32_t k, float xmax, u64& rank, u64& m) {
  if (!(k > kp.Kt || (k == kp.Kt && (kp.r == S_ALL || rank++ < kp.r)))) return false;
  m = s_mass(x, xmax);
  if constexpr (WARP) {
    if (m < kp.mfloor) return false;
    if (kp.band && s_tkey(s_dist(x, xmax), kp.D) > kp.Tt) return false;
  }
  return true;
}

// The keys and weights a radix select runs over: key(v, k) is false for a column that does not take part and sets its
// key; weight() is that column's weight, asked for only when its key is still in the race; reset() starts a pass.
struct SelCount {                               // top-k: every candidate, weight 1
  float temp;
  MK_DEV void reset() {}
  MK_DEV bool key(float v, uint32_t& k) {
    if (!s_cand(v)) return false;
    k = s_key(v / temp);
    return true;
  }
  MK_DEV u64 weight() const { return 1ull; }
};
struct SelMass {                                // top-p: the candidates with key > kfloor, weight m_c
  float temp, xmax;
  uint32_t kfloor;
  float x;
  MK_DEV void reset() {}
  MK_DEV bool key(float v, uint32_t& k) {
    if (!s_cand(v)) return false;
    x = v / temp;
    k = s_key(x);
    return k > kfloor;
  }
  MK_DEV u64 weight() const { return s_mass(x, xmax); }
};
struct SelTypical {                             // typical-p: the survivors so far, key ~t_c (smaller t first), weight m_c
  float temp, xmax;
  SampleKeep kp;
  u64 rank, m;
  MK_DEV void reset() { rank = kp.rank0; }
  MK_DEV bool key(float v, uint32_t& k) {
    if (!s_cand(v)) return false;
    const float x = v / temp;
    if (!s_kept<true>(kp, x, s_key(x), xmax, rank, m)) return false;
    k = ~s_tkey(s_dist(x, xmax), kp.D);
    return true;
  }
  MK_DEV u64 weight() const { return m; }
};

// Radix select over the columns and keys of f, weighted by f's weights: the key Kt with
// W(keys > Kt) < target <= W(keys >= Kt), and rem = target - W(keys > Kt).  False (uniformly) when the whole weight is
// below the target.
template <typename T, typename F>
__device__ bool s_radix_select(const T* xr, int c0, int c1, F f, u64 target, SampleLds& s, uint32_t& Kt, u64& rem) {
  const int tid = threadIdx.x;
  uint32_t prefix = 0;
  for (int shift = 24; shift >= 0; shift -= 8) {
    const uint32_t himask = shift == 24 ? 0u : (0xffffffffu << (shift + 8));
    __syncthreads();
    if (tid < 256) s.hist[tid] = 0;
    if (tid == 0) s.digit = S_NONE;
    __syncthreads();
    f.reset();
    for (int c = c0; c < c1; ++c) {
      uint32_t k;
      if (!f.key(to_f32<T>(xr[c]), k) || (k & himask) != prefix) continue;
      atomicAdd(&s.hist[(k >> shift) & 255u], f.weight());
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

// warpers: s.zZ = sum of m_c, s.zS = sum of trunc(m_c * d_c), s.zM = max of m_c over the columns kp keeps (integers, so
// the order of arrival does not matter), and s.D = zS / zZ in fp64 rounded once to fp32
template <typename T>
__device__ void s_stats(const T* xr, int c0, int c1, float temp, float xmax, const SampleKeep& kp, SampleLds& s) {
  const int tid = threadIdx.x, lane = tid & 63;
  __syncthreads();
  if (tid == 0) { s.zZ = 0; s.zS = 0; s.zM = 0; }
  __syncthreads();
  u64 z = 0, sd = 0, mx = 0, rank = kp.rank0;
  for (int c = c0; c < c1; ++c) {
    const float v = to_f32<T>(xr[c]);
    if (!s_cand(v)) continue;
    const float x = v / temp;
    u64 m;
    if (!s_kept<true>(kp, x, s_key(x), xmax, rank, m)) continue;
    z += m;
    if (m) sd += (u64)((double)m * (double)s_dist(x, xmax));         // d e^-d <= 1/e: below 2^39 each
    mx = max(mx, m);
  }
  z = s_wave_sum(z);
  sd = s_wave_sum(sd);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = max(mx, (u64)__shfl_xor(mx, o, 64));
  if (lane == 0 && z) { atomicAdd(&s.zZ, z); atomicAdd(&s.zS, sd); atomicMax(&s.zM, mx); }
  __syncthreads();
  if (tid == 0) s.D = s.zZ ? (float)((double)s.zS / (double)s.zZ) : 0.f;
  __syncthreads();
}

// what greedy emits for a row without a finite logit (decode_emit_kernel's order)
template <typename T>
__device__ int s_greedy(const T* xr, int c0, int c1, SampleLds& s) {
  const int tid = threadIdx.x, lane = tid & 63;
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

// The filter: rules 1-3 and, with WARP, the four stages of rule 6 -> the kept set kp and x_max.  False (uniformly) for
// a row without a finite logit.  Every thread of the workgroup calls it on its chunk [c0, c1).
template <typename T, bool WARP>
__device__ bool s_filter(const T* xr, int c0, int c1, float temp, int top_k, float top_p, const SampleWarp& w,
                         SampleLds& s, SampleKeep& kp, float& xmax_out) {
  const int tid = threadIdx.x, lane = tid & 63;

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
  if (s.nfin == 0) return false;
  const float xmax = s_unkey(s.kmax);
  xmax_out = xmax;

  // ---- top-k: exactly k columns, ties at the k-th value to the lower column
  uint32_t Kt = 0;                              // (no candidate has key 0: that is a NaN pattern)
  u64 r = S_ALL;
  const bool kon = top_k > 0 && top_k < ncand;
  if (kon) s_radix_select<T>(xr, c0, c1, SelCount{temp}, (u64)top_k, s, Kt, r);

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
      s_radix_select<T>(xr, c0, c1, SelMass{temp, xmax, Kt, 0.f}, tp, s, Kt, rem);
      r = S_ALL;
    }
  }

  // ---- the tie group of Kt in column order: the columns of that key to the left of this thread's chunk
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
  kp.Kt = Kt; kp.r = r; kp.rank0 = rank0; kp.mfloor = 0; kp.Tt = 0; kp.D = 0.f; kp.band = false;

  if constexpr (WARP) {
    // ---- min-p: e_c >= min_p, as m_c >= ceil(min_p * 2^40) (exact: a float times a power of two)
    if (w.min_p > 0.f) kp.mfloor = (u64)ceil((double)w.min_p * 1099511627776.0);
    // ---- typical-p: the top-p criterion on the key t_c = |d_c - D|, ascending; mass-0 survivors leave first
    if (w.typical_p < 1.f) {
      if (kp.mfloor < 1) kp.mfloor = 1;
      s_stats<T>(xr, c0, c1, temp, xmax, kp, s);
      kp.D = s.D;
      const u64 tp = (u64)ceil((double)w.typical_p * (double)s.zZ);
      uint32_t Kn;
      u64 rem;
      if (s_radix_select<T>(xr, c0, c1, SelTypical{temp, xmax, kp, 0, 0}, tp, s, Kn, rem)) {
        kp.Tt = ~Kn;
        kp.band = true;
      }
    }
    // ---- epsilon: m_c >= ceil(eps * Z); no survivor passes: the largest survivors stay
    if (w.eps > 0.f) {
      s_stats<T>(xr, c0, c1, temp, xmax, kp, s);
      const u64 fl = min((u64)ceil((double)w.eps * (double)s.zZ), s.zM);
      kp.mfloor = max(kp.mfloor, fl);
    }
    // ---- eta: the same with min(eta, sqrt(eta) * exp(-H)), H = log Z + D the entropy of the survivors
    if (w.eta > 0.f) {
      s_stats<T>(xr, c0, c1, temp, xmax, kp, s);
      if (tid == 0) {
        const double Z = (double)s.zZ;
        const double H = log(Z * 0x1p-40) + (double)s.zS / Z;
        const double th = fmin((double)w.eta, sqrt((double)w.eta) * exp(-H));
        s.fl = min((u64)ceil(th * Z), s.zM);
      }
      __syncthreads();
      kp.mfloor = max(kp.mfloor, s.fl);
    }
  }
  return true;
}

// the draw, in column order over the kept columns; every thread gets the same column
template <typename T, bool WARP>
__device__ int s_draw(const T* xr, int c0, int c1, float temp, float xmax, const SampleKeep& kp, uint64_t seed,
                      uint32_t step, uint32_t row, SampleLds& s) {
  u64 tot;
  u64 local = 0, rank = kp.rank0, m;
  for (int c = c0; c < c1; ++c) {
    const float v = to_f32<T>(xr[c]);
    if (!s_cand(v)) continue;
    const float x = v / temp;
    if (s_kept<WARP>(kp, x, s_key(x), xmax, rank, m)) local += m;
  }
  const u64 excl = s_block_scan(local, s.ws, tot);
  const u64 a = 2ull * (mk_hash32(seed, ((uint64_t)step << 32) | row) >> 8) + 1ull;     // u = a * 2^-25
  const u64 thr = (__umul64hi(a, tot) << 39) | ((a * tot) >> 25);                      // floor(u * Z_kept) < Z_kept
  if (excl <= thr && thr < excl + local) {      // exactly one thread: the cumulative mass crosses u * Z_kept here
    u64 cum = excl;
    rank = kp.rank0;
    int sel = c1 - 1;
    for (int c = c0; c < c1; ++c) {
      const float v = to_f32<T>(xr[c]);
      if (!s_cand(v)) continue;
      const float x = v / temp;
      if (s_kept<WARP>(kp, x, s_key(x), xmax, rank, m)) {
        cum += m;
        if (cum > thr) { sel = c; break; }
      }
    }
    s.sel = sel;
  }
  __syncthreads();
  return s.sel;
}

MK_DEV void s_chunk(int V, int& c0, int& c1) {
  const long ch = ((long)V + SNT - 1) / SNT;
  const long lo = (long)threadIdx.x * ch, hi = lo + ch;
  c0 = (int)(lo < V ? lo : V);
  c1 = (int)(hi < V ? hi : V);
}

// the token of one row; every thread of the workgroup calls it and gets the same column
template <typename T, bool WARP>
__device__ int sample_row(const T* xr, int V, float temp, int top_k, float top_p, const SampleWarp& w, uint64_t seed,
                          uint32_t step, uint32_t row, SampleLds& s) {
  int c0, c1;
  s_chunk(V, c0, c1);
  SampleKeep kp;
  float xmax;
  if (!s_filter<T, WARP>(xr, c0, c1, temp, top_k, top_p, w, s, kp, xmax)) return s_greedy<T>(xr, c0, c1, s);
  return s_draw<T, WARP>(xr, c0, c1, temp, xmax, kp, seed, step, row, s);
}

template <typename T, bool WARP>
__global__ __launch_bounds__(SNT) void sample_rows_kernel(const T* logits, long ld, int V, float temp, int top_k,
                                                          float top_p, SampleWarp w, uint64_t seed, uint32_t step,
                                                          int64_t* out) {
  __shared__ SampleLds s;
  const int idx = sample_row<T, WARP>(logits + (long)blockIdx.x * ld, V, temp, top_k, top_p, w, seed, step, blockIdx.x,
                                      s);
  if (threadIdx.x == 0) out[blockIdx.x] = idx;
}

// the kept mask of the filter: keep[row][c] = 1 where the draw could land, 0 elsewhere; all 0 without a finite logit
template <typename T>
__global__ __launch_bounds__(SNT) void sample_keep_kernel(const T* logits, long ld, int V, float temp, int top_k,
                                                          float top_p, SampleWarp w, unsigned char* keep, long keep_ld) {
  __shared__ SampleLds s;
  const T* xr = logits + (long)blockIdx.x * ld;
  unsigned char* kr = keep + (long)blockIdx.x * keep_ld;
  int c0, c1;
  s_chunk(V, c0, c1);
  SampleKeep kp;
  float xmax = 0.f;
  const bool fin = s_filter<T, true>(xr, c0, c1, temp, top_k, top_p, w, s, kp, xmax);
  u64 rank = kp.rank0, m;
  for (int c = c0; c < c1; ++c) {
    const float v = to_f32<T>(xr[c]);
    bool b = false;
    if (fin && s_cand(v)) {
      const float x = v / temp;
      b = s_kept<true>(kp, x, s_key(x), xmax, rank, m);
    }
    kr[c] = b;
  }
}

// decode_emit_kernel's bookkeeping for sample b at output column col, by one thread: pad for a finished sample, the eos
// flag, the token fed next, and the step's hand-off by the last arriving workgroup
MK_DEV void s_emit_books(int b, int col, bool fin, int idx, long pad, long eos, int64_t* tok, unsigned char* done,
                         int64_t* out, long out_ld, int32_t* state) {
  const long nxt = fin ? pad : (long)idx;
  out[(long)b * out_ld + col] = nxt;
  if (nxt == eos) done[b] = 1;
  tok[b] = nxt;
  __threadfence();
  const int old = __hip_atomic_fetch_add(state + 2, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
  if (old == (int)gridDim.x - 1) {              // every sample has read state[1]: advance the step
    state[0] += 1;
    state[1] = col + 1;
    state[2] = 0;
  }
}

// the domain of the scalar entries, and whether one of the four warpers is on (host: the C entries; device: a record)
__host__ __device__ inline bool sample_args_ok(float temperature, int32_t top_k, float top_p) {
  return isfinite(temperature) && temperature > 0.f && top_p > 0.f && top_p <= 1.f && top_k >= 0;
}
__host__ __device__ inline bool warp_args_ok(const SampleWarp& w) {        // (NaN fails every comparison)
  return w.min_p >= 0.f && w.min_p <= 1.f && w.typical_p > 0.f && w.typical_p <= 1.f && w.eps >= 0.f && w.eps < 1.f &&
         w.eta >= 0.f && w.eta < 1.f;
}
__host__ __device__ inline bool warp_on(const SampleWarp& w) {
  return w.min_p > 0.f || w.typical_p < 1.f || w.eps > 0.f || w.eta > 0.f;
}

// decode_emit_kernel (decode.hip) with the argmax replaced by the draw; the RNG counter is the output column state[1]
template <typename T, bool WARP>
__global__ __launch_bounds__(SNT) void decode_emit_sample_kernel(const T* logits, long ld, int V, long pad, long eos,
                                                                 int64_t* tok, unsigned char* done, int64_t* out,
                                                                 long out_ld, int32_t* state, float temp, int top_k,
                                                                 float top_p, SampleWarp w, uint64_t seed) {
  __shared__ SampleLds s;
  const int b = blockIdx.x;
  const int col = state[1];                     // read by every thread before this workgroup's arrival below
  const bool fin = done[b];
  const int idx =
      fin ? 0 : sample_row<T, WARP>(logits + (long)b * ld, V, temp, top_k, top_p, w, seed, (uint32_t)col, b, s);
  if (threadIdx.x == 0) s_emit_books(b, col, fin, idx, pad, eos, tok, done, out, out_ld, state);
}

// The record of one row of the per-row sampling table ("Per-row sampling table", include/macaw_hip.h): 48 bytes.
struct SampleRec {
  float temp;
  int32_t top_k;
  float top_p;
  SampleWarp w;
  uint32_t stream;
  uint64_t seed;
  int32_t mode;       // 0 greedy, 1 sampled
  int32_t rsv;
};
static_assert(sizeof(SampleRec) == 48 && offsetof(SampleRec, seed) == 32 && offsetof(SampleRec, mode) == 40,
              "the per-row sampling record is 48 bytes");

// the token of one row by its record: greedy (what mk_argmax_rows returns), sample_row<T, false>, or sample_row<T, true>
// when one of the record's four warpers is on.  The record is the workgroup's own, so the branch is uniform; a record
// outside the scalar entries' domain is greedy.
template <typename T>
MK_DEV int sample_row_rec(const T* xr, int V, const SampleRec* rec, uint32_t step, SampleLds& s) {
  const SampleRec r = *rec;
  int form = 0;
  if (r.mode == 1 && sample_args_ok(r.temp, r.top_k, r.top_p) && warp_args_ok(r.w)) form = warp_on(r.w) ? 2 : 1;
  form = __builtin_amdgcn_readfirstlane(form);
  // (the warpers by reference to the table itself: a copy would have to live in scratch for the filter to address it)
  if (form == 2) return sample_row<T, true>(xr, V, r.temp, r.top_k, r.top_p, rec->w, r.seed, step, r.stream, s);
  if (form == 1) return sample_row<T, false>(xr, V, r.temp, r.top_k, r.top_p, rec->w, r.seed, step, r.stream, s);
  int c0, c1;
  s_chunk(V, c0, c1);
  return s_greedy<T>(xr, c0, c1, s);
}

template <typename T>
__global__ __launch_bounds__(SNT) void sample_rows_table_kernel(const T* logits, long ld, int V, const SampleRec* table,
                                                                uint32_t step, int64_t* out) {
  __shared__ SampleLds s;
  const int idx = sample_row_rec<T>(logits + (long)blockIdx.x * ld, V, table + blockIdx.x, step, s);
  if (threadIdx.x == 0) out[blockIdx.x] = idx;
}

// decode_emit_sample_kernel with the parameters of sample b read from table[b]
template <typename T>
__global__ __launch_bounds__(SNT) void decode_emit_sample_table_kernel(const T* logits, long ld, int V, long pad,
                                                                       long eos, int64_t* tok, unsigned char* done,
                                                                       int64_t* out, long out_ld, int32_t* state,
                                                                       const SampleRec* table) {
  __shared__ SampleLds s;
  const int b = blockIdx.x;
  const int col = state[1];                     // read by every thread before this workgroup's arrival
  const bool fin = done[b];
  const int idx = fin ? 0 : sample_row_rec<T>(logits + (long)b * ld, V, table + b, (uint32_t)col, s);
  if (threadIdx.x == 0) s_emit_books(b, col, fin, idx, pad, eos, tok, done, out, out_ld, state);
}

constexpr int SAMPLE_MAX_V = 1 << 23;          // V masses of at most 2^40 each sum inside 64 bits

template <typename T>
void launch_rows(bool warp, int rows, hipStream_t st, const void* logits, long ld, int V, float temperature, int top_k,
                 float top_p, const SampleWarp& w, uint64_t seed, uint32_t step, int64_t* out) {
  if (warp)
    MK_LAUNCH((sample_rows_kernel<T, true>), dim3(rows), dim3(SNT), 0, st, (const T*)logits, ld, V, temperature, top_k,
              top_p, w, seed, step, out);
  else
    MK_LAUNCH((sample_rows_kernel<T, false>), dim3(rows), dim3(SNT), 0, st, (const T*)logits, ld, V, temperature, top_k,
              top_p, w, seed, step, out);
}

template <typename T>
void launch_emit(bool warp, int B, hipStream_t st, const void* logits, long ld, int V, long pad, long eos, int64_t* tok,
                 void* done, int64_t* out, long out_ld, int32_t* state, float temperature, int top_k, float top_p,
                 const SampleWarp& w, uint64_t seed) {
  if (warp)
    MK_LAUNCH((decode_emit_sample_kernel<T, true>), dim3(B), dim3(SNT), 0, st, (const T*)logits, ld, V, pad, eos, tok,
              (unsigned char*)done, out, out_ld, state, temperature, top_k, top_p, w, seed);
  else
    MK_LAUNCH((decode_emit_sample_kernel<T, false>), dim3(B), dim3(SNT), 0, st, (const T*)logits, ld, V, pad, eos, tok,
              (unsigned char*)done, out, out_ld, state, temperature, top_k, top_p, w, seed);
}

int sample_rows_impl(const void* logits, int64_t ld, int32_t rows, int32_t V, float temperature, int32_t top_k,
                     float top_p, const SampleWarp& w, uint64_t seed, int32_t step, int64_t* out_ids, int32_t dtype,
                     void* stream) {
  if (!logits || !out_ids || rows <= 0 || V <= 0 || ld < V || !sample_args_ok(temperature, top_k, top_p) ||
      !warp_args_ok(w))
    return MK_ERR_BAD_ARG;
  if (V > SAMPLE_MAX_V) return MK_ERR_UNSUPPORTED;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const bool warp = warp_on(w);                 // all four off: the kernel without them
  if (dtype == MK_BF16)
    launch_rows<bf16>(warp, rows, st, logits, (long)ld, V, temperature, top_k, top_p, w, seed, (uint32_t)step, out_ids);
  else if (dtype == MK_F16)
    launch_rows<_Float16>(warp, rows, st, logits, (long)ld, V, temperature, top_k, top_p, w, seed, (uint32_t)step,
                          out_ids);
  else if (dtype == MK_F32)
    launch_rows<float>(warp, rows, st, logits, (long)ld, V, temperature, top_k, top_p, w, seed, (uint32_t)step, out_ids);
  else return MK_ERR_UNSUPPORTED;
  return mk_check_launch();
}

int emit_sample_impl(const void* logits, int64_t ld, int32_t V, int32_t B, int64_t pad, int64_t eos, int64_t* tok,
                     void* done, int64_t* out, int64_t out_ld, int32_t* state, float temperature, int32_t top_k,
                     float top_p, const SampleWarp& w, uint64_t seed, int32_t dtype, void* stream) {
  if (!logits || !tok || !done || !out || !state || V <= 0 || B <= 0 || ld < V ||
      !sample_args_ok(temperature, top_k, top_p) || !warp_args_ok(w))
    return MK_ERR_BAD_ARG;
  if (V > SAMPLE_MAX_V) return MK_ERR_UNSUPPORTED;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const bool warp = warp_on(w);
  if (dtype == MK_BF16)
    launch_emit<bf16>(warp, B, st, logits, (long)ld, V, (long)pad, (long)eos, tok, done, out, (long)out_ld, state,
                      temperature, top_k, top_p, w, seed);
  else if (dtype == MK_F16)
    launch_emit<_Float16>(warp, B, st, logits, (long)ld, V, (long)pad, (long)eos, tok, done, out, (long)out_ld, state,
                          temperature, top_k, top_p, w, seed);
  else if (dtype == MK_F32)
    launch_emit<float>(warp, B, st, logits, (long)ld, V, (long)pad, (long)eos, tok, done, out, (long)out_ld, state,
                       temperature, top_k, top_p, w, seed);
  else return MK_ERR_UNSUPPORTED;
  return mk_check_launch();
}

constexpr SampleWarp WARP_OFF = {0.f, 1.f, 0.f, 0.f};

}  // namespace

extern "C" int mk_sample_rows(const void* logits, int64_t ld, int32_t rows, int32_t V, float temperature,
                              int32_t top_k, float top_p, uint64_t seed, int32_t step, int64_t* out_ids,
                              int32_t dtype, void* stream) {
  return sample_rows_impl(logits, ld, rows, V, temperature, top_k, top_p, WARP_OFF, seed, step, out_ids, dtype, stream);
}

extern "C" int mk_sample_rows_warp(const void* logits, int64_t ld, int32_t rows, int32_t V, float temperature,
                                   int32_t top_k, float top_p, float min_p, float typical_p, float epsilon_cutoff,
                                   float eta_cutoff, uint64_t seed, int32_t step, int64_t* out_ids, int32_t dtype,
                                   void* stream) {
  return sample_rows_impl(logits, ld, rows, V, temperature, top_k, top_p,
                          SampleWarp{min_p, typical_p, epsilon_cutoff, eta_cutoff}, seed, step, out_ids, dtype, stream);
}

extern "C" int mk_decode_emit_sample(const void* logits, int64_t ld, int32_t V, int32_t B, int64_t pad, int64_t eos,
                                     int64_t* tok, void* done, int64_t* out, int64_t out_ld, int32_t* state,
                                     float temperature, int32_t top_k, float top_p, uint64_t seed, int32_t dtype,
                                     void* stream) {
  return emit_sample_impl(logits, ld, V, B, pad, eos, tok, done, out, out_ld, state, temperature, top_k, top_p, WARP_OFF,
                          seed, dtype, stream);
}

extern "C" int mk_decode_emit_sample_warp(const void* logits, int64_t ld, int32_t V, int32_t B, int64_t pad,
                                          int64_t eos, int64_t* tok, void* done, int64_t* out, int64_t out_ld,
                                          int32_t* state, float temperature, int32_t top_k, float top_p, float min_p,
                                          float typical_p, float epsilon_cutoff, float eta_cutoff, uint64_t seed,
                                          int32_t dtype, void* stream) {
  return emit_sample_impl(logits, ld, V, B, pad, eos, tok, done, out, out_ld, state, temperature, top_k, top_p,
                          SampleWarp{min_p, typical_p, epsilon_cutoff, eta_cutoff}, seed, dtype, stream);
}

extern "C" int mk_sample_rows_table(const void* logits, int64_t ld, int32_t rows, int32_t V, const void* table,
                                    int32_t step, int64_t* out_ids, int32_t dtype, void* stream) {
  if (!logits || !table || !out_ids || rows <= 0 || V <= 0 || ld < V) return MK_ERR_BAD_ARG;
  if (V > SAMPLE_MAX_V || (reinterpret_cast<uintptr_t>(table) & 15)) return MK_ERR_UNSUPPORTED;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const SampleRec* tb = (const SampleRec*)table;
  if (dtype == MK_BF16)
    MK_LAUNCH((sample_rows_table_kernel<bf16>), dim3(rows), dim3(SNT), 0, st, (const bf16*)logits, (long)ld, V, tb,
              (uint32_t)step, out_ids);
  else if (dtype == MK_F16)
    MK_LAUNCH((sample_rows_table_kernel<_Float16>), dim3(rows), dim3(SNT), 0, st, (const _Float16*)logits, (long)ld, V,
              tb, (uint32_t)step, out_ids);
  else if (dtype == MK_F32)
    MK_LAUNCH((sample_rows_table_kernel<float>), dim3(rows), dim3(SNT), 0, st, (const float*)logits, (long)ld, V, tb,
              (uint32_t)step, out_ids);
  else return MK_ERR_UNSUPPORTED;
  return mk_check_launch();
}

extern "C" int mk_decode_emit_sample_table(const void* logits, int64_t ld, int32_t V, int32_t B, int64_t pad,
                                           int64_t eos, int64_t* tok, void* done, int64_t* out, int64_t out_ld,
                                           int32_t* state, const void* table, int32_t dtype, void* stream) {
  if (!logits || !tok || !done || !out || !state || !table || V <= 0 || B <= 0 || ld < V) return MK_ERR_BAD_ARG;
  if (V > SAMPLE_MAX_V || (reinterpret_cast<uintptr_t>(table) & 15)) return MK_ERR_UNSUPPORTED;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const SampleRec* tb = (const SampleRec*)table;
  if (dtype == MK_BF16)
    MK_LAUNCH((decode_emit_sample_table_kernel<bf16>), dim3(B), dim3(SNT), 0, st, (const bf16*)logits, (long)ld, V,
              (long)pad, (long)eos, tok, (unsigned char*)done, out, (long)out_ld, state, tb);
  else if (dtype == MK_F16)
    MK_LAUNCH((decode_emit_sample_table_kernel<_Float16>), dim3(B), dim3(SNT), 0, st, (const _Float16*)logits, (long)ld,
              V, (long)pad, (long)eos, tok, (unsigned char*)done, out, (long)out_ld, state, tb);
  else if (dtype == MK_F32)
    MK_LAUNCH((decode_emit_sample_table_kernel<float>), dim3(B), dim3(SNT), 0, st, (const float*)logits, (long)ld, V,
              (long)pad, (long)eos, tok, (unsigned char*)done, out, (long)out_ld, state, tb);
  else return MK_ERR_UNSUPPORTED;
  return mk_check_launch();
}

extern "C" int mk_sample_keep_rows(const void* logits, int64_t ld, int32_t rows, int32_t V, float temperature,
                                   int32_t top_k, float top_p, float min_p, float typical_p, float epsilon_cutoff,
                                   float eta_cutoff, uint8_t* keep, int64_t keep_ld, int32_t dtype, void* stream) {
  const SampleWarp w{min_p, typical_p, epsilon_cutoff, eta_cutoff};
  if (!logits || !keep || rows <= 0 || V <= 0 || ld < V || keep_ld < V || !sample_args_ok(temperature, top_k, top_p) ||
      !warp_args_ok(w))
    return MK_ERR_BAD_ARG;
  if (V > SAMPLE_MAX_V) return MK_ERR_UNSUPPORTED;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (dtype == MK_BF16)
    MK_LAUNCH((sample_keep_kernel<bf16>), dim3(rows), dim3(SNT), 0, st, (const bf16*)logits, (long)ld, V, temperature,
              top_k, top_p, w, keep, (long)keep_ld);
  else if (dtype == MK_F16)
    MK_LAUNCH((sample_keep_kernel<_Float16>), dim3(rows), dim3(SNT), 0, st, (const _Float16*)logits, (long)ld, V,
              temperature, top_k, top_p, w, keep, (long)keep_ld);
  else if (dtype == MK_F32)
    MK_LAUNCH((sample_keep_kernel<float>), dim3(rows), dim3(SNT), 0, st, (const float*)logits, (long)ld, V, temperature,
              top_k, top_p, w, keep, (long)keep_ld);
  else return MK_ERR_UNSUPPORTED;
  return mk_check_launch();
}
