// Beam search for generate(num_beams=K): the whole bookkeeping of one decode step in one launch, with every piece of
// state on the device, so that a beam step stays a fixed launch sequence that one hipGraph replays per token (the beam
// twin of mk_decode_emit, decode.hip, and mk_decode_emit_sample, sample.hip; classic HF BeamSearchScorer semantics: the
// rule is written down in include/macaw_hip.h and restated in tests/beam_ref.py).
//
// One workgroup of 1024 threads per sample.  Its K_in rows of logits are re-read from L2 for every pass; thread t owns
// the columns t, t + 1024, ... of every row (coalesced), and "lower flat index first" is decided by comparing indices,
// never by the order of arrival.  Everything that decides WHICH candidates win is exact:
//   lse_k    fp32 maximum; the sum of expf(x - max) accumulated in fp64 in a fixed order (thread, lane tree, wave order)
//   cand     s_k + (x_kc - lse_k) in fp32, two roundings, the same for every thread that recomputes it
//   key      the order-preserving uint32 image of cand (sample.hip's s_key): larger key <=> larger value
//   floor    every thread's best key; the 2K-th largest of those 1024 keys is a lower bound of the 2K-th largest
//            candidate (2K distinct candidates reach it), so the passes below skip nearly every column
//   select   sample.hip's 8-bit-per-pass radix select (256-bin LDS histogram of counts) for the 2K-th largest key Kt and
//            how many of its tie group are still admitted, r; when r cuts the tie group, a second select over the
//            inverted flat index k * V + c picks its r lowest members
//   order    the <= 2K winners are ranked by (key descending, flat index ascending) in LDS; thread 0 walks them
// The indirection table is updated IN PLACE: column i of the sample's table (the slots that hold key S0 + i for its K
// beams) is permuted by exactly one thread, which reads its K entries before it writes any; columns do not depend on
// each other, so the only barrier needed is the one that publishes the parents.  No second table, no parity.
#include "common.h"
#include "../../include/macaw_hip.h"
#include <math.h>

namespace {

typedef uint32_t u32;
constexpr int BNT = 1024;                       // threads per sample
constexpr int BKM = 16;                         // most beams
constexpr int BCM = 2 * BKM;                    // most ranked candidates

struct BeamLds {
  u32 hist[256];
  int digit;
  u32 above, tie;                               // radix select: weight above the digit found / weight of the digit
  float wmax[BKM][BNT / 64];
  double wsum[BKM][BNT / 64];
  float s_in[BKM], lse[BKM];
  int cn;
  u32 ckey[BCM], cidx[BCM], skey[BCM], sidx[BCM];
  int parent[BKM];
  long ntok[BKM];
  float nscore[BKM];
};

MK_DEV bool b_logit_ok(float v) { return !__builtin_isnan(v) && v != -INFINITY; }
MK_DEV bool b_finite(float v) { return fabsf(v) < INFINITY; }     // false for NaN
MK_DEV u32 b_key(float x) {
  if (x == 0.f) x = 0.f;                        // -0 == +0: one key
  const u32 u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
MK_DEV float b_unkey(u32 k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// Radix select over the keys `each` enumerates (every thread its own; all keys non-zero), each of weight 1: the key Kt
// with #(keys > Kt) < target <= #(keys >= Kt), rem = target - #(keys > Kt) and tie = #(keys == Kt).  False (uniformly)
// when fewer than target keys exist.
template <typename Each>
__device__ bool b_radix_select(Each each, u32 target, BeamLds& s, u32& Kt, u32& rem, u32& tie) {
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

struct BeamArgs {
  const void* logits; long ld; int V, B, K, K_in;
  long pad, eos;
  float lp; int early;
  int64_t* tok; float* scores; int32_t* hist; int32_t* ind; int n_max;
  float* pool_score; int32_t* pool_info; unsigned char* done; int32_t* state;
};

template <typename T>
__global__ __launch_bounds__(BNT) void beam_emit_kernel(BeamArgs a) {
  __shared__ BeamLds s;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = a.K, K_in = a.K_in, V = a.V;
  const int col = a.state[1];                   // read by every thread before this workgroup's arrival below
  const bool in_books = col >= 0 && col < a.n_max;          // the history and the table have a column for this step
  const bool fin = a.done[b];
  const long bK = (long)b * K;
  const T* rows = (const T*)a.logits + (long)b * K_in * a.ld;

  if (!fin) {
    if (tid < BKM) s.s_in[tid] = tid < K_in ? a.scores[bK + tid] : -INFINITY;
    // ---- lse of every row: maximum, then the fp64 sum of expf(x - max)
    for (int k = 0; k < K_in; ++k) {
      const T* xr = rows + (long)k * a.ld;
      float m = -INFINITY;
      for (int c = tid; c < V; c += BNT) {
        const float v = to_f32<T>(xr[c]);
        if (b_logit_ok(v)) m = fmaxf(m, v);
      }
      m = wave_max(m);
      if (lane == 0) s.wmax[k][wave] = m;
    }
    __syncthreads();
    for (int k = 0; k < K_in; ++k) {
      float m = s.wmax[k][0];
#pragma unroll
      for (int w = 1; w < BNT / 64; ++w) m = fmaxf(m, s.wmax[k][w]);
      double sum = 0.0;
      if (b_finite(m)) {
        const T* xr = rows + (long)k * a.ld;
        for (int c = tid; c < V; c += BNT) {
          const float v = to_f32<T>(xr[c]);
          if (b_logit_ok(v)) sum += (double)expf(v - m);
        }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
      if (lane == 0) s.wsum[k][wave] = sum;
    }
    __syncthreads();
    if (tid < K_in) {
      float m = s.wmax[tid][0];
      double sum = s.wsum[tid][0];
      for (int w = 1; w < BNT / 64; ++w) { m = fmaxf(m, s.wmax[tid][w]); sum += s.wsum[tid][w]; }
      // a row without a finite logit, or with +inf in it, has no candidate: lse = +inf makes every cand -inf or NaN
      s.lse[tid] = (b_finite(m) && sum > 0.0) ? (float)((double)m + log(sum)) : INFINITY;
    }
    if (tid == 0) s.cn = 0;
    __syncthreads();

    // this thread's candidates as (key, flat index); a row whose score or lse leaves no finite cand is skipped whole
    auto each = [&](auto&& f) {
      for (int k = 0; k < K_in; ++k) {
        const float sk = s.s_in[k], ls = s.lse[k];
        if (!b_finite(sk) || !b_finite(ls)) continue;
        const T* xr = rows + (long)k * a.ld;
        for (int c = tid; c < V; c += BNT) {
          const float cd = sk + (to_f32<T>(xr[c]) - ls);
          if (b_finite(cd)) f(b_key(cd), (u32)(k * V + c));
        }
      }
    };
    // ---- floor: the 2K-th largest of the threads' best keys
    u32 best = 0;
    each([&](u32 k, u32) { best = max(best, k); });
    const u32 want = 2u * (u32)K;
    u32 floor_k = 1, rem = 0, tie = 0;
    if (!b_radix_select([&](auto&& f) { if (best) f(best); }, want, s, floor_k, rem, tie)) floor_k = 1;
    // ---- the 2K-th largest candidate key and how much of its tie group is admitted
    u32 Kt = 0;
    const bool full = b_radix_select([&](auto&& f) { each([&](u32 k, u32) { if (k >= floor_k) f(k); }); }, want, s, Kt,
                                     rem, tie);
    u32 imax = 0xffffffffu;                     // admitted members of the tie group: flat index <= imax
    if (!full) {
      Kt = 0;                                   // fewer than 2K candidates: all of them (no key is 0)
    } else if (rem < tie) {                     // the r = rem lowest flat indices of the tie group
      u32 It = 0, r2 = 0, t2 = 0;
      b_radix_select([&](auto&& f) { each([&](u32 k, u32 i) { if (k == Kt) f(~i); }); }, rem, s, It, r2, t2);
      imax = ~It;
    }
    // ---- gather the winners, rank them by (key descending, flat index ascending)
    each([&](u32 k, u32 i) {
      if (k > Kt || (full && k == Kt && i <= imax)) {
        const int at = atomicAdd(&s.cn, 1);
        if (at < BCM) { s.ckey[at] = k; s.cidx[at] = i; }
      }
    });
    __syncthreads();
    const int n = min(s.cn, (int)want);
    if (tid < n) {
      const u32 k = s.ckey[tid], i = s.cidx[tid];
      int rank = 0;
      for (int j = 0; j < n; ++j) rank += s.ckey[j] > k || (s.ckey[j] == k && s.cidx[j] < i);
      s.skey[rank] = k;
      s.sidx[rank] = i;
    }
    __syncthreads();
    // ---- the walk: eos hypotheses into the pool, the others become the next beams
    if (tid == 0) {
      const int L = col + 1;
      const float pen = powf((float)L, a.lp);
      float* ps = a.pool_score + bK;
      int32_t* pi = a.pool_info + (bK + b) * 4;           // [K + 1][4] per sample: (step, parent, seq, 0); row K = (n, seq)
      int pn = pi[K * 4], pseq = pi[K * 4 + 1];
      int filled = 0;
      for (int r = 0; r < n && filled < K; ++r) {
        const float cd = b_unkey(s.skey[r]);
        const int k = (int)(s.sidx[r] / (u32)V), c = (int)(s.sidx[r] % (u32)V);
        if ((long)c == a.eos) {
          if (r >= K) continue;
          const float sc = cd / pen;
          int at = -1;
          if (pn < K) {
            at = pn++;
          } else {                              // the worst entry, among equal worst the latest inserted
            int w = 0;
            for (int e = 1; e < K; ++e)
              if (ps[e] < ps[w] || (ps[e] == ps[w] && pi[e * 4 + 2] > pi[w * 4 + 2])) w = e;
            if (sc > ps[w]) at = w;
          }
          if (at >= 0) { ps[at] = sc; pi[at * 4] = col; pi[at * 4 + 1] = k; pi[at * 4 + 2] = pseq++; pi[at * 4 + 3] = 0; }
        } else {
          s.parent[filled] = k; s.ntok[filled] = c; s.nscore[filled] = cd;
          ++filled;
        }
      }
      for (; filled < K; ++filled) { s.parent[filled] = 0; s.ntok[filled] = a.pad; s.nscore[filled] = -INFINITY; }
      pi[K * 4] = pn;
      pi[K * 4 + 1] = pseq;
      if (pn >= K) {
        bool dn = a.early != 0;
        if (!dn) {
          float worst = ps[0];
          for (int e = 1; e < K; ++e) worst = fminf(worst, ps[e]);
          dn = s.nscore[0] / pen <= worst;
        }
        if (dn) a.done[b] = 1;
      }
    }
    __syncthreads();
  } else if (tid < K) {                         // a finished sample: its books stay, its rows are fed pad
    s.ntok[tid] = a.pad;
  }
  if (fin) __syncthreads();

  if (tid < K) {
    a.tok[bK + tid] = s.ntok[tid];
    if (!fin) a.scores[bK + tid] = s.nscore[tid];
    if (in_books) {
      int32_t* h = a.hist + (((long)col * a.B + b) * K + tid) * 2;
      h[0] = (int32_t)s.ntok[tid];
      h[1] = fin ? tid : s.parent[tid];
    }
  }
  if (!fin && in_books) {                       // table column i: new row j = old row parent[j] (read all, then write)
    for (int i = tid; i < col; i += BNT) {
      int32_t v[BKM];
#pragma unroll
      for (int j = 0; j < BKM; ++j)
        if (j < K) v[j] = a.ind[(bK + s.parent[j]) * a.n_max + i];
#pragma unroll
      for (int j = 0; j < BKM; ++j)
        if (j < K) a.ind[(bK + j) * a.n_max + i] = v[j];
    }
  }
  if (tid < K && in_books) a.ind[(bK + tid) * a.n_max + col] = tid;       // the token about to be fed goes to its own slot
  __syncthreads();
  if (tid == 0) {
    __threadfence();
    const int old = __hip_atomic_fetch_add(a.state + 2, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (old == (int)gridDim.x - 1) {            // every sample has read state[1]: advance the step
      a.state[0] += 1;
      a.state[1] = col + 1;
      a.state[2] = 0;
    }
  }
}

constexpr int BEAM_MAX_V = 1 << 23;             // 16 rows of 2^23 columns: a flat index stays inside 32 bits

}  // namespace

extern "C" int mk_beam_emit(const void* logits, int64_t ld, int32_t V, int32_t B, int32_t K, int32_t K_in, int64_t pad,
                            int64_t eos, float length_penalty, int32_t early_stopping, int64_t* tok, float* scores,
                            int32_t* hist, int32_t* ind, int32_t n_max, float* pool_score, int32_t* pool_info,
                            void* done, int32_t* state, int32_t dtype, void* stream) {
  if (!logits || !tok || !scores || !hist || !ind || !pool_score || !pool_info || !done || !state || B <= 0 ||
      K < 1 || K > BKM || (K_in != 1 && K_in != K) || V < 2 * K || ld < V || n_max <= 0 || !isfinite(length_penalty))
    return MK_ERR_BAD_ARG;
  if (V > BEAM_MAX_V) return MK_ERR_UNSUPPORTED;
  BeamArgs a;
  a.logits = logits; a.ld = (long)ld; a.V = V; a.B = B; a.K = K; a.K_in = K_in;
  a.pad = (long)pad; a.eos = (long)eos; a.lp = length_penalty; a.early = early_stopping;
  a.tok = tok; a.scores = scores; a.hist = hist; a.ind = ind; a.n_max = n_max;
  a.pool_score = pool_score; a.pool_info = pool_info; a.done = (unsigned char*)done; a.state = state;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (dtype == MK_BF16) MK_LAUNCH((beam_emit_kernel<bf16>), dim3(B), dim3(BNT), 0, st, a);
  else if (dtype == MK_F16) MK_LAUNCH((beam_emit_kernel<_Float16>), dim3(B), dim3(BNT), 0, st, a);
  else if (dtype == MK_F32) MK_LAUNCH((beam_emit_kernel<float>), dim3(B), dim3(BNT), 0, st, a);
  else return MK_ERR_UNSUPPORTED;
  return mk_check_launch();
}
