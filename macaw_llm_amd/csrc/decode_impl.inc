// 16-bit-element kernels of decode.hip (decode attention, fused RoPE + append + attention step) and their
// entry points, included once per element type (MK_E16_T / MK_E16_NS): e16 = bf16 or _Float16.
namespace {
namespace MK_E16_NS {
typedef MK_E16_T e16;
typedef E16<e16>::x8 e16x8;
typedef E16<e16>::x4 e16x4;
typedef e16 e16x2 __attribute__((ext_vector_type(2)));
struct DecodeArgs {
  const e16* q; const e16* k; const e16* v; e16* o;
  const int32_t* t_dev;
  int t_add, t_max;
  long q_bs, k_ld, k_bs, v_ld, v_bs, o_bs;
  float scale;
};

// One workgroup per (head, sample); LPK = HD / 8 lanes share a key (16 bytes each: a key row is
// one coalesced HD * 2-byte segment), 64 / LPK keys per wave and pass, 4 waves.
//   pass 1  scores s_t = scale * q . k_t  -> LDS, running maximum
//   pass 2  p_t = exp(s_t - max), sum
//   pass 3  o = sum_t p_t v_t / sum   (fp32 accumulation; one rounding to e16)
template <int HD>
__global__ __launch_bounds__(256) void decode_attn_kernel(DecodeArgs a) {
  constexpr int LPK = HD / 8, KPW = 64 / LPK, KPP = 4 * KPW;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* sc = reinterpret_cast<float*>(smem_raw);          // [t_max] scores / probabilities
  __shared__ float red[4][HD];
  __shared__ float redw[8];
  const int h = blockIdx.x, b = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int T = min(max(*a.t_dev + a.t_add, 1), a.t_max);
  const int sub = lane % LPK, grp = lane / LPK;            // my 8 dims / my key inside the wave's pass
  const e16* Q = a.q + (long)b * a.q_bs + (long)h * HD + sub * 8;
  const e16* K = a.k + (long)b * a.k_bs + (long)h * HD + sub * 8;
  const e16* V = a.v + (long)b * a.v_bs + (long)h * HD + sub * 8;
  float qf[8];
  {
    const e16x8 qv = *reinterpret_cast<const e16x8*>(Q);
#pragma unroll
    for (int e = 0; e < 8; ++e) qf[e] = (float)qv[e];
  }
  // ---- pass 1
  float mx = -INFINITY;
  for (int t0 = 0; t0 < T; t0 += KPP) {
    const int t = t0 + wave * KPW + grp;
    float s = 0.f;
    if (t < T) {
      const e16x8 kv = *reinterpret_cast<const e16x8*>(K + (long)t * a.k_ld);
#pragma unroll
      for (int e = 0; e < 8; ++e) s += qf[e] * (float)kv[e];
    }
#pragma unroll
    for (int o = 1; o < LPK; o <<= 1) s += __shfl_xor(s, o, 64);
    s *= a.scale;
    if (t < T) {
      if (sub == 0) sc[t] = s;
      mx = fmaxf(mx, s);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  if (lane == 0) redw[wave] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(redw[0], redw[1]), fmaxf(redw[2], redw[3]));
  // ---- pass 2
  float sum = 0.f;
  for (int t = tid; t < T; t += 256) {
    const float p = __expf(sc[t] - mx);
    sc[t] = p;
    sum += p;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
  if (lane == 0) redw[4 + wave] = sum;
  __syncthreads();
  sum = redw[4] + redw[5] + redw[6] + redw[7];
  // ---- pass 3
  float acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = 0.f;
  for (int t0 = 0; t0 < T; t0 += KPP) {
    const int t = t0 + wave * KPW + grp;
    if (t < T) {
      const float p = sc[t];
      const e16x8 vv = *reinterpret_cast<const e16x8*>(V + (long)t * a.v_ld);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] += p * (float)vv[e];
    }
  }
  // keys of one wave: lanes with the same `sub`
#pragma unroll
  for (int o = LPK; o < 64; o <<= 1)
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] += __shfl_xor(acc[e], o, 64);
  if (grp == 0) {
#pragma unroll
    for (int e = 0; e < 8; ++e) red[wave][sub * 8 + e] = acc[e];
  }
  __syncthreads();
  if (tid < HD) {
    const float v = (red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid]) / sum;
    a.o[(long)b * a.o_bs + (long)h * HD + tid] = (e16)v;
  }
}

// The whole attention block of a decode step in ONE launch: RoPE of the new query and key
// (modeling.py:76-91, same rounding points as rope_kernel: each product and the sum rounded to
// e16), append of the rotated key and the value to cache row p = *t_dev, and the attention of the
// query over keys 0 ... p (the new key / value straight from registers).  NWV waves per (head, sample).
struct DecodeStepArgs {
  const e16* q; const e16* kn; const e16* vn; long in_bs;   // new rows [H * hd] per sample
  const e16* cos_t; const e16* sin_t;                       // [positions][hd]
  e16* kc; e16* vc; long kv_ld, kv_bs;                      // caches [t_max][H * hd] per sample
  e16* o; long o_bs;
  const int32_t* t_dev;
  int t_max;
  float scale;
  const int32_t* t_off;                                     // VAR kernels only: [B] per-sample offsets to *t_dev
};

// BEAM kernels only (mk_decode_step_attn_beam): the launch's rows are (sample, beam) pairs of a [B][K][t_max][2D] cache
struct DecodeStepBeamArgs : DecodeStepArgs {
  const int32_t* ind;                                       // [B * K][n_ind]: slot that holds key S0 + i of a row
  int K, S0, n_ind;
};
template <bool BEAM> struct StepArgsOf { typedef DecodeStepArgs type; };
template <> struct StepArgsOf<true> { typedef DecodeStepBeamArgs type; };

MK_DEV float rnd_e16(float x) { return rnd<e16>(x); }

// BEAM: the element offset from a row's OWN cache slot to the slot that holds its key t -- slot 0 of the sample for the
// shared prompt (t < S0), slot ind[row][t - S0] behind it (clamped into [0, K): an address, whatever the table holds).
// Everything after the address of a key is the plain kernel's code, so a row's arithmetic is that of the plain kernel
// on a physically gathered cache.
template <bool BEAM, typename A>
MK_DEV long beam_slot_off(const A& a, int row, int t) {
  if constexpr (BEAM) {
    int s = 0;
    if (t >= a.S0) s = min(max(a.ind[(long)row * a.n_ind + (t - a.S0)], 0), a.K - 1);
    return (long)(s - row % a.K) * a.kv_bs;
  } else {
    return 0;
  }
}

// VAR (mk_decode_step_attn_var): p = clamp(*t_dev + t_off[b]) per sample, a padded batch's ragged cache; everything
// after p is the same code, so a sample's arithmetic is that of the plain kernel at *t_dev = p.
// RoPE of the 8 elements a lane holds of a head's row (its partner half comes from lane +- LPK / 2), rope_kernel's
// rounding points: each product and the sum rounded to e16.  first half: x cos - partner sin; second half: x cos + partner sin
template <int LPK>
MK_DEV void rope8(const e16x8& xv, const e16x8& cv, const e16x8& sv, bool first, float (&out)[8]) {
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float cs = (float)cv[e], sn = (float)sv[e];
    const float xo = (float)xv[e];
    const float xp = __shfl_xor(xo, LPK / 2, 64);
    const float sx = first ? rnd_e16(-xp * sn) : rnd_e16(xp * sn);
    out[e] = rnd_e16(rnd_e16(xo * cs) + sx);
  }
}

// The step of ONE query row at position p, shared by every form of the kernel: the new q / k / v row at element offset
// in_row, the output row at o_row, b = the sample (BEAM: the row) whose cache slot the row appends to and reads.
// MULTI (mk_decode_step_attn_multi): keys p0 ... p - 1 are the EARLIER rows of the same step, which other workgroups append
// at the same time: their rotated keys come from knew (LDS, rotated by this workgroup) and their values from the step's
// v_new rows (row 0 of the sample at element offset vn0) -- the bits the cache will hold -- and no cache row >= p0 is read.
// SHARED (mk_decode_step_attn_shared): b = the ROW, whose slot of a.kc / a.vc is its tail cache, p0 = the prompt's length:
// key t < p0 is row t of the prompt cache of sample b / a.n, key p0 <= t < p tail row t - p0, and the new key goes to tail
// row p - p0.  Only the address of a key differs.
// APPEND = false (mk_score_attn): the row's rotated key and value are already in the tail cache (score_append_kernel wrote
// them, the same rope8 bits) and the body stores nothing but o; key p still comes from registers.
template <int HD, int NWV, bool BEAM, bool MULTI = false, bool SHARED = false, bool APPEND = true, typename A>
MK_DEV void decode_step_attn_body(const A& a, float (*red)[HD], float* redw, int h, int b, long in_row, long o_row, int p,
                                  int p0 = 0, const e16 (*knew)[HD] = nullptr, long vn0 = 0) {
  constexpr int LPK = HD / 8, KPW = 64 / LPK, KPP = NWV * KPW;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int T = p + 1;
  const int sub = lane % LPK, grp = lane / LPK;
  const int d0 = sub * 8;
  const bool first = d0 < HD / 2;
  const long in_off = in_row + (long)h * HD + d0;
  float qf[8], kf[8];
  e16x8 vnew = *reinterpret_cast<const e16x8*>(a.vn + in_off);
  {
    const e16x8 qv = *reinterpret_cast<const e16x8*>(a.q + in_off);
    const e16x8 kv = *reinterpret_cast<const e16x8*>(a.kn + in_off);
    const e16x8 cv = *reinterpret_cast<const e16x8*>(a.cos_t + (long)p * HD + d0);
    const e16x8 sv = *reinterpret_cast<const e16x8*>(a.sin_t + (long)p * HD + d0);
    rope8<LPK>(qv, cv, sv, first, qf);
    rope8<LPK>(kv, cv, sv, first, kf);
  }
  if constexpr (APPEND) {
    if (wave == 0 && grp == 0) {   // append the new key / value (cache row p)
      e16x8 kb;
#pragma unroll
      for (int e = 0; e < 8; ++e) kb[e] = (e16)kf[e];
      long off = (long)b * a.kv_bs + (long)p * a.kv_ld + (long)h * HD + d0;
      if constexpr (SHARED) off = (long)b * a.kv_bs + (long)(p - p0) * a.kv_ld + (long)h * HD + d0;
      *reinterpret_cast<e16x8*>(a.kc + off) = kb;
      *reinterpret_cast<e16x8*>(a.vc + off) = vnew;
    }
  }
  const e16* K = a.kc + (long)b * a.kv_bs + (long)h * HD + d0;
  const e16* V = a.vc + (long)b * a.kv_bs + (long)h * HD + d0;
  // Key t belongs to lane group (wave, grp), t = wave * KPW + grp (mod KPP); NB keys per group and
  // trip, their K AND V rows requested together (one memory round trip per KPP * NB keys: a 7B decode
  // step at a few hundred tokens is latency, not bandwidth), online softmax across trips.
  constexpr int NB = 8;
  float m_run = -INFINITY, lsum = 0.f, acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = 0.f;
  for (int t0 = wave * KPW + grp; t0 < T; t0 += KPP * NB) {
    e16x8 kv[NB], vv[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const int t = t0 + j * KPP;
      if (MULTI && t >= p0 && t < p) {
        kv[j] = *reinterpret_cast<const e16x8*>(&knew[t - p0][d0]);
        vv[j] = *reinterpret_cast<const e16x8*>(a.vn + vn0 + (long)(t - p0) * a.in_bs + (long)h * HD + d0);
      } else if (t < p) {
        if constexpr (SHARED) {
          const long po = (long)(b / a.n) * a.p_bs + (long)t * a.p_ld + (long)h * HD + d0;
          kv[j] = *reinterpret_cast<const e16x8*>(t < p0 ? a.kp + po : K + (long)(t - p0) * a.kv_ld);
          vv[j] = *reinterpret_cast<const e16x8*>(t < p0 ? a.vp + po : V + (long)(t - p0) * a.kv_ld);
        } else {
          const long so = beam_slot_off<BEAM>(a, b, t);
          kv[j] = *reinterpret_cast<const e16x8*>(K + so + (long)t * a.kv_ld);
          vv[j] = *reinterpret_cast<const e16x8*>(V + so + (long)t * a.kv_ld);
        }
      } else {
        vv[j] = vnew;
      }
    }
    float sj[NB], mt = m_run;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const int t = t0 + j * KPP;
      float s = 0.f;
      if (t < p) {
#pragma unroll
        for (int e = 0; e < 8; ++e) s += qf[e] * (float)kv[j][e];
      } else if (t == p) {
#pragma unroll
        for (int e = 0; e < 8; ++e) s += qf[e] * kf[e];
      }
#pragma unroll
      for (int o = 1; o < LPK; o <<= 1) s += __shfl_xor(s, o, 64);
      sj[j] = t < T ? s * a.scale : -INFINITY;
      mt = fmaxf(mt, sj[j]);
    }
    const float corr = __expf(m_run - mt);       // (0 on the first trip: m_run = -inf, mt finite)
    lsum *= corr;
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] *= corr;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const float pr = __expf(sj[j] - mt);       // exp(-inf) = 0 for keys past the end
      lsum += pr;
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] += pr * (float)vv[j][e];
    }
    m_run = mt;
  }
  // merge the lane groups: common maximum, then rescaled sums
  float mx = m_run;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  if (lane == 0) redw[wave] = mx;
  __syncthreads();
  mx = redw[0];
#pragma unroll
  for (int i = 1; i < NWV; ++i) mx = fmaxf(mx, redw[i]);
  {
    const float corr = __expf(m_run - mx);       // groups without a key: m_run = -inf -> 0
    lsum *= corr;
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] *= corr;
  }
#pragma unroll
  for (int o = LPK; o < 64; o <<= 1) {
    lsum += __shfl_xor(lsum, o, 64);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] += __shfl_xor(acc[e], o, 64);
  }
  if (grp == 0) {
#pragma unroll
    for (int e = 0; e < 8; ++e) red[wave][d0 + e] = acc[e];
  }
  if (lane == 0) redw[NWV + wave] = lsum;
  __syncthreads();
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < NWV; ++i) sum += redw[NWV + i];
  if (tid < HD) {
    float v = 0.f;
#pragma unroll
    for (int i = 0; i < NWV; ++i) v += red[i][tid];
    a.o[o_row + (long)h * HD + tid] = (e16)(v / sum);
  }
}

template <int HD, int NWV, bool VAR = false, bool BEAM = false>
__global__ __launch_bounds__(NWV * 64) void decode_step_attn_kernel(typename StepArgsOf<BEAM>::type a) {
  __shared__ float red[NWV][HD];
  __shared__ float redw[2 * NWV];
  const int h = blockIdx.x, b = blockIdx.y;
  int tp = *a.t_dev;
  if constexpr (VAR) tp += a.t_off[b];
  const int p = min(max(tp, 0), a.t_max - 1);
  decode_step_attn_body<HD, NWV, BEAM>(a, red, redw, h, b, (long)b * a.in_bs, (long)b * a.o_bs, p);
}

// MULTI (mk_decode_step_attn_multi): Q query rows per sample, row (b, g) at position pos[b] + g (a.t_dev = pos [B]).  One
// workgroup per (head, sample, ROW), so the Q rows of a step run side by side at the latency of one plain launch.  Row g
// appends cache row pos[b] + g and attends over rows 0 ... pos[b] + g; the g rows before it belong to the same step and are
// being appended by its sister workgroups, so it rotates their keys itself (one lane group per row, into LDS) and takes
// their values from the step's input: the same bits, no cross-workgroup order needed.  Everything else IS the plain
// kernel's code -- the same key -> lane / wave assignment and reduction order, so the same bits.  With H a multiple of 8
// the Q workgroups of a (head, sample) have linear ids H apart and land on one XCD: the cached prefix is read from HBM once
// and from that XCD's L2 by the others.  A row at or past t_max appends nothing and its output is zeros.
constexpr int MULTI_MAX_Q = 16;
template <int HD, int NWV>
__global__ __launch_bounds__(NWV * 64) void decode_step_attn_multi_kernel(DecodeStepArgs a, int Q) {
  constexpr int LPK = HD / 8, KPW = 64 / LPK;
  static_assert(NWV * KPW >= MULTI_MAX_Q - 1, "one lane group per earlier row");
  __shared__ float red[NWV][HD];
  __shared__ float redw[2 * NWV];
  __shared__ __attribute__((aligned(16))) e16 knew[MULTI_MAX_Q - 1][HD];
  const int h = blockIdx.x, b = blockIdx.y / Q, g = blockIdx.y % Q;
  const long row = blockIdx.y;
  const int p0 = max(a.t_dev[b], 0);
  if (p0 >= a.t_max - g) {             // (p0 + g cannot overflow here)
    if (threadIdx.x < HD) a.o[row * a.o_bs + (long)h * HD + threadIdx.x] = (e16)0.f;
    return;
  }
  if (g > 0) {                         // the rotated keys of rows 0 ... g - 1: lane group (wave, grp) takes row wave * KPW + grp
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane % LPK, grp = lane / LPK, d0 = sub * 8;
    const int jr = wave * KPW + grp, jc = min(jr, g - 1);        // (every lane runs the shuffles: a clamped row)
    const e16x8 kv = *reinterpret_cast<const e16x8*>(a.kn + ((long)b * Q + jc) * a.in_bs + (long)h * HD + d0);
    const e16x8 cv = *reinterpret_cast<const e16x8*>(a.cos_t + (long)(p0 + jc) * HD + d0);
    const e16x8 sv = *reinterpret_cast<const e16x8*>(a.sin_t + (long)(p0 + jc) * HD + d0);
    float kf[8];
    rope8<LPK>(kv, cv, sv, d0 < HD / 2, kf);
    if (jr < g) {
      e16x8 kb;
#pragma unroll
      for (int e = 0; e < 8; ++e) kb[e] = (e16)kf[e];
      *reinterpret_cast<e16x8*>(&knew[jr][d0]) = kb;
    }
    __syncthreads();
  }
  decode_step_attn_body<HD, NWV, false, true>(a, red, redw, h, b, row * a.in_bs, row * a.o_bs, p0 + g, p0, knew,
                                              (long)b * Q * a.in_bs);
}

// Greedy token selection and the bookkeeping of a decode step in one launch (HF greedy_search as the
// reference calls it, modeling.py:959: argmax, pad for finished samples, eos marks a sample
// finished): one workgroup per sample; the last workgroup to finish advances the step state.
//   state[0] = position of the token being fed (t_dev of the other decode kernels), state[1] = output
//   column, state[2] = arrival counter (zero between launches).

// The same step for MANY (sample, head) pairs (B x H >= 512: batch >= 16 at 32 heads): one workgroup per
// (sample, FOUR adjacent heads).  The cache row of a token is [k of all heads | v of all heads]: with one workgroup
// per head (above) every 16-byte lane load belongs to a 256-byte segment whose neighbours are 16 KB apart, and at
// B = 32 the launch is 1024 workgroups reading 75 MB in such segments: 34.8 us per layer = 2.2 TB/s, DRAM-page
// bound (r03_decode_step_B32.txt).  Here a WAVE reads one key of four heads = 1 KiB of contiguous memory per load
// (lanes 16 g ... 16 g + 15 <-> head 4 x + g), the eight waves take keys t = wave, wave + 8, ..., eight keys per
// lane in flight (64 keys per trip), and the grid is B x H / 4 = 256 workgroups at B = 32: one per CU, one round.
// Partial results meet in LDS per head (8 waves x 4 heads).  hd = 128 only.
template <int NWV, bool VAR = false, bool BEAM = false>
__global__ __launch_bounds__(NWV * 64) void decode_step_attn4_kernel(typename StepArgsOf<BEAM>::type a) {
  constexpr int HD = 128, LPK = 16, HG = 4;
  __shared__ float red[NWV][HG * HD];
  __shared__ float redm[NWV][HG], reds[NWV][HG];
  const int b = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int grp = lane / LPK, sub = lane % LPK;
  const int h = blockIdx.x * HG + grp;
  int tp = *a.t_dev;
  if constexpr (VAR) tp += a.t_off[b];
  const int p = min(max(tp, 0), a.t_max - 1);
  const int T = p + 1;
  const int d0 = sub * 8;
  const bool first = d0 < HD / 2;
  const long in_off = (long)b * a.in_bs + (long)h * HD + d0;
  float qf[8], kf[8];
  e16x8 vnew = *reinterpret_cast<const e16x8*>(a.vn + in_off);
  {
    const e16x8 qv = *reinterpret_cast<const e16x8*>(a.q + in_off);
    const e16x8 kv = *reinterpret_cast<const e16x8*>(a.kn + in_off);
    const e16x8 cv = *reinterpret_cast<const e16x8*>(a.cos_t + (long)p * HD + d0);
    const e16x8 sv = *reinterpret_cast<const e16x8*>(a.sin_t + (long)p * HD + d0);
#pragma unroll
    for (int e = 0; e < 8; ++e) {        // RoPE with rope_kernel's rounding points (see decode_step_attn_kernel)
      const float cs = (float)cv[e], sn = (float)sv[e];
      const float qo = (float)qv[e], ko = (float)kv[e];
      const float qp = __shfl_xor(qo, LPK / 2, 64), kp = __shfl_xor(ko, LPK / 2, 64);
      const float sq = first ? rnd_e16(-qp * sn) : rnd_e16(qp * sn);
      const float sk = first ? rnd_e16(-kp * sn) : rnd_e16(kp * sn);
      qf[e] = rnd_e16(rnd_e16(qo * cs) + sq);
      kf[e] = rnd_e16(rnd_e16(ko * cs) + sk);
    }
  }
  if (wave == 0) {                       // append the new key / value of this lane group's head (cache row p)
    e16x8 kb;
#pragma unroll
    for (int e = 0; e < 8; ++e) kb[e] = (e16)kf[e];
    const long off = (long)b * a.kv_bs + (long)p * a.kv_ld + (long)h * HD + d0;
    *reinterpret_cast<e16x8*>(a.kc + off) = kb;
    *reinterpret_cast<e16x8*>(a.vc + off) = vnew;
  }
  const e16* K = a.kc + (long)b * a.kv_bs + (long)h * HD + d0;
  const e16* V = a.vc + (long)b * a.kv_bs + (long)h * HD + d0;
  constexpr int NB = 8;          // (16 keys per lane and trip: 220 VGPRs, spills in the f16 build, 5.85 vs 5.49 ms per token)
  float m_run = -INFINITY, lsum = 0.f, acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = 0.f;
  for (int t0 = wave; t0 < T; t0 += NWV * NB) {
    e16x8 kv[NB], vv[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) {       // unconditional loads from a clamped row (no branch around a load)
      const int tc = min(t0 + j * NWV, max(p - 1, 0));
      const long so = beam_slot_off<BEAM>(a, b, tc);
      kv[j] = *reinterpret_cast<const e16x8*>(K + so + (long)tc * a.kv_ld);
      vv[j] = *reinterpret_cast<const e16x8*>(V + so + (long)tc * a.kv_ld);
    }
    float sj[NB], mt = m_run;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const int t = t0 + j * NWV;
      float s = 0.f, sn = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) { s += qf[e] * (float)kv[j][e]; sn += qf[e] * kf[e]; }
      s = t < p ? s : sn;                 // (t >= p: the clamped row's values never enter the arithmetic)
#pragma unroll
      for (int o = 1; o < LPK; o <<= 1) s += __shfl_xor(s, o, 64);
      sj[j] = t < T ? s * a.scale : -INFINITY;
      mt = fmaxf(mt, sj[j]);
    }
    const float corr = __expf(m_run - mt);
    lsum *= corr;
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] *= corr;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const int t = t0 + j * NWV;
      const float pr = __expf(sj[j] - mt);       // exp(-inf) = 0 for keys past the end
      lsum += pr;
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] += pr * (t < p ? (float)vv[j][e] : (float)vnew[e]);
    }
    m_run = mt;
  }
  // merge the eight waves per head: common maximum, then rescaled sums
  if (sub == 0) redm[wave][grp] = m_run;
  __syncthreads();
  float mx = redm[0][grp];
#pragma unroll
  for (int i = 1; i < NWV; ++i) mx = fmaxf(mx, redm[i][grp]);
  {
    const float corr = __expf(m_run - mx);       // waves without a key: m_run = -inf -> 0
    lsum *= corr;
#pragma unroll
    for (int e = 0; e < 8; ++e) red[wave][grp * HD + d0 + e] = acc[e] * corr;
  }
  if (sub == 0) reds[wave][grp] = lsum;
  __syncthreads();
  if (tid < HG * HD) {
    const int g = tid / HD;
    float sum = 0.f, v = 0.f;
#pragma unroll
    for (int i = 0; i < NWV; ++i) { sum += reds[i][g]; v += red[i][tid]; }
    a.o[(long)b * a.o_bs + (long)(blockIdx.x * HG) * HD + tid] = (e16)(v / sum);
  }
}

int decode_step_attn_impl(const void* q, const void* k_new, const void* v_new, int64_t in_bs,
                                   const void* cos_t, const void* sin_t, void* k_cache, void* v_cache,
                                   int64_t kv_ld, int64_t kv_bs, void* o, int64_t o_bs,
                                   const int32_t* t_dev, int32_t t_max, int32_t B, int32_t H,
                                   int32_t hd, float scale, int32_t dtype, void* stream,
                                   bool var = false, const int32_t* t_off = nullptr) {
  if (!q || !k_new || !v_new || !cos_t || !sin_t || !k_cache || !v_cache || !o || !t_dev || B <= 0 ||
      H <= 0 || t_max <= 0 || (var && !t_off))
    return MK_ERR_BAD_ARG;
  if (dtype != E16<e16>::dtype || (hd != 16 && hd != 32 && hd != 64 && hd != 128)) return MK_ERR_UNSUPPORTED;
  const uintptr_t al = reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k_new) |
                       reinterpret_cast<uintptr_t>(v_new) | reinterpret_cast<uintptr_t>(cos_t) |
                       reinterpret_cast<uintptr_t>(sin_t) | reinterpret_cast<uintptr_t>(k_cache) |
                       reinterpret_cast<uintptr_t>(v_cache);
  if ((al & 15) || (in_bs % 8) || (kv_ld % 8) || (kv_bs % 8)) return MK_ERR_UNSUPPORTED;
  DecodeStepArgs a;
  a.q = (const e16*)q; a.kn = (const e16*)k_new; a.vn = (const e16*)v_new; a.in_bs = in_bs;
  a.cos_t = (const e16*)cos_t; a.sin_t = (const e16*)sin_t;
  a.kc = (e16*)k_cache; a.vc = (e16*)v_cache; a.kv_ld = kv_ld; a.kv_bs = kv_bs;
  a.o = (e16*)o; a.o_bs = o_bs;
  a.t_dev = t_dev; a.t_max = t_max; a.scale = scale; a.t_off = t_off;
  dim3 grid(H, B), block(512);
  const size_t lds = 0;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  static const bool no4 = getenv("MK_DECODE_ATTN_NO4") != nullptr;
  if (var) {          // the same selection, the per-sample-position instantiations
    if (hd == 128 && (H % 4) == 0 && (long)B * H >= 512 && !no4)
      MK_LAUNCH((decode_step_attn4_kernel<8, true>), dim3(H / 4, B), block, lds, st, a);
    else if (hd == 128) MK_LAUNCH((decode_step_attn_kernel<128, 8, true>), grid, block, lds, st, a);
    else if (hd == 64) MK_LAUNCH((decode_step_attn_kernel<64, 8, true>), grid, block, lds, st, a);
    else if (hd == 32) MK_LAUNCH((decode_step_attn_kernel<32, 8, true>), grid, block, lds, st, a);
    else MK_LAUNCH((decode_step_attn_kernel<16, 8, true>), grid, block, lds, st, a);
    return mk_check_launch();
  }
  if (hd == 128 && (H % 4) == 0 && (long)B * H >= 512 && !no4)
    MK_LAUNCH((decode_step_attn4_kernel<8>), dim3(H / 4, B), block, lds, st, a);
  else if (hd == 128) MK_LAUNCH((decode_step_attn_kernel<128, 8>), grid, block, lds, st, a);
  else if (hd == 64) MK_LAUNCH((decode_step_attn_kernel<64, 8>), grid, block, lds, st, a);
  else if (hd == 32) MK_LAUNCH((decode_step_attn_kernel<32, 8>), grid, block, lds, st, a);
  else MK_LAUNCH((decode_step_attn_kernel<16, 8>), grid, block, lds, st, a);
  return mk_check_launch();
}

// mk_decode_step_attn_multi: the plain entry point's checks over B * Q rows, positions per sample from pos [B]
int decode_step_attn_multi_impl(const void* q, const void* k_new, const void* v_new, int64_t in_bs, const void* cos_t,
                                const void* sin_t, void* k_cache, void* v_cache, int64_t kv_ld, int64_t kv_bs, void* o,
                                int64_t o_bs, const int32_t* pos, int32_t t_max, int32_t B, int32_t Q, int32_t H,
                                int32_t hd, float scale, int32_t dtype, void* stream) {
  if (!q || !k_new || !v_new || !cos_t || !sin_t || !k_cache || !v_cache || !o || !pos || B <= 0 || H <= 0 ||
      t_max <= 0 || Q < 1)
    return MK_ERR_BAD_ARG;
  if (dtype != E16<e16>::dtype || (hd != 16 && hd != 32 && hd != 64 && hd != 128) || Q > MULTI_MAX_Q) return MK_ERR_UNSUPPORTED;
  const uintptr_t al = reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k_new) |
                       reinterpret_cast<uintptr_t>(v_new) | reinterpret_cast<uintptr_t>(cos_t) |
                       reinterpret_cast<uintptr_t>(sin_t) | reinterpret_cast<uintptr_t>(k_cache) |
                       reinterpret_cast<uintptr_t>(v_cache);
  if ((al & 15) || (reinterpret_cast<uintptr_t>(pos) & 3) || (in_bs % 8) || (kv_ld % 8) || (kv_bs % 8))
    return MK_ERR_UNSUPPORTED;
  DecodeStepArgs a;
  a.q = (const e16*)q; a.kn = (const e16*)k_new; a.vn = (const e16*)v_new; a.in_bs = in_bs;
  a.cos_t = (const e16*)cos_t; a.sin_t = (const e16*)sin_t;
  a.kc = (e16*)k_cache; a.vc = (e16*)v_cache; a.kv_ld = kv_ld; a.kv_bs = kv_bs;
  a.o = (e16*)o; a.o_bs = o_bs;
  a.t_dev = pos; a.t_max = t_max; a.scale = scale; a.t_off = nullptr;
  dim3 grid(H, B * Q), block(512);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (hd == 128) MK_LAUNCH((decode_step_attn_multi_kernel<128, 8>), grid, block, 0, st, a, (int)Q);
  else if (hd == 64) MK_LAUNCH((decode_step_attn_multi_kernel<64, 8>), grid, block, 0, st, a, (int)Q);
  else if (hd == 32) MK_LAUNCH((decode_step_attn_multi_kernel<32, 8>), grid, block, 0, st, a, (int)Q);
  else MK_LAUNCH((decode_step_attn_multi_kernel<16, 8>), grid, block, 0, st, a, (int)Q);
  return mk_check_launch();
}

// mk_decode_step_attn_beam: the plain entry point's checks and kernel selection over B * K rows, plus the table
int decode_step_attn_beam_impl(const void* q, const void* k_new, const void* v_new, int64_t in_bs, const void* cos_t,
                               const void* sin_t, void* k_cache, void* v_cache, int64_t kv_ld, int64_t kv_bs, void* o,
                               int64_t o_bs, const int32_t* t_dev, const int32_t* ind, int32_t n_ind, int32_t S0,
                               int32_t t_max, int32_t B, int32_t K, int32_t H, int32_t hd, float scale, int32_t dtype,
                               void* stream) {
  if (!q || !k_new || !v_new || !cos_t || !sin_t || !k_cache || !v_cache || !o || !t_dev || !ind || B <= 0 || H <= 0 ||
      t_max <= 0 || K < 1 || K > 16 || S0 < 0 || S0 > t_max || n_ind < 1 || n_ind < t_max - S0)
    return MK_ERR_BAD_ARG;
  if (dtype != E16<e16>::dtype || (hd != 16 && hd != 32 && hd != 64 && hd != 128)) return MK_ERR_UNSUPPORTED;
  const uintptr_t al = reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k_new) |
                       reinterpret_cast<uintptr_t>(v_new) | reinterpret_cast<uintptr_t>(cos_t) |
                       reinterpret_cast<uintptr_t>(sin_t) | reinterpret_cast<uintptr_t>(k_cache) |
                       reinterpret_cast<uintptr_t>(v_cache);
  if ((al & 15) || (reinterpret_cast<uintptr_t>(ind) & 3) || (in_bs % 8) || (kv_ld % 8) || (kv_bs % 8))
    return MK_ERR_UNSUPPORTED;
  DecodeStepBeamArgs a;
  a.q = (const e16*)q; a.kn = (const e16*)k_new; a.vn = (const e16*)v_new; a.in_bs = in_bs;
  a.cos_t = (const e16*)cos_t; a.sin_t = (const e16*)sin_t;
  a.kc = (e16*)k_cache; a.vc = (e16*)v_cache; a.kv_ld = kv_ld; a.kv_bs = kv_bs;
  a.o = (e16*)o; a.o_bs = o_bs;
  a.t_dev = t_dev; a.t_max = t_max; a.scale = scale; a.t_off = nullptr;
  a.ind = ind; a.K = K; a.S0 = S0; a.n_ind = n_ind;
  const int R = B * K;
  dim3 grid(H, R), block(512);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  static const bool no4 = getenv("MK_DECODE_ATTN_NO4") != nullptr;
  if (hd == 128 && (H % 4) == 0 && (long)R * H >= 512 && !no4)
    MK_LAUNCH((decode_step_attn4_kernel<8, false, true>), dim3(H / 4, R), block, 0, st, a);
  else if (hd == 128) MK_LAUNCH((decode_step_attn_kernel<128, 8, false, true>), grid, block, 0, st, a);
  else if (hd == 64) MK_LAUNCH((decode_step_attn_kernel<64, 8, false, true>), grid, block, 0, st, a);
  else if (hd == 32) MK_LAUNCH((decode_step_attn_kernel<32, 8, false, true>), grid, block, 0, st, a);
  else MK_LAUNCH((decode_step_attn_kernel<16, 8, false, true>), grid, block, 0, st, a);
  return mk_check_launch();
}

// SHARED (mk_decode_step_attn_shared): parallel sampling, n rows per sample over ONE prompt cache [B][S0] plus a tail cache
// per row [B * n][Tn].  Row r = b * n + j is at position p = L_b + i, L_b = the sample's (compacted) prompt length and i the
// tail row of the step: keys 0 ... L_b - 1 are prompt rows of sample b, keys L_b ... p - 1 tail rows 0 ... i - 1 of row r, key p
// the new one.  The base's kc / vc / kv_ld / kv_bs describe the TAIL cache (one slot per row), t_max is not read.
struct DecodeStepSharedArgs : DecodeStepArgs {
  const e16* kp; const e16* vp; long p_ld, p_bs;            // prompt cache [S0][H * hd] per sample, read only
  int S0, Tn, n;
};

// One workgroup per (head, sample, tile of R rows).  The rows of a tile run one after the other through
// decode_step_attn_body -- the plain kernel's code, so its bits: the compiler decides where it contracts a product and a sum
// inside that body, and a second formulation of the same arithmetic (one load of a key applied to R queries held in
// registers was built first) comes out with other choices and other last bits of the fp32 sums.  The rows of a tile
// therefore share the prompt's keys through the cache hierarchy: row 0 brings a key from HBM, rows 1 ... R - 1 of the same
// workgroup re-read it from this CU's L1 or its XCD's L2 right behind it.  The last tile of a sample holds n - j0 < R rows.
// R = 1 is the untiled form, one workgroup per row, and the default (shared_attn_rows below).
template <int HD, int NWV, int R>
__global__ __launch_bounds__(NWV * 64) void decode_step_attn_shared_kernel(DecodeStepSharedArgs a) {
  __shared__ float red[NWV][HD];
  __shared__ float redw[2 * NWV];
  const int tiles = (a.n + R - 1) / R;
  const int h = blockIdx.x, b = blockIdx.y / tiles, j0 = (blockIdx.y % tiles) * R;
  const int nr = min(R, a.n - j0);
  const int i = (int)min(max((long)*a.t_dev - a.S0, 0L), (long)a.Tn - 1);
  const int L = (int)min(max((long)a.S0 + (a.t_off ? a.t_off[b] : 0), 0L), (long)a.S0);
#pragma unroll 1
  for (int r = 0; r < nr; ++r) {
    const long row = (long)b * a.n + j0 + r;
    if (r > 0) __syncthreads();          // red / redw serve the next row
    decode_step_attn_body<HD, NWV, false, false, true>(a, red, redw, h, (int)row, row * a.in_bs, row * a.o_bs, L + i, L);
  }
}

// rows per workgroup of the tiled form, and the instantiation MK_SHARED_ATTN_ROWS selects (read at every call, so one
// process can measure both; a captured step keeps the one it was captured with).  The default is the untiled form: with H a
// multiple of 8 the workgroups of a (head, sample) already share an XCD's L2, and the tile's serial rows cost more than its
// locality returns (profiles/decode_nsample_generate.txt, 1916-row prompt: -0.3 % at (B, n) = (2, 16), +12 % at (8, 4), +59 % at (1, 4))
constexpr int SHARED_ROWS = 4, SHARED_ROWS_DEFAULT = 1;
inline int shared_attn_rows() {
  const char* e = getenv("MK_SHARED_ATTN_ROWS");
  if (e && atoi(e) == 1) return 1;
  if (e && atoi(e) == SHARED_ROWS) return SHARED_ROWS;
  return SHARED_ROWS_DEFAULT;
}

template <int HD>
void decode_step_attn_shared_launch(const DecodeStepSharedArgs& a, int B, int H, hipStream_t st) {
  const dim3 block(512);
  if (shared_attn_rows() == 1)
    MK_LAUNCH((decode_step_attn_shared_kernel<HD, 8, 1>), dim3(H, B * a.n), block, 0, st, a);
  else
    MK_LAUNCH((decode_step_attn_shared_kernel<HD, 8, SHARED_ROWS>), dim3(H, B * ((a.n + SHARED_ROWS - 1) / SHARED_ROWS)),
              block, 0, st, a);
}

// mk_decode_step_attn_shared: the plain entry point's checks over B * n rows and two caches
int decode_step_attn_shared_impl(const void* q, const void* k_new, const void* v_new, int64_t in_bs, const void* cos_t,
                                 const void* sin_t, const void* kp, const void* vp, int64_t p_ld, int64_t p_bs, void* kt,
                                 void* vt, int64_t t_ld, int64_t t_bs, void* o, int64_t o_bs, const int32_t* t_dev,
                                 const int32_t* t_off, int32_t S0, int32_t Tn, int32_t B, int32_t n, int32_t H, int32_t hd,
                                 float scale, int32_t dtype, void* stream) {
  if (!q || !k_new || !v_new || !cos_t || !sin_t || !kt || !vt || !o || !t_dev || B <= 0 || H <= 0 || S0 < 0 || Tn < 1 ||
      n < 1 || (S0 > 0 && (!kp || !vp)))
    return MK_ERR_BAD_ARG;
  if (dtype != E16<e16>::dtype || (hd != 16 && hd != 32 && hd != 64 && hd != 128) || n > 32) return MK_ERR_UNSUPPORTED;
  const uintptr_t al = reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k_new) |
                       reinterpret_cast<uintptr_t>(v_new) | reinterpret_cast<uintptr_t>(cos_t) |
                       reinterpret_cast<uintptr_t>(sin_t) | reinterpret_cast<uintptr_t>(kp) |
                       reinterpret_cast<uintptr_t>(vp) | reinterpret_cast<uintptr_t>(kt) | reinterpret_cast<uintptr_t>(vt);
  if ((al & 15) || ((reinterpret_cast<uintptr_t>(t_dev) | reinterpret_cast<uintptr_t>(t_off)) & 3) || (in_bs % 8) ||
      (p_ld % 8) || (p_bs % 8) || (t_ld % 8) || (t_bs % 8) || (long)B * ((n + SHARED_ROWS - 1) / SHARED_ROWS) > 65535 ||
      (long)B * n > 65535)
    return MK_ERR_UNSUPPORTED;
  DecodeStepSharedArgs a;
  a.q = (const e16*)q; a.kn = (const e16*)k_new; a.vn = (const e16*)v_new; a.in_bs = in_bs;
  a.cos_t = (const e16*)cos_t; a.sin_t = (const e16*)sin_t;
  a.kp = (const e16*)kp; a.vp = (const e16*)vp; a.p_ld = p_ld; a.p_bs = p_bs;
  a.kc = (e16*)kt; a.vc = (e16*)vt; a.kv_ld = t_ld; a.kv_bs = t_bs;
  a.o = (e16*)o; a.o_bs = o_bs;
  a.t_dev = t_dev; a.t_off = t_off; a.t_max = Tn; a.S0 = S0; a.Tn = Tn; a.n = n; a.scale = scale;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (hd == 128) decode_step_attn_shared_launch<128>(a, B, H, st);
  else if (hd == 64) decode_step_attn_shared_launch<64>(a, B, H, st);
  else if (hd == 32) decode_step_attn_shared_launch<32>(a, B, H, st);
  else decode_step_attn_shared_launch<16>(a, B, H, st);
  return mk_check_launch();
}

// SCORE (mk_score_attn): F teacher-forced rows per option over a prompt cache [B][S0] and a tail cache per option
// [B * n][F].  Row r = (b * n + j) * F + g is fed token g of option (b, j), at position p = L_b + g; it is live while
// g < f = clamp(len[b * n + j], 0, F).  Two kernels on one stream: score_append_kernel rotates every live row's key (rope8:
// the body's own bits) and stores it with the value in tail row g; score_attn_kernel then runs the SHARED body per live row
// WITHOUT its append, so that a row reads its earlier sisters' tail rows, which other workgroups of the first kernel wrote.
struct ScoreArgs : DecodeStepSharedArgs {
  const int32_t* len;                                       // [B * n] on the device: fed rows per option
  int F;
  long rows, row0;                                          // B * n * F; first row of this launch (score_attn_kernel)
};

// one lane group of LPK lanes per (row, head): thread i of the grid-stride loop holds 8 elements of unit i / LPK
template <int HD>
__global__ __launch_bounds__(256) void score_append_kernel(ScoreArgs a, int H) {
  constexpr int LPK = HD / 8;
  const int sub = threadIdx.x % LPK, d0 = sub * 8;
  const long units = a.rows * H;
  const long stride = (long)gridDim.x * (256 / LPK);
  // (units rounded up to the stride, so that all lanes of a wave make the same trips: the shuffles need every partner)
  for (long u0 = (long)blockIdx.x * (256 / LPK); u0 < units; u0 += stride) {
    const long u = u0 + threadIdx.x / LPK;
    bool live = u < units;
    long row = 0;
    int h = 0, opt = 0, g = 0;
    if (live) {
      row = u / H; h = (int)(u % H);
      opt = (int)(row / a.F); g = (int)(row % a.F);
      live = g < min(max(a.len[opt], 0), a.F);
    }
    e16x8 kv, vv, cv, sv;
#pragma unroll
    for (int e = 0; e < 8; ++e) { kv[e] = (e16)0.f; vv[e] = (e16)0.f; cv[e] = (e16)0.f; sv[e] = (e16)0.f; }
    if (live) {
      const int b = opt / a.n;
      const int L = (int)min(max((long)a.S0 + (a.t_off ? a.t_off[b] : 0), 0L), (long)a.S0);
      const long in_off = row * a.in_bs + (long)h * HD + d0;
      kv = *reinterpret_cast<const e16x8*>(a.kn + in_off);
      vv = *reinterpret_cast<const e16x8*>(a.vn + in_off);
      cv = *reinterpret_cast<const e16x8*>(a.cos_t + (long)(L + g) * HD + d0);
      sv = *reinterpret_cast<const e16x8*>(a.sin_t + (long)(L + g) * HD + d0);
    }
    float kf[8];
    rope8<LPK>(kv, cv, sv, d0 < HD / 2, kf);
    if (live) {
      e16x8 kb;
#pragma unroll
      for (int e = 0; e < 8; ++e) kb[e] = (e16)kf[e];
      const long off = (long)opt * a.kv_bs + (long)g * a.kv_ld + (long)h * HD + d0;
      *reinterpret_cast<e16x8*>(a.kc + off) = kb;
      *reinterpret_cast<e16x8*>(a.vc + off) = vv;
    }
  }
}

// one workgroup per (head, row); a dead row's output is zeros
template <int HD, int NWV>
__global__ __launch_bounds__(NWV * 64) void score_attn_kernel(ScoreArgs a) {
  __shared__ float red[NWV][HD];
  __shared__ float redw[2 * NWV];
  const int h = blockIdx.x;
  const long row = a.row0 + blockIdx.y;
  const int opt = (int)(row / a.F), g = (int)(row % a.F);
  if (g >= min(max(a.len[opt], 0), a.F)) {
    if (threadIdx.x < HD) a.o[row * a.o_bs + (long)h * HD + threadIdx.x] = (e16)0.f;
    return;
  }
  const int b = opt / a.n;
  const int L = (int)min(max((long)a.S0 + (a.t_off ? a.t_off[b] : 0), 0L), (long)a.S0);
  decode_step_attn_body<HD, NWV, false, false, true, false>(a, red, redw, h, opt, row * a.in_bs, row * a.o_bs, L + g, L);
}

template <int HD>
void score_attn_launch(ScoreArgs a, int H, hipStream_t st) {
  constexpr int UPB = 256 / (HD / 8);                       // (row, head) units per workgroup of the append
  const long units = a.rows * H;
  const long want = (units + UPB - 1) / UPB, blocks = want < (1L << 20) ? want : (1L << 20);
  MK_LAUNCH((score_append_kernel<HD>), dim3((unsigned)blocks), dim3(256), 0, st, a, H);
  // grid.y carries at most 65535 rows, and a launch at most 2^31 threads: the rows go in as many launches as that takes
  long per = (1L << 22) / H;
  per = per > 65535 ? 65535 : per < 1 ? 1 : per;
  for (long r0 = 0; r0 < a.rows; r0 += per) {
    a.row0 = r0;
    const long nr = a.rows - r0 < per ? a.rows - r0 : per;
    MK_LAUNCH((score_attn_kernel<HD, 8>), dim3(H, (unsigned)nr), dim3(512), 0, st, a);
  }
}

// mk_score_attn: the shared entry point's checks over B * n * F rows
int score_attn_impl(const void* q, const void* k_new, const void* v_new, int64_t in_bs, const void* cos_t, const void* sin_t,
                    const void* kp, const void* vp, int64_t p_ld, int64_t p_bs, void* kt, void* vt, int64_t t_ld,
                    int64_t t_bs, void* o, int64_t o_bs, const int32_t* len, const int32_t* t_off, int32_t S0, int32_t F,
                    int32_t B, int32_t n, int32_t H, int32_t hd, float scale, int32_t dtype, void* stream) {
  if (!q || !k_new || !v_new || !cos_t || !sin_t || !kt || !vt || !o || !len || B < 1 || H < 1 || n < 1 || F < 1 || S0 < 0 ||
      (S0 > 0 && (!kp || !vp)))
    return MK_ERR_BAD_ARG;
  if (dtype != E16<e16>::dtype || (hd != 16 && hd != 32 && hd != 64 && hd != 128)) return MK_ERR_UNSUPPORTED;
  const uintptr_t al = reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k_new) |
                       reinterpret_cast<uintptr_t>(v_new) | reinterpret_cast<uintptr_t>(cos_t) |
                       reinterpret_cast<uintptr_t>(sin_t) | reinterpret_cast<uintptr_t>(kp) |
                       reinterpret_cast<uintptr_t>(vp) | reinterpret_cast<uintptr_t>(kt) | reinterpret_cast<uintptr_t>(vt);
  if ((al & 15) || ((reinterpret_cast<uintptr_t>(len) | reinterpret_cast<uintptr_t>(t_off)) & 3) || (in_bs % 8) ||
      (p_ld % 8) || (p_bs % 8) || (t_ld % 8) || (t_bs % 8) || H > 65535 || (int64_t)B * n > INT32_MAX ||
      (int64_t)S0 + F > INT32_MAX)
    return MK_ERR_UNSUPPORTED;
  ScoreArgs a;
  a.q = (const e16*)q; a.kn = (const e16*)k_new; a.vn = (const e16*)v_new; a.in_bs = in_bs;
  a.cos_t = (const e16*)cos_t; a.sin_t = (const e16*)sin_t;
  a.kp = (const e16*)kp; a.vp = (const e16*)vp; a.p_ld = p_ld; a.p_bs = p_bs;
  a.kc = (e16*)kt; a.vc = (e16*)vt; a.kv_ld = t_ld; a.kv_bs = t_bs;
  a.o = (e16*)o; a.o_bs = o_bs;
  a.t_dev = nullptr; a.t_off = t_off; a.t_max = F; a.S0 = S0; a.Tn = F; a.n = n; a.scale = scale;
  a.len = len; a.F = F; a.rows = (long)B * n * F; a.row0 = 0;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (hd == 128) score_attn_launch<128>(a, H, st);
  else if (hd == 64) score_attn_launch<64>(a, H, st);
  else if (hd == 32) score_attn_launch<32>(a, H, st);
  else score_attn_launch<16>(a, H, st);
  return mk_check_launch();
}

int decode_attn_impl(const void* q, const void* k, const void* v, void* o,
                              const int32_t* t_dev, int32_t t_add, int32_t t_max, int32_t B,
                              int32_t H, int32_t hd, int64_t q_bs, int64_t k_ld, int64_t k_bs,
                              int64_t v_ld, int64_t v_bs, int64_t o_bs, float scale, int32_t dtype,
                              void* stream) {
  if (!q || !k || !v || !o || !t_dev || B <= 0 || H <= 0 || t_max <= 0) return MK_ERR_BAD_ARG;
  if (dtype != E16<e16>::dtype || (hd != 16 && hd != 32 && hd != 64 && hd != 128)) return MK_ERR_UNSUPPORTED;
  if ((long)t_max * 4 > 60 * 1024) return MK_ERR_UNSUPPORTED;     // scores live in LDS
  const uintptr_t al = reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k) |
                       reinterpret_cast<uintptr_t>(v);
  if ((al & 15) || (q_bs % 8) || (k_ld % 8) || (k_bs % 8) || (v_ld % 8) || (v_bs % 8)) return MK_ERR_UNSUPPORTED;
  DecodeArgs a;
  a.q = (const e16*)q; a.k = (const e16*)k; a.v = (const e16*)v; a.o = (e16*)o;
  a.t_dev = t_dev; a.t_add = t_add; a.t_max = t_max;
  a.q_bs = q_bs; a.k_ld = k_ld; a.k_bs = k_bs; a.v_ld = v_ld; a.v_bs = v_bs; a.o_bs = o_bs;
  a.scale = scale;
  dim3 grid(H, B), block(256);
  const size_t lds = (size_t)t_max * 4;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (hd == 128) MK_LAUNCH((decode_attn_kernel<128>), grid, block, lds, st, a);
  else if (hd == 64) MK_LAUNCH((decode_attn_kernel<64>), grid, block, lds, st, a);
  else if (hd == 32) MK_LAUNCH((decode_attn_kernel<32>), grid, block, lds, st, a);
  else MK_LAUNCH((decode_attn_kernel<16>), grid, block, lds, st, a);
  return mk_check_launch();
}
}  // namespace MK_E16_NS
}  // namespace
