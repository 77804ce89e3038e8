// e4m3 KV cache (generate(kv_cache="fp8")): the prefill's quantising cache write and the decode step's attention
// block over the quantised cache, included once per element type (MK_E16_T / MK_E16_NS, see decode.hip).
// e16 = bf16 or _Float16: the type of q, the new k / v rows, the RoPE tables and the output.
//
// Cache format (include/macaw_hip.h): bytes uint8 [B][t_max][2D], a row = [keys of all heads | values of all
// heads], OCP e4m3fn; scales f32 [B][t_max][2H] = [key scale of every head | value scale of every head], one per
// (sample, position, key or value, head): amax / 448 over that head's hd elements, 1 for an all-zero head.
namespace {
namespace MK_E16_NS {
typedef MK_E16_T e16;
typedef E16<e16>::x8 e16x8;

struct Kv8AppendArgs {
  const e16* k; const e16* v; long ld, in_bs;     // Sn rows per sample at pitch ld, samples in_bs apart (elements)
  uint8_t* cache; float* scales;
  int t0, Sn, t_max, H;
  const int32_t* slot;                            // ROWS kernels only: [B][Sn] destination rows, < 0 = skip
};

// amax over the LPK lanes that share a head, then the project's row quantisation (fp8_rowquant_kernel's
// arithmetic: sc = 448 / amax in fp32, x * sc, clamp, RNE): NCH chunks of 8 elements per lane.
template <int LPK, int NCH>
MK_DEV float kv8_quant(const float (&x)[NCH * 8], unsigned (&q)[NCH * 2]) {
  float m = 0.f;
#pragma unroll
  for (int e = 0; e < NCH * 8; ++e) m = fmaxf(m, fabsf(x[e]));
#pragma unroll
  for (int o = 1; o < LPK; o <<= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  const float sc = m > 0.f ? 448.f / m : 1.f;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    float t[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) t[e] = x[c * 8 + e];
    const int2 pk = fp8_pack8(t, sc);
    q[2 * c] = (unsigned)pk.x;
    q[2 * c + 1] = (unsigned)pk.y;
  }
  return m > 0.f ? m / 448.f : 1.f;
}

// One lane group of HD / 8 lanes per (new row, head): 16 bytes of k and of v per lane in, 8 + 8 bytes out.
// Writes cache rows [t0, t0 + Sn) of every sample and nothing else.  ROWS (mk_kv_quant_append_rows): source row s of
// sample b goes to cache row slot[b][s] instead, a row whose slot is outside [0, t_max) is not written.
template <int HD, bool ROWS = false>
__global__ __launch_bounds__(256) void kv_quant_append_kernel(Kv8AppendArgs a) {
  constexpr int LPK = HD / 8;
  const int b = blockIdx.y;
  const int per_row = a.H * LPK;
  const long n = (long)a.Sn * per_row;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  const bool live = idx < n;                       // (n is a multiple of LPK: a lane group is live as a whole)
  const long ic = live ? idx : n - 1;              // clamped: every lane takes part in the shuffles
  const int s = (int)(ic / per_row), r = (int)(ic % per_row);
  const int h = r / LPK, sub = r % LPK;
  const long in_off = (long)b * a.in_bs + (long)s * a.ld + (long)h * HD + sub * 8;
  const e16x8 kv = *reinterpret_cast<const e16x8*>(a.k + in_off);
  const e16x8 vv = *reinterpret_cast<const e16x8*>(a.v + in_off);
  float kf[8], vf[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { kf[e] = (float)kv[e]; vf[e] = (float)vv[e]; }
  unsigned kq[2], vq[2];
  const float ks = kv8_quant<LPK, 1>(kf, kq);
  const float vs = kv8_quant<LPK, 1>(vf, vq);
  if (!live) return;
  const long D = (long)a.H * HD;
  int dr = a.t0 + s;
  if constexpr (ROWS) {
    dr = a.slot[(long)b * a.Sn + s];
    if (dr < 0 || dr >= a.t_max) return;
  }
  const long row = (long)b * a.t_max + dr;
  uint8_t* dst = a.cache + row * 2 * D + (long)h * HD + sub * 8;
  *reinterpret_cast<uint2*>(dst) = make_uint2(kq[0], kq[1]);
  *reinterpret_cast<uint2*>(dst + D) = make_uint2(vq[0], vq[1]);
  if (sub == 0) {
    a.scales[row * 2 * a.H + h] = ks;
    a.scales[row * 2 * a.H + a.H + h] = vs;
  }
}

struct DecodeStepKv8Args {
  const e16* q; const e16* kn; const e16* vn; long in_bs;   // new rows [H * hd] per sample
  const e16* cos_t; const e16* sin_t;                       // [positions][hd]
  uint8_t* cache; float* scales;                            // [B][t_max][2 H hd] bytes, [B][t_max][2 H] scales
  e16* o; long o_bs;
  const int32_t* t_dev;
  int t_max, H;
  float scale;
  const int32_t* t_off;                                     // VAR kernels only: [B] per-sample offsets to *t_dev
};

// E e4m3 bytes (E / 4 dwords, element index ascending with the byte address) against E fp32 values
template <int E>
MK_DEV float kv8_dot(const float (&q)[E], const unsigned (&w)[E / 4]) {
  float s = 0.f;
#pragma unroll
  for (int d = 0; d < E / 4; ++d) {
    const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8(w[d], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8(w[d], true);
    s += q[4 * d] * lo[0]; s += q[4 * d + 1] * lo[1]; s += q[4 * d + 2] * hi[0]; s += q[4 * d + 3] * hi[1];
  }
  return s;
}
template <int E>
MK_DEV void kv8_axpy(float (&acc)[E], float p, const unsigned (&w)[E / 4]) {
#pragma unroll
  for (int d = 0; d < E / 4; ++d) {
    const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8(w[d], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8(w[d], true);
    acc[4 * d] += p * lo[0]; acc[4 * d + 1] += p * lo[1]; acc[4 * d + 2] += p * hi[0]; acc[4 * d + 3] += p * hi[1];
  }
}
template <int E>
MK_DEV void kv8_load(const uint8_t* p, unsigned (&w)[E / 4]) {
  if constexpr (E == 16) {
    const uint4 r = *reinterpret_cast<const uint4*>(p);
    w[0] = r.x; w[1] = r.y; w[2] = r.z; w[3] = r.w;
  } else {
    const uint2 r = *reinterpret_cast<const uint2*>(p);
    w[0] = r.x; w[1] = r.y;
  }
}
template <int E>
MK_DEV void kv8_store(uint8_t* p, const unsigned (&w)[E / 4]) {
  if constexpr (E == 16) *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[2], w[3]);
  else *reinterpret_cast<uint2*>(p) = make_uint2(w[0], w[1]);
}

// decode_step_attn_kernel / decode_step_attn4_kernel (decode_impl.inc) over the e4m3 cache, both dispatch regimes
// from one body: RoPE of the new q and k with rope_kernel's rounding points, per-head quantisation of the rotated key
// and of the value, append of bytes + scales at row p = clamp(*t_dev), and the attention of the rotated 16-bit query
// over rows 0 ... p of the cache AS STORED AFTER THE APPEND (row p enters as the de-quantised quantised value: what
// every later step reads).  De-quantisation in fp32, the scale once per key:
//   s_t = scale * k_scale[t] * sum q . e4m3,   o += p_t * v_scale[t] * e4m3;  nothing is rounded to 16 bits between.
// Kept from the 16-bit kernels: the online softmax, eight keys per lane group in flight per trip (K and V bytes and
// both scales of all eight requested before the first use), unconditional loads from a clamped row.
//
// A wave is KPW keys x HG heads x LPK lanes, a lane holds E = HD / LPK consecutive dims of one head of one key:
//   <HD, 8, 1>    one workgroup per (head, sample), 8-byte loads.  This regime is few workgroups at short contexts:
//                 latency, not bandwidth, by the 16-bit kernel's own measurement.  E = 8 keeps that kernel's lane <->
//                 dims map (LPK >= 2 at hd = 16, so the rotate-half partner is always another lane) and its 64 / LPK
//                 keys per wave and pass.
//   <128, 16, 4>  one workgroup per (sample, four adjacent heads), B x H >= 512: the bandwidth regime.  A key of four
//                 heads is ONE contiguous 512-byte run; with 16-byte loads 32 lanes cover it and a wave load is two
//                 such runs (keys t and t + 1: 2 x 512 B), with 8-byte loads a wave would cover one run with twice as
//                 many load instructions for the same bytes.  16 bytes per lane is the widest vector access (1 KiB per
//                 wave instruction), and L2-served streaming reads of 8 bytes per lane run at 0.54 - 0.70 of the 16-byte
//                 rate on this part, so the stream that decides this regime takes the 16-byte form.  Registers per lane in flight: 8 keys x (4 + 4 dwords + 2 scales), the same 64
//                 dwords of payload as the 16-bit kernel's 8 keys x 2 x 16 bytes.
// VAR (mk_decode_step_attn_kv8_var): p = clamp(*t_dev + t_off[b]) per sample, as in decode_step_attn_kernel.
template <int HD, int E, int HG, int NWV, bool VAR = false>
__global__ __launch_bounds__(NWV * 64) void decode_step_attn_kv8_kernel(DecodeStepKv8Args a) {
  constexpr int LPK = HD / E, KPW = 64 / (LPK * HG), KPP = NWV * KPW, NCH = E / 8, NB = 8;
  static_assert(LPK >= 2 && KPW >= 1, "rotate-half partner in another lane; at least one key per wave");
  __shared__ float red[NWV][HG * HD];
  __shared__ float redm[NWV][HG], reds[NWV][HG];
  const int b = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int sub = lane % LPK, hg = (lane / LPK) % HG, grp = lane / (LPK * HG);
  const int h = blockIdx.x * HG + hg;
  int tp = *a.t_dev;
  if constexpr (VAR) tp += a.t_off[b];
  const int p = min(max(tp, 0), a.t_max - 1);
  const int T = p + 1;
  const int d0 = sub * E;
  const bool first = d0 < HD / 2;
  const long in_off = (long)b * a.in_bs + (long)h * HD + d0;
  float qf[E], kf[E], vf[E];
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const e16x8 qv = *reinterpret_cast<const e16x8*>(a.q + in_off + c * 8);
    const e16x8 kv = *reinterpret_cast<const e16x8*>(a.kn + in_off + c * 8);
    const e16x8 vv = *reinterpret_cast<const e16x8*>(a.vn + in_off + c * 8);
    const e16x8 cv = *reinterpret_cast<const e16x8*>(a.cos_t + (long)p * HD + d0 + c * 8);
    const e16x8 sv = *reinterpret_cast<const e16x8*>(a.sin_t + (long)p * HD + d0 + c * 8);
#pragma unroll
    for (int e = 0; e < 8; ++e) {        // RoPE with rope_kernel's rounding points (see decode_step_attn_kernel)
      const float cs = (float)cv[e], sn = (float)sv[e];
      const float qo = (float)qv[e], ko = (float)kv[e];
      const float qp = __shfl_xor(qo, LPK / 2, 64), kp = __shfl_xor(ko, LPK / 2, 64);
      const float sq = first ? rnd_e16(-qp * sn) : rnd_e16(qp * sn);
      const float sk = first ? rnd_e16(-kp * sn) : rnd_e16(kp * sn);
      qf[c * 8 + e] = rnd_e16(rnd_e16(qo * cs) + sq);
      kf[c * 8 + e] = rnd_e16(rnd_e16(ko * cs) + sk);
      vf[c * 8 + e] = (float)vv[e];
    }
  }
  // every lane group quantises the new row of its head itself (same arithmetic, same bytes in every wave): the new
  // position then takes the path of a cached one, selected on the bytes
  unsigned knq[E / 4], vnq[E / 4];
  const float kns = kv8_quant<LPK, NCH>(kf, knq);
  const float vns = kv8_quant<LPK, NCH>(vf, vnq);
  const long D = (long)a.H * HD;
  uint8_t* crow = a.cache + (long)b * a.t_max * 2 * D + (long)h * HD + d0;       // + t * 2D: key bytes; + D: value bytes
  float* srow = a.scales + (long)b * a.t_max * 2 * a.H + h;                      // + t * 2H: key scale; + H: value scale
  if (wave == 0 && grp == 0) {           // append (cache row p)
    kv8_store<E>(crow + (long)p * 2 * D, knq);
    kv8_store<E>(crow + (long)p * 2 * D + D, vnq);
    if (sub == 0) {
      srow[(long)p * 2 * a.H] = kns;
      srow[(long)p * 2 * a.H + a.H] = vns;
    }
  }
  float m_run = -INFINITY, lsum = 0.f, acc[E];
#pragma unroll
  for (int e = 0; e < E; ++e) acc[e] = 0.f;
  // key t belongs to lane group (wave, grp): t = wave * KPW + grp (mod KPP); NB keys per group and trip
  for (int t0 = wave * KPW + grp; t0 < T; t0 += KPP * NB) {
    unsigned kq[NB][E / 4], vq[NB][E / 4];
    float ks[NB], vs[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) {       // unconditional loads from a clamped row (no branch around a load)
      const int tc = min(t0 + j * KPP, max(p - 1, 0));
      kv8_load<E>(crow + (long)tc * 2 * D, kq[j]);
      kv8_load<E>(crow + (long)tc * 2 * D + D, vq[j]);
      ks[j] = srow[(long)tc * 2 * a.H];
      vs[j] = srow[(long)tc * 2 * a.H + a.H];
    }
    float sj[NB], mt = m_run;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const int t = t0 + j * KPP;
      if (t >= p) {                      // (t >= p: the clamped row's bytes never enter the arithmetic)
#pragma unroll
        for (int d = 0; d < E / 4; ++d) { kq[j][d] = knq[d]; vq[j][d] = vnq[d]; }
        ks[j] = kns; vs[j] = vns;
      }
      float s = kv8_dot<E>(qf, kq[j]);
#pragma unroll
      for (int o = 1; o < LPK; o <<= 1) s += __shfl_xor(s, o, 64);
      {
        // the product is rounded ONCE: contracted into `sj - mt` below as an fma it would enter unrounded there and
        // turn exp(0) of the maximal key into exp(rounding residual)
#pragma clang fp contract(off)
        sj[j] = t < T ? s * (a.scale * ks[j]) : -INFINITY;
      }
      mt = fmaxf(mt, sj[j]);
    }
    const float corr = __expf(m_run - mt);       // (0 on the first trip: m_run = -inf, mt finite: key t0 < T)
    lsum *= corr;
#pragma unroll
    for (int e = 0; e < E; ++e) acc[e] *= corr;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const float pr = __expf(sj[j] - mt);       // exp(-inf) = 0 for keys past the end
      lsum += pr;
      kv8_axpy<E>(acc, pr * vs[j], vq[j]);
    }
    m_run = mt;
  }
  // merge the lane groups of a head: common maximum (wave, then workgroup), then rescaled sums
  float mx = m_run;
#pragma unroll
  for (int o = LPK * HG; o < 64; o <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  if (sub == 0 && grp == 0) redm[wave][hg] = mx;
  __syncthreads();
  mx = redm[0][hg];
#pragma unroll
  for (int i = 1; i < NWV; ++i) mx = fmaxf(mx, redm[i][hg]);
  {
    const float corr = __expf(m_run - mx);       // groups without a key: m_run = -inf -> 0
    lsum *= corr;
#pragma unroll
    for (int e = 0; e < E; ++e) acc[e] *= corr;
  }
#pragma unroll
  for (int o = LPK * HG; o < 64; o <<= 1) {
    lsum += __shfl_xor(lsum, o, 64);
#pragma unroll
    for (int e = 0; e < E; ++e) acc[e] += __shfl_xor(acc[e], o, 64);
  }
  if (grp == 0) {
#pragma unroll
    for (int e = 0; e < E; ++e) red[wave][hg * HD + d0 + e] = acc[e];
    if (sub == 0) reds[wave][hg] = lsum;
  }
  __syncthreads();
  if (tid < HG * HD) {
    const int g = tid / HD;
    float sum = 0.f, v = 0.f;
#pragma unroll
    for (int i = 0; i < NWV; ++i) { sum += reds[i][g]; v += red[i][tid]; }      // fixed order: deterministic
    a.o[(long)b * a.o_bs + (long)(blockIdx.x * HG) * HD + tid] = (e16)(v / sum);
  }
}

bool kv8_hd_ok(int hd) { return hd == 16 || hd == 32 || hd == 64 || hd == 128; }

int kv_quant_append_impl(const void* k, const void* v, int64_t ld, int64_t in_bs, void* cache, float* scales,
                         int32_t t0, int32_t Sn, int32_t t_max, int32_t B, int32_t H, int32_t hd, int32_t dtype,
                         void* stream, bool rows = false, const int32_t* slot = nullptr) {
  if (!k || !v || !cache || !scales || B <= 0 || H <= 0 || Sn <= 0 || t_max <= 0 || t0 < 0 ||
      (!rows && (int64_t)t0 + Sn > t_max) || (rows && !slot))
    return MK_ERR_BAD_ARG;
  if (dtype != E16<e16>::dtype || !kv8_hd_ok(hd)) return MK_ERR_UNSUPPORTED;
  const uintptr_t al = reinterpret_cast<uintptr_t>(k) | reinterpret_cast<uintptr_t>(v) |
                       reinterpret_cast<uintptr_t>(cache) | reinterpret_cast<uintptr_t>(scales);
  const int64_t D = (int64_t)H * hd;
  if ((al & 15) || (ld % 8) || (in_bs % 8) || ld < D || (B > 1 && in_bs < D)) return MK_ERR_UNSUPPORTED;
  Kv8AppendArgs a;
  a.k = (const e16*)k; a.v = (const e16*)v; a.ld = ld; a.in_bs = in_bs;
  a.cache = (uint8_t*)cache; a.scales = scales;
  a.t0 = t0; a.Sn = Sn; a.t_max = t_max; a.H = H; a.slot = slot;
  const long n = (long)Sn * H * (hd / 8);
  dim3 grid((unsigned)mk_cdiv(n, 256), B), block(256);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (rows) {
    if (hd == 128) MK_LAUNCH((kv_quant_append_kernel<128, true>), grid, block, 0, st, a);
    else if (hd == 64) MK_LAUNCH((kv_quant_append_kernel<64, true>), grid, block, 0, st, a);
    else if (hd == 32) MK_LAUNCH((kv_quant_append_kernel<32, true>), grid, block, 0, st, a);
    else MK_LAUNCH((kv_quant_append_kernel<16, true>), grid, block, 0, st, a);
    return mk_check_launch();
  }
  if (hd == 128) MK_LAUNCH((kv_quant_append_kernel<128>), grid, block, 0, st, a);
  else if (hd == 64) MK_LAUNCH((kv_quant_append_kernel<64>), grid, block, 0, st, a);
  else if (hd == 32) MK_LAUNCH((kv_quant_append_kernel<32>), grid, block, 0, st, a);
  else MK_LAUNCH((kv_quant_append_kernel<16>), grid, block, 0, st, a);
  return mk_check_launch();
}

int decode_step_attn_kv8_impl(const void* q, const void* k_new, const void* v_new, int64_t in_bs, const void* cos_t,
                              const void* sin_t, void* cache, float* scales, void* o, int64_t o_bs,
                              const int32_t* t_dev, int32_t t_max, int32_t B, int32_t H, int32_t hd, float scale,
                              int32_t dtype, void* stream, bool var = false, const int32_t* t_off = nullptr) {
  if (!q || !k_new || !v_new || !cos_t || !sin_t || !cache || !scales || !o || !t_dev || B <= 0 || H <= 0 ||
      t_max <= 0 || (var && !t_off))
    return MK_ERR_BAD_ARG;
  if (dtype != E16<e16>::dtype || !kv8_hd_ok(hd)) return MK_ERR_UNSUPPORTED;
  const uintptr_t al = reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k_new) |
                       reinterpret_cast<uintptr_t>(v_new) | reinterpret_cast<uintptr_t>(cos_t) |
                       reinterpret_cast<uintptr_t>(sin_t) | reinterpret_cast<uintptr_t>(cache) |
                       reinterpret_cast<uintptr_t>(scales);
  const int64_t D = (int64_t)H * hd;
  if ((al & 15) || (in_bs % 8) || (B > 1 && in_bs < D) || (B > 1 && o_bs < D)) return MK_ERR_UNSUPPORTED;
  DecodeStepKv8Args a;
  a.q = (const e16*)q; a.kn = (const e16*)k_new; a.vn = (const e16*)v_new; a.in_bs = in_bs;
  a.cos_t = (const e16*)cos_t; a.sin_t = (const e16*)sin_t;
  a.cache = (uint8_t*)cache; a.scales = scales;
  a.o = (e16*)o; a.o_bs = o_bs;
  a.t_dev = t_dev; a.t_max = t_max; a.H = H; a.scale = scale; a.t_off = t_off;
  dim3 grid(H, B), block(512);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (var) {          // the same selection, the per-sample-position instantiations
    if (hd == 128 && (H % 4) == 0 && (long)B * H >= 512)
      MK_LAUNCH((decode_step_attn_kv8_kernel<128, 16, 4, 8, true>), dim3(H / 4, B), block, 0, st, a);
    else if (hd == 128) MK_LAUNCH((decode_step_attn_kv8_kernel<128, 8, 1, 8, true>), grid, block, 0, st, a);
    else if (hd == 64) MK_LAUNCH((decode_step_attn_kv8_kernel<64, 8, 1, 8, true>), grid, block, 0, st, a);
    else if (hd == 32) MK_LAUNCH((decode_step_attn_kv8_kernel<32, 8, 1, 8, true>), grid, block, 0, st, a);
    else MK_LAUNCH((decode_step_attn_kv8_kernel<16, 8, 1, 8, true>), grid, block, 0, st, a);
    return mk_check_launch();
  }
  // the dispatch of decode_step_attn_impl: four heads per workgroup where there are many (sample, head) pairs
  if (hd == 128 && (H % 4) == 0 && (long)B * H >= 512)
    MK_LAUNCH((decode_step_attn_kv8_kernel<128, 16, 4, 8>), dim3(H / 4, B), block, 0, st, a);
  else if (hd == 128) MK_LAUNCH((decode_step_attn_kv8_kernel<128, 8, 1, 8>), grid, block, 0, st, a);
  else if (hd == 64) MK_LAUNCH((decode_step_attn_kv8_kernel<64, 8, 1, 8>), grid, block, 0, st, a);
  else if (hd == 32) MK_LAUNCH((decode_step_attn_kv8_kernel<32, 8, 1, 8>), grid, block, 0, st, a);
  else MK_LAUNCH((decode_step_attn_kv8_kernel<16, 8, 1, 8>), grid, block, 0, st, a);
  return mk_check_launch();
}
}  // namespace MK_E16_NS
}  // namespace
