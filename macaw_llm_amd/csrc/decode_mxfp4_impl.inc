// The MXFP4 row quantiser, the MXFP4 weight-streaming kernel of mk_decode_linear_mxfp4 and its launcher, included once
// per element type (MK_E16_T / MK_E16_NS, see decode_mxfp4.hip).  e16 = bf16 or _Float16: the type of the tokens, the
// residual and the output, and the type the e2m1 codes are widened to in registers.
#include "skinny16_parts.inc"   // the token prologue and the cross-wave reduction of the skinny16 stream kernels

namespace {
namespace MK_E16_NS {
typedef MK_E16_T e16;
typedef E16<e16>::x8 e16x8;
typedef e16 e16x2 __attribute__((ext_vector_type(2)));

// smallest block exponent: 0.5 * 2^EMIN is the smallest NORMAL number of e16, so every de-quantised value is one
constexpr int EMIN = E16<e16>::narrow_exponent ? -13 : -125;

// one byte (two e2m1 codes) of d, selected by SEL, times the block scale -> two e16: v_cvt_scalef32_pk_{bf16,f16}_fp4
template <int SEL> MK_DEV e16x2 widen2(unsigned d, float s) {
  if constexpr (E16<e16>::narrow_exponent) return __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(d, s, SEL);
  else return __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, s, SEL);
}

// 8 e2m1 codes (one dword: element 2 j in the low nibble of byte j, element 2 j + 1 in the high nibble) times the
// power-of-two block scale -> 8 e16, k ascending.  A code times a power of two is an exact number of e16 (1 mantissa
// bit; the quantiser's EMIN keeps it normal), so the de-quantisation is folded into the widening without a rounding
// point.  4 VALU instructions per MFMA operand, half of what the e4m3 kernel spends.
MK_DEV e16x8 widen8(unsigned d, float s) {
  const e16x2 p0 = widen2<0>(d, s), p1 = widen2<1>(d, s), p2 = widen2<2>(d, s), p3 = widen2<3>(d, s);
  e16x8 o;
  o[0] = p0[0]; o[1] = p0[1]; o[2] = p1[0]; o[3] = p1[1];
  o[4] = p2[0]; o[5] = p2[1]; o[6] = p3[0]; o[7] = p3[1];
  return o;
}

// OCP MX v1.0 round-to-nearest quantiser of one block of 32 along K per thread: E = clamp(floor(log2(amax)) - 2,
// EMIN, 125) (EMIN for an all-zero block), element = x * 2^-E rounded to the nearest of {0, .5, 1, 1.5, 2, 3, 4, 6}
// with ties to the even code and saturated at 6.  The thresholds are compared one by one: every value and every
// comparison is exact in fp32, so the codes do not depend on a rounding or denormal mode (a product below 2^-126
// is below the first threshold whether it is flushed or not).  A zero code is written without a sign.
__global__ __launch_bounds__(256) void mxfp4_quantize_rows_kernel(const e16* __restrict__ x, int rows, int nblk, long ld,
                                                                  uint8_t* __restrict__ q, long ldq,
                                                                  uint8_t* __restrict__ ex, long lde) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long)rows * nblk) return;
  const int r = (int)(t / nblk), b = (int)(t % nblk);
  const e16* xp = x + (long)r * ld + 32 * b;
  float v[32];
  float amax = 0.f;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const e16x8 xv = *reinterpret_cast<const e16x8*>(xp + 8 * c);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      v[8 * c + i] = (float)xv[i];
      amax = fmaxf(amax, fabsf(v[8 * c + i]));
    }
  }
  // a bf16 / f16 value is a normal fp32 number or zero: floor(log2) is its exponent field
  int E = amax > 0.f ? (int)((__float_as_uint(amax) >> 23) & 0xFF) - 127 - 2 : EMIN;
  E = min(max(E, EMIN), 125);
  const float inv = __uint_as_float((unsigned)(127 - E) << 23);   // 2^-E, a normal number for every E in range
  unsigned out[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    unsigned d = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float xv = v[8 * c + i];
      const float a = fabsf(xv) * inv;
      unsigned code = (a > 0.25f) + (a >= 0.75f) + (a > 1.25f) + (a >= 1.75f) + (a > 2.5f) + (a >= 3.5f) + (a > 5.f);
      if (xv < 0.f && code != 0) code |= 8u;
      d |= code << (4 * i);
    }
    out[c] = d;
  }
  *reinterpret_cast<uint4*>(q + (long)r * ldq + 16 * b) = make_uint4(out[0], out[1], out[2], out[3]);
  ex[(long)r * lde + b] = (uint8_t)(E + 127);
}

void launch_mxfp4_quantize_rows(const void* x, int rows, int cols, long ld, uint8_t* q, long ldq, uint8_t* ex, long lde,
                                hipStream_t st) {
  const int nblk = cols / 32;
  MK_LAUNCH(mxfp4_quantize_rows_kernel, dim3(mk_cdiv((long)rows * nblk, 256)), dim3(256), 0, st,
            reinterpret_cast<const e16*>(x), rows, nblk, ld, q, ldq, ex, lde);
}

// decode_linear_fp8_kernel (decode_fp8_impl.inc) with the weight operand read as MXFP4: 16 weight rows per workgroup
// (N / 16 workgroups), NW waves that split K in blocks, a ring of NBUF register buffers so that the loads of the next
// trips are in flight under the MFMAs of this one, the same three token prologues (PRO 1 RMSNorm / 2 SwiGLU, token
// rows prepared in LDS), MT = 2 token tiles for 17 ... 32 plain rows, and the same fixed-order cross-wave reduction:
// the code of both is skinny16_parts.inc.
// A K-block is 128 elements = 64 BYTES of a weight row, so one 16-byte load per lane still covers it: lane (r16, kq)
// holds k = 32 kq ... 32 kq + 31 of weight row r16 -- exactly one MX block, one scale -- and dword j of the load
// feeds MFMA j of the block's four.  The token operand follows: its four 16-byte loads of a block are the 64
// contiguous bytes x[k = 32 kq ... 32 kq + 31] (in LDS likewise).  The MFMA sums over (lane group, element) pairs, so
// any k mapping the two operands share gives the same product.
// The four exponent bytes of a (row, K-block) are one aligned dword: one dword load per lane, byte kq selected, and
// the scale is as_float(byte << 23) -- a normal power of two.  It enters the widening instruction; the epilogue has
// no scale left to apply.
template <int NW, int U, int PRO, int NBUF = 2, int MT = 1>
__global__ __launch_bounds__(NW * 64) void decode_linear_mxfp4_kernel(DecodeMxfp4Args g) {
  static_assert(MT == 1 || PRO == 0, "two token tiles: plain token operand only");
  extern __shared__ __attribute__((aligned(16))) char sk_smem[];
  __shared__ float red[NW][4 * MT][64];
  __shared__ float ssq[NW][16];
  const int l = threadIdx.x & 63, w = threadIdx.x >> 6, r16 = l & 15, kq = l >> 4;
  const int n0 = blockIdx.x * 16;
  const e16* A = reinterpret_cast<const e16*>(g.x);
  const int wrow = min(n0 + r16, g.N - 1);
  const uint8_t* wp = g.Wq + (long)wrow * g.ldw + 16 * kq;
  const unsigned* ep = reinterpret_cast<const unsigned*>(g.e + (long)wrow * g.lde);
  const int trow = min(r16, g.M - 1);
  const e16* xp = A + (long)trow * g.ldx + 32 * kq;
  const e16* xp2 = A + (long)min(16 + r16, g.M - 1) * g.ldx + 32 * kq;   // MT == 2: token rows 16 ... 31
  const int ldt = g.K + 8;                                  // LDS token row pitch (elements)
  const e16* tp = reinterpret_cast<const e16*>(sk_smem) + trow * ldt + 32 * kq;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f}, acc2 = {0.f, 0.f, 0.f, 0.f};
  const int nkb = g.K / 128;
  constexpr int XN = PRO == 0 ? 4 * U * MT : 1;
  // trip t of wave w covers K blocks w + NW * (t * U + u), u < U (neighbouring waves read
  // neighbouring 64-byte halves of a 128-byte line of a row)
  auto load = [&](uint4 (&wf)[U], unsigned (&ef)[U], e16x8 (&xf)[XN], int kb) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int kk = min(kb + u * NW, nkb - 1);       // clamped: the MFMA of a clamped block is skipped
      wf[u] = *reinterpret_cast<const uint4*>(wp + kk * 64);
      ef[u] = ep[kk];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if constexpr (PRO == 0) xf[4 * u + j] = *reinterpret_cast<const e16x8*>(xp + kk * 128 + 8 * j);
        if constexpr (MT == 2) xf[4 * U + 4 * u + j] = *reinterpret_cast<const e16x8*>(xp2 + kk * 128 + 8 * j);
      }
    }
  };
  auto mma = [&](const uint4 (&wf)[U], const unsigned (&ef)[U], const e16x8 (&xf)[XN], int kb) {
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (kb + u * NW < nkb) {
        const float s = __uint_as_float(((ef[u] >> (8 * kq)) & 0xFFu) << 23);
        const unsigned wd[4] = {wf[u].x, wf[u].y, wf[u].z, wf[u].w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          e16x8 t;
          if constexpr (PRO == 0) t = xf[4 * u + j];
          else t = *reinterpret_cast<const e16x8*>(tp + (kb + u * NW) * 128 + 8 * j);
          const e16x8 wv = widen8(wd[j], s);
          acc = E16<e16>::mma16(wv, t, acc);
          if constexpr (MT == 2) acc2 = E16<e16>::mma16(wv, xf[4 * U + 4 * u + j], acc2);
        }
      }
  };
  // ring of NBUF register buffers: NBUF - 1 trips of this wave are in flight under the MFMAs of one
  uint4 wbuf[NBUF][U];
  unsigned ebuf[NBUF][U];
  e16x8 xbuf[NBUF][XN];
  constexpr int STEP = NW * U;
  int kb = w;
#pragma unroll
  for (int i = 0; i < NBUF - 1; ++i)
    if (kb + i * STEP < nkb) load(wbuf[i], ebuf[i], xbuf[i], kb + i * STEP);
  if constexpr (PRO != 0)         // the token rows, prepared once per workgroup
    skinny16_stage_tokens<NW, PRO>(A, g.ldx, g.M, g.K, g.pro_w, g.pro_eps, sk_smem, ssq, l, w);
  while (kb < nkb) {
#pragma unroll
    for (int i = 0; i < NBUF; ++i) {
      if (kb + (NBUF - 1) * STEP < nkb)
        load(wbuf[(i + NBUF - 1) % NBUF], ebuf[(i + NBUF - 1) % NBUF], xbuf[(i + NBUF - 1) % NBUF], kb + (NBUF - 1) * STEP);
      mma(wbuf[i], ebuf[i], xbuf[i], kb);
      kb += STEP;
      if (kb >= nkb) break;
    }
  }
  skinny16_reduce_put<NW, MT>(red, acc, acc2, l, w);
  e16* C = reinterpret_cast<e16*>(g.y);
  const e16* Rp = reinterpret_cast<const e16*>(g.residual);
  for (int t = threadIdx.x; t < 256 * MT; t += NW * 64) {
    int m, n;
    float v = skinny16_reduce_get<NW, MT>(red, t, n0, m, n);
    if (m >= g.M || n >= g.N) continue;
    if (Rp) v += (float)Rp[(long)m * g.ldr + n];
    C[(long)m * g.ldy + n] = (e16)v;
  }
}

// 16 waves where N / 16 workgroups are few, else 8 waves, as the e4m3 launcher chooses.  The token fragments of a
// K-block are 16 VGPRs per token tile (twice the e4m3 kernel's per weight load), so the plain forms, which keep them in
// the register ring, take ONE block per trip (U = 1) and a ring of 4 (8 waves) / 3 (16 waves) / 2 (two token tiles); the
// prologue forms read their tokens from LDS and keep the e4m3 kernel's U = 2 with a ring of 3 / 2.
void launch_decode_linear_mxfp4(const DecodeMxfp4Args& g, int prologue, bool wide, size_t lds, hipStream_t st) {
  const dim3 g16(mk_cdiv(g.N, 16));
  if (g.M > 16) MK_LAUNCH((decode_linear_mxfp4_kernel<8, 1, 0, 2, 2>), g16, dim3(512), 0, st, g);
  else if (prologue == 0) {
    if (wide) MK_LAUNCH((decode_linear_mxfp4_kernel<16, 1, 0, 3>), g16, dim3(1024), 0, st, g);
    else MK_LAUNCH((decode_linear_mxfp4_kernel<8, 1, 0, 4>), g16, dim3(512), 0, st, g);
  } else if (prologue == 1) {
    if (wide) MK_LAUNCH((decode_linear_mxfp4_kernel<16, 2, 1>), g16, dim3(1024), lds, st, g);
    else MK_LAUNCH((decode_linear_mxfp4_kernel<8, 2, 1, 3>), g16, dim3(512), lds, st, g);
  } else {
    if (wide) MK_LAUNCH((decode_linear_mxfp4_kernel<16, 2, 2>), g16, dim3(1024), lds, st, g);
    else MK_LAUNCH((decode_linear_mxfp4_kernel<8, 2, 2, 3>), g16, dim3(512), lds, st, g);
  }
}
}  // namespace MK_E16_NS
}  // namespace
