// The e4m3 weight-streaming kernel of mk_decode_linear_fp8 + its launcher, included once per element type
// (MK_E16_T / MK_E16_NS, see decode_fp8.hip).  e16 = bf16 or _Float16: the type of the tokens, the
// residual and the output, and the type the weight bytes are widened to in registers.
#include "skinny16_parts.inc"   // the token prologue and the cross-wave reduction of the skinny16 stream kernels

namespace {
namespace MK_E16_NS {
typedef MK_E16_T e16;
typedef E16<e16>::x8 e16x8;

// 8 e4m3 bytes (two dwords, k ascending with the byte address) -> 8 e16.  v_cvt_pk_f32_fp8 decodes OCP e4m3fn
// on gfx950, subnormals and the two NaN codes included; every e4m3 value is a normal number of bf16 and of f16
// (2^-9 ... 448, 3 mantissa bits), so the f32 -> e16 conversion that follows rounds nothing: the widening is exact.
// 8 VALU instructions per MFMA operand; the stream leaves a SIMD some 200 cycles per 16 x 16 x 32 MFMA at the
// HBM rate, so the conversions hide under the loads like the MFMAs do.
MK_DEV e16x8 widen8(unsigned lo, unsigned hi) {
  e16x8 o;
  f32x2 p;
  p = __builtin_amdgcn_cvt_pk_f32_fp8(lo, false); o[0] = (e16)p[0]; o[1] = (e16)p[1];
  p = __builtin_amdgcn_cvt_pk_f32_fp8(lo, true);  o[2] = (e16)p[0]; o[3] = (e16)p[1];
  p = __builtin_amdgcn_cvt_pk_f32_fp8(hi, false); o[4] = (e16)p[0]; o[5] = (e16)p[1];
  p = __builtin_amdgcn_cvt_pk_f32_fp8(hi, true);  o[6] = (e16)p[0]; o[7] = (e16)p[1];
  return o;
}

// gemm_skinny16_kernel (gemm_impl.inc) with the weight operand read as e4m3 bytes: 16 weight rows per workgroup
// (N / 16 workgroups: every CU pulls from the first microsecond), NW waves that split K in blocks of 64, a ring
// of NBUF register buffers so that the loads of the next trips are in flight under the MFMAs of this one, the
// same three token prologues (PRO 1 RMSNorm / 2 SwiGLU, token rows prepared in LDS), MT = 2 token tiles for
// 17 ... 32 plain rows, and the same fixed-order cross-wave reduction: the code of both is skinny16_parts.inc.
// What differs is the k-index of a lane.  A K-block of 64 is 64 BYTES of a weight row, so ONE 16-byte load per
// lane covers it: lane (r16, kq) holds k = 16 kq ... 16 kq + 15 of weight row r16, bytes 0 ... 7 feed the first
// MFMA of the block and bytes 8 ... 15 the second.  The token operand follows: its two 16-byte loads of a block
// are the 32 contiguous bytes x[k = 16 kq ... 16 kq + 15] (in LDS likewise).  The MFMA sums over (lane group,
// element) pairs, so any k mapping the two operands share gives the same product.
// The de-quantisation scale of an output channel multiplies the fp32 sum in the epilogue, before the residual
// add and the one rounding to e16.
template <int NW, int U, int PRO, int NBUF = 2, int MT = 1>
__global__ __launch_bounds__(NW * 64) void decode_linear_fp8_kernel(DecodeFp8Args g) {
  static_assert(MT == 1 || PRO == 0, "two token tiles: plain token operand only");
  extern __shared__ __attribute__((aligned(16))) char sk_smem[];
  __shared__ float red[NW][4 * MT][64];
  __shared__ float ssq[NW][16];
  const int l = threadIdx.x & 63, w = threadIdx.x >> 6, r16 = l & 15, kq = l >> 4;
  const int n0 = blockIdx.x * 16;
  const e16* A = reinterpret_cast<const e16*>(g.x);
  const uint8_t* wp = g.Wq + (long)min(n0 + r16, g.N - 1) * g.ldw + 16 * kq;
  const int trow = min(r16, g.M - 1);
  const e16* xp = A + (long)trow * g.ldx + 16 * kq;
  const e16* xp2 = A + (long)min(16 + r16, g.M - 1) * g.ldx + 16 * kq;   // MT == 2: token rows 16 ... 31
  const int ldt = g.K + 8;                                  // LDS token row pitch (elements)
  const e16* tp = reinterpret_cast<const e16*>(sk_smem) + trow * ldt + 16 * kq;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f}, acc2 = {0.f, 0.f, 0.f, 0.f};
  const int nkb = g.K / 64;
  constexpr int XN = PRO == 0 ? 2 * U * MT : 1;
  // trip t of wave w covers K blocks w + NW * (t * U + u), u < U (neighbouring waves read
  // neighbouring 64-byte halves of a 128-byte line of a row)
  auto load = [&](uint4 (&wf)[U], e16x8 (&xf)[XN], int kb) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int kk = min(kb + u * NW, nkb - 1);       // clamped: the MFMA of a clamped block is skipped
      wf[u] = *reinterpret_cast<const uint4*>(wp + kk * 64);
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
        if constexpr (PRO == 0) xf[2 * u + hh] = *reinterpret_cast<const e16x8*>(xp + kk * 64 + 8 * hh);
        if constexpr (MT == 2) xf[2 * U + 2 * u + hh] = *reinterpret_cast<const e16x8*>(xp2 + kk * 64 + 8 * hh);
      }
    }
  };
  auto mma = [&](const uint4 (&wf)[U], const e16x8 (&xf)[XN], int kb) {
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (kb + u * NW < nkb) {
        e16x8 t0, t1;
        if constexpr (PRO == 0) {
          t0 = xf[2 * u]; t1 = xf[2 * u + 1];
        } else {
          t0 = *reinterpret_cast<const e16x8*>(tp + (kb + u * NW) * 64);
          t1 = *reinterpret_cast<const e16x8*>(tp + (kb + u * NW) * 64 + 8);
        }
        const e16x8 w0 = widen8(wf[u].x, wf[u].y), w1 = widen8(wf[u].z, wf[u].w);
        acc = E16<e16>::mma16(w0, t0, acc);
        acc = E16<e16>::mma16(w1, t1, acc);
        if constexpr (MT == 2) {
          acc2 = E16<e16>::mma16(w0, xf[2 * U + 2 * u], acc2);
          acc2 = E16<e16>::mma16(w1, xf[2 * U + 2 * u + 1], acc2);
        }
      }
  };
  // ring of NBUF register buffers: NBUF - 1 trips of this wave are in flight under the MFMAs of one
  uint4 wbuf[NBUF][U];
  e16x8 xbuf[NBUF][XN];
  constexpr int STEP = NW * U;
  int kb = w;
#pragma unroll
  for (int i = 0; i < NBUF - 1; ++i)
    if (kb + i * STEP < nkb) load(wbuf[i], xbuf[i], kb + i * STEP);
  if constexpr (PRO != 0)         // the token rows, prepared once per workgroup
    skinny16_stage_tokens<NW, PRO>(A, g.ldx, g.M, g.K, g.pro_w, g.pro_eps, sk_smem, ssq, l, w);
  while (kb < nkb) {
#pragma unroll
    for (int i = 0; i < NBUF; ++i) {
      if (kb + (NBUF - 1) * STEP < nkb) load(wbuf[(i + NBUF - 1) % NBUF], xbuf[(i + NBUF - 1) % NBUF], kb + (NBUF - 1) * STEP);
      mma(wbuf[i], xbuf[i], kb);
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
    v *= g.scale[n];
    if (Rp) v += (float)Rp[(long)m * g.ldr + n];
    C[(long)m * g.ldy + n] = (e16)v;
  }
}

// cfg as the 16-bit launcher chooses: 16 waves where N / 16 workgroups are few, else 8 waves and a ring of 3;
// 17 ... 32 plain rows: two token tiles per weight fragment
void launch_decode_linear_fp8(const DecodeFp8Args& g, int prologue, bool wide, size_t lds, hipStream_t st) {
  const dim3 g16(mk_cdiv(g.N, 16));
  if (g.M > 16) MK_LAUNCH((decode_linear_fp8_kernel<8, 2, 0, 2, 2>), g16, dim3(512), 0, st, g);
  else if (prologue == 0) {
    if (wide) MK_LAUNCH((decode_linear_fp8_kernel<16, 2, 0>), g16, dim3(1024), 0, st, g);
    else MK_LAUNCH((decode_linear_fp8_kernel<8, 2, 0, 3>), g16, dim3(512), 0, st, g);
  } else if (prologue == 1) {
    if (wide) MK_LAUNCH((decode_linear_fp8_kernel<16, 2, 1>), g16, dim3(1024), lds, st, g);
    else MK_LAUNCH((decode_linear_fp8_kernel<8, 2, 1, 3>), g16, dim3(512), lds, st, g);
  } else {
    if (wide) MK_LAUNCH((decode_linear_fp8_kernel<16, 2, 2>), g16, dim3(1024), lds, st, g);
    else MK_LAUNCH((decode_linear_fp8_kernel<8, 2, 2, 3>), g16, dim3(512), lds, st, g);
  }
}
}  // namespace MK_E16_NS
}  // namespace
