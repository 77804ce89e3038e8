// What the three skinny16 weight-streaming kernels have in common whatever the weight format: gemm_skinny16_kernel
// (gemm_impl.inc, 16-bit weights), decode_linear_fp8_kernel (decode_fp8_impl.inc, e4m3) and decode_linear_mxfp4_kernel
// (decode_mxfp4_impl.inc, MXFP4).  The token prologue and the cross-wave reduction hold the rounding points and the
// summation order that the tests pin bit for bit across the formats, so they exist once, here.  All are force-inlined
// into kernels that keep their own __shared__ arrays and pass them in; none touches the K loop.  The lane -> k mapping,
// `load`, `mma`, the register ring and the epilogue depend on the weight format and stay in each kernel (DESIGN.md,
// "The skinny16 stream kernels": what was measured, and why l and w are arguments).  e16 is deduced from the token
// pointer, so one copy serves both element-type passes of a translation unit.
#pragma once

namespace {
// The M token rows, prepared once per workgroup into sk_smem ([M][K + 8] e16) while the first weight fragments are in
// flight: PRO 1 RMSNorm, y = w * rnd(x * rstd) with the rounding points of rmsnorm_fwd_kernel; PRO 2 SwiGLU of
// A = [gate | up] ([M, 2K]), rnd(rnd(silu(gate)) * up) as swiglu2d_fwd_kernel.  Called by all NW * 64 threads;
// l, w: the caller's lane and wave index.
template <int NW, int PRO, typename e16>
MK_DEV void skinny16_stage_tokens(const e16* A, long ld, int M, int K, const void* pro_w, float pro_eps, char* sk_smem,
                                  float (&ssq)[NW][16], int l, int w) {
  typedef typename E16<e16>::x8 e16x8;
  const int ldt = K + 8;                                    // LDS token row pitch (elements)
  e16* ts = reinterpret_cast<e16*>(sk_smem);
  const int nch = K / 8;                                    // 16-byte chunks per row
  for (int m = 0; m < M; ++m) {
    const e16* xr = A + (long)m * ld;
    float rstd = 1.f;
    if constexpr (PRO == 1) {
      float ss = 0.f;
      for (int c = threadIdx.x; c < nch; c += NW * 64) {
        const e16x8 xv = *reinterpret_cast<const e16x8*>(xr + c * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) ss += (float)xv[e] * (float)xv[e];
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
      __syncthreads();                                    // ssq of the previous row consumed
      if (l == 0) ssq[w][0] = ss;
      __syncthreads();
      float tot = 0.f;
#pragma unroll
      for (int ww = 0; ww < NW; ++ww) tot += ssq[ww][0];   // fixed order: deterministic
      rstd = rsqrtf(tot / (float)K + pro_eps);
    }
    for (int c = threadIdx.x; c < nch; c += NW * 64) {
      const e16x8 av = *reinterpret_cast<const e16x8*>(xr + c * 8);
      e16x8 bv;
      if constexpr (PRO == 1) bv = *reinterpret_cast<const e16x8*>(reinterpret_cast<const e16*>(pro_w) + c * 8);
      else bv = *reinterpret_cast<const e16x8*>(xr + K + c * 8);
      e16x8 o;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float a = (float)av[e], b = (float)bv[e];
        if constexpr (PRO == 1) o[e] = (e16)(b * rnd<e16>(a * rstd));
        else o[e] = (e16)(rnd<e16>(a / (1.f + __expf(-a))) * b);
      }
      *reinterpret_cast<e16x8*>(ts + m * ldt + c * 8) = o;
    }
  }
  __syncthreads();
}

// The cross-wave reduction: every wave summed its own K blocks.  skinny16_reduce_put parks the partial accumulators
// in red (acc2: token tile 1, MT == 2) and ends with the barrier; skinny16_reduce_get then gives output t < 256 * MT
// of the workgroup: the sum over the waves in a fixed order, and its token m and weight row n -- which the caller
// still has to check against [M, N] before its epilogue.
// D[i = weight row][j = token]: lane holds j = l & 15, i = 4 * (l >> 4) + e
template <int NW, int MT>
MK_DEV void skinny16_reduce_put(float (&red)[NW][4 * MT][64], const f32x4& acc, const f32x4& acc2, int l, int w) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    red[w][e][l] = acc[e];
    if constexpr (MT == 2) red[w][4 + e][l] = acc2[e];
  }
  __syncthreads();
}
template <int NW, int MT>
MK_DEV float skinny16_reduce_get(const float (&red)[NW][4 * MT][64], int t, int n0, int& m, int& n) {
  const int e = (t >> 6) & 3, ll = t & 63, mt = t >> 8;
  float v = 0.f;
#pragma unroll
  for (int ww = 0; ww < NW; ++ww) v += red[ww][4 * mt + e][ll];   // fixed order: deterministic
  m = 16 * mt + (ll & 15);
  n = n0 + 4 * (ll >> 4) + e;
  return v;
}
}  // namespace
