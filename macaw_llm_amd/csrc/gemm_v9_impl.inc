// body of gemm_v9.hip, included once per 16-bit element type (MK_E16_T / MK_E16_NS / MK_V9_SFX): see gemm_v9.hip

namespace {
namespace MK_E16_NS {
using namespace mkg;
typedef MK_E16_T e16;
typedef E16<e16>::x8 e16x8;
typedef E16<e16>::x4 e16x4;

constexpr int BM9 = 256, BN9 = 256, BK7 = 64;
constexpr int HALF_BYTES = 128 * BK7 * 2;        // 16 KiB: 128 rows x 64 k
constexpr int A_SLOT = 2 * HALF_BYTES;           // 32 KiB
constexpr int B_BASE9 = 3 * A_SLOT;              // A: 3 slots, then B: 2 slots
constexpr int LDS9 = 5 * A_SLOT;                 // 163,840 B
// the 288 x 256 x 64 tile (gemm_bf16_tile288_kernel below; the slots are the generator's: gemm_v9_loop288.inc): A two slots
// of 288 rows, then B two slots
constexpr int BM288 = 288, A_SLOT288 = V9_A_SLOT288, B_BASE288 = V9_B_BASE288, LDS288 = V9_LDS288;
static_assert(A_SLOT288 == BM288 * BK7 * 2 && LDS288 == B_BASE288 + 2 * A_SLOT && LDS288 <= LDS9, "gemm_v9_loop288.inc");

#include "gemm_lds_image.inc"

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// Whole tiles only (M % 256 == N % 256 == K % 64 == 0, K >= 128: the launcher checks): the asm derives every LDS-DMA
// voffset from piece 0's by adding strides, which is the C++ formula without its edge clamp.
// everything of one tile that the LDS-DMA requests and the asm block need.  A wave owns the 1-KiB pieces w + 4 i of an
// operand's tile image: i < BM / 32 of A (8 rows of a K-major image each; a half-tile of 128 rows is 16 pieces), i < 8 of B.
// (ONE struct for both tile heights, the 256-row tile leaves voA[8] unused: as a class template it would be instantiated in
// the host pass as well, where a member of the buffer resource type is ill-formed -- hipcc then drops every kernel that
// uses it from the host object without a diagnostic.)
struct V9Tile {
  int m0, n0;
  e16* C;
  const e16* Rp;
  __amdgpu_buffer_rsrc_t rsA, rsB;
  u32x4 dA, dB;
  int voA[BM288 / 32], voB[8];
};

#ifndef V9_MFMA16
#define V9_MFMA16 0
#endif
// LDS-DMA source offset of a lane's 16 bytes for the layouts on the 16 x 16 x 32 loop.  K-major operands keep v7's image.
// Reduction-major ones add ONE bit to its swizzle: the 16-byte chunk index is also XORed with 2 * ((k-row >> 3) & 1).  A
// 16 x 32 fragment is read by four 16-lane groups that hold k-rows 8 g .. 8 g + 7 of the SAME 16 columns; without the bit
// groups g and g + 1 hit the same banks (rows 8 apart = 2048 bytes).  (k-row >> 3) & 1 = (piece >> 1) & 1 = (wave >> 1) & 1
// for every piece of a wave, so the asm still derives a wave's voffsets from piece 0's by adding strides.
template <bool RED_MAJOR, bool M16>
MK_DEV int v9_voffset(int row0, int R, long ld, int half, int p, int l) {
  if constexpr (!RED_MAJOR || !M16) {
    return v7_voffset<RED_MAJOR>(row0, R, ld, half, p, l);
  } else {
    const int kr = p * 4 + (l >> 4);
    const int mc = (l & 15) ^ (4 * (kr & 3)) ^ (2 * ((kr >> 3) & 1));
    return (int)((long)kr * ld * 2 + (half * 128 + mc * 8) * 2);
  }
}
// LDS read address (relative to the operand's half-tile image) of fragment 0, k32-step 0 on the 16 x 16 x 32 loop.
// K-major: lane -> row l & 15, 16-byte chunk l >> 4 (k32-step 1: chunk ^ 4, fragments + 2048).  Reduction-major (two
// transposing reads per fragment): lane group g = l >> 4 holds k-rows 8 g + (li >> 2) (+ 4), columns 4 (li & 3) .. + 3 of
// the fragment; fragment f = 2 a + b: chunk ^ (4 a + 2 b) (the asm XORs (a << 6) | (b << 5)), k32-step 1: + 8192.
template <bool RED_MAJOR>
MK_DEV int v9_read_offset16(int l) {
  if constexpr (!RED_MAJOR) {
    const int row = l & 15;
    return row * 128 + (((l >> 4) ^ ((row >> 1) & 7)) << 4);
  } else {
    const int g = l >> 4, li = l & 15, t = li >> 2, c = li & 3;
    const int kr = 8 * g + t;
    const int chunk = (4 * t) ^ (2 * (g & 1)) ^ (c >> 1);
    return kr * 256 + (chunk << 4) + ((c & 1) << 3);
  }
}

// The operand part of a tile's set-up, for gemm_bf16_v9_kernel and gemm_bf16_grp_kernel alike: descriptors of the A and B
// panels of the tile at (m0, n0) (the compiler's form and four scalar words each for the asm block) and the lane's LDS-DMA
// voffsets.  P: the problem (GemmArgs or GrpProb: M, N, K, lda, ldb); A, B: its operands.  CLAMP: a K-major panel's record
// ends at the matrix edge when fewer than 256 rows are left (a launch of whole tiles needs no clamp).
template <bool A_RED, bool B_RED, bool CLAMP, int BM = BM9, typename P>
MK_DEV void v9_operand_setup(const P& g, const e16* A, const e16* B, int m0, int n0, int w, int l, V9Tile& t) {
  static_assert(BM == BM9 || !A_RED, "a taller tile exists for a K-major A only (its image is one run of 8-row pieces)");
  constexpr bool M16 = ((V9_MFMA16 >> (2 * (A_RED ? 1 : 0) + (B_RED ? 1 : 0))) & 1) != 0;
  t.m0 = m0; t.n0 = n0;
  const e16* abase = uniform_ptr(A_RED ? A + m0 : A + (long)m0 * g.lda);
  const e16* bbase = uniform_ptr(B_RED ? B + n0 : B + (long)n0 * g.ldb);
  const long a_bytes = A_RED ? ((long)(g.K - 1) * g.lda + ((g.M - m0 + 1) & ~1)) * 2
                             : ((long)((CLAMP ? min(g.M - m0, BM) : BM) - 1) * g.lda + ((g.K + 1) & ~1)) * 2;
  const long b_bytes = B_RED ? ((long)(g.K - 1) * g.ldb + ((g.N - n0 + 1) & ~1)) * 2
                             : ((long)((CLAMP ? min(g.N - n0, BN9) : BN9) - 1) * g.ldb + ((g.K + 1) & ~1)) * 2;
  const int a_rec = __builtin_amdgcn_readfirstlane((int)min(a_bytes, 0x7fffffffL));
  const int b_rec = __builtin_amdgcn_readfirstlane((int)min(b_bytes, 0x7fffffffL));
  t.rsA = __builtin_amdgcn_make_buffer_rsrc((void*)abase, 0, a_rec, 0x00020000);
  t.rsB = __builtin_amdgcn_make_buffer_rsrc((void*)bbase, 0, b_rec, 0x00020000);
  // the same descriptors as four scalar words each, for the asm block (base, base_hi | stride 0, bytes, flags)
  const uint64_t pa = reinterpret_cast<uint64_t>(abase), pb = reinterpret_cast<uint64_t>(bbase);
  t.dA[0] = __builtin_amdgcn_readfirstlane((uint32_t)pa);
  t.dA[1] = __builtin_amdgcn_readfirstlane((uint32_t)(pa >> 32) & 0xffffu);
  t.dA[2] = (uint32_t)a_rec;
  t.dA[3] = 0x00020000u;
  t.dB[0] = __builtin_amdgcn_readfirstlane((uint32_t)pb);
  t.dB[1] = __builtin_amdgcn_readfirstlane((uint32_t)(pb >> 32) & 0xffffu);
  t.dB[2] = (uint32_t)b_rec;
  t.dB[3] = 0x00020000u;
  // piece w + 4 i = piece w + 4 (i & 3) of half-tile i >> 2
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      t.voA[4 * h + i] = v9_voffset<A_RED, M16>(m0, g.M, g.lda, h, w + 4 * i, l);
      t.voB[4 * h + i] = v9_voffset<B_RED, M16>(n0, g.N, g.ldb, h, w + 4 * i, l);
    }
#pragma unroll
  for (int i = 8; i < BM / 32; ++i) t.voA[i] = v9_voffset<A_RED, M16>(m0, g.M, g.lda, i >> 2, w + 4 * (i & 3), l);
}

// element (z1, z2) of a batched operand.  (A function on purpose: as a call it stays beside the tile index until the
// inliner has run, and hipcc then orders the set-up as it did before v9_operand_setup was split off:
// profiles/v9_shared_tile_isa.txt)
template <typename T>
MK_DEV T* v9_batch_elem(T* p, long z1, long s1, long z2, long s2) {
  return p + z1 * s1 + z2 * s2;
}
// mk_gemm's tile: the XCD-aware tile order, the batch element of blockIdx.z, the residual
template <bool A_RED, bool B_RED, int BM = BM9>
MK_DEV void v9_tile_setup(const GemmArgs& g, int tile, int w, int l, V9Tile& t) {
  int tm, tn;
  tile_from_index(xcd_remap(tile, g.dp_tiles), g.tiles_m, g.tiles_n, tm, tn, 8);
  const int z = blockIdx.z, z1 = z / g.nb2, z2 = z - z1 * g.nb2;
  const e16* A = v9_batch_elem(reinterpret_cast<const e16*>(g.A), z1, g.sA1, z2, g.sA2);
  const e16* B = v9_batch_elem(reinterpret_cast<const e16*>(g.B), z1, g.sB1, z2, g.sB2);
  t.C = v9_batch_elem(reinterpret_cast<e16*>(g.C), z1, g.sC1, z2, g.sC2);
  t.Rp = g.R ? v9_batch_elem(reinterpret_cast<const e16*>(g.R), z1, g.sR1, z2, g.sR2) : nullptr;
  v9_operand_setup<A_RED, B_RED, true, BM>(g, A, B, tm * BM, tn * BN9, w, l, t);
}

// the first LDS-DMA requests of a tile (as gemm_v8).  256 rows: tile 0 (A, B piece by piece), A(1), half 0 of B(1) -- 28
// pieces per wave.  288 rows (two slots per operand): tile 0, A(1) -- 26 pieces.  The wait for tile 0 is the asm block's
template <int BM = BM9>
MK_DEV void v9_tile_request(const V9Tile& t, char* smem, int w, int stepA, int stepB) {
  constexpr int NPA = BM / 32, A_SLOT_ = BM * BK7 * 2, B_BASE_ = BM == BM9 ? B_BASE9 : B_BASE288;
#define V9_DMA_A(DST, I, KO)                                                                      \
  __builtin_amdgcn_raw_ptr_buffer_load_lds(                                                       \
      t.rsA, (__attribute__((address_space(3))) void*)(smem + (DST) + ((I) >> 2) * HALF_BYTES + (w + 4 * ((I) & 3)) * 1024), \
      16, t.voA[I], KO, 0, 0)
#define V9_DMA_B(DST, I, KO)                                                                      \
  __builtin_amdgcn_raw_ptr_buffer_load_lds(                                                       \
      t.rsB, (__attribute__((address_space(3))) void*)(smem + (DST) + ((I) >> 2) * HALF_BYTES + (w + 4 * ((I) & 3)) * 1024), \
      16, t.voB[I], KO, 0, 0)
#pragma unroll
  for (int i = 0; i < 8; ++i) { V9_DMA_A(0, i, 0); V9_DMA_B(B_BASE_, i, 0); }
#pragma unroll
  for (int i = 8; i < NPA; ++i) V9_DMA_A(0, i, 0);
#pragma unroll
  for (int i = 0; i < NPA; ++i) V9_DMA_A(A_SLOT_, i, stepA);
  if constexpr (BM == BM9) {
#pragma unroll
    for (int i = 0; i < 4; ++i) V9_DMA_B(B_BASE9 + A_SLOT, i, stepB);
  }
#undef V9_DMA_A
#undef V9_DMA_B
}

// ---- shared by gemm_bf16_v9_kernel and gemm_bf16_grp_kernel (#undef'd at the end of this file).
// The K loop (it names the kernel's locals t, adA, adB, iA, iB, stepA, stepB, nk, wv): ONE asm statement around a generated text (scripts/gen_v9_loop.py: register map, placement rule and the
// slot / wait protocol there) with that text's clobber list.
#define V9_ASM_IN                                                                                 \
  [voA] "v"(t.voA[0]), [voB] "v"(t.voB[0]), [adA] "v"(adA), [adB] "v"(adB), [rsA] "s"(t.dA), [rsB] "s"(t.dB),       \
      [iA] "s"(iA), [iB] "s"(iB), [stA] "s"(stepA), [stB] "s"(stepB), [nk] "s"(nk), [wv] "s"(wv)
#define V9_ASM(TEXT, CLOBBERS) asm volatile(TEXT : : V9_ASM_IN : CLOBBERS)
// the 288-row tile's loop: its ninth fragment row accumulates in eight VGPR quadruples of the compiler's (c8_0 .. c8_7)
#define V9_ASM288(TEXT, CLOBBERS)                                                                 \
  asm volatile(TEXT                                                                               \
               : [c0] "+v"(c8_0), [c1] "+v"(c8_1), [c2] "+v"(c8_2), [c3] "+v"(c8_3), [c4] "+v"(c8_4), [c5] "+v"(c8_5),  \
                 [c6] "+v"(c8_6), [c7] "+v"(c8_7)                                                  \
               : V9_ASM_IN                                                                        \
               : CLOBBERS)
#if V9_MFMA16
// Register epilogue of the 16 x 16 fragments: D[n = 4 (l >> 4) + e][m = l & 15] of fragment (i, j) -> a lane owns 4
// consecutive columns of ONE row: row m0 + wm0 + 16 i + (l & 15), columns n0 + wn0 + 16 j + 4 (l >> 4) .. + 3 = one
// 8-byte access per lane and fragment; CROW points at the lane's four columns of fragment (0, 0).
// (MK_V9_NT_STORE: experiment build -- the C stores with the non-temporal hint, so that a round's 4 MiB of output per
// XCD do not displace the operand panels from its L2; measured in profiles/r06_gemm_v9_nt_store.txt)
#ifdef MK_V9_NT_STORE
typedef unsigned int v9_u32x2 __attribute__((ext_vector_type(2)));
#define V9_ST8(PTR, VAL) __builtin_nontemporal_store(__builtin_bit_cast(v9_u32x2, VAL), reinterpret_cast<v9_u32x2*>(PTR))
#else
#define V9_ST8(PTR, VAL) (*reinterpret_cast<e16x4*>(PTR) = (VAL))
#endif
#define V9_F16P(I, J, CROW, LDC, ALPHA)   /* alpha only */                                        \
  do {                                                                                            \
    float t_[4];                                                                                  \
    V9_ACC16_READ_##I##_##J(t_);                                                                  \
    e16x4 o_;                                                                                     \
    _Pragma("unroll") for (int e_ = 0; e_ < 4; ++e_) o_[e_] = (e16)(t_[e_] * (ALPHA));           \
    V9_ST8((CROW) + (long)(16 * (I)) * (LDC) + 16 * (J), o_);                                     \
  } while (0)
#define V9_F16R(I, J, CROW, LDC, ALPHA)   /* + residual (requested for the whole tile up front: the kernel's rv_) */ \
  do {                                                                                            \
    float t_[4];                                                                                  \
    V9_ACC16_READ_##I##_##J(t_);                                                                  \
    e16x4 o_;                                                                                     \
    _Pragma("unroll") for (int e_ = 0; e_ < 4; ++e_) o_[e_] = (e16)(t_[e_] * (ALPHA) + (float)rv_[I][J][e_]); \
    V9_ST8((CROW) + (long)(16 * (I)) * (LDC) + 16 * (J), o_);                                     \
  } while (0)
// The same two with gemm_v7's arithmetic (gemm_common.h wave_epilogue16), rounding for rounding: the product with alpha is
// rounded to fp32, then the residual is added and rounded to fp32, then the sum is rounded to 16 bits.  In the two forms
// above hipcc contracts the first two steps into one fma and, for fp16, the product and the conversion into
// v_fma_mixlo_f16 (one rounding instead of two): whenever alpha is no power of two they differ from v7 in the last bit of
// about one output in 10^4.  The 288-row tile uses these (tests/test_gemm_tile288_gpu.py pins it to v7 bit for bit at such an
// alpha); the 256-row kernels keep their code.  V9_FP32 holds a fragment's four values in fp32 registers between two steps;
// it emits nothing.
#define V9_FP32(X) asm("" : "+v"(X))
#define V9_F16PS(I, J, CROW, LDC, ALPHA)                                                          \
  do {                                                                                            \
    float t_[4];                                                                                  \
    V9_ACC16_READ_##I##_##J(t_);                                                                  \
    f32x4 p_ = {t_[0], t_[1], t_[2], t_[3]};                                                      \
    p_ *= (ALPHA);                                                                                \
    V9_FP32(p_);                                                                                  \
    e16x4 o_;                                                                                     \
    _Pragma("unroll") for (int e_ = 0; e_ < 4; ++e_) o_[e_] = (e16)p_[e_];                        \
    V9_ST8((CROW) + (long)(16 * (I)) * (LDC) + 16 * (J), o_);                                     \
  } while (0)
#define V9_F16RS(I, J, CROW, LDC, ALPHA)                                                          \
  do {                                                                                            \
    float t_[4];                                                                                  \
    V9_ACC16_READ_##I##_##J(t_);                                                                  \
    f32x4 p_ = {t_[0], t_[1], t_[2], t_[3]};                                                      \
    p_ *= (ALPHA);                                                                                \
    V9_FP32(p_);                                                                                  \
    _Pragma("unroll") for (int e_ = 0; e_ < 4; ++e_) p_[e_] += (float)rv_[I][J][e_];              \
    V9_FP32(p_);                                                                                  \
    e16x4 o_;                                                                                     \
    _Pragma("unroll") for (int e_ = 0; e_ < 4; ++e_) o_[e_] = (e16)p_[e_];                        \
    V9_ST8((CROW) + (long)(16 * (I)) * (LDC) + 16 * (J), o_);                                     \
  } while (0)
// (a scheduling fence per fragment row: without it hipcc hoists all 256 accumulator reads and spills)
#define V9_R16(F, I, CROW, LDC, ALPHA)                                                            \
  do {                                                                                            \
    F(I, 0, CROW, LDC, ALPHA); F(I, 1, CROW, LDC, ALPHA); F(I, 2, CROW, LDC, ALPHA); F(I, 3, CROW, LDC, ALPHA); \
    F(I, 4, CROW, LDC, ALPHA); F(I, 5, CROW, LDC, ALPHA); F(I, 6, CROW, LDC, ALPHA); F(I, 7, CROW, LDC, ALPHA); \
    __builtin_amdgcn_sched_barrier(0);                                                            \
  } while (0)
#define V9_EPI16(F, CROW, LDC, ALPHA)                                                             \
  do {                                                                                            \
    V9_R16(F, 0, CROW, LDC, ALPHA); V9_R16(F, 1, CROW, LDC, ALPHA); V9_R16(F, 2, CROW, LDC, ALPHA); \
    V9_R16(F, 3, CROW, LDC, ALPHA); V9_R16(F, 4, CROW, LDC, ALPHA); V9_R16(F, 5, CROW, LDC, ALPHA); \
    V9_R16(F, 6, CROW, LDC, ALPHA); V9_R16(F, 7, CROW, LDC, ALPHA);                               \
  } while (0)
#endif

// Whole tiles only (M % 256 == N % 256 == K % 64 == 0, K >= 128: the launcher checks): the asm derives every LDS-DMA
// voffset from piece 0's by adding strides, which is the C++ formula without its edge clamp.
//
// Workgroup b computes tiles b, b + gridDim.x, ... < dp_tiles (the launcher sends one workgroup per planned CU when the
// tiles are whole rounds, else one per tile).  A walking workgroup requests the first K-tiles of its NEXT tile before
// the epilogue of the current one (behind a barrier: every wave has read the last fragments of the ring), so the
// descriptor set-up and the first LDS-DMA round trip run under the epilogue's stores.
template <bool A_RED, bool B_RED>
__global__ __launch_bounds__(256, 1) void gemm_bf16_v9_kernel(GemmArgs g) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int l = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wr = w >> 1, wc = w & 1;      // this wave's A half / B half
  const int wm0 = wr * 128, wn0 = wc * 128;
  const int stepA = A_RED ? (int)(BK7 * g.lda * 2) : BK7 * 2;   // bytes per K-tile
  const int stepB = B_RED ? (int)(BK7 * g.ldb * 2) : BK7 * 2;
  // bytes between a wave's consecutive pieces (p -> p + 4): 32 rows of a K-major image, 16 k-rows of a reduction-major one
  const int iA = (int)((A_RED ? 16 : 32) * g.lda * 2);
  const int iB = (int)((B_RED ? 16 : 32) * g.ldb * 2);
  int offA[4], offB[4];
  v7_read_offsets<A_RED>(0, l, offA);
  v7_read_offsets<B_RED>(0, l, offB);
  const int nk = __builtin_amdgcn_readfirstlane((g.K + BK7 - 1) / BK7);
  const uint32_t lds0 = __builtin_amdgcn_readfirstlane(
      (uint32_t)(size_t)((__attribute__((address_space(3))) char*)smem));
  const uint32_t wv = lds0 + (uint32_t)w * 1024u;
  // layouts whose K loop runs on 16 x 16 x 32 MFMAs (scripts/gen_v9_loop.py: V9_MFMA16 bit mask)
  constexpr bool M16 = ((V9_MFMA16 >> (2 * (A_RED ? 1 : 0) + (B_RED ? 1 : 0))) & 1) != 0;
  const uint32_t adA = lds0 + wr * HALF_BYTES + (M16 ? v9_read_offset16<A_RED>(l) : offA[0]);
  const uint32_t adB = lds0 + B_BASE9 + wc * HALF_BYTES + (M16 ? v9_read_offset16<B_RED>(l) : offB[0]);
  const bool plain = g.bias_mode == 0 && g.act == 0 && g.R == nullptr && g.accumulate == 0 && (g.c_vec == 2 || (M16 && g.c_vec >= 1)) &&
                     g.scale_a == nullptr && g.scale_b == nullptr && g.ablate != 9;

  int tile = blockIdx.x;
  const int stride = (int)gridDim.x;
  V9Tile t;
  v9_tile_setup<A_RED, B_RED>(g, tile, w, l, t);
  v9_tile_request(t, smem, w, stepA, stepB);
  bool first = true;
  for (;;) {
    __builtin_amdgcn_sched_barrier(0);
    // ---- the K loop
#define V9_LOOPS(W)                                                                               \
  do {                                                                                            \
    if constexpr (!A_RED && !B_RED) V9_ASM(V9_LOOP_TEXT_00##W, V9_LOOP_CLOBBERS);                 \
    else if constexpr (!A_RED && B_RED) V9_ASM(V9_LOOP_TEXT_01##W, V9_LOOP_CLOBBERS);             \
    else if constexpr (A_RED && !B_RED) V9_ASM(V9_LOOP_TEXT_10##W, V9_LOOP_CLOBBERS);             \
    else V9_ASM(V9_LOOP_TEXT_11##W, V9_LOOP_CLOBBERS);                                            \
  } while (0)
#if V9_MFMA16
#define V9_LOOPS16(W)                                                                             \
  do {                                                                                            \
    if constexpr (!A_RED && !B_RED) V9_ASM(V9_LOOP16_TEXT_00##W, V9_LOOP16_CLOBBERS);             \
    else if constexpr (!A_RED && B_RED) V9_ASM(V9_LOOP16_TEXT_01##W, V9_LOOP16_CLOBBERS);         \
    else if constexpr (A_RED && !B_RED) V9_ASM(V9_LOOP16_TEXT_10##W, V9_LOOP16_CLOBBERS);         \
    else V9_ASM(V9_LOOP16_TEXT_11##W, V9_LOOP16_CLOBBERS);                                        \
  } while (0)
    if constexpr (M16) {
      if (first) V9_LOOPS16();
      else V9_LOOPS16(_W);
    } else
#endif
    {
      if (first) V9_LOOPS();
      else V9_LOOPS(_W);
    }
#undef V9_LOOPS
#undef V9_LOOPS16
    __builtin_amdgcn_sched_barrier(0);
#ifdef MK_V9_NOEPI      // timing-only experiment builds (scripts/probe/build_v9_variants.sh): no epilogue
    return;
#endif
    // this tile's output position, then (walking) the next tile: its requests go out BEFORE the epilogue
    const int m0 = t.m0, n0 = t.n0;
    e16* C = t.C;
    const e16* Rp = t.Rp;
    const int ntile = tile + stride;
    const bool more = ntile < g.dp_tiles;      // (wave-uniform: kernel arguments and blockIdx only)
    if (more) {
      v9_tile_setup<A_RED, B_RED>(g, ntile, w, l, t);
      __builtin_amdgcn_s_barrier();            // every wave has read its last fragments: the ring may be refilled
      v9_tile_request(t, smem, w, stepA, stepB);
    }
#if V9_MFMA16
    if constexpr (M16) {
      // the register epilogue (V9_EPI16 above) in two forms: alpha only, and alpha + residual (o_proj / down_proj forward);
      // bias / activation / accumulate never reach this kernel (pick_cfg).  (A form with run-time switches per fragment
      // made hipcc keep 64-bit addresses per fragment live: 270 spilled registers.)
      const float alpha = g.alpha;
      const int mrow = m0 + wm0 + (l & 15), ncol = n0 + wn0 + 4 * (l >> 4);
      e16* crow = C + (long)mrow * g.ldc + ncol;
      const e16* rrow = Rp ? Rp + (long)mrow * g.ldr + ncol : nullptr;
      if (rrow == nullptr) {
        V9_EPI16(V9_F16P, crow, g.ldc, alpha);
      } else {
        // all 64 residual fragments of the lane are requested before the first accumulator is read (128 registers: the
        // K loop's fragment registers are free now) -- one HBM round trip for the tile instead of one per fragment row
        // (measured: 4096^3 + residual 113 -> see profiles/r06_gemm_v9_mfma16.txt section 4)
        e16x4 rv_[8][8];
#pragma unroll
        for (int i_ = 0; i_ < 8; ++i_)
#pragma unroll
          for (int j_ = 0; j_ < 8; ++j_)
            rv_[i_][j_] = *reinterpret_cast<const e16x4*>(rrow + (long)(16 * i_) * g.ldr + 16 * j_);
        __builtin_amdgcn_sched_barrier(0);
        V9_EPI16(V9_F16R, crow, g.ldc, alpha);
      }
    } else
#endif
    if (plain) {
      // (a) the plain product (alpha only: every LLaMA projection and its gradients): straight from the registers.  A
      // lane owns ONE output row of each fragment and 4-column groups 8 apart; one v_permlane32_swap per dword between
      // neighbouring groups leaves 8 consecutive columns = 16 bytes per lane (cdna_hip_programming.md T21), 2 stores
      // per fragment, no LDS, no barrier.  (gemm_v7 measured this form 1-2 % slower than its LDS-transposed one --
      // there the staging costs 5 us per tile on eight waves; on four waves it costs 14 us: profiles/r05_gemm_v9.txt.)
      const int half = l >> 5;
      const float alpha = g.alpha;
      e16* crow = C + (long)(m0 + wm0 + (l & 31)) * g.ldc + n0 + wn0 + 8 * half;
#define V9_FRAG(I, J)                                                                             \
  do {                                                                                            \
    float t_[16];                                                                                 \
    V9_ACC_READ_##I##_##J(t_);                                                                    \
    e16* rp_ = crow + (long)(32 * (I)) * g.ldc + 32 * (J);                                        \
    _Pragma("unroll") for (int p_ = 0; p_ < 2; ++p_) {                                            \
      e16x4 lo_, hi_;                                                                             \
      _Pragma("unroll") for (int e_ = 0; e_ < 4; ++e_) {                                          \
        lo_[e_] = (e16)(t_[8 * p_ + e_] * alpha);                                                 \
        hi_[e_] = (e16)(t_[8 * p_ + 4 + e_] * alpha);                                             \
      }                                                                                           \
      const uint2 a_ = __builtin_bit_cast(uint2, lo_), b_ = __builtin_bit_cast(uint2, hi_);       \
      const auto sx_ = __builtin_amdgcn_permlane32_swap(a_.x, b_.x, false, false);                \
      const auto sy_ = __builtin_amdgcn_permlane32_swap(a_.y, b_.y, false, false);                \
      u32x4 o_;                                                                                   \
      o_[0] = sx_[0]; o_[1] = sy_[0]; o_[2] = sx_[1]; o_[3] = sy_[1];                             \
      *reinterpret_cast<u32x4*>(rp_ + 16 * p_) = o_;                                              \
    }                                                                                             \
  } while (0)
#define V9_FROW(I) V9_FRAG(I, 0); V9_FRAG(I, 1); V9_FRAG(I, 2); V9_FRAG(I, 3)
      V9_FROW(0); V9_FROW(1); V9_FROW(2); V9_FROW(3);
#undef V9_FROW
#undef V9_FRAG
    } else {
      // (b) everything else (bias, activation, residual, accumulate, unaligned C): gemm_v7's LDS-transposed epilogue,
      // one fragment row at a time out of the accumulator file.  It stages through the ring: one workgroup per tile
      // (the launcher does not let these launches walk)
#define V9_ROW(I)                                                                                 \
  do {                                                                                            \
    float t0_[16], t1_[16], t2_[16], t3_[16];                                                     \
    V9_ACC_READ_##I##_0(t0_); V9_ACC_READ_##I##_1(t1_); V9_ACC_READ_##I##_2(t2_); V9_ACC_READ_##I##_3(t3_); \
    f32x16 r_[1][4];                                                                              \
    _Pragma("unroll") for (int e_ = 0; e_ < 16; ++e_) {                                           \
      r_[0][0][e_] = t0_[e_]; r_[0][1][e_] = t1_[e_]; r_[0][2][e_] = t2_[e_]; r_[0][3][e_] = t3_[e_]; \
    }                                                                                             \
    wave_epilogue16<false, e16, 1, 4>(r_, g, C, Rp, m0, n0, wm0 + 32 * (I), wn0, smem, (I) == 0); \
  } while (0)
      V9_ROW(0);
      V9_ROW(1);
      V9_ROW(2);
      V9_ROW(3);
#undef V9_ROW
    }
    if (!more) break;
    tile = ntile;
    first = false;
  }
}

#if V9_MFMA16 == 15
// ---- grouped launch (mk_gemm_grouped): one persistent workgroup per planned CU runs whole tiles of SEVERAL problems:
// its tiles b, b + n, ... of the main problem g.p[0] (grad-input: A K-major, B reduction-major), then its run of filler
// tiles (grad-weight: both reduction-major; GrpArgs in gemm_common.h, the plan in gemm_group_plan.h).  Per tile it is
// gemm_bf16_v9_kernel's protocol with the problem looked up per tile: set-up, the first LDS-DMA requests, the generated
// loop of the tile's layout, and the next tile's set-up and requests behind the barrier before this tile's epilogue --
// also when the next tile has the other layout (the ring's slots and the wait protocol do not depend on the layout).
// Every tile is computed by the instruction stream that gemm_bf16_v9_kernel runs on it, and by the same source: the
// two kernels share v9_operand_setup (descriptor bounds and words, voffsets), v9_tile_request, v9_voffset,
// v9_read_offset16, the generated loops inside V9_ASM and the alpha-only register epilogue V9_EPI16(V9_F16P) with its
// V9_ACC16_READ macros and V9_ST8 (so the MK_V9_NT_STORE experiment build reaches this kernel as well).  Per kernel
// remain: which tile comes next and whose it is (v9_tile_setup / grp_next + grp_tile_setup), the wave preamble, the
// loop's scalars (here per tile: GRP_SETUP) and the choice of loop text.
// tests/test_gemm_grouped_gpu.py compares the two paths bit for bit; scripts/kernel_isa_diff.py compares builds.
//
// a grouped tile: tile `lin` of problem p in plain order (grp_next has applied the XCD remap of the main problem); B is
// reduction-major in both layouts, whole tiles by mk_gemm_grouped's domain check (no record clamp), no residual
template <bool A_RED>
MK_DEV void grp_tile_setup(const GrpProb& p, int lin, int w, int l, V9Tile& t) {
  int tm, tn;
  tile_from_index(lin, p.tiles_m, p.tiles_n, tm, tn, 8);
  t.C = reinterpret_cast<e16*>(p.C);
  t.Rp = nullptr;
  v9_operand_setup<A_RED, true, false>(p, reinterpret_cast<const e16*>(p.A), reinterpret_cast<const e16*>(p.B), tm * BM9,
                                       tn * BN9, w, l, t);
}

// The workgroup's work list (wave-uniform throughout): its main tiles b, b + n, ..., then its filler tiles.  Fillers are
// dealt ROUND by round inside a group of workgroups (gemm_group_plan.h: the workgroups of one XCD): the group owns the
// indices [start[g0], start[g1]) of the taken filler tiles laid end to end, and in round j the workgroups that still
// have a j-th tile (count > j) take the next indices in rank order.  Lane i holds the count of the group's i-th member.
struct GrpCursor {
  int mt, stride;          // next main tile and the stride n
  int j, cnt, base;        // filler round, this workgroup's count, first index of round j
  int cl;                  // per lane: count of the group's member `lane`
  uint64_t below;          // lanes of the members before this workgroup
};
template <bool HAS_MAIN>
MK_DEV bool grp_next(const GrpArgs& g, GrpCursor& c, int& pi, int& lin) {
  if (HAS_MAIN && c.mt < g.main_tiles) {
    pi = 0;
    lin = xcd_remap(c.mt, g.main_tiles);
    c.mt += c.stride;
    return true;
  }
  if (c.j >= c.cnt) return false;
  const uint64_t act = __builtin_amdgcn_ballot_w64(c.cl > c.j);
  int at = c.base + __builtin_popcountll(act & c.below), f = 1;
  c.base += __builtin_popcountll(act);
  ++c.j;
  while (f < g.n_fill && at >= g.p[f].count) at -= g.p[f++].count;
  pi = f;
  lin = g.p[f].first + at;
  return true;
}

template <bool HAS_MAIN>
__global__ __launch_bounds__(256, 1) void gemm_bf16_grp_kernel(GrpArgs g) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int l = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wr = w >> 1, wc = w & 1;
  const int wm0 = wr * 128, wn0 = wc * 128;
  const uint32_t lds0 = __builtin_amdgcn_readfirstlane(
      (uint32_t)(size_t)((__attribute__((address_space(3))) char*)smem));
  const uint32_t wv = lds0 + (uint32_t)w * 1024u;
  const uint32_t adA_k = lds0 + wr * HALF_BYTES + v9_read_offset16<false>(l);
  const uint32_t adA_r = lds0 + wr * HALF_BYTES + v9_read_offset16<true>(l);
  const uint32_t adB = lds0 + B_BASE9 + wc * HALF_BYTES + v9_read_offset16<true>(l);
  const int n = (int)gridDim.x, b = (int)blockIdx.x;
  const int rank = (n & 7) == 0 ? (b & 7) * (n >> 3) + (b >> 3) : b;      // gemm_group_plan.h wg_rank
  const int gw = (n & 7) == 0 ? n >> 3 : 64;                             // gemm_group_plan.h group_width
  const int g0 = rank / gw * gw, gsz = min(gw, n - g0);
  GrpCursor cur;
  cur.mt = b; cur.stride = n;
  cur.j = 0; cur.cnt = (int)g.start[rank + 1] - (int)g.start[rank]; cur.base = g.start[g0];
  cur.cl = l < gsz ? (int)g.start[g0 + l + 1] - (int)g.start[g0 + l] : 0;
  cur.below = (1ull << (rank - g0)) - 1;
  int pi, lin;
  if (!grp_next<HAS_MAIN>(g, cur, pi, lin)) return;      // (a workgroup without work is legal)
  V9Tile t;
  bool a_red;
  int nk, stepA, stepB, iA, iB;
  uint32_t adA;
  // set-up of one tile: the descriptor words and offsets in t, the loop's scalars beside it
#define GRP_SETUP()                                                                               \
  do {                                                                                            \
    pi = __builtin_amdgcn_readfirstlane(pi);                                                      \
    const GrpProb& p_ = g.p[pi];                                                                  \
    a_red = !HAS_MAIN || pi != 0;                                                                 \
    if (a_red) grp_tile_setup<true>(p_, lin, w, l, t);                                            \
    else grp_tile_setup<false>(p_, lin, w, l, t);                                                 \
    nk = __builtin_amdgcn_readfirstlane(p_.K / BK7);                                              \
    stepA = __builtin_amdgcn_readfirstlane(a_red ? (int)(BK7 * p_.lda * 2) : BK7 * 2);            \
    stepB = __builtin_amdgcn_readfirstlane((int)(BK7 * p_.ldb * 2));                              \
    iA = __builtin_amdgcn_readfirstlane((int)((a_red ? 16 : 32) * p_.lda * 2));                   \
    iB = __builtin_amdgcn_readfirstlane((int)(16 * p_.ldb * 2));                                  \
    adA = a_red ? adA_r : adA_k;                                                                  \
  } while (0)
  GRP_SETUP();
  v9_tile_request(t, smem, w, stepA, stepB);
  bool first = true;
  for (;;) {
    __builtin_amdgcn_sched_barrier(0);
    if (HAS_MAIN && !a_red) {
      if (first) V9_ASM(V9_LOOP16_TEXT_01, V9_LOOP16_CLOBBERS);
      else V9_ASM(V9_LOOP16_TEXT_01_W, V9_LOOP16_CLOBBERS);
    } else {
      if (first) V9_ASM(V9_LOOP16_TEXT_11, V9_LOOP16_CLOBBERS);
      else V9_ASM(V9_LOOP16_TEXT_11_W, V9_LOOP16_CLOBBERS);
    }
    __builtin_amdgcn_sched_barrier(0);
    // this tile's output position, then the next tile: its requests go out BEFORE the epilogue
    const int m0 = t.m0, n0 = t.n0;
    e16* C = t.C;
    const long ldc = g.p[pi].ldc;
    const float alpha = g.p[pi].alpha;
    const bool more = grp_next<HAS_MAIN>(g, cur, pi, lin);
    if (more) {
      GRP_SETUP();
      __builtin_amdgcn_s_barrier();            // every wave has read its last fragments: the ring may be refilled
      v9_tile_request(t, smem, w, stepA, stepB);
    }
    // the register epilogue, alpha only
    e16* crow = C + (long)(m0 + wm0 + (l & 15)) * ldc + n0 + wn0 + 4 * (l >> 4);
    V9_EPI16(V9_F16P, crow, ldc, alpha);
    if (!more) break;
    first = false;
  }
#undef GRP_SETUP
}

int launch_grp(const GrpArgs& g, bool has_main, int n_wg, hipStream_t st) {
  static bool attr_done = false;
  if (!attr_done) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_bf16_grp_kernel<true>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, LDS9) != hipSuccess ||
        hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_bf16_grp_kernel<false>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, LDS9) != hipSuccess)
      return MK_ERR_LAUNCH;
    attr_done = true;
  }
  if (has_main) MK_LAUNCH((gemm_bf16_grp_kernel<true>), dim3(n_wg), dim3(256), LDS9, st, g);
  else MK_LAUNCH((gemm_bf16_grp_kernel<false>), dim3(n_wg), dim3(256), LDS9, st, g);
  return mk_check_launch();
}
#endif  // V9_MFMA16 == 15

#if V9_MFMA16 == 15
// ---- the 288 x 256 x 64 tile: forward projections whose M is a multiple of 288 and not of 256 rounds of tiles (M = 4608 =
// 16 x 288: o_proj / down_proj are exactly 256 tiles, q|k|v 768).  Both operands K-major, alpha (+ residual) only, whole
// tiles only (M % 288 == N % 256 == K % 64 == 0, K >= 128: the launcher checks).  It is gemm_bf16_v9_kernel's protocol on the
// shared pieces at BM = 288: v9_tile_setup / v9_operand_setup, v9_tile_request, the generated loop inside V9_ASM288
// (gemm_v9_loop288.inc: 4 waves of 144 x 128 = 9 x 8 fragments, two LDS slots per operand) and V9_EPI16 plus a ninth
// fragment row, whose accumulators are VGPRs (a[0:255] hold rows 0 .. 7 as on the 256 tile).  Every element sees the K order
// and the MFMA of the 256 tile's loop, and the epilogue rounds as gemm_v7's does (V9_F16PS / V9_F16RS): the results are
// configuration 11's bits (tests/test_gemm_tile288_gpu.py).
#define V9_C8_READ(X, C) do { (X)[0] = (C)[0]; (X)[1] = (C)[1]; (X)[2] = (C)[2]; (X)[3] = (C)[3]; } while (0)
#define V9_ACC16_READ_8_0(X) V9_C8_READ(X, c8_0)
#define V9_ACC16_READ_8_1(X) V9_C8_READ(X, c8_1)
#define V9_ACC16_READ_8_2(X) V9_C8_READ(X, c8_2)
#define V9_ACC16_READ_8_3(X) V9_C8_READ(X, c8_3)
#define V9_ACC16_READ_8_4(X) V9_C8_READ(X, c8_4)
#define V9_ACC16_READ_8_5(X) V9_C8_READ(X, c8_5)
#define V9_ACC16_READ_8_6(X) V9_C8_READ(X, c8_6)
#define V9_ACC16_READ_8_7(X) V9_C8_READ(X, c8_7)
__global__ __launch_bounds__(256, 1) void gemm_bf16_tile288_kernel(GemmArgs g) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int l = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wr = w >> 1, wc = w & 1;      // this wave's 144 rows of A / B half
  const int wm0 = wr * (BM288 / 2), wn0 = wc * 128;
  const int stepA = BK7 * 2, stepB = BK7 * 2;          // bytes per K-tile
  const int iA = (int)(32 * g.lda * 2), iB = (int)(32 * g.ldb * 2);      // bytes between a wave's consecutive pieces
  const int nk = __builtin_amdgcn_readfirstlane(g.K / BK7);
  const uint32_t lds0 = __builtin_amdgcn_readfirstlane(
      (uint32_t)(size_t)((__attribute__((address_space(3))) char*)smem));
  const uint32_t wv = lds0 + (uint32_t)w * 1024u;
  const uint32_t adA = lds0 + wr * (A_SLOT288 / 2) + v9_read_offset16<false>(l);
  const uint32_t adB = lds0 + B_BASE288 + wc * HALF_BYTES + v9_read_offset16<false>(l);
  int tile = blockIdx.x;
  const int stride = (int)gridDim.x;
  V9Tile t;
  v9_tile_setup<false, false, BM288>(g, tile, w, l, t);
  v9_tile_request<BM288>(t, smem, w, stepA, stepB);
  bool first = true;
  for (;;) {
    f32x4 c8_0 = 0.f, c8_1 = 0.f, c8_2 = 0.f, c8_3 = 0.f, c8_4 = 0.f, c8_5 = 0.f, c8_6 = 0.f, c8_7 = 0.f;
    __builtin_amdgcn_sched_barrier(0);
    if (first) V9_ASM288(V9_LOOP288_TEXT_00, V9_LOOP288_CLOBBERS);
    else V9_ASM288(V9_LOOP288_TEXT_00_W, V9_LOOP288_CLOBBERS);
    __builtin_amdgcn_sched_barrier(0);
    // this tile's output position, then (walking) the next tile: its requests go out BEFORE the epilogue
    const int m0 = t.m0, n0 = t.n0;
    e16* C = t.C;
    const e16* Rp = t.Rp;
    const int ntile = tile + stride;
    const bool more = ntile < g.dp_tiles;      // (wave-uniform: kernel arguments and blockIdx only)
    if (more) {
      v9_tile_setup<false, false, BM288>(g, ntile, w, l, t);
      __builtin_amdgcn_s_barrier();            // every wave has read its last fragments: the slots may be refilled
      v9_tile_request<BM288>(t, smem, w, stepA, stepB);
    }
    const float alpha = g.alpha;
    const int mrow = m0 + wm0 + (l & 15), ncol = n0 + wn0 + 4 * (l >> 4);
    e16* crow = C + (long)mrow * g.ldc + ncol;
    const e16* rrow = Rp ? Rp + (long)mrow * g.ldr + ncol : nullptr;
    if (rrow == nullptr) {
      V9_EPI16(V9_F16PS, crow, g.ldc, alpha);
      V9_R16(V9_F16PS, 8, crow, g.ldc, alpha);
    } else {
      // the lane's 72 residual fragments up front, as on the 256 tile
      e16x4 rv_[9][8];
#pragma unroll
      for (int i_ = 0; i_ < 9; ++i_)
#pragma unroll
        for (int j_ = 0; j_ < 8; ++j_)
          rv_[i_][j_] = *reinterpret_cast<const e16x4*>(rrow + (long)(16 * i_) * g.ldr + 16 * j_);
      __builtin_amdgcn_sched_barrier(0);
      V9_EPI16(V9_F16RS, crow, g.ldc, alpha);
      V9_R16(V9_F16RS, 8, crow, g.ldc, alpha);
    }
    if (!more) break;
    tile = ntile;
    first = false;
  }
}
#undef V9_C8_READ
#undef V9_ACC16_READ_8_0
#undef V9_ACC16_READ_8_1
#undef V9_ACC16_READ_8_2
#undef V9_ACC16_READ_8_3
#undef V9_ACC16_READ_8_4
#undef V9_ACC16_READ_8_5
#undef V9_ACC16_READ_8_6
#undef V9_ACC16_READ_8_7

int launch_tile288(const GemmArgs& g, dim3 grid, hipStream_t st) {
  static bool attr_done = false;
  if (!attr_done) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_bf16_tile288_kernel),
                            hipFuncAttributeMaxDynamicSharedMemorySize, LDS288) != hipSuccess)
      return MK_ERR_LAUNCH;
    attr_done = true;
  }
  MK_LAUNCH(gemm_bf16_tile288_kernel, grid, dim3(256), LDS288, st, g);
  return mk_check_launch();
}
#endif  // V9_MFMA16 == 15

template <bool A_RED, bool B_RED>
int launch_v9(const GemmArgs& g, dim3 grid, hipStream_t st) {
  static bool attr_done = false;
  if (!attr_done) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_bf16_v9_kernel<A_RED, B_RED>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, LDS9) != hipSuccess)
      return MK_ERR_LAUNCH;
    attr_done = true;
  }
  MK_LAUNCH((gemm_bf16_v9_kernel<A_RED, B_RED>), grid, dim3(256), LDS9, st, g);
  return mk_check_launch();
}
}  // namespace MK_E16_NS
}  // namespace
#undef V9_ASM
#undef V9_ASM288
#undef V9_ASM_IN
#if V9_MFMA16
#undef V9_EPI16
#undef V9_R16
#undef V9_F16P
#undef V9_F16R
#undef V9_F16PS
#undef V9_F16RS
#undef V9_FP32
#undef V9_ST8
#endif
