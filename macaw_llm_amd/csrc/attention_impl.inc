// body of attention.hip (fused attention forward / backward), included once per 16-bit element type
// (MK_E16_T / MK_E16_NS): e16 = bf16 or _Float16.
namespace {
namespace MK_E16_NS {
typedef MK_E16_T e16;
typedef E16<e16>::x8 e16x8;
typedef E16<e16>::x4 e16x4;
typedef e16 e16x2 __attribute__((ext_vector_type(2)));


struct FlashArgs {
  const e16* q; const e16* k; const e16* v; e16* o; float* lse; const int32_t* kmask;
  int B, H, Lq, Lk;
  long q_ld, q_bs, k_ld, k_bs, v_ld, v_bs, o_ld, o_bs;
  float scale;
  int nblk;     // non-causal forward: query blocks per (b, h) of the XCD-grouped 1-D grid (0: 3-D grid)
  // RoPE applied to q and k on their way in (short-sequence kernels only; null otherwise): cos / sin tables
  // [positions][head_dim] of the element type, rpos[b * Lq + row] = the position of a token
  const e16* rcos; const e16* rsin; const int32_t* rpos;
};

template <int HD>
MK_DEV int k_off(int row, int chunk) {  // K tile [64][HD] e16, 16-B chunk swizzle
  if constexpr (HD == 128) return row * 256 + ((chunk ^ (row & 15)) << 4);
  else return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4);
}
template <int HD>
MK_DEV int v_off(int key, int chunk) {  // V tile [64][HD] e16, read through tr_b16
  if constexpr (HD == 128) return key * 256 + ((chunk ^ (4 * (key & 3))) << 4);
  else return key * 128 + ((chunk ^ (4 * ((key >> 1) & 1))) << 4);
}

// Loads are issued UNCONDITIONALLY from a clamped row and zeroed by a select afterwards: a load
// under `if (row < n)` sits in its own basic block, the compiler then waits (vmcnt(0)) for each
// 16-byte chunk before issuing the next one -- eight serialised HBM round trips per tile, which
// was ~2/3 of the run time of every fused-attention kernel at S = 144.
MK_DEV uint4 ld16_or_zero(const e16* rowptr_clamped, bool ok) {
  uint4 v = *reinterpret_cast<const uint4*>(rowptr_clamped);
  if (!ok) v = make_uint4(0, 0, 0, 0);
  return v;
}
MK_DEV e16x8 ld8_or_zero(const e16* rowptr_clamped, bool ok) {
  const uint4 v = ld16_or_zero(rowptr_clamped, ok);
  return __builtin_bit_cast(e16x8, v);
}

// One output row per lane pair (l, l + 32): fragment d of `acc` holds this row's columns 32 d + 8 q + 4 (l >> 5) + e
// in registers 4 q + e.  Rounded to 16 bits a 4-column group is 8 bytes; one v_permlane32_swap per dword between
// groups 2 p and 2 p + 1 (guide T21) leaves 8 consecutive columns in each lane: 16-byte stores, half as many store
// instructions for the same bytes and addresses (the store tail of these kernels is issue-bound).  Executed by the
// WHOLE wave (the swap needs both halves), `ok` predicates the stores only.
template <int NDB>
MK_DEV void store_row16(e16* row, const f32x16 (&acc)[NDB], float mul, int half, bool ok) {
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
#pragma unroll
  for (int d = 0; d < NDB; ++d)
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      e16x4 lo, hi;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        lo[e] = (e16)(acc[d][8 * p + e] * mul);
        hi[e] = (e16)(acc[d][8 * p + 4 + e] * mul);
      }
      const uint2 a = __builtin_bit_cast(uint2, lo), b = __builtin_bit_cast(uint2, hi);
      const auto sx = __builtin_amdgcn_permlane32_swap(a.x, b.x, false, false);
      const auto sy = __builtin_amdgcn_permlane32_swap(a.y, b.y, false, false);
      u32x4 o;
      o[0] = sx[0]; o[1] = sy[0]; o[2] = sx[1]; o[3] = sy[1];
      if (ok) *reinterpret_cast<u32x4*>(row + d * 32 + 16 * p + 8 * half) = o;
    }
}

// x of this lane and of its partner in the other half-wave (lane ^ 32), as (value of the lower lane, value of the upper
// lane) in BOTH lanes: one v_permlane32_swap (VALU) instead of the LDS round trip of __shfl_xor / ds_bpermute, which a
// softmax segment would wait for twice with nothing to overlap it.  max / sum of the pair are symmetric in the two.
MK_DEV void half_pair(float x, float& lower, float& upper) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  lower = __uint_as_float(r[0]);
  upper = __uint_as_float(r[1]);
}

// One 32-key block of the online softmax in the exp2 domain, shared by flash_fwd_kernel and flash_fwd_short_kernel
// (the two must stay BIT-IDENTICAL: tests/test_kernels_gpu.py).  s: this lane's 16 raw scores q.k (keys
// (r & 3) + 8 (r >> 2) + 4 half of the block) -> p in place; pf: p rounded to 16 bits, the B operand of V^T P^T.
// `okbits` bit r: key r is valid and visible to this row (ignored when `interior`: every key of the block valid and
// visible to every row of the wave).  Round 5: the kernels spent 10.7 VALU instructions per MFMA (PMC:
// profiles/r05_attn_pmc.txt); per score now max (v_max3: half an instruction), ONE fma folding the scale and the
// running maximum (2^(s c2 - m)), the exponential, the row-sum add and half a convert -- the maximum is taken over the
// RAW scores and scaled once per row (c2 > 0: max(round(s c2)) = round(max(s) c2), the running maximum is the
// value it was).  Lazy rescaling (cdna_hip_programming.md T13): a row's accumulators are rescaled only when its
// maximum grew by more than 2^DEFER since its last rescale -- decided PER ROW (a row's arithmetic must not depend
// on its neighbours in the wave); only the branch around the O rescale is wave-uniform, rows that keep their
// maximum multiply by exactly 1.  NaN-safe: -inf - -inf compares false -> "grow" with alpha = 0.
template <int NDB>
MK_DEV void softmax_block(f32x16& s, bool interior, uint32_t okbits, float c2, float& m_run, float& l_run,
                          f32x16 (&oacc)[NDB], e16x8 (&pf)[2]) {
  constexpr float DEFER = 6.0f;          // 2^6 = 64: p, l stay far inside fp32 / e16 range
  if (!interior) {
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = ((okbits >> r) & 1u) ? s[r] : -INFINITY;
  }
  float mx = fmaxf(fmaxf(s[0], s[1]), s[2]);
#pragma unroll
  for (int r = 3; r < 15; r += 2) mx = fmaxf(fmaxf(mx, s[r]), s[r + 1]);
  mx = fmaxf(mx, s[15]);
  float mlo_, mhi_;
  half_pair(mx, mlo_, mhi_);               // (round 5: v_permlane32_swap instead of the LDS round trip of __shfl_xor; same value)
  mx = fmaxf(mlo_, mhi_) * c2;
  const bool grow = !(mx - m_run <= DEFER);
  if (__any(grow ? 1 : 0)) {
    const float m_new = grow ? fmaxf(m_run, mx) : m_run;
    const float alpha = !grow ? 1.f : ((m_run == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f(m_run - m_new));
    l_run *= alpha;
    m_run = m_new;
#pragma unroll
    for (int d = 0; d < NDB; ++d)
#pragma unroll
      for (int e = 0; e < 16; ++e) oacc[d][e] *= alpha;
  }
  float ps = 0.f;
  const float nm = -m_run;
  if (interior) {
#pragma unroll
    for (int r = 0; r < 16; ++r) { s[r] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[r], c2, nm)); ps += s[r]; }
  } else {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      s[r] = (s[r] == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f(__builtin_fmaf(s[r], c2, nm));
      ps += s[r];
    }
  }
  float plo_, phi_;
  half_pair(ps, plo_, phi_);
  ps = plo_ + phi_;                        // (own + partner, as before: the sum is commutative, bit-identical)
  l_run += ps;
#pragma unroll
  for (int e = 0; e < 8; ++e) { pf[0][e] = (e16)s[e]; pf[1][e] = (e16)s[8 + e]; }
}

// The 4-wave forward, one template for two argument blocks: FlashArgs (one (Lq, Lk) for the launch) and FlashVarlenArgs
// (VARLEN below; always causal: the lengths of sample b are read on the device, clamped to the launch's bounds a.Lq /
// a.Lk, and take their place in the tile count, the causal shift, the interior-tile test, the key-validity bytes, the
// K / V descriptor ranges and the stores -- mk_flash_attn_varlen_fwd in macaw_hip.h states the rule).  Every
// `if constexpr (VARLEN)` is outside the tile loop; with FlashArgs Lq / Lk ARE a.Lq / a.Lk and the kernel compiles to
// the code it was before the second form existed.
struct FlashVarlenArgs : FlashArgs {
  const int32_t* q_len; const int32_t* k_len;   // int32 [B] on the device
};
template <int HD, bool CAUSAL, typename Args = FlashArgs>
__global__ __launch_bounds__(256, 2) void flash_fwd_kernel(Args a) {
  constexpr bool VARLEN = std::is_same<Args, FlashVarlenArgs>::value;
  static_assert(CAUSAL || !VARLEN, "the variable-length forward is causal");
  constexpr int KT = 64;                 // keys per LDS tile
  constexpr int NKD = HD / 16;           // MFMA k-steps over d for Q K^T
  constexpr int NDB = HD / 32;           // 32-wide d blocks of the output
  constexpr int CPR = HD / 8;            // 16-B chunks per row
  // Round 5: TWO tile buffers (K, V, key validity): the staged registers of tile kt + 1 are written into the other
  // buffer BEHIND the MFMAs of tile kt and one barrier per tile publishes them (rounds 1-4: one buffer, write phase
  // between two barriers at the top of every tile -- PMC: 27 % of the wave cycles parked in s_waitcnt / s_barrier).
  // 2 x 32.1 KiB at head_dim 128: two workgroups per CU still fit (128.5 of 160 KiB).
  constexpr int BUFSZ = 2 * KT * HD * 2 + 128;
  __shared__ __attribute__((aligned(16))) char lds[2 * BUFSZ];
  // grid = (H, B, blocks): the sequence-block index is the SLOWEST dimension, so blocks of equal
  // cost are dispatched together (heaviest first) instead of one heavy + one light block per
  // (b, h) alternating -- at S = 144 the second block has 16 rows and a quarter of the work, and
  // pairing them made every dispatch round as long as a heavy block (LPT order: -35 %).
  int b = blockIdx.y, h = blockIdx.x;
  int blk = CAUSAL ? (int)(gridDim.z - 1 - blockIdx.z) : (int)blockIdx.z;
  if (!CAUSAL && a.nblk > 0) {
    // Non-causal (Whisper: 12 query blocks per head, all of equal cost): a 1-D grid in which the query blocks of
    // one (b, h) are CONSECUTIVE workgroups OF ONE XCD (workgroup id % 8 = XCD), so its K / V (384 KB at S =
    // 1500) is fetched into that XCD's L2 once and re-read there.  With blocks as the slowest grid dimension
    // (the causal LPT order) the 12 readers of a head ran ~256 workgroups apart on 8 different L2s: 7.6 GB of
    // fabric reads for 2.1 GB of q / k / v per Whisper pass (r03f_step_traffic_pmc.csv).  Measured (profiles/
    // r04_attn_ab.txt): Whisper forward 291 -> 267 us; CLIP (3 blocks) +-0; the same grouping of the CAUSAL grid
    // (heaviest block of a head first) LOSES 22 % at S = 2048 -- there the global heaviest-first order matters more.
    const int id = blockIdx.x, xcd = id & 7, slot = id >> 3;
    const int bh = (slot / a.nblk) * 8 + xcd;
    blk = slot % a.nblk;
    if (bh >= a.B * a.H) return;         // (grid rounded up to 8 x nblk; whole workgroup, before any barrier)
    b = bh / a.H; h = bh - b * a.H;
  }
  int Lq = a.Lq, Lk = a.Lk;              // the rows and keys of THIS sample (VARLEN: a.Lq / a.Lk bound them and size the grid)
  if constexpr (VARLEN) {
    Lq = min(max(__builtin_amdgcn_readfirstlane(a.q_len[b]), 0), a.Lq);
    Lk = min(max(__builtin_amdgcn_readfirstlane(a.k_len[b]), 0), a.Lk);
    if (blk * 128 >= Lq) {
      // the whole block lies at or past the sample's last query row: its rows of o are zeros, its lse -inf, and the
      // workgroup leaves as a whole before its first barrier (no q, k or v byte is read)
      e16* O = a.o + (long)b * a.o_bs + (long)h * HD;
      const int rows = min(128, a.Lq - blk * 128);
      for (int i = threadIdx.x; i < rows * (HD / 8); i += 256)
        *reinterpret_cast<uint4*>(O + (long)(blk * 128 + i / (HD / 8)) * a.o_ld + (i % (HD / 8)) * 8) = make_uint4(0, 0, 0, 0);
      if (a.lse && (int)threadIdx.x < rows) a.lse[((long)b * a.H + h) * a.Lq + blk * 128 + threadIdx.x] = -INFINITY;
      return;
    }
  }
  const int l = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int half = l >> 5, lq = l & 31;
  const int q0 = blk * 128 + w * 32;
  const int qg = q0 + lq;                // this lane's query row
  const e16* Q = a.q + (long)b * a.q_bs + (long)h * HD;
  const e16* K = a.k + (long)b * a.k_bs + (long)h * HD;
  const e16* V = a.v + (long)b * a.v_bs + (long)h * HD;
  const int32_t* km = a.kmask ? a.kmask + (long)b * a.Lk : nullptr;

  // Q fragments (B operand of K Q^T): lane holds Q[qg][16*kd + 8*half .. +8]
  e16x8 qf[NKD];
#pragma unroll
  for (int kd = 0; kd < NKD; ++kd) {
    qf[kd] = ld8_or_zero(Q + (long)min(qg, Lq - 1) * a.q_ld + 16 * kd + 8 * half, qg < Lq);
  }
  f32x16 oacc[NDB];
#pragma unroll
  for (int d = 0; d < NDB; ++d)
#pragma unroll
    for (int e = 0; e < 16; ++e) oacc[d][e] = 0.f;
  // Online softmax state in the exp2 domain: m_run = running max of t = s * scale * log2(e), l_run =
  // sum of 2^(t - m_run).  (v_exp_f32 IS exp2: folding scale and log2(e) into one FMA with the max
  // removes a multiply per score; the natural-log lse is recovered at the end.)
  float m_run = -INFINITY, l_run = 0.f;
  const float c2 = a.scale * 1.4426950408889634f;
  // Lazy rescaling (cdna_hip_programming.md T13): a row's accumulators are rescaled only when its
  // maximum grew by more than 2^DEFER since its last rescale; otherwise the old maximum is kept and
  // p = 2^(t - m_old) <= 2^DEFER.  Every quantity still at the old maximum (O, l) is rescaled in the
  // same place, before this sub-block's P exists, and all earlier P V products are complete (the
  // code is sequential per wave): the "textbook order", no pending-tile hazard.  DEFER = 0 rescales
  // on every growth (the round-2 behaviour).

  // keys this block has to visit (causal: up to the last query row of the block)
  const int shift = Lk - Lq;             // query i may see keys <= i + shift
  int k_end = Lk;
  if (CAUSAL) k_end = min(Lk, blk * 128 + 128 + shift);
  const int ntiles = (k_end + KT - 1) / KT;

  // K / V staging is split (cdna_hip_programming.md T14, "async-STAGE"): the global loads of tile kt + 1 are
  // ISSUED behind the barrier that publishes tile kt and stay in flight under the whole QK^T / softmax / PV of
  // tile kt; they are waited for and written to LDS at the top of the next iteration.  (Rounds 1-3 loaded,
  // waited and wrote inside one barrier pair: every tile paid an exposed HBM round trip that only the second
  // workgroup of the CU could hide.)  The zero fill of rows beyond Lk is applied at the WRITE: a select right
  // behind the load would make the compiler wait for it there.
  // Round 5: the tile loads are raw buffer loads (one descriptor per operand over the rows [0, Lk) of this (b, h):
  // rows beyond Lk read as ZEROS through the hardware range check -- no clamp, no select), the per-lane part of the
  // address is ONE constant voffset, tile and chunk advance through the scalar offset, and the LDS destinations are
  // one constant per lane + immediates: the staging of a tile costs no VALU instruction besides its 8 loads and 8
  // LDS writes (before: ~100 of the ~340 VALU instructions a wave issued per tile; PMC: 10.7 VALU per MFMA).
  constexpr int NCH = (KT * CPR) / 256;
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  u32x4 kv4[NCH], vv4[NCH];
  // (VARLEN: the range ends behind row Lk - 1 of THIS sample -- no byte of a later row is read; Lk = 0: an empty range)
  auto range = [&](long ld) {
    long n = ((long)(Lk - 1) * ld + HD) * 2;
    if constexpr (VARLEN) n = max(n, 0L);
    return (int)min(n, 0x7fffffffL);
  };
  const __amdgpu_buffer_rsrc_t rsK = __builtin_amdgcn_make_buffer_rsrc((void*)K, 0, range(a.k_ld), 0x00020000);
  const __amdgpu_buffer_rsrc_t rsV = __builtin_amdgcn_make_buffer_rsrc((void*)V, 0, range(a.v_ld), 0x00020000);
  const int srow = threadIdx.x / CPR, sch = threadIdx.x % CPR;        // chunk i of this thread: row srow + i * 256 / CPR
  const int kvo = (int)(((long)srow * a.k_ld + sch * 8) * 2), vvo = (int)(((long)srow * a.v_ld + sch * 8) * 2);
  const int k_step = (int)((256 / CPR) * a.k_ld * 2), v_step = (int)((256 / CPR) * a.v_ld * 2);   // bytes per chunk index
  // (the swizzles of k_off / v_off depend on row bits below 256 / CPR = 16 / 32 only: chunk i lands 4096 B further)
  char* const ldsKw = lds + k_off<HD>(srow, sch);                      // (buffer 0; buffer 1 is BUFSZ further)
  char* const ldsVw = lds + KT * HD * 2 + v_off<HD>(srow, sch);
  static_assert((256 / CPR) * CPR * 16 == 4096, "a chunk index is 4 KiB of the LDS image");
  auto issue_tile = [&](int kb) {
    const int ks = (int)((long)kb * a.k_ld * 2), vs = (int)((long)kb * a.v_ld * 2);
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      kv4[i] = __builtin_amdgcn_raw_buffer_load_b128(rsK, kvo, ks + i * k_step, 0);
      vv4[i] = __builtin_amdgcn_raw_buffer_load_b128(rsV, vvo, vs + i * v_step, 0);
    }
  };
  // the staged registers -> tile buffer `buf` (rows beyond Lk arrived as zeros), its key-validity bytes
  auto write_tile = [&](int bufoff, int kb) {
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      *reinterpret_cast<u32x4*>(ldsKw + bufoff + i * 4096) = kv4[i];
      *reinterpret_cast<u32x4*>(ldsVw + bufoff + i * 4096) = vv4[i];
    }
    if (threadIdx.x < KT) {
      const int kg = kb + threadIdx.x;
      lds[bufoff + 2 * KT * HD * 2 + threadIdx.x] = ((kg < Lk) && (!km || km[kg] != 0)) ? 1 : 0;
    }
  };
  if (ntiles > 0) { issue_tile(0); write_tile(0, 0); }
  __syncthreads();
  // one tile out of buffer BI (a compile-time constant: every LDS address of the body is a per-lane constant + an
  // immediate); the loop below alternates the two instantiations
  auto tile_body = [&](auto BI, int kt) {
    constexpr int bufoff = decltype(BI)::value * BUFSZ;
    const char* ldsK = lds + bufoff;
    const char* ldsV = lds + bufoff + KT * HD * 2;
    const uint8_t* ldsM = reinterpret_cast<const uint8_t*>(lds + bufoff + 2 * KT * HD * 2);   // one byte per key
    const int kbase = kt * KT;
    const bool more = kt + 1 < ntiles;
    if (more) issue_tile(kbase + KT);      // in flight under this tile's MFMAs
    // causal: a 32-key sub-block entirely above this wave's 32 rows contributes exact zeros (p = 0, running
    // maximum and sums untouched): skipped, bit-identically (wave-uniform; at S = 144 the first two waves of a
    // block need one of its two key tiles)
    const bool need0 = !(CAUSAL && kbase > q0 + 31 + shift);
    const bool need1 = !(CAUSAL && kbase + 32 > q0 + 31 + shift);
    if (q0 < Lq && need0) {            // (a wave without rows still stages and takes part in the barriers)
    // Interior tile: every key of the tile is valid and visible to every query row of this wave --
    // no mask arithmetic at all (at S = 2048 all but the last two tiles of a block).  Wave-uniform.
    bool interior = (__builtin_amdgcn_ballot_w64(ldsM[l] != 0) == ~0ull);
    if (CAUSAL) interior = interior && (kbase + KT - 1 <= q0 + shift);

    // Round 5: the LDS operands are requested AHEAD of the MFMA chains that consume them.  Rounds 1-4 read a K
    // fragment (or the four transposed V parts of a d block) right in front of its MFMA: the ISA was
    // `ds_read x2; s_waitcnt lgkmcnt(1); mfma; s_waitcnt lgkmcnt(0); mfma` sixteen times per sub-block, i.e. every
    // pair of MFMAs paid an exposed LDS round trip (~100+ cycles beside 64 cycles of matrix work), and only the
    // co-resident workgroup's waves could fill the holes.  Now: the 8 K fragments of sub-block 0 up front, those
    // of sub-block 1 behind the MFMAs of chain 0, the 8 V fragments of a sub-block BEFORE its softmax (they land
    // under it).  The arithmetic of a row is unchanged
    // instruction for instruction (sub-block 0's softmax / rescale / P V, then sub-block 1's): bit-identical.
    auto load_k = [&](int sb, e16x8 (&kf)[NKD]) {
#pragma unroll
      for (int kd = 0; kd < NKD; ++kd)
        kf[kd] = *reinterpret_cast<const e16x8*>(ldsK + k_off<HD>(sb * 32 + lq, 2 * kd + half));
    };
    const int li = l & 15;
    constexpr int NDH = NDB / 2;           // the V fragments travel in two halves of the d blocks (register budget)
    auto load_v = [&](int sb, int dh, e16x8 (&vf)[NDH][2]) {
#pragma unroll
      for (int dd = 0; dd < NDH; ++dd) {
        const int d = dh * NDH + dd;
        const int col = d * 32 + 16 * ((l >> 4) & 1) + 4 * (li & 3);   // d index of this lane group
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
          for (int r = 0; r < 2; ++r) {
            const int key = sb * 32 + ks * 16 + 8 * r + 4 * half + (li >> 2);
            const int off = v_off<HD>(key, col >> 3) + ((col & 7) << 1);
            const e16x4 t = E16<e16>::tr_read(ldsV + off);
            vf[dd][ks][4 * r] = t[0]; vf[dd][ks][4 * r + 1] = t[1]; vf[dd][ks][4 * r + 2] = t[2]; vf[dd][ks][4 * r + 3] = t[3];
          }
      }
    };
    // mask + online softmax of one sub-block (this lane: query qg, keys key(r)); s -> p in place, pf = p in 16 bits
    auto softmax = [&](int sb, f32x16& s, e16x8 (&pf)[2]) {
      uint32_t okbits = 0xffffu;
      if (!interior) {
        okbits = 0;
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {     // four keys per word (this lane's 4-key groups are 8 keys apart)
          const uint32_t m4 = *reinterpret_cast<const uint32_t*>(ldsM + sb * 32 + 8 * g4 + 4 * half);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int kg = kbase + sb * 32 + e + 8 * g4 + 4 * half;
            bool ok = ((m4 >> (8 * e)) & 0xffu) != 0;
            if (CAUSAL) ok = ok && (kg <= qg + shift);
            okbits |= (ok ? 1u : 0u) << (4 * g4 + e);
          }
        }
      }
      softmax_block<NDB>(s, interior, okbits, c2, m_run, l_run, oacc, pf);
    };
    auto pv = [&](int dh, const e16x8 (&vf)[NDH][2], const e16x8 (&pf)[2]) {   // O^T += V^T P^T
#pragma unroll
      for (int dd = 0; dd < NDH; ++dd)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) oacc[dh * NDH + dd] = E16<e16>::mma32(vf[dd][ks], pf[ks], oacc[dh * NDH + dd]);
    };
    // one sub-block behind its scores: the first half of its V fragments is requested before the softmax and lands
    // under it, the second half behind the softmax and lands under the first half's MFMAs
    auto finish = [&](int sb, f32x16& s) {
      e16x8 pf[2];
      e16x8 va[NDH][2], vb[NDH][2];
      load_v(sb, 0, va);
      softmax(sb, s, pf);
      load_v(sb, 1, vb);
      pv(0, va, pf);
      pv(1, vb, pf);
    };
    f32x16 s0, s1;
#pragma unroll
    for (int e = 0; e < 16; ++e) { s0[e] = 0.f; s1[e] = 0.f; }
    if (need1) {
      {
        // (one fragment set: the fragment of sub-block 1 is requested into the registers its sub-block-0 twin has
        //  just left, right behind the MFMA that read them -- 32 registers instead of 64, and every load of the
        //  second chain has the rest of the first chain to land)
        e16x8 kf[NKD];
        load_k(0, kf);
#pragma unroll
        for (int kd = 0; kd < NKD; ++kd) {        // S^T = K Q^T, 32 keys x 32 queries
          s0 = E16<e16>::mma32(kf[kd], qf[kd], s0);
          kf[kd] = *reinterpret_cast<const e16x8*>(ldsK + k_off<HD>(32 + lq, 2 * kd + half));
        }
#pragma unroll
        for (int kd = 0; kd < NKD; ++kd) s1 = E16<e16>::mma32(kf[kd], qf[kd], s1);
      }
      finish(0, s0);
      finish(1, s1);
    } else {
      {
        e16x8 kf0[NKD];
        load_k(0, kf0);
#pragma unroll
        for (int kd = 0; kd < NKD; ++kd) s0 = E16<e16>::mma32(kf0[kd], qf[kd], s0);
      }
      finish(0, s0);
    }
    }
    if (more) write_tile((1 - decltype(BI)::value) * BUFSZ, kbase + KT);   // (all waves left that buffer one barrier ago)
    __syncthreads();
  };
  for (int kt = 0; kt < ntiles; kt += 2) {
    tile_body(std::integral_constant<int, 0>{}, kt);
    if (kt + 1 < ntiles) tile_body(std::integral_constant<int, 1>{}, kt + 1);
  }
  if (q0 >= a.Lq) return;                // (wave-uniform: the stores below need both half-waves)
  // (the lane's row index is re-derived from a laundered thread index: formed at the kernel entry and carried through
  //  the tile loop, the epilogue's addresses cost three spilled registers at the 256-register budget)
  int tid_e = threadIdx.x;
  asm volatile("" : "+v"(tid_e));
  const int half_e = (tid_e >> 5) & 1, qg_e = blk * 128 + (tid_e >> 6) * 32 + (tid_e & 31);
  if constexpr (VARLEN) {
    // rows [Lq, a.Lq) of a live block are stored too, as exact zeros and -inf: a wave past Lq computed nothing, a row
    // past Lq inside a live wave ran on a zero q -- its sums are dropped here, not scaled (0 x inf would be NaN)
    if (qg_e >= Lq) {
      l_run = 0.f;
#pragma unroll
      for (int d = 0; d < NDB; ++d)
#pragma unroll
        for (int e = 0; e < 16; ++e) oacc[d][e] = 0.f;
    }
  }
  const float inv = l_run > 0.f ? 1.f / l_run : 0.f;
  e16* O = a.o + (long)b * a.o_bs + (long)min(qg_e, a.Lq - 1) * a.o_ld + (long)h * HD;
  store_row16<NDB>(O, oacc, inv, half_e, qg_e < a.Lq);
  if (qg_e >= a.Lq) return;
  if (a.lse && half_e == 0)   // natural-log lse = (m2 + log2(l)) * ln(2)
    a.lse[((long)b * a.H + h) * a.Lq + qg_e] =
        (l_run > 0.f) ? (m_run + __log2f(l_run)) * 0.6931471805599453f : -INFINITY;
}


// ---- long sequences: the 8-wave forward (round 5) ----------------------------------------------------------------
// One workgroup = 8 waves = 256 query rows (32 per wave, lane <-> query as above), one workgroup per CU, two waves per
// SIMD; K / V tiles of 64 keys in 2-deep LDS rings, staged through registers by all 512 threads (2 + 2 16-byte chunks per
// thread and tile: half the staging instructions and half the L2 reads per query row of the 4-wave kernel); the softmax
// of a tile takes ONE maximum over its 64 keys, so that P(t) is complete before any of it is consumed and P V can move
// one tile behind the scores; the mask enters the scores as the INITIAL VALUE of the Q K^T accumulators (0 / -inf).
//
// SHIPPED structure (MK_F8_MIXED = 1): one segment per tile and wave, all eight waves in phase, ONE barrier per tile:
//     Q K^T of tile t (16 MFMAs, K fragments requested a quarter of the d range ahead), then
//     P V of tile t - 1 (16 MFMAs) with the softmax of tile t -- part A: maximum, exponentials, row sum; touches neither
//     O nor l -- placed BETWEEN those MFMAs by sched_group_barrier (1 MFMA : 7 VALU), then behind them the (rare) rescale
//     of O, the l update and the conversion of P(t) (P(t - 1) has been consumed), then the staging writes of K(t + 1) /
//     V(t) (their slots were last read one barrier ago) and the loads of K(t + 2) / V(t + 1).
// Why: profiles/r05_attn8.txt D.  The first structure (MK_F8_MIXED = 0, kept below as an experiment build) split a tile
// into a matrix segment M_t (scores of t + P V of t - 1) and a softmax segment S_t and ran waves 4-7 one segment behind
// waves 0-3, so that on every SIMD one wave was in M while its partner (w + 4: verified) was in S -- the guide's 8-wave
// ping-pong.  Timing-only builds showed the two segments do NOT overlap (no softmax: 167 us, no MFMAs: 188 us, both:
// 331 us): VALU issued by the PARTNER wave costs the computing wave its MFMA cover (MI355X_MICROARCH "Two waves per
// SIMD" 1-3); what hides a wave's softmax is its OWN MFMAs.  The mixed form is +3 % (325 vs 334 us non-causal S = 2048).
//
// Ring protocol of the experiment build, with sigma = the global segment count (waves 0-3 run M_t at sigma = 2 t,
// waves 4-7 at 2 t + 1): K(t) is read during sigma in {2 t, 2 t + 1}, V(t) (by M_(t+1)) during {2 t + 2, 2 t + 3};
// every wave WRITES K(t + 1) and V(t) inside its own M_t, i.e. at sigma in {2 t, 2 t + 1}: K(t + 1)'s slot held K(t - 1),
// last read at sigma = 2 t - 1; V(t)'s slot held V(t - 2), last read at 2 t - 1; both are first read at sigma = 2 t + 2,
// behind the barrier that ends sigma = 2 t + 1.  In BOTH forms the global loads of K(t + 2) / V(t + 1) are issued at the
// end of the matrix work of tile t and waited for by the LDS writes one tile later; the barriers are raw `s_barrier`s
// behind `s_waitcnt lgkmcnt(0)` -- never a vmcnt wait.  Key validity (padding mask, keys beyond Lk) travels as one byte
// per key in a 4-deep ring written by wave 0 with K (the first two-group version read it in the softmax segment, where
// a 2-deep ring is overwritten under the late group's reads; read in the matrix segment two slots would do).  Both
// forms of the ring / barrier protocol are simulated for every tile count in tests/test_fwd8_protocol_cpu.py.
// s0 / s1: the raw scores of a 64-key tile with the MASK ALREADY IN THEM (-inf where a key is padded or invisible: the
// matrix segment starts the Q K^T accumulators from a 0 / -inf bias instead of zeros, see flash_fwd8_kernel) -> p
template <int NDB>
MK_DEV void softmax_tile64(f32x16& s0, f32x16& s1, float c2, float& m_run, float& l_run, f32x16 (&oacc)[NDB],
                           e16x8 (&pf)[4]) {
  constexpr float DEFER = 6.0f;          // (softmax_block)
  float mx = fmaxf(fmaxf(s0[0], s0[1]), s0[2]);
#pragma unroll
  for (int r = 3; r < 15; r += 2) mx = fmaxf(fmaxf(mx, s0[r]), s0[r + 1]);
#pragma unroll
  for (int r = 0; r < 16; r += 2) mx = fmaxf(fmaxf(mx, s1[r]), s1[r + 1]);
  mx = fmaxf(mx, s0[15]);
  float mlo, mhi;
  half_pair(mx, mlo, mhi);
  mx = fmaxf(mlo, mhi) * c2;
  const bool grow = !(mx - m_run <= DEFER);
  if (__any(grow ? 1 : 0)) {
    const float m_new = grow ? fmaxf(m_run, mx) : m_run;
    const float alpha = !grow ? 1.f : ((m_run == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f(m_run - m_new));
    l_run *= alpha;
    m_run = m_new;
#pragma unroll
    for (int d = 0; d < NDB; ++d)
#pragma unroll
      for (int e = 0; e < 16; ++e) oacc[d][e] *= alpha;
  }
  // ONE exponential path, masked or not: a masked score is -inf and 2^(-inf c2 + nm) = 0 as long as nm is finite.
  // nm = +inf only for a row that has not seen a visible key yet (m_run = -inf; all its scores of this tile are -inf
  // too, or the rescale above would have made m_run finite): 0 stands in for it there -- one select per ROW instead of a
  // compare + select per score and two copies of the loop.
  const float nm = (m_run == -INFINITY) ? 0.f : -m_run;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    s0[r] = __builtin_amdgcn_exp2f(__builtin_fmaf(s0[r], c2, nm));
    s1[r] = __builtin_amdgcn_exp2f(__builtin_fmaf(s1[r], c2, nm));
  }
  // row sum over NEIGHBOURING registers (v_pk_add_f32 on the pairs as they lie; summing s0[r] beside s1[r] made the
  // compiler pack each pair with two v_mov first)
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  f32x2 acc2 = {0.f, 0.f};
#pragma unroll
  for (int r = 0; r < 16; r += 2) {
    acc2 += f32x2{s0[r], s0[r + 1]};
    acc2 += f32x2{s1[r], s1[r + 1]};
  }
  float plo, phi;
  half_pair(acc2[0] + acc2[1], plo, phi);
  l_run += plo + phi;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    pf[0][e] = (e16)s0[e]; pf[1][e] = (e16)s0[8 + e];
    pf[2][e] = (e16)s1[e]; pf[3][e] = (e16)s1[8 + e];
  }
}

// The same arithmetic split for the MIXED segment of flash_fwd8_kernel (MK_F8_MIXED): part A is branch-free and touches
// neither O nor l -- it runs in the shadow of the P V MFMAs of the previous tile, which still accumulate into O; the
// caller applies `alpha` to O / l behind them.  Rows that keep their maximum get alpha = 1 exactly.
MK_DEV void softmax_part_a(f32x16& s0, f32x16& s1, float c2, float& m_run, float& alpha, float& psum) {
  constexpr float DEFER = 6.0f;
  float mx = fmaxf(fmaxf(s0[0], s0[1]), s0[2]);
#pragma unroll
  for (int r = 3; r < 15; r += 2) mx = fmaxf(fmaxf(mx, s0[r]), s0[r + 1]);
#pragma unroll
  for (int r = 0; r < 16; r += 2) mx = fmaxf(fmaxf(mx, s1[r]), s1[r + 1]);
  mx = fmaxf(mx, s0[15]);
  float mlo, mhi;
  half_pair(mx, mlo, mhi);
  mx = fmaxf(mlo, mhi) * c2;
  const bool grow = !(mx - m_run <= DEFER);
  const float m_new = grow ? fmaxf(m_run, mx) : m_run;
  const float a_grow = (m_run == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f(m_run - m_new);
  alpha = grow ? a_grow : 1.f;
  m_run = m_new;
  const float nm = (m_run == -INFINITY) ? 0.f : -m_run;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    s0[r] = __builtin_amdgcn_exp2f(__builtin_fmaf(s0[r], c2, nm));
    s1[r] = __builtin_amdgcn_exp2f(__builtin_fmaf(s1[r], c2, nm));
  }
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  f32x2 acc2 = {0.f, 0.f};
#pragma unroll
  for (int r = 0; r < 16; r += 2) {
    acc2 += f32x2{s0[r], s0[r + 1]};
    acc2 += f32x2{s1[r], s1[r + 1]};
  }
  float plo, phi;
  half_pair(acc2[0] + acc2[1], plo, phi);
  psum = plo + phi;
}

// MK_F8_ABLATE = n: TIMING-ONLY experiment builds of flash_fwd8_kernel (wrong results; scripts/probe/build_f8_variants.sh):
// 1 no softmax segment, 2 no MFMAs, 3 no LDS fragment reads, 4 no K / V staging, 5 no barriers.  The shipped build has none.
#ifndef MK_F8_ABLATE
#define MK_F8_ABLATE 0
#endif
#ifndef MK_F8_MIXED     // 1: ONE segment per tile and wave -- Q K^T of tile t, then P V of tile t - 1 with the softmax of tile t
#define MK_F8_MIXED 1   // interleaved between its MFMAs (same wave); all eight waves in phase, one barrier per tile
#endif
#ifndef MK_F8_PRIO      // 0: no s_setprio; 1: priority 1 during matrix segments (shipped: 226 vs 227-229 us at S = 2048,
#define MK_F8_PRIO 1    // profiles/r05_attn8.txt D); 2: static priority 1 for waves 4-7
#endif
#if MK_F8_ABLATE == 5
#define MK_F8_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")
#else
#define MK_F8_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")
#endif
#if MK_F8_ABLATE == 2
#define MK_F8_MMA(A, B, C) ([&] { auto a_ = (A); auto b_ = (B); asm volatile("" :: "v"(a_), "v"(b_)); return (C); }())
#else
#define MK_F8_MMA(A, B, C) E16<e16>::mma32((A), (B), (C))
#endif

template <int HD, bool CAUSAL>
__global__ __launch_bounds__(512, 1) void flash_fwd8_kernel(FlashArgs a) {
  constexpr int KT = 64;                 // keys per LDS tile
  constexpr int NKD = HD / 16;           // MFMA k-steps over d for Q K^T
  constexpr int NDB = HD / 32;           // 32-wide d blocks of the output
  constexpr int CPR = HD / 8;            // 16-B chunks per row
  constexpr int KBYTES = KT * HD * 2;    // one K (or V) tile
  constexpr int SLOT = 2 * KBYTES;       // ring slot: K | V
  constexpr int MASK0 = 2 * SLOT;        // 4 x 64 key-validity bytes
  __shared__ __attribute__((aligned(16))) char lds[2 * SLOT + 4 * KT];
  int b = blockIdx.y, h = blockIdx.x;
  int blk = CAUSAL ? (int)(gridDim.z - 1 - blockIdx.z) : (int)blockIdx.z;   // (causal: heaviest blocks first)
  if (!CAUSAL && a.nblk > 0) {           // query blocks of one (b, h) on ONE XCD (see flash_fwd_kernel)
    const int id = blockIdx.x, xcd = id & 7, slot = id >> 3;
    const int bh = (slot / a.nblk) * 8 + xcd;
    blk = slot % a.nblk;
    if (bh >= a.B * a.H) return;
    b = bh / a.H; h = bh - b * a.H;
  }
  const int l = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
#ifndef MK_F8_LATE       // which waves form the group that runs one segment behind: 0: w >= 4, 1: odd w, 2: (w >> 1) & 1
#define MK_F8_LATE 0
#endif
#if MK_F8_LATE == 1
  const bool late = (w & 1) != 0;
#elif MK_F8_LATE == 2
  const bool late = ((w >> 1) & 1) != 0;
#else
  const bool late = w >= 4;              // (wave-uniform, scalar: the barrier counts below depend on it)
#endif
  const int half = l >> 5, lq = l & 31;
  const int q0 = blk * 256 + w * 32;
  const int qg = q0 + lq;
  const bool active = q0 < a.Lq;         // (a wave without rows still stages and takes part in the barriers)
  const e16* Q = a.q + (long)b * a.q_bs + (long)h * HD;
  const e16* K = a.k + (long)b * a.k_bs + (long)h * HD;
  const e16* V = a.v + (long)b * a.v_bs + (long)h * HD;

  e16x8 qf[NKD];
#pragma unroll
  for (int kd = 0; kd < NKD; ++kd)
    qf[kd] = ld8_or_zero(Q + (long)min(qg, a.Lq - 1) * a.q_ld + 16 * kd + 8 * half, qg < a.Lq);
  f32x16 oacc[NDB];
#pragma unroll
  for (int d = 0; d < NDB; ++d)
#pragma unroll
    for (int e = 0; e < 16; ++e) oacc[d][e] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;
  const float c2 = a.scale * 1.4426950408889634f;
  const int shift = a.Lk - a.Lq;         // query i may see keys <= i + shift
  int k_end = a.Lk;
  if (CAUSAL) k_end = min(a.Lk, blk * 256 + 256 + shift);
  const int ntiles = k_end > 0 ? (k_end + KT - 1) / KT : 0;

  // ---- staging: raw buffer loads (rows beyond Lk read as zeros), one constant voffset per lane, constant LDS addresses
  constexpr int NCH = (KT * CPR) / 512;
  constexpr int RSTEP = 512 / CPR;       // rows between a thread's consecutive chunks: 8 KiB of the LDS image
  static_assert(NCH >= 1 && RSTEP * CPR * 16 == 8192, "a chunk index is 8 KiB of the LDS image");
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  u32x4 kreg[NCH], vreg[NCH];
  int mreg = 1;
  const __amdgpu_buffer_rsrc_t rsK = __builtin_amdgcn_make_buffer_rsrc(
      (void*)K, 0, (int)min(((long)(a.Lk - 1) * a.k_ld + HD) * 2, 0x7fffffffL), 0x00020000);
  const __amdgpu_buffer_rsrc_t rsV = __builtin_amdgcn_make_buffer_rsrc(
      (void*)V, 0, (int)min(((long)(a.Lk - 1) * a.v_ld + HD) * 2, 0x7fffffffL), 0x00020000);
  const bool has_km = a.kmask != nullptr;
  const __amdgpu_buffer_rsrc_t rsM = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(has_km ? a.kmask + (long)b * a.Lk : (const int32_t*)K), 0, has_km ? a.Lk * 4 : 0, 0x00020000);
  const int srow = threadIdx.x / CPR, sch = threadIdx.x % CPR;
  const int kvo = (int)(((long)srow * a.k_ld + sch * 8) * 2), vvo = (int)(((long)srow * a.v_ld + sch * 8) * 2);
  const int k_step = (int)(RSTEP * a.k_ld * 2), v_step = (int)(RSTEP * a.v_ld * 2);
  char* const ldsKw = lds + k_off<HD>(srow, sch);
  char* const ldsVw = lds + KBYTES + v_off<HD>(srow, sch);
  auto issue_k = [&](int kb) {           // K tile at key kb -> kreg, its validity words -> mreg (wave 0)
    const int ks = (int)((long)kb * a.k_ld * 2);
#pragma unroll
    for (int i = 0; i < NCH; ++i) kreg[i] = __builtin_amdgcn_raw_buffer_load_b128(rsK, kvo, ks + i * k_step, 0);
    // (only ever WRITTEN by the load: a second, computed definition makes the compiler wait for the loads just issued)
    if (w == 0 && has_km) mreg = (int)__builtin_amdgcn_raw_buffer_load_b32(rsM, l * 4, kb * 4, 0);   // (beyond Lk: 0)
  };
  auto issue_v = [&](int kb) {
    const int vs = (int)((long)kb * a.v_ld * 2);
#pragma unroll
    for (int i = 0; i < NCH; ++i) vreg[i] = __builtin_amdgcn_raw_buffer_load_b128(rsV, vvo, vs + i * v_step, 0);
  };
  auto write_k = [&](int slotoff, int t) {   // kreg -> K of ring slot, validity of tile t -> its byte ring
#pragma unroll
    for (int i = 0; i < NCH; ++i) *reinterpret_cast<u32x4*>(ldsKw + slotoff + i * 8192) = kreg[i];
    if (w == 0) lds[MASK0 + (t & 3) * KT + l] = (has_km ? mreg != 0 : t * KT + l < a.Lk) ? 1 : 0;
  };
  auto write_v = [&](int slotoff) {
#pragma unroll
    for (int i = 0; i < NCH; ++i) *reinterpret_cast<u32x4*>(ldsVw + slotoff + i * 8192) = vreg[i];
  };

  // ---- the two products of a matrix segment.  LDS read addresses: ONE lane constant per operand; a fragment's address
  // is that constant XOR a compile-time value (the XOR swizzles of k_off / v_off act on the bits the fragment index
  // occupies) + an immediate.  The constants are laundered at the top of every segment: derived once at the kernel
  // entry the compiler keeps all 8 + 4 addresses live across the loop and spills (the budget is 256 registers).
  const int li = l & 15;
  constexpr int NDH = NDB / 2;
  const int col0 = 16 * ((l >> 4) & 1) + 4 * (li & 3);
  const int kb_lane = k_off<HD>(lq, half);                                     // K fragment kd = 0 of sub-block 0
  const int vb_lane = v_off<HD>(4 * half + (li >> 2), col0 >> 3) + ((col0 & 7) << 1);   // V part (d 0, key group 0)
  auto k_frag = [&](const char* ldsK, int kb, int sb, int kd) {
#if MK_F8_ABLATE == 3
    return qf[kd];
#else
    return *reinterpret_cast<const e16x8*>(ldsK + (kb ^ (kd << 5)) + sb * 32 * HD * 2);
#endif
  };
  auto load_v = [&](const char* ldsV, int vb, int sb, int dh, e16x8 (&vf)[NDH][2]) {
#pragma unroll
    for (int dd = 0; dd < NDH; ++dd) {
      const int d = dh * NDH + dd;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int r = 0; r < 2; ++r) {
#if MK_F8_ABLATE == 3
          const e16x4 t = {qf[0][0], qf[0][1], qf[0][2], qf[0][3]};
#else
          const e16x4 t = E16<e16>::tr_read(ldsV + (vb ^ (d << 6)) + (sb * 32 + ks * 16 + 8 * r) * HD * 2);
#endif
          vf[dd][ks][4 * r] = t[0]; vf[dd][ks][4 * r + 1] = t[1]; vf[dd][ks][4 * r + 2] = t[2]; vf[dd][ks][4 * r + 3] = t[3];
        }
    }
  };
  auto pv = [&](int dh, const e16x8 (&vf)[NDH][2], const e16x8& p0, const e16x8& p1) {   // O^T += V^T P^T
#pragma unroll
    for (int dd = 0; dd < NDH; ++dd) {
      oacc[dh * NDH + dd] = MK_F8_MMA(vf[dd][0], p0, oacc[dh * NDH + dd]);
      oacc[dh * NDH + dd] = MK_F8_MMA(vf[dd][1], p1, oacc[dh * NDH + dd]);
    }
  };
  // causal: can this wave's 32 rows see any key of tile t (wave-uniform; the keys of a visited tile that a row may not
  // see are masked per score in the softmax segment, the products run over whole tiles)
  auto need0 = [&](int t) { return !(CAUSAL && t * KT > q0 + 31 + shift); };

  f32x16 s0, s1;
  e16x8 pf[4];
  // The order inside a matrix segment is pinned (sched_barrier): left to itself the scheduler requests each fragment
  // right in front of its MFMA (`ds_read x2; s_waitcnt; mfma; mfma` -- an exposed LDS round trip per pair, and with the
  // partner wave in a softmax segment nothing fills the matrix pipe meanwhile).  Every LDS operand is requested at least
  // eight MFMAs ahead of its use.
  constexpr int QK4 = NKD / 4;           // the K fragments travel in quarters of the d range, at most three resident
  e16x8 kf0[NKD], kf1[NKD];
  auto k_quarter = [&](const char* ldsK, int kba, int qt) {
#pragma unroll
    for (int kd = qt * QK4; kd < (qt + 1) * QK4; ++kd) {
      kf0[kd] = k_frag(ldsK, kba, 0, kd);
      kf1[kd] = k_frag(ldsK, kba, 1, kd);
    }
  };
  auto qk_quarter = [&](int qt) {
#pragma unroll
    for (int kd = qt * QK4; kd < (qt + 1) * QK4; ++kd) {
      s0 = MK_F8_MMA(kf0[kd], qf[kd], s0);
      s1 = MK_F8_MMA(kf1[kd], qf[kd], s1);
    }
  };
  auto pv_sb = [&](const e16x8 (&v0)[NDH][2], const e16x8 (&v1)[NDH][2], const e16x8& p0, const e16x8& p1) {
#pragma unroll
    for (int dd = 0; dd < NDH; ++dd) oacc[dd] = MK_F8_MMA(v0[dd][0], p0, oacc[dd]);
#pragma unroll
    for (int dd = 0; dd < NDH; ++dd) oacc[NDH + dd] = MK_F8_MMA(v1[dd][0], p0, oacc[NDH + dd]);
#pragma unroll
    for (int dd = 0; dd < NDH; ++dd) oacc[dd] = MK_F8_MMA(v0[dd][1], p1, oacc[dd]);
#pragma unroll
    for (int dd = 0; dd < NDH; ++dd) oacc[NDH + dd] = MK_F8_MMA(v1[dd][1], p1, oacc[NDH + dd]);
  };
  // scores of the tile in `ldsK` (QK) and / or P V of the previous tile out of `ldsVp` (PV).  With both: P V FIRST (P dies
  // with it), then the scores -- the two never hold their operand fragments at the same time (both resident: the
  // allocator spills Q fragments).
  auto products = [&](auto QK, auto PV, const char* ldsK, const char* ldsVp, int kbase) __attribute__((always_inline)) {
    constexpr bool qk = decltype(QK)::value, pvp = decltype(PV)::value;
    int kba = kb_lane, vba = vb_lane;
    asm volatile("" : "+v"(kba), "+v"(vba));
    uint8_t mbyte = 1;                     // this lane's byte of the tile's 64 key-validity bytes (published with K)
    if constexpr (qk) mbyte = reinterpret_cast<const uint8_t*>(lds + MASK0 + ((kbase / KT) & 3) * KT)[l];
    e16x8 va[NDH][2], vb[NDH][2], vc[NDH][2], vd[NDH][2];
    if constexpr (pvp) {
      load_v(ldsVp, vba, 0, 0, va);
      load_v(ldsVp, vba, 0, 1, vb);
      load_v(ldsVp, vba, 1, 0, vc);
      load_v(ldsVp, vba, 1, 1, vd);
      __builtin_amdgcn_sched_barrier(0);
      pv_sb(va, vb, pf[0], pf[1]);
      __builtin_amdgcn_sched_barrier(0);
    }
    if constexpr (qk) {
      k_quarter(ldsK, kba, 0);
      k_quarter(ldsK, kba, 1);
      __builtin_amdgcn_sched_barrier(0);
    }
    if constexpr (pvp) {
      pv_sb(vc, vd, pf[2], pf[3]);
      __builtin_amdgcn_sched_barrier(0);
    }
    if constexpr (qk) {
      k_quarter(ldsK, kba, 2);
      // The mask enters the scores as the INITIAL VALUE of the Q K^T accumulators: 0 where a key is visible, -inf where
      // it is padded / beyond Lk / above the causal diagonal (-inf + finite products = -inf).  Built HERE, in the matrix
      // segment, whose VALU is idle (16 instructions beside 32 MFMAs) and behind the first 16 MFMAs (the validity bytes
      // were requested at the top of the segment): the softmax segment -- the one that sets the barrier cadence -- has
      // no mask arithmetic, no mask branches and none of the register copies their merges cost.  Interior tiles: zeros.
      const bool allv = __builtin_amdgcn_ballot_w64(mbyte != 0) == ~0ull;
      if (allv && (!CAUSAL || kbase + KT - 1 <= q0 + shift)) {
#pragma unroll
        for (int e = 0; e < 16; ++e) { s0[e] = 0.f; s1[e] = 0.f; }
      } else if (allv) {                   // no padding in the tile: the causal limit only (key c of the tile visible iff
        const int lim = qg + shift - kbase - 4 * half;      // c <= lim; this lane's keys: (r & 3) + 8 (r >> 2) [+ 32])
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int c = (r & 3) + 8 * (r >> 2);
          s0[r] = (c <= lim) ? 0.f : -INFINITY;
          s1[r] = (32 + c <= lim) ? 0.f : -INFINITY;
        }
      } else {                             // validity bytes (+ the causal limit) per key
        const uint8_t* ldsM = reinterpret_cast<const uint8_t*>(lds + MASK0 + ((kbase / KT) & 3) * KT);
#pragma unroll
        for (int sb = 0; sb < 2; ++sb)
#pragma unroll
          for (int g4 = 0; g4 < 4; ++g4) {
            const uint32_t m4 = *reinterpret_cast<const uint32_t*>(ldsM + sb * 32 + 8 * g4 + 4 * half);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const int kg = kbase + sb * 32 + e + 8 * g4 + 4 * half;
              bool okk = ((m4 >> (8 * e)) & 0xffu) != 0;
              if (CAUSAL) okk = okk && (kg <= qg + shift);
              (sb ? s1 : s0)[4 * g4 + e] = okk ? 0.f : -INFINITY;
            }
          }
      }
      __builtin_amdgcn_sched_barrier(0);
      qk_quarter(0);
      __builtin_amdgcn_sched_barrier(0);
      k_quarter(ldsK, kba, 3);
      __builtin_amdgcn_sched_barrier(0);
      qk_quarter(1);
      __builtin_amdgcn_sched_barrier(0);
      qk_quarter(2);
      __builtin_amdgcn_sched_barrier(0);
      qk_quarter(3);
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  constexpr std::true_type YES{};
  constexpr std::false_type NO{};
  // M_t with K(t) in ring slot BI: scores of tile t, P V of tile t - 1 (V slot 1 - BI), the staging writes
  auto m_seg = [&](auto BI, int t) __attribute__((always_inline)) {
    constexpr int kslot = decltype(BI)::value * SLOT, oslot = (1 - decltype(BI)::value) * SLOT;
    const char* ldsK = lds + kslot;
    const char* ldsVp = lds + oslot + KBYTES;
    // ONE path through the loop (alternatives that each update the 64 output accumulators make the register allocator
    // keep two copies of them): the first tile multiplies P = 0 with the zero-filled V slot, the tile behind a wave's last
    // visible one computes scores nobody reads.  need0 is monotone: tile t visible => tile t - 1 visible.
#if MK_F8_PRIO == 1
    __builtin_amdgcn_s_setprio(1);
#endif
    if (active && need0(t > 0 ? t - 1 : 0)) products(YES, YES, ldsK, ldsVp, t * KT);
#if MK_F8_PRIO == 1
    __builtin_amdgcn_s_setprio(0);
#endif
#if MK_F8_ABLATE != 4
    if (t + 1 < ntiles) write_k(oslot, t + 1);
    write_v(kslot);
    if (t + 2 < ntiles) issue_k((t + 2) * KT);
    if (t + 1 < ntiles) issue_v((t + 1) * KT);
#endif
    MK_F8_BARRIER();
  };
  // S_t: online softmax of tile t (the mask is in the scores already): s0 / s1 -> pf
  auto s_seg = [&](int t) __attribute__((always_inline)) {
#if MK_F8_ABLATE != 1
    if (active && need0(t)) softmax_tile64<NDB>(s0, s1, c2, m_run, l_run, oacc, pf);
#endif
    MK_F8_BARRIER();
  };

#if MK_F8_MIXED
  // The MIXED segment (profiles/r05_attn8.txt D: matrix and softmax segments of the two waves of a SIMD do not overlap --
  // what hides a wave's softmax is its OWN MFMAs): scores of tile t first, then the 16 P V MFMAs of tile t - 1 with the
  // softmax of tile t (part A: no O, no l) placed between them by sched_group_barrier; behind them the rare O rescale,
  // the l update and the conversion of P (P(t - 1) has been consumed).  All eight waves in phase; K(t + 1) / V(t) are
  // written behind the products (their slots were last read one barrier ago), ONE barrier per tile.
  auto mixed_seg = [&](auto BI, int t) __attribute__((always_inline)) {
    constexpr int kslot = decltype(BI)::value * SLOT, oslot = (1 - decltype(BI)::value) * SLOT;
    const char* ldsK = lds + kslot;
    const char* ldsVp = lds + oslot + KBYTES;
    const int kbase = t * KT;
    if (active && need0(t > 0 ? t - 1 : 0)) {
      int kba = kb_lane, vba = vb_lane;
      asm volatile("" : "+v"(kba), "+v"(vba));
      const uint8_t mbyte = reinterpret_cast<const uint8_t*>(lds + MASK0 + (t & 3) * KT)[l];
      e16x8 va[NDH][2], vb[NDH][2], vc[NDH][2], vd[NDH][2];
      k_quarter(ldsK, kba, 0);
      k_quarter(ldsK, kba, 1);
      const bool allv = __builtin_amdgcn_ballot_w64(mbyte != 0) == ~0ull;
      if (allv && (!CAUSAL || kbase + KT - 1 <= q0 + shift)) {
#pragma unroll
        for (int e = 0; e < 16; ++e) { s0[e] = 0.f; s1[e] = 0.f; }
      } else if (allv) {
        const int lim = qg + shift - kbase - 4 * half;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int c = (r & 3) + 8 * (r >> 2);
          s0[r] = (c <= lim) ? 0.f : -INFINITY;
          s1[r] = (32 + c <= lim) ? 0.f : -INFINITY;
        }
      } else {
        const uint8_t* ldsM = reinterpret_cast<const uint8_t*>(lds + MASK0 + (t & 3) * KT);
#pragma unroll
        for (int sb = 0; sb < 2; ++sb)
#pragma unroll
          for (int g4 = 0; g4 < 4; ++g4) {
            const uint32_t m4 = *reinterpret_cast<const uint32_t*>(ldsM + sb * 32 + 8 * g4 + 4 * half);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const int kg = kbase + sb * 32 + e + 8 * g4 + 4 * half;
              bool okk = ((m4 >> (8 * e)) & 0xffu) != 0;
              if (CAUSAL) okk = okk && (kg <= qg + shift);
              (sb ? s1 : s0)[4 * g4 + e] = okk ? 0.f : -INFINITY;
            }
          }
      }
      __builtin_amdgcn_sched_barrier(0);
      qk_quarter(0);
      __builtin_amdgcn_sched_barrier(0);
      k_quarter(ldsK, kba, 2);
      load_v(ldsVp, vba, 0, 0, va);
      load_v(ldsVp, vba, 0, 1, vb);
      __builtin_amdgcn_sched_barrier(0);
      qk_quarter(1);
      __builtin_amdgcn_sched_barrier(0);
      k_quarter(ldsK, kba, 3);
      __builtin_amdgcn_sched_barrier(0);
      qk_quarter(2);
      __builtin_amdgcn_sched_barrier(0);
      qk_quarter(3);
      __builtin_amdgcn_sched_barrier(0);
      // ---- P V of tile t - 1 beside the softmax of tile t: 16 MFMAs, ~115 VALU instructions, one region (the V
      // fragments of sub-block 1 are requested at its top and land under the 8 MFMAs of sub-block 0: with them
      // requested earlier, beside the K fragments, the allocator spills)
      float alpha, psum;
      load_v(ldsVp, vba, 1, 0, vc);
      load_v(ldsVp, vba, 1, 1, vd);
      pv_sb(va, vb, pf[0], pf[1]);
      pv_sb(vc, vd, pf[2], pf[3]);
#if MK_F8_ABLATE != 1
      softmax_part_a(s0, s1, c2, m_run, alpha, psum);
#else
      alpha = 1.f; psum = 0.f;
#endif
#ifndef MK_F8_VPG        // VALU instructions placed behind each P V MFMA (profiles/r05_attn8.txt G)
#define MK_F8_VPG 7
#endif
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);           // one MFMA
        __builtin_amdgcn_sched_group_barrier(0x002, MK_F8_VPG, 0);   // its VALU fillers (exponentials included)
      }
      __builtin_amdgcn_sched_barrier(0);
      if (__any(alpha != 1.f ? 1 : 0)) {
#pragma unroll
        for (int d = 0; d < NDB; ++d)
#pragma unroll
          for (int e = 0; e < 16; ++e) oacc[d][e] *= alpha;
      }
      l_run = l_run * alpha + psum;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        pf[0][e] = (e16)s0[e]; pf[1][e] = (e16)s0[8 + e];
        pf[2][e] = (e16)s1[e]; pf[3][e] = (e16)s1[8 + e];
      }
    }
#if MK_F8_ABLATE != 4
    if (t + 1 < ntiles) write_k(oslot, t + 1);
    write_v(kslot);
    if (t + 2 < ntiles) issue_k((t + 2) * KT);
    if (t + 1 < ntiles) issue_v((t + 1) * KT);
#endif
    MK_F8_BARRIER();
  };
#endif

  // ---- prologue: K(0) and its validity in slot 0, V(0) / K(1) in flight
  if (ntiles > 0) { issue_k(0); issue_v(0); write_k(0, 0); if (ntiles > 1) issue_k(KT); }
#pragma unroll
  for (int i = 0; i < NCH; ++i)          // V slot 1 = zeros: the first matrix segment multiplies it with P = 0
    *reinterpret_cast<u32x4*>(ldsVw + SLOT + i * 8192) = u32x4{0u, 0u, 0u, 0u};
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int e = 0; e < 8; ++e) pf[i][e] = (e16)0.f;
  MK_F8_BARRIER();
#if MK_F8_MIXED
  for (int t = 0; t < ntiles; t += 2) {
    mixed_seg(std::integral_constant<int, 0>{}, t);
    if (t + 1 < ntiles) mixed_seg(std::integral_constant<int, 1>{}, t + 1);
  }
#else
#if MK_F8_PRIO == 2
  if (late) __builtin_amdgcn_s_setprio(1);   // (static priority for the second-dispatched half, MI355X_MICROARCH "Two waves per SIMD" 4)
#endif
  if (late) MK_F8_BARRIER();             // waves 4-7: one segment behind
  for (int t = 0; t < ntiles; t += 2) {
    m_seg(std::integral_constant<int, 0>{}, t);
    s_seg(t);
    if (t + 1 < ntiles) {
      m_seg(std::integral_constant<int, 1>{}, t + 1);
      s_seg(t + 1);
    }
  }
#endif
  // the last P V (tile ntiles - 1): no staging.  (Waves 0-3 run it beside the last softmax segment of waves 4-7.)
  if (active && ntiles > 0 && need0(ntiles - 1))
    products(NO, YES, lds, lds + ((ntiles - 1) & 1) * SLOT + KBYTES, 0);
  if (active) {                          // (wave-uniform: the stores need both half-waves)
    const float inv = l_run > 0.f ? 1.f / l_run : 0.f;
    e16* O = a.o + (long)b * a.o_bs + (long)min(qg, a.Lq - 1) * a.o_ld + (long)h * HD;
    store_row16<NDB>(O, oacc, inv, half, qg < a.Lq);
    if (a.lse && half == 0 && qg < a.Lq)   // natural-log lse = (m2 + log2(l)) * ln(2)
      a.lse[((long)b * a.H + h) * a.Lq + qg] =
          (l_run > 0.f) ? (m_run + __log2f(l_run)) * 0.6931471805599453f : -INFINITY;
  }
#if !MK_F8_MIXED
  if (!late) MK_F8_BARRIER();            // pairs with the last barrier of waves 4-7: every wave counts the same barriers
#endif
}

// ---- long sequences, head_dim 128: 4 waves x 64 query rows, ONE wave per SIMD, the whole 512-entry register file ----
// What the 8-wave kernel's ablations say (profiles/r05_attn8.txt D, E): a wave's softmax is hidden by its OWN MFMAs, and
// with 32 rows per wave every wave re-reads the whole K + V tile from LDS for 32 MFMAs -- 1 KiB per MFMA and SIMD, the
// LDS read rate at full matrix rate.  Here a wave owns TWO 32-row query blocks: every K / V fragment read feeds two
// MFMAs (half the LDS bytes per FLOP), 64 MFMAs per tile and wave in one stream, the softmax of both blocks (2 x ~115
// VALU) placed between the 32 P V MFMAs, nothing to arbitrate with on the SIMD.  Registers: O 2 x 64 (accumulators), scores
// 2 x 32, Q 2 x 32, P 2 x 16, K / V fragments, 32 staging registers (256 threads move the 32-KiB tile): ~440 of 512.
// Same tile walk, rings, staging, mask-as-accumulator-bias, lazy rescale and epilogue as flash_fwd8_kernel's mixed form.
// MEASURED AND NOT SHIPPED (profiles/r05_attn8.txt F): parity-green on the first run, but 765-813 TFLOP/s non-causal and
// 602-618 causal at S = 2048 against 854-935 / 653-731 for the 8-wave mixed kernel on the same box -- a lone
// compiler-scheduled wave exposes every LDS round trip, the barrier and the mask set-up that a second wave covers.
// Built only with MK_EXPERIMENTS=1 (build.py: -DMK_WITH_FWD4X64), selected with MK_ATTN_FWD4X64=1.
#ifdef MK_WITH_FWD4X64
template <bool CAUSAL>
__global__ __launch_bounds__(256, 1) void flash_fwd4x64_kernel(FlashArgs a) {
  constexpr int HD = 128, KT = 64, NKD = HD / 16, NDB = HD / 32, CPR = HD / 8;
  constexpr int KBYTES = KT * HD * 2, SLOT = 2 * KBYTES, MASK0 = 2 * SLOT;
  __shared__ __attribute__((aligned(16))) char lds[2 * SLOT + 4 * KT];
  int b = blockIdx.y, h = blockIdx.x;
  int blk = CAUSAL ? (int)(gridDim.z - 1 - blockIdx.z) : (int)blockIdx.z;
  if (!CAUSAL && a.nblk > 0) {
    const int id = blockIdx.x, xcd = id & 7, slot = id >> 3;
    const int bh = (slot / a.nblk) * 8 + xcd;
    blk = slot % a.nblk;
    if (bh >= a.B * a.H) return;
    b = bh / a.H; h = bh - b * a.H;
  }
  const int l = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int half = l >> 5, lq = l & 31;
  const int q0 = blk * 256 + w * 64;     // this wave's 64 rows: query blocks j = 0, 1 at q0 + 32 j
  const bool active = q0 < a.Lq;
  const e16* Q = a.q + (long)b * a.q_bs + (long)h * HD;
  const e16* K = a.k + (long)b * a.k_bs + (long)h * HD;
  const e16* V = a.v + (long)b * a.v_bs + (long)h * HD;
  const int shift = a.Lk - a.Lq;

  e16x8 qf[2][NKD];
  f32x16 oacc[2][NDB];
  float m_run[2] = {-INFINITY, -INFINITY}, l_run[2] = {0.f, 0.f};
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int qg = q0 + 32 * j + lq;
#pragma unroll
    for (int kd = 0; kd < NKD; ++kd)
      qf[j][kd] = ld8_or_zero(Q + (long)min(qg, a.Lq - 1) * a.q_ld + 16 * kd + 8 * half, qg < a.Lq);
#pragma unroll
    for (int d = 0; d < NDB; ++d)
#pragma unroll
      for (int e = 0; e < 16; ++e) oacc[j][d][e] = 0.f;
  }
  const float c2 = a.scale * 1.4426950408889634f;
  int k_end = a.Lk;
  if (CAUSAL) k_end = min(a.Lk, blk * 256 + 256 + shift);
  const int ntiles = k_end > 0 ? (k_end + KT - 1) / KT : 0;

  // ---- staging (256 threads: 4 + 4 16-byte chunks per thread and tile, rows 16 apart = 4 KiB of the LDS image)
  constexpr int NCH = (KT * CPR) / 256;
  constexpr int RSTEP = 256 / CPR;
  static_assert(NCH == 4 && RSTEP * CPR * 16 == 4096, "a chunk index is 4 KiB of the LDS image");
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  u32x4 kreg[NCH], vreg[NCH];
  int mreg = 1;
  const __amdgpu_buffer_rsrc_t rsK = __builtin_amdgcn_make_buffer_rsrc(
      (void*)K, 0, (int)min(((long)(a.Lk - 1) * a.k_ld + HD) * 2, 0x7fffffffL), 0x00020000);
  const __amdgpu_buffer_rsrc_t rsV = __builtin_amdgcn_make_buffer_rsrc(
      (void*)V, 0, (int)min(((long)(a.Lk - 1) * a.v_ld + HD) * 2, 0x7fffffffL), 0x00020000);
  const bool has_km = a.kmask != nullptr;
  const __amdgpu_buffer_rsrc_t rsM = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(has_km ? a.kmask + (long)b * a.Lk : (const int32_t*)K), 0, has_km ? a.Lk * 4 : 0, 0x00020000);
  const int srow = threadIdx.x / CPR, sch = threadIdx.x % CPR;
  const int kvo = (int)(((long)srow * a.k_ld + sch * 8) * 2), vvo = (int)(((long)srow * a.v_ld + sch * 8) * 2);
  const int k_step = (int)(RSTEP * a.k_ld * 2), v_step = (int)(RSTEP * a.v_ld * 2);
  char* const ldsKw = lds + k_off<HD>(srow, sch);
  char* const ldsVw = lds + KBYTES + v_off<HD>(srow, sch);
  auto issue_k = [&](int kb) {
    const int ks = (int)((long)kb * a.k_ld * 2);
#pragma unroll
    for (int i = 0; i < NCH; ++i) kreg[i] = __builtin_amdgcn_raw_buffer_load_b128(rsK, kvo, ks + i * k_step, 0);
    if (w == 0 && has_km) mreg = (int)__builtin_amdgcn_raw_buffer_load_b32(rsM, l * 4, kb * 4, 0);
  };
  auto issue_v = [&](int kb) {
    const int vs = (int)((long)kb * a.v_ld * 2);
#pragma unroll
    for (int i = 0; i < NCH; ++i) vreg[i] = __builtin_amdgcn_raw_buffer_load_b128(rsV, vvo, vs + i * v_step, 0);
  };
  auto write_k = [&](int slotoff, int t) {
#pragma unroll
    for (int i = 0; i < NCH; ++i) *reinterpret_cast<u32x4*>(ldsKw + slotoff + i * 4096) = kreg[i];
    if (w == 0) lds[MASK0 + (t & 3) * KT + l] = (has_km ? mreg != 0 : t * KT + l < a.Lk) ? 1 : 0;
  };
  auto write_v = [&](int slotoff) {
#pragma unroll
    for (int i = 0; i < NCH; ++i) *reinterpret_cast<u32x4*>(ldsVw + slotoff + i * 4096) = vreg[i];
  };

  // ---- fragments (addresses: one laundered lane constant per operand XOR a compile-time value, see flash_fwd8_kernel)
  const int li = l & 15;
  constexpr int NDH = NDB / 2;
  const int col0 = 16 * ((l >> 4) & 1) + 4 * (li & 3);
  const int kb_lane = k_off<HD>(lq, half);
  const int vb_lane = v_off<HD>(4 * half + (li >> 2), col0 >> 3) + ((col0 & 7) << 1);
  auto k_frag = [&](const char* ldsK, int kb, int sb, int kd) {
    return *reinterpret_cast<const e16x8*>(ldsK + (kb ^ (kd << 5)) + sb * 32 * HD * 2);
  };
  auto load_v = [&](const char* ldsV, int vb, int sb, int dh, e16x8 (&vf)[NDH][2]) {
#pragma unroll
    for (int dd = 0; dd < NDH; ++dd) {
      const int d = dh * NDH + dd;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          const e16x4 t = E16<e16>::tr_read(ldsV + (vb ^ (d << 6)) + (sb * 32 + ks * 16 + 8 * r) * HD * 2);
          vf[dd][ks][4 * r] = t[0]; vf[dd][ks][4 * r + 1] = t[1]; vf[dd][ks][4 * r + 2] = t[2]; vf[dd][ks][4 * r + 3] = t[3];
        }
    }
  };
  auto need0 = [&](int t) { return !(CAUSAL && t * KT > q0 + 63 + shift); };     // any row of the wave sees tile t

  f32x16 s[2][2];                        // [query block][32-key sub-block]
  e16x8 pf[2][4];
  constexpr int QK4 = NKD / 4;
  e16x8 kf0[NKD], kf1[NKD];
  auto k_quarter = [&](const char* ldsK, int kba, int qt) {
#pragma unroll
    for (int kd = qt * QK4; kd < (qt + 1) * QK4; ++kd) {
      kf0[kd] = k_frag(ldsK, kba, 0, kd);
      kf1[kd] = k_frag(ldsK, kba, 1, kd);
    }
  };
  auto qk_quarter = [&](int qt) {        // (8 MFMAs: every K fragment feeds both query blocks)
#pragma unroll
    for (int kd = qt * QK4; kd < (qt + 1) * QK4; ++kd) {
      s[0][0] = E16<e16>::mma32(kf0[kd], qf[0][kd], s[0][0]);
      s[1][0] = E16<e16>::mma32(kf0[kd], qf[1][kd], s[1][0]);
      s[0][1] = E16<e16>::mma32(kf1[kd], qf[0][kd], s[0][1]);
      s[1][1] = E16<e16>::mma32(kf1[kd], qf[1][kd], s[1][1]);
    }
  };
  auto pv_sb = [&](const e16x8 (&v0)[NDH][2], const e16x8 (&v1)[NDH][2], int sb) {   // 16 MFMAs
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
      for (int dd = 0; dd < NDH; ++dd)
#pragma unroll
        for (int j = 0; j < 2; ++j) oacc[j][dd] = E16<e16>::mma32(v0[dd][ks], pf[j][2 * sb + ks], oacc[j][dd]);
#pragma unroll
      for (int dd = 0; dd < NDH; ++dd)
#pragma unroll
        for (int j = 0; j < 2; ++j) oacc[j][NDH + dd] = E16<e16>::mma32(v1[dd][ks], pf[j][2 * sb + ks], oacc[j][NDH + dd]);
    }
  };
  // the products of one tile: QK (scores of tile kbase / KT out of ldsK) and / or PV (P V of the previous tile out of ldsVp)
  auto tile = [&](auto QK, auto PV, const char* ldsK, const char* ldsVp, int kbase) __attribute__((always_inline)) {
    constexpr bool qk = decltype(QK)::value, pvp = decltype(PV)::value;
    int kba = kb_lane, vba = vb_lane;
    asm volatile("" : "+v"(kba), "+v"(vba));
    e16x8 va[NDH][2], vb[NDH][2], vc[NDH][2], vd[NDH][2];
    if constexpr (qk) {
      const uint8_t mbyte = reinterpret_cast<const uint8_t*>(lds + MASK0 + ((kbase / KT) & 3) * KT)[l];
      k_quarter(ldsK, kba, 0);
      k_quarter(ldsK, kba, 1);
      // the mask as the initial value of the score accumulators (0 visible / -inf not), per query block
      const bool allv = __builtin_amdgcn_ballot_w64(mbyte != 0) == ~0ull;
      if (allv && (!CAUSAL || kbase + KT - 1 <= q0 + shift)) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int e = 0; e < 16; ++e) { s[j][0][e] = 0.f; s[j][1][e] = 0.f; }
      } else if (allv) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int lim = q0 + 32 * j + lq + shift - kbase - 4 * half;
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int c = (r & 3) + 8 * (r >> 2);
            s[j][0][r] = (c <= lim) ? 0.f : -INFINITY;
            s[j][1][r] = (32 + c <= lim) ? 0.f : -INFINITY;
          }
        }
      } else {
        const uint8_t* ldsM = reinterpret_cast<const uint8_t*>(lds + MASK0 + ((kbase / KT) & 3) * KT);
#pragma unroll
        for (int sb = 0; sb < 2; ++sb)
#pragma unroll
          for (int g4 = 0; g4 < 4; ++g4) {
            const uint32_t m4 = *reinterpret_cast<const uint32_t*>(ldsM + sb * 32 + 8 * g4 + 4 * half);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const int kg = kbase + sb * 32 + e + 8 * g4 + 4 * half;
              const bool okv = ((m4 >> (8 * e)) & 0xffu) != 0;
#pragma unroll
              for (int j = 0; j < 2; ++j) {
                bool okk = okv;
                if (CAUSAL) okk = okk && (kg <= q0 + 32 * j + lq + shift);
                s[j][sb][4 * g4 + e] = okk ? 0.f : -INFINITY;
              }
            }
          }
      }
      __builtin_amdgcn_sched_barrier(0);
      qk_quarter(0);
      __builtin_amdgcn_sched_barrier(0);
      k_quarter(ldsK, kba, 2);
      if constexpr (pvp) { load_v(ldsVp, vba, 0, 0, va); load_v(ldsVp, vba, 0, 1, vb); }
      __builtin_amdgcn_sched_barrier(0);
      qk_quarter(1);
      __builtin_amdgcn_sched_barrier(0);
      k_quarter(ldsK, kba, 3);
      __builtin_amdgcn_sched_barrier(0);
      qk_quarter(2);
      __builtin_amdgcn_sched_barrier(0);
      qk_quarter(3);
      __builtin_amdgcn_sched_barrier(0);
    } else {
      load_v(ldsVp, vba, 0, 0, va);
      load_v(ldsVp, vba, 0, 1, vb);
    }
    float alpha[2] = {1.f, 1.f}, psum[2] = {0.f, 0.f};
    if constexpr (pvp) {
      load_v(ldsVp, vba, 1, 0, vc);
      load_v(ldsVp, vba, 1, 1, vd);
      pv_sb(va, vb, 0);
      pv_sb(vc, vd, 1);
    }
    if constexpr (qk) {
      softmax_part_a(s[0][0], s[0][1], c2, m_run[0], alpha[0], psum[0]);
      softmax_part_a(s[1][0], s[1][1], c2, m_run[1], alpha[1], psum[1]);
    }
    if constexpr (qk && pvp) {
#pragma unroll
      for (int i = 0; i < 32; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);      // one MFMA
        __builtin_amdgcn_sched_group_barrier(0x002, 7, 0);      // seven VALU
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (qk) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        if (__any(alpha[j] != 1.f ? 1 : 0)) {
#pragma unroll
          for (int d = 0; d < NDB; ++d)
#pragma unroll
            for (int e = 0; e < 16; ++e) oacc[j][d][e] *= alpha[j];
        }
        l_run[j] = l_run[j] * alpha[j] + psum[j];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          pf[j][0][e] = (e16)s[j][0][e]; pf[j][1][e] = (e16)s[j][0][8 + e];
          pf[j][2][e] = (e16)s[j][1][e]; pf[j][3][e] = (e16)s[j][1][8 + e];
        }
      }
    }
  };
  constexpr std::true_type YES{};
  constexpr std::false_type NO{};
  auto seg = [&](auto BI, int t) __attribute__((always_inline)) {
    constexpr int kslot = decltype(BI)::value * SLOT, oslot = (1 - decltype(BI)::value) * SLOT;
    // (one path through the loop: the first tile multiplies P = 0 with the zero-filled V slot; need0 is monotone)
    if (active && need0(t > 0 ? t - 1 : 0)) tile(YES, YES, lds + kslot, lds + oslot + KBYTES, t * KT);
    if (t + 1 < ntiles) write_k(oslot, t + 1);
    write_v(kslot);
    if (t + 2 < ntiles) issue_k((t + 2) * KT);
    if (t + 1 < ntiles) issue_v((t + 1) * KT);
    MK_F8_BARRIER();
  };

  if (ntiles > 0) { issue_k(0); issue_v(0); write_k(0, 0); if (ntiles > 1) issue_k(KT); }
#pragma unroll
  for (int i = 0; i < NCH; ++i)
    *reinterpret_cast<u32x4*>(ldsVw + SLOT + i * 4096) = u32x4{0u, 0u, 0u, 0u};
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int e = 0; e < 8; ++e) pf[j][i][e] = (e16)0.f;
  MK_F8_BARRIER();
  for (int t = 0; t < ntiles; t += 2) {
    seg(std::integral_constant<int, 0>{}, t);
    if (t + 1 < ntiles) seg(std::integral_constant<int, 1>{}, t + 1);
  }
  if (active && ntiles > 0 && need0(ntiles - 1))
    tile(NO, YES, lds, lds + ((ntiles - 1) & 1) * SLOT + KBYTES, 0);
  if (active) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int qg = q0 + 32 * j + lq;
      if (q0 + 32 * j < a.Lq) {          // (wave-uniform: the stores need both half-waves)
        const float inv = l_run[j] > 0.f ? 1.f / l_run[j] : 0.f;
        e16* O = a.o + (long)b * a.o_bs + (long)min(qg, a.Lq - 1) * a.o_ld + (long)h * HD;
        store_row16<NDB>(O, oacc[j], inv, half, qg < a.Lq);
        if (a.lse && half == 0 && qg < a.Lq)
          a.lse[((long)b * a.H + h) * a.Lq + qg] =
              (l_run[j] > 0.f) ? (m_run[j] + __log2f(l_run[j])) * 0.6931471805599453f : -INFINITY;
      }
    }
  }
}

#endif  // MK_WITH_FWD4X64

// (defined next to the short-sequence backward, further down)
template <int HD, bool CAUSAL, bool ROPE>
__global__ __launch_bounds__(256, 2) void flash_fwd_short_kernel(FlashArgs a);

int flash_attn_fwd_impl(const void* q, const void* k, const void* v, void* o, float* lse,
                                 const int32_t* kmask, int32_t B, int32_t H, int32_t Lq,
                                 int32_t Lk, int32_t hd, int64_t q_ld, int64_t q_bs, int64_t k_ld,
                                 int64_t k_bs, int64_t v_ld, int64_t v_bs, int64_t o_ld,
                                 int64_t o_bs, float scale, int32_t causal, int32_t dtype,
                                 void* stream, const void* rope_cos = nullptr,
                                 const void* rope_sin = nullptr, const int32_t* rope_pos = nullptr) {
  if (!q || !k || !v || !o || B <= 0 || H <= 0 || Lq <= 0 || Lk <= 0) return MK_ERR_BAD_ARG;
  const bool rope = rope_cos || rope_sin || rope_pos;
  if (rope && (!rope_cos || !rope_sin || !rope_pos)) return MK_ERR_BAD_ARG;
  if (rope && ((reinterpret_cast<uintptr_t>(rope_cos) | reinterpret_cast<uintptr_t>(rope_sin)) & 15))
    return MK_ERR_UNSUPPORTED;
  if (dtype != E16<e16>::dtype || (hd != 64 && hd != 128)) return MK_ERR_UNSUPPORTED;
  const uintptr_t al = reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k) |
                       reinterpret_cast<uintptr_t>(v) | reinterpret_cast<uintptr_t>(o);
  if ((al & 15) || (q_ld % 8) || (k_ld % 8) || (v_ld % 8) || (o_ld % 8) || (q_bs % 8) ||
      (k_bs % 8) || (v_bs % 8) || (o_bs % 8))
    return MK_ERR_UNSUPPORTED;
  FlashArgs a;
  a.q = (const e16*)q; a.k = (const e16*)k; a.v = (const e16*)v; a.o = (e16*)o;
  a.lse = lse; a.kmask = kmask;
  a.B = B; a.H = H; a.Lq = Lq; a.Lk = Lk;
  a.q_ld = q_ld; a.q_bs = q_bs; a.k_ld = k_ld; a.k_bs = k_bs; a.v_ld = v_ld; a.v_bs = v_bs;
  a.o_ld = o_ld; a.o_bs = o_bs;
  a.scale = scale;
  a.nblk = 0;
  a.rcos = (const e16*)rope_cos; a.rsin = (const e16*)rope_sin; a.rpos = rope_pos;
  dim3 grid(H, B, mk_cdiv(Lq, 128)), block(256);
  static const bool no_group = getenv("MK_ATTN_NO_XCD_GROUP") != nullptr;
  if (!causal && !no_group && mk_cdiv(Lq, 128) >= 4) {
    a.nblk = mk_cdiv(Lq, 128);
    grid = dim3((unsigned)(8 * mk_cdiv((long)B * H, 8) * a.nblk), 1, 1);
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  // algorithmic FLOPs: QK^T and PV, 2 * Lq * Lk * hd each per (b, h); causal counts the lower
  // triangle only (what a masked dense formulation would not skip is not work)
  const double pairs = causal ? ((double)Lq * Lk - 0.5 * (double)min(Lq, Lk) * (min(Lq, Lk) - 1)) : (double)Lq * Lk;
  const int prof = mkp::begin(st, 1, 4.0 * pairs * hd * B * H, Lq, Lk, hd, B * H, causal, 0);
  static const bool no_short = getenv("MK_ATTN_NO_SHORT_FWD") != nullptr;
  if (hd == 128 && Lq == Lk && Lk <= 160 && !no_short) {
    const int lds_bytes = 2 * Lk * 128 * 2 + 160 * 4;
    static bool attr_done = false;
    if (!attr_done) {
      const int max_lds = 2 * 160 * 128 * 2 + 160 * 4;
      if (hipFuncSetAttribute(reinterpret_cast<const void*>(&flash_fwd_short_kernel<128, true, false>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, max_lds) != hipSuccess ||
          hipFuncSetAttribute(reinterpret_cast<const void*>(&flash_fwd_short_kernel<128, false, false>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, max_lds) != hipSuccess ||
          hipFuncSetAttribute(reinterpret_cast<const void*>(&flash_fwd_short_kernel<128, true, true>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, max_lds) != hipSuccess ||
          hipFuncSetAttribute(reinterpret_cast<const void*>(&flash_fwd_short_kernel<128, false, true>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, max_lds) != hipSuccess)
        return MK_ERR_LAUNCH;
      attr_done = true;
    }
    if (rope) {
      if (causal) MK_LAUNCH((flash_fwd_short_kernel<128, true, true>), dim3(H, B), block, lds_bytes, st, a);
      else MK_LAUNCH((flash_fwd_short_kernel<128, false, true>), dim3(H, B), block, lds_bytes, st, a);
    } else {
      if (causal) MK_LAUNCH((flash_fwd_short_kernel<128, true, false>), dim3(H, B), block, lds_bytes, st, a);
      else MK_LAUNCH((flash_fwd_short_kernel<128, false, false>), dim3(H, B), block, lds_bytes, st, a);
    }
    mkp::end(prof, st);
    return mk_check_launch();
  }
  if (rope) return MK_ERR_UNSUPPORTED;     // the rotation lives in the short-sequence kernel only
  // long sequences: the 8-wave kernel (256 query rows per workgroup, matrix / softmax segments of its two wave groups
  // interleaved).  MK_ATTN_FWD8_MIN=<rows> moves the threshold (0: never); head_dim 64 only with MK_ATTN_FWD8_HD64=1
  // (read per call: the tests and scripts/bench_attn.py switch kernels inside one process)
  const char* env_min = getenv("MK_ATTN_FWD8_MIN");
  const int fwd8_min = env_min ? atoi(env_min) : 1024;
  const bool fwd8_hd64 = getenv("MK_ATTN_FWD8_HD64") != nullptr;
  if (fwd8_min > 0 && Lq >= fwd8_min && (hd == 128 || fwd8_hd64)) {
    const int nb = mk_cdiv(Lq, 256);
    dim3 grid8(H, B, nb);
    a.nblk = 0;
    if (!causal && !no_group && nb >= 2) {
      a.nblk = nb;
      grid8 = dim3((unsigned)(8 * mk_cdiv((long)B * H, 8) * nb), 1, 1);
    }
#ifdef MK_WITH_FWD4X64
    const char* env_464 = getenv("MK_ATTN_FWD4X64");          // 4 waves x 64 rows, one wave per SIMD (experiment build)
    if (hd == 128 && env_464 && atoi(env_464) != 0) {
      if (causal) MK_LAUNCH((flash_fwd4x64_kernel<true>), grid8, dim3(256), 0, st, a);
      else MK_LAUNCH((flash_fwd4x64_kernel<false>), grid8, dim3(256), 0, st, a);
    } else
#endif
    if (hd == 128) {
      if (causal) MK_LAUNCH((flash_fwd8_kernel<128, true>), grid8, dim3(512), 0, st, a);
      else MK_LAUNCH((flash_fwd8_kernel<128, false>), grid8, dim3(512), 0, st, a);
    } else {
      if (causal) MK_LAUNCH((flash_fwd8_kernel<64, true>), grid8, dim3(512), 0, st, a);
      else MK_LAUNCH((flash_fwd8_kernel<64, false>), grid8, dim3(512), 0, st, a);
    }
    mkp::end(prof, st);
    return mk_check_launch();
  }
  if (hd == 128) {
    if (causal) MK_LAUNCH((flash_fwd_kernel<128, true>), grid, block, 0, st, a);
    else MK_LAUNCH((flash_fwd_kernel<128, false>), grid, block, 0, st, a);
  } else {
    if (causal) MK_LAUNCH((flash_fwd_kernel<64, true>), grid, block, 0, st, a);
    else MK_LAUNCH((flash_fwd_kernel<64, false>), grid, block, 0, st, a);
  }
  mkp::end(prof, st);
  return mk_check_launch();
}

// The causal forward with per-sample lengths read on the device (macaw_hip.h: mk_flash_attn_varlen_fwd).  Always the
// 4-wave kernel: Lq / Lk are upper bounds, the grid is sized by Lq and a block past its sample's q_len leaves at once.
int flash_attn_varlen_fwd_impl(const void* q, const void* k, const void* v, void* o, float* lse, const int32_t* q_len,
                               const int32_t* k_len, int32_t B, int32_t H, int32_t Lq, int32_t Lk, int32_t hd,
                               int64_t q_ld, int64_t q_bs, int64_t k_ld, int64_t k_bs, int64_t v_ld, int64_t v_bs,
                               int64_t o_ld, int64_t o_bs, float scale, int32_t dtype, void* stream) {
  if (!q || !k || !v || !o || !q_len || !k_len || B <= 0 || H <= 0 || Lq <= 0 || Lk <= 0) return MK_ERR_BAD_ARG;
  if (dtype != E16<e16>::dtype || (hd != 64 && hd != 128)) return MK_ERR_UNSUPPORTED;
  const uintptr_t al = reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k) |
                       reinterpret_cast<uintptr_t>(v) | reinterpret_cast<uintptr_t>(o);
  if ((al & 15) || (q_ld % 8) || (k_ld % 8) || (v_ld % 8) || (o_ld % 8) || (q_bs % 8) ||
      (k_bs % 8) || (v_bs % 8) || (o_bs % 8))
    return MK_ERR_UNSUPPORTED;
  FlashVarlenArgs a;
  a.q = (const e16*)q; a.k = (const e16*)k; a.v = (const e16*)v; a.o = (e16*)o;
  a.lse = lse; a.kmask = nullptr;
  a.B = B; a.H = H; a.Lq = Lq; a.Lk = Lk;
  a.q_ld = q_ld; a.q_bs = q_bs; a.k_ld = k_ld; a.k_bs = k_bs; a.v_ld = v_ld; a.v_bs = v_bs;
  a.o_ld = o_ld; a.o_bs = o_bs;
  a.scale = scale;
  a.nblk = 0;
  a.rcos = nullptr; a.rsin = nullptr; a.rpos = nullptr;
  a.q_len = q_len; a.k_len = k_len;
  dim3 grid(H, B, mk_cdiv(Lq, 128)), block(256);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  // (the lengths live on the device: the FLOP figure is the bound's, every sample at (Lq, Lk))
  const double pairs = (double)Lq * Lk - 0.5 * (double)min(Lq, Lk) * (min(Lq, Lk) - 1);
  const int prof = mkp::begin(st, 1, 4.0 * pairs * hd * B * H, Lq, Lk, hd, B * H, 1, 0);
  if (hd == 128) MK_LAUNCH((flash_fwd_kernel<128, true, FlashVarlenArgs>), grid, block, 0, st, a);
  else MK_LAUNCH((flash_fwd_kernel<64, true, FlashVarlenArgs>), grid, block, 0, st, a);
  mkp::end(prof, st);
  return mk_check_launch();
}

// =====================================================================================
// Fused attention BACKWARD (recompute form): given q, k, v, o, do and the forward's
// log-sum-exp, produce dq, dk, dv without ever storing P.  Three kernels:
//   flash_bwd_prep : Dv[b,h,q] = sum_d do[q,d] * o[q,d]                       (HBM-bound)
//   flash_bwd_dq   : block = 128 queries, walks the key tiles  (lane <-> query, as forward)
//   flash_bwd_dkv  : block = 128 keys,    walks the query tiles (lane <-> key)
// In both MFMA kernels every product is arranged so that the softmax-shaped tile (P, dS) is
// consumed as the B operand straight out of the accumulator registers that produced it:
//   dq kernel : S^T = K Q^T, dP^T = V dO^T  -> dS^T (lane = query)  -> dQ^T += K^T dS^T
//   dkv kernel: S   = Q K^T, dP   = dO V^T  -> P, dS (lane = key)   -> dV^T += dO^T P,
//                                                                     dK^T += Q^T dS
// with the transposed operands (K^T, dO^T, Q^T) read from row-major LDS tiles through
// ds_read_b64_tr_b16 using the same k-slot <-> row mapping as the accumulator layout.
// =====================================================================================

struct FlashBwdArgs {
  const e16* q; const e16* k; const e16* v; const e16* o; const e16* dout;
  e16* dq; e16* dk; e16* dv;
  const float* lse; float* dvec; const int32_t* kmask;
  int B, H, Lq, Lk;
  long q_ld, q_bs, k_ld, k_bs, v_ld, v_bs, o_ld, o_bs;  // dq/dk/dv/do share q/k/v/o geometry
  float scale;
  // q and k arrive UNROTATED, dq and dk leave as gradients of the unrotated tensors (short-sequence kernel only)
  const e16* rcos; const e16* rsin; const int32_t* rpos;
};

// D[b, h, q] = sum_d dO * O.  HD / 8 lanes per row, 16-byte loads; consecutive lane groups take
// consecutive HEADS of one token (contiguous in memory), so a wave reads whole 128-byte lines.
template <int HD>
__global__ __launch_bounds__(256) void flash_bwd_prep_kernel(FlashBwdArgs a) {
  constexpr int LPR = HD / 8;                       // lanes per (token, head) row
  const long g = ((long)blockIdx.x * 256 + threadIdx.x) / LPR;   // (b, q, h) flattened, h fastest
  const int c = threadIdx.x % LPR;
  const long total = (long)a.B * a.Lq * a.H;
  const bool ok = g < total;
  const long gc = ok ? g : total - 1;
  const int h = (int)(gc % a.H);
  const long bq = gc / a.H;
  const int qi = (int)(bq % a.Lq);
  const long b = bq / a.Lq;
  const long off = b * a.o_bs + (long)qi * a.o_ld + (long)h * HD + c * 8;
  float o[8], d[8];
  VecIO<e16>::load(a.o + off, o);
  VecIO<e16>::load(a.dout + off, d);
  float s = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) s += o[e] * d[e];
#pragma unroll
  for (int m = LPR / 2; m > 0; m >>= 1) s += __shfl_xor(s, m, 64);
  if (ok && c == 0) a.dvec[(b * a.H + h) * a.Lq + qi] = s;
}

// tile stored twice: [rows][HD] with the b128 swizzle (k_off) and with the tr swizzle (v_off)
template <int HD, int ROWS>
MK_DEV void stage_rows(const e16* src, long ld, int row0, int nrows_valid, char* lds_b128,
                       char* lds_tr) {
  constexpr int CPR = HD / 8, N = (ROWS * CPR) / 256;
  uint4 v[N];
#pragma unroll
  for (int i = 0; i < N; ++i) {          // all loads in flight before the first LDS write
    const int c = threadIdx.x + 256 * i;
    const int row = c / CPR, ch = c % CPR;
    v[i] = ld16_or_zero(src + (long)min(row0 + row, nrows_valid - 1) * ld + ch * 8,
                        row0 + row < nrows_valid);
  }
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const int c = threadIdx.x + 256 * i;
    const int row = c / CPR, ch = c % CPR;
    if (lds_b128) *reinterpret_cast<uint4*>(lds_b128 + k_off<HD>(row, ch)) = v[i];
    if (lds_tr) *reinterpret_cast<uint4*>(lds_tr + v_off<HD>(row, ch)) = v[i];
  }
}
// two tensors at once (one wait for both)
template <int HD, int ROWS>
MK_DEV void stage_rows2(const e16* s0, long ld0, char* b0, char* t0, const e16* s1, long ld1,
                        char* b1, char* t1, int row0, int nrows_valid) {
  constexpr int CPR = HD / 8, N = (ROWS * CPR) / 256;
  uint4 v0[N], v1[N];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const int c = threadIdx.x + 256 * i;
    const int row = c / CPR, ch = c % CPR;
    const long r = min(row0 + row, nrows_valid - 1);
    v0[i] = ld16_or_zero(s0 + r * ld0 + ch * 8, row0 + row < nrows_valid);
    v1[i] = ld16_or_zero(s1 + r * ld1 + ch * 8, row0 + row < nrows_valid);
  }
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const int c = threadIdx.x + 256 * i;
    const int row = c / CPR, ch = c % CPR;
    if (b0) *reinterpret_cast<uint4*>(b0 + k_off<HD>(row, ch)) = v0[i];
    if (t0) *reinterpret_cast<uint4*>(t0 + v_off<HD>(row, ch)) = v0[i];
    if (b1) *reinterpret_cast<uint4*>(b1 + k_off<HD>(row, ch)) = v1[i];
    if (t1) *reinterpret_cast<uint4*>(t1 + v_off<HD>(row, ch)) = v1[i];
  }
}

// A-operand fragment X^T[d-block rows][k-slots <-> rows r0 + kappa] from a row-major LDS tile
template <int HD>
MK_DEV e16x8 tr_frag(const char* lds_tr, int rowbase16, int dblk) {
  const int l = threadIdx.x & 63, li = l & 15, half = l >> 5;
  const int col = dblk * 32 + 16 * ((l >> 4) & 1) + 4 * (li & 3);
  e16x8 f;
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int row = rowbase16 + 8 * r + 4 * half + (li >> 2);
    const int off = v_off<HD>(row, col >> 3) + ((col & 7) << 1);
    const e16x4 t = E16<e16>::tr_read(lds_tr + off);
    f[4 * r] = t[0]; f[4 * r + 1] = t[1]; f[4 * r + 2] = t[2]; f[4 * r + 3] = t[3];
  }
  return f;
}

// ---- round 5: staging without address arithmetic ------------------------------------------------------------
// A [ROWS][HD] tile of a row-pitched operand as 16-byte chunks, 256 threads: chunk i of a thread is row
// srow + i * (256 / CPR), 16-byte column sch.  Loads are raw buffer loads -- ONE per-lane voffset, the tile and the
// chunk index advance through the scalar offset, rows beyond `nrows` read as zeros through the descriptor's range
// check (no clamp, no select) -- and the LDS images' swizzles depend on row bits below 256 / CPR only, so chunk i
// lands 4 KiB behind chunk 0 in either image: one constant per lane and image, immediates for the rest.  (PMC, round
// 5: the attention kernels issued 8.7 - 10.7 VALU instructions per MFMA; ~100 per tile were this arithmetic.)
typedef uint32_t att_u32x4 __attribute__((ext_vector_type(4)));
template <int HD, int ROWS>
struct TileStager {
  static constexpr int CPR = HD / 8, N = (ROWS * CPR) / 256;
  static_assert((256 / CPR) * CPR * 16 == 4096, "a chunk index is 4 KiB of an LDS image");
  __amdgpu_buffer_rsrc_t rs;
  int vo, step, row_bytes;
  MK_DEV void init(const e16* base, long ld, int nrows) {
    rs = __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, (int)min(((long)(nrows - 1) * ld + HD) * 2, 0x7fffffffL),
                                           0x00020000);
    const int srow = threadIdx.x / CPR, sch = threadIdx.x % CPR;
    vo = (int)(((long)srow * ld + sch * 8) * 2);
    step = (int)((256 / CPR) * ld * 2);
    row_bytes = (int)(ld * 2);
  }
  MK_DEV void load(att_u32x4 (&v)[N], int row0) const {
    const int so = row0 * row_bytes;
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = __builtin_amdgcn_raw_buffer_load_b128(rs, vo, so + i * step, 0);
  }
  // this thread's chunk-0 byte offset in a b128 image (k_off) / a transposed-read image (v_off)
  MK_DEV static int off_b128() { return k_off<HD>(threadIdx.x / CPR, threadIdx.x % CPR); }
  MK_DEV static int off_tr() { return v_off<HD>(threadIdx.x / CPR, threadIdx.x % CPR); }
  MK_DEV static void write(const att_u32x4 (&v)[N], char* img_at_lane) {
#pragma unroll
    for (int i = 0; i < N; ++i) *reinterpret_cast<att_u32x4*>(img_at_lane + i * 4096) = v[i];
  }
};

// byte offsets of this lane's transposed reads for d block `d` at row base 0 of a tr image (v_off swizzle): the
// swizzle term depends on the row through (row & 3) only and every row base used is a multiple of 8, so a
// fragment at row base R is `tr_base[d] + R * HD * 2` (+ 8 rows for its second half): 4 registers, set up once.
template <int HD>
MK_DEV void tr_bases(int (&tb)[HD / 32]) {
  const int l = threadIdx.x & 63, li = l & 15, half = l >> 5;
#pragma unroll
  for (int d = 0; d < HD / 32; ++d) {
    const int col = d * 32 + 16 * ((l >> 4) & 1) + 4 * (li & 3);
    tb[d] = v_off<HD>(4 * half + (li >> 2), col >> 3) + ((col & 7) << 1);
  }
}
template <int HD>
MK_DEV e16x8 tr_frag_at(const char* img, int tbase_d, int rowbase16) {
  e16x8 f;
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const e16x4 t = E16<e16>::tr_read(img + tbase_d + (rowbase16 + 8 * r) * (HD * 2));
    f[4 * r] = t[0]; f[4 * r + 1] = t[1]; f[4 * r + 2] = t[2]; f[4 * r + 3] = t[3];
  }
  return f;
}

// ------------------------------------------------------------------ dQ kernel --
// ASYNC: the K / V tile of key tile kt + 1 is fetched into registers under the MFMAs of tile kt (32 more VGPRs:
// one workgroup per CU instead of two); !ASYNC: load, wait and write between the two barriers, two workgroups
// per CU hiding each other's round trips.  Measured (scripts/bench_attn.py, profiles/r04_attn_ab.txt, whole
// backward at B4 H32 S2048 hd128 causal): 300 TFLOP/s with the synchronous form, 254 with the asynchronous one
// -- here the second workgroup is worth more than the prefetch (the 252-VGPR body has no room for both), so
// !ASYNC ships; MK_ATTN_DQ_ASYNC=1 selects the other (A/B).
template <int HD, bool CAUSAL, bool ASYNC = false>
__global__ __launch_bounds__(256, 2) void flash_bwd_dq_kernel(FlashBwdArgs a) {
  constexpr int KT = 64, NKD = HD / 16, NDB = HD / 32;
  __shared__ __attribute__((aligned(16))) char lds[3 * KT * HD * 2 + KT * 4];
  int* ldsM = reinterpret_cast<int*>(lds + 3 * KT * HD * 2);
  char* ldsK = lds;                      // K tile, b128 image (A operand of S^T = K Q^T)
  char* ldsKt = lds + KT * HD * 2;       // K tile, tr image   (K^T for dQ^T += K^T dS^T)
  char* ldsV = lds + 2 * KT * HD * 2;    // V tile, b128 image (A operand of dP^T = V dO^T)
  // grid = (H, B, blocks), heaviest sequence blocks dispatched first (see flash_fwd_kernel)
  const int b = blockIdx.y, h = blockIdx.x;
  const int l = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int half = l >> 5, lq = l & 31;
  const int blk = CAUSAL ? (int)(gridDim.z - 1 - blockIdx.z) : (int)blockIdx.z;
  const int q0 = blk * 128 + w * 32;
  const int qg = q0 + lq;
  const e16* Q = a.q + (long)b * a.q_bs + (long)h * HD;
  const e16* dO = a.dout + (long)b * a.o_bs + (long)h * HD;
  const e16* K = a.k + (long)b * a.k_bs + (long)h * HD;
  const e16* V = a.v + (long)b * a.v_bs + (long)h * HD;
  const int32_t* km = a.kmask ? a.kmask + (long)b * a.Lk : nullptr;
  e16x8 qf[NKD], dof[NKD];
#pragma unroll
  for (int kd = 0; kd < NKD; ++kd) {
    const int qc = min(qg, a.Lq - 1);
    qf[kd] = ld8_or_zero(Q + (long)qc * a.q_ld + 16 * kd + 8 * half, qg < a.Lq);
    dof[kd] = ld8_or_zero(dO + (long)qc * a.o_ld + 16 * kd + 8 * half, qg < a.Lq);
  }
  const long rowid = ((long)b * a.H + h) * a.Lq + min(qg, a.Lq - 1);
  // exp2 domain, mask applied BEFORE the exponential (valid scores are <= lse up to rounding), the `scale` of
  // dS = p (dP - D) scale folded into the accumulators at the store: three VALU instructions less per score
  // (round 4; as flash_bwd_short_kernel)
  const float lse = a.lse[rowid] * 1.44269504088896341f, dv_ = a.dvec[rowid];
  const float c1 = a.scale * 1.44269504088896341f;
  // bf16: the `scale` of dS multiplies the fp32 accumulators at the store; fp16: dS is scaled before it is rounded
  const float ds_mul = E16<e16>::narrow_exponent ? a.scale : 1.0f;
  const float st_mul = E16<e16>::narrow_exponent ? 1.0f : a.scale;
  f32x16 acc[NDB];
#pragma unroll
  for (int d = 0; d < NDB; ++d)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[d][e] = 0.f;
  const int shift = a.Lk - a.Lq;
  int k_end = a.Lk;
  if (CAUSAL) k_end = min(a.Lk, blk * 128 + 128 + shift);
  const int ntiles = (k_end + KT - 1) / KT;
  // round 5: staging through TileStager (no address arithmetic, zeros from the range check), transposed-read
  // bases set up once, and an INTERIOR path: a sub-block whose 32 keys are all valid and visible to every row of
  // the wave skips the mask arithmetic (at S = 2048 all but the diagonal tiles)
  typedef TileStager<HD, KT> St;
  St stK, stV;
  stK.init(K, a.k_ld, a.Lk);
  stV.init(V, a.v_ld, a.Lk);
  char* const wK = ldsK + St::off_b128();
  char* const wKt = ldsKt + St::off_tr();
  char* const wV = ldsV + St::off_b128();
  int tb[NDB];
  tr_bases<HD>(tb);
  att_u32x4 pk[St::N], pv[St::N];
  if constexpr (ASYNC) { if (ntiles > 0) { stK.load(pk, 0); stV.load(pv, 0); } }
  for (int kt = 0; kt < ntiles; ++kt) {
    const int kbase = kt * KT;
    __syncthreads();
    if constexpr (!ASYNC) {
      stK.load(pk, kbase);
      stV.load(pv, kbase);
      __builtin_amdgcn_sched_barrier(0);
    }
    St::write(pk, wK);
    St::write(pk, wKt);
    St::write(pv, wV);
    if (threadIdx.x < KT) {
      const int kg = kbase + threadIdx.x;
      ldsM[threadIdx.x] = (kg < a.Lk) && (!km || km[kg] != 0);
    }
    __syncthreads();
    if constexpr (ASYNC) { if (kt + 1 < ntiles) { stK.load(pk, kbase + KT); stV.load(pv, kbase + KT); } }
    if (q0 >= a.Lq) continue;
#pragma unroll
    for (int sb = 0; sb < 2; ++sb) {
      if (CAUSAL && kbase + sb * 32 > q0 + 31 + shift) continue;     // entirely masked for this wave: dS = 0
      f32x16 s, dp;
#pragma unroll
      for (int e = 0; e < 16; ++e) { s[e] = 0.f; dp[e] = 0.f; }
#pragma unroll
      for (int kd = 0; kd < NKD; ++kd) {
        const e16x8 kf = *reinterpret_cast<const e16x8*>(ldsK + k_off<HD>(sb * 32 + lq, 2 * kd + half));
        const e16x8 vf = *reinterpret_cast<const e16x8*>(ldsV + k_off<HD>(sb * 32 + lq, 2 * kd + half));
        s = E16<e16>::mma32(kf, qf[kd], s);
        dp = E16<e16>::mma32(vf, dof[kd], dp);
      }
      e16x8 dsf[2];
      bool interior = (__builtin_amdgcn_ballot_w64(ldsM[sb * 32 + lq] != 0) == ~0ull) && (q0 + 31 < a.Lq);
      if (CAUSAL) interior = interior && (kbase + sb * 32 + 31 <= q0 + shift);
      if (interior) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(s[r], c1, -lse));
          dsf[r >> 3][r & 7] = (e16)(p * (dp[r] - dv_) * ds_mul);
        }
      } else {
        int mk[16];
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
          const int4 m4 = *reinterpret_cast<const int4*>(ldsM + sb * 32 + 8 * g4 + 4 * half);
          mk[4 * g4] = m4.x; mk[4 * g4 + 1] = m4.y; mk[4 * g4 + 2] = m4.z; mk[4 * g4 + 3] = m4.w;
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int kg = kbase + sb * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
          bool ok = mk[r] != 0;
          if (CAUSAL) ok = ok && (kg <= qg + shift);
          const float p = __builtin_amdgcn_exp2f(ok ? __builtin_fmaf(s[r], c1, -lse) : -1.0e30f);
          dsf[r >> 3][r & 7] = (e16)(p * (dp[r] - dv_) * ds_mul);
        }
      }
#pragma unroll
      for (int d = 0; d < NDB; ++d)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
          acc[d] = E16<e16>::mma32(tr_frag_at<HD>(ldsKt, tb[d], sb * 32 + ks * 16), dsf[ks], acc[d]);
    }
  }
  if (q0 >= a.Lq) return;                // (wave-uniform)
  e16* DQ = a.dq + (long)b * a.q_bs + (long)min(qg, a.Lq - 1) * a.q_ld + (long)h * HD;
  store_row16<NDB>(DQ, acc, st_mul, half, qg < a.Lq);
}

// ---------------------------------------------------------------- dK/dV kernel --
template <int HD, bool CAUSAL>
__global__ __launch_bounds__(256) void flash_bwd_dkv_kernel(FlashBwdArgs a) {
  constexpr int QT = 64, NKD = HD / 16, NDB = HD / 32;
  __shared__ __attribute__((aligned(16))) char lds[4 * QT * HD * 2 + 2 * QT * 4];
  char* ldsQ = lds;                      // Q tile b128 image  (A operand of S  = Q K^T)
  char* ldsQt = lds + QT * HD * 2;       // Q tile tr image    (Q^T for dK^T += Q^T dS)
  char* ldsD = lds + 2 * QT * HD * 2;    // dO tile b128 image (A operand of dP = dO V^T)
  char* ldsDt = lds + 3 * QT * HD * 2;   // dO tile tr image   (dO^T for dV^T += dO^T P)
  float* ldsLse = reinterpret_cast<float*>(lds + 4 * QT * HD * 2);
  float* ldsDv = ldsLse + QT;
  // grid = (H, B, blocks), heaviest sequence blocks dispatched first (see flash_fwd_kernel)
  const int b = blockIdx.y, h = blockIdx.x;
  const int l = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int half = l >> 5, lk = l & 31;
  const int blk = blockIdx.z;
  const int k0 = blk * 128 + w * 32;
  const int kg = k0 + lk;                // this lane's key
  const e16* Q = a.q + (long)b * a.q_bs + (long)h * HD;
  const e16* dO = a.dout + (long)b * a.o_bs + (long)h * HD;
  const e16* K = a.k + (long)b * a.k_bs + (long)h * HD;
  const e16* V = a.v + (long)b * a.v_bs + (long)h * HD;
  const int32_t* km = a.kmask ? a.kmask + (long)b * a.Lk : nullptr;
  e16x8 kf[NKD], vf[NKD];               // B operands: lane holds K/V[kg][16*kd + 8*half .. +8]
#pragma unroll
  for (int kd = 0; kd < NKD; ++kd) {
    const int kc = min(kg, a.Lk - 1);
    kf[kd] = ld8_or_zero(K + (long)kc * a.k_ld + 16 * kd + 8 * half, kg < a.Lk);
    vf[kd] = ld8_or_zero(V + (long)kc * a.v_ld + 16 * kd + 8 * half, kg < a.Lk);
  }
  const bool key_ok = (kg < a.Lk) && (!km || km[kg < a.Lk ? kg : 0] != 0);
  const float c1 = a.scale * 1.44269504088896341f;
  // bf16: the `scale` of dS multiplies the fp32 accumulators at the store; fp16: dS is scaled before it is rounded
  const float ds_mul = E16<e16>::narrow_exponent ? a.scale : 1.0f;
  const float st_mul = E16<e16>::narrow_exponent ? 1.0f : a.scale;
  f32x16 dka[NDB], dva[NDB];
#pragma unroll
  for (int d = 0; d < NDB; ++d)
#pragma unroll
    for (int e = 0; e < 16; ++e) { dka[d][e] = 0.f; dva[d][e] = 0.f; }
  const int shift = a.Lk - a.Lq;
  // queries that can see this block's keys: q >= key - shift
  int q_begin = 0;
  if (CAUSAL) q_begin = max(0, blk * 128 - shift) / QT * QT;
  const long rowbase = ((long)b * a.H + h) * a.Lq;
  // This kernel runs one workgroup per CU (354 registers), so nothing else hides the latency of
  // the next query tile: its Q / dO chunks and lse / D values are fetched into registers while
  // the current tile is being multiplied, and only written to LDS at the top of the next round.
  // The loads are RAW (clamped row, no select behind them): the zero fill of rows beyond Lq happens at
  // the LDS write.  Rounds 1-3 zeroed right behind the load; the select sits in the load's basic block,
  // so the compiler waited (vmcnt) for every chunk BEFORE the tile's MFMAs -- the prefetch was a
  // synchronous load in front of the compute, one exposed HBM round trip per query tile.
  // round 5: TileStager (no address arithmetic, zeros beyond Lq from the range check), transposed-read bases set up
  // once, both sub-blocks unrolled (every LDS address a per-lane constant + an immediate), INTERIOR path
  typedef TileStager<HD, QT> St;
  St stQ, stD;
  stQ.init(Q, a.q_ld, a.Lq);
  stD.init(dO, a.o_ld, a.Lq);
  char* const wQ = ldsQ + St::off_b128();
  char* const wQt = ldsQt + St::off_tr();
  char* const wD = ldsD + St::off_b128();
  char* const wDt = ldsDt + St::off_tr();
  int tb[NDB];
  tr_bases<HD>(tb);
  att_u32x4 pq[St::N], pd[St::N];
  float plse = 0.f, pdv = 0.f;
  auto prefetch = [&](int qt) {
    stQ.load(pq, qt);
    stD.load(pd, qt);
    const int qi = qt + (threadIdx.x & (QT - 1));
    const long rid = rowbase + min(qi, a.Lq - 1);
    plse = a.lse[rid];
    pdv = a.dvec[rid];
  };
  const bool keys_all_ok = __builtin_amdgcn_ballot_w64(key_ok) == ~0ull;    // (per wave)
  prefetch(q_begin);
  for (int qt = q_begin; qt < a.Lq; qt += QT) {
    __syncthreads();
    St::write(pq, wQ);
    St::write(pq, wQt);
    St::write(pd, wD);
    St::write(pd, wDt);
    if (threadIdx.x < QT) {
      const bool ok = qt + (int)threadIdx.x < a.Lq;
      ldsLse[threadIdx.x] = ok ? plse * 1.44269504088896341f : 0.f;     // exp2 domain (see the dq kernel)
      ldsDv[threadIdx.x] = ok ? pdv : 0.f;
    }
    __syncthreads();
    if (qt + QT < a.Lq) prefetch(qt + QT);   // in flight during this tile's MFMAs
    if (k0 >= a.Lk) continue;
#pragma unroll
    for (int sb = 0; sb < 2; ++sb) {
      if (CAUSAL && k0 > qt + sb * 32 + 31 + shift) continue;       // no query of this sub-block sees this wave's keys
      // S = Q K^T and dP = dO V^T for 32 queries x 32 keys: D[i = q][j = key]
      f32x16 s, dp;
#pragma unroll
      for (int e = 0; e < 16; ++e) { s[e] = 0.f; dp[e] = 0.f; }
#pragma unroll
      for (int kd = 0; kd < NKD; ++kd) {
        const e16x8 qa = *reinterpret_cast<const e16x8*>(ldsQ + k_off<HD>(sb * 32 + lk, 2 * kd + half));
        const e16x8 da = *reinterpret_cast<const e16x8*>(ldsD + k_off<HD>(sb * 32 + lk, 2 * kd + half));
        s = E16<e16>::mma32(qa, kf[kd], s);
        dp = E16<e16>::mma32(da, vf[kd], dp);
      }
      e16x8 pf[2], dsf[2];
      // per-query lse / D loaded unconditionally as float4 (a load under the mask predicate
      // cannot be speculated and turned every element into its own branch)
      float lse_r[16], dv_r[16];
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const float4 l4 = *reinterpret_cast<const float4*>(ldsLse + sb * 32 + 8 * g4 + 4 * half);
        const float4 d4 = *reinterpret_cast<const float4*>(ldsDv + sb * 32 + 8 * g4 + 4 * half);
        lse_r[4 * g4] = l4.x; lse_r[4 * g4 + 1] = l4.y; lse_r[4 * g4 + 2] = l4.z; lse_r[4 * g4 + 3] = l4.w;
        dv_r[4 * g4] = d4.x; dv_r[4 * g4 + 1] = d4.y; dv_r[4 * g4 + 2] = d4.z; dv_r[4 * g4 + 3] = d4.w;
      }
      // interior: every key of the wave valid, every query of the sub-block inside the sequence and (causal) at or
      // behind every key of the wave -- no mask arithmetic (wave-uniform)
      bool interior = keys_all_ok && (qt + sb * 32 + 31 < a.Lq);
      if (CAUSAL) interior = interior && (k0 + 31 <= qt + sb * 32 + shift);
      if (interior) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(s[r], c1, -lse_r[r]));
          pf[r >> 3][r & 7] = (e16)p;
          dsf[r >> 3][r & 7] = (e16)(p * (dp[r] - dv_r[r]) * ds_mul);
        }
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int ql = sb * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;   // query row inside the tile
          const int qi = qt + ql;
          bool ok = key_ok & (qi < a.Lq);
          if (CAUSAL) ok = ok & (kg <= qi + shift);
          const float p = __builtin_amdgcn_exp2f(ok ? __builtin_fmaf(s[r], c1, -lse_r[r]) : -1.0e30f);
          pf[r >> 3][r & 7] = (e16)p;
          dsf[r >> 3][r & 7] = (e16)(p * (dp[r] - dv_r[r]) * ds_mul);
        }
      }
#pragma unroll
      for (int d = 0; d < NDB; ++d)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          dva[d] = E16<e16>::mma32(tr_frag_at<HD>(ldsDt, tb[d], sb * 32 + ks * 16), pf[ks], dva[d]);
          dka[d] = E16<e16>::mma32(tr_frag_at<HD>(ldsQt, tb[d], sb * 32 + ks * 16), dsf[ks], dka[d]);
        }
    }
  }
  if (k0 >= a.Lk) return;                // (wave-uniform)
  const long kc_ = min(kg, a.Lk - 1);
  store_row16<NDB>(a.dk + (long)b * a.k_bs + kc_ * a.k_ld + (long)h * HD, dka, st_mul, half, kg < a.Lk);
  store_row16<NDB>(a.dv + (long)b * a.v_bs + kc_ * a.v_ld + (long)h * HD, dva, 1.f, half, kg < a.Lk);
}


// ------------------------------------------------- short sequences: ONE backward kernel --
// Lq == Lk <= 160, head_dim 128 (the LLaMA layers of BASELINE cfg 1-3 and 5: S = 144).  At this length the three
// kernels above are latency chains, not MFMA work (all five products of a (b, h) are ~12 us of matrix-pipe time per
// layer on the whole chip; prep + dq + dkv took 14 + 68 + 109 us): 128-row blocks leave the second block 16 valid
// rows, every workgroup waits for its own K / V or Q / dO tiles, and q, k, v, dO are read from HBM twice.
// Here a workgroup owns one (b, h) from start to finish:
//   phase 1 (lane <-> query, the dq kernel's products): K and V of the whole sequence in LDS; a wave owns the
//     32-row query blocks w and w + 4, keeps their q / dO rows in registers, computes D = rowsum(dO * O) itself
//     (the prep kernel), walks the key blocks its rows can see and stores dQ;
//   phase 2 (lane <-> key, the dkv kernel's products): Q and dO take the place of K and V in LDS; the wave keeps
//     the k / v rows of key blocks w and w + 4 in registers, walks the query blocks that can see them, stores
//     dK and dV.  lse and D of every row pass from phase 1 to phase 2 through LDS.
// ONE image per tensor: the swizzle u_off is conflict-free for the row reads (ds_read_b128, 16 rows x 1 chunk)
// AND for the transposed reads (ds_read_b64_tr_b16, 4 rows x 4 chunks) -- the two-kernel form stages every
// tile twice.  2 x S x 256 B + 2 KiB of LDS: two workgroups per CU up to S = 156; the 32-row blocks are rotated
// over the waves by the workgroup index so that the two heaviest waves (blocks 0 and 4) of co-resident
// workgroups do not share a SIMD.  Rows beyond the sequence are never staged: reads clamp to the last row
// (finite values, masked to zero weight).
template <int HD>
MK_DEV int u_off(int row, int chunk) {
  static_assert(HD == 128, "short-sequence backward: head_dim 128");
  return row * 256 + ((chunk ^ (4 * (row & 3) + ((row >> 2) & 3))) << 4);
}
template <int HD>
MK_DEV e16x8 tr_frag_u(const char* img, int rowbase16, int dblk, int rmax) {
  const int l = threadIdx.x & 63, li = l & 15, half = l >> 5;
  const int col = dblk * 32 + 16 * ((l >> 4) & 1) + 4 * (li & 3);
  e16x8 f;
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int row = min(rowbase16 + 8 * r + 4 * half + (li >> 2), rmax);
    const e16x4 t = E16<e16>::tr_read(img + u_off<HD>(row, col >> 3) + ((col & 7) << 1));
    f[4 * r] = t[0]; f[4 * r + 1] = t[1]; f[4 * r + 2] = t[2]; f[4 * r + 3] = t[3];
  }
  return f;
}
// two [n][HD] tensors -> LDS images (all 256 threads; every chunk of both tensors in flight before the first write)
// (the chunk loop is unrolled in the FRONT END -- a fold over an index sequence -- because `#pragma unroll` over
// the ten-element register arrays ran after the pass that promotes arrays to registers: they were stored to and
// reloaded from scratch)
template <int... I, typename F>
MK_DEV void static_for(std::integer_sequence<int, I...>, F&& f) { (f(std::integral_constant<int, I>{}), ...); }
template <int HD>
MK_DEV void stage_seq2(const e16* s0, long ld0, char* i0, const e16* s1, long ld1, char* i1, int n, int tid) {
  constexpr int CPR = HD / 8, MAXC = (160 * CPR + 255) / 256;
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  u32x4 v0[MAXC], v1[MAXC];
  const int total = n * CPR;
  // chunk indices clamp to the last one (threads past the end re-write it with the same bytes): no per-chunk
  // branches, so the loads stay in one basic block
  static_for(std::make_integer_sequence<int, MAXC>{}, [&](auto ic) {
    constexpr int i = decltype(ic)::value;
    const int c = min(tid + 256 * i, total - 1);
    const int row = c / CPR, ch = c % CPR;
    v0[i] = *reinterpret_cast<const u32x4*>(s0 + (long)row * ld0 + ch * 8);
    v1[i] = *reinterpret_cast<const u32x4*>(s1 + (long)row * ld1 + ch * 8);
  });
  __builtin_amdgcn_sched_barrier(0);
  static_for(std::make_integer_sequence<int, MAXC>{}, [&](auto ic) {
    constexpr int i = decltype(ic)::value;
    const int c = min(tid + 256 * i, total - 1);
    const int row = c / CPR, ch = c % CPR;
    *reinterpret_cast<u32x4*>(i0 + u_off<HD>(row, ch)) = v0[i];
    *reinterpret_cast<u32x4*>(i1 + u_off<HD>(row, ch)) = v1[i];
  });
}

// ---- RoPE inside the short-sequence kernels (round 6) -------------------------------------------------------------
// At S <= 160 every q / k element enters its kernel exactly once per phase (Q rows into registers, K rows into the LDS
// image), so the rotation (modeling.py:76-91) costs no HBM traffic when it is applied on the way in: the separate
// in-place launches read and wrote q | k once more per layer and pass (2 x 151 MB at S = 144, 32 samples: 1.9 ms of
// the cfg-3 step).  The arithmetic is rope_kernel's (elementwise.hip) -- each product and the sum rounded to the
// element type -- so q and k as the products see them are BIT-IDENTICAL to the two-launch form; the backward rotates
// dQ / dK back AFTER rounding them to the element type, which is exactly what the separate inverse launch read.
// Columns c and c + HD / 2 of a head row are partners; cos[c] == cos[c + HD / 2] (only the first half of a table row
// is read, as rope_kernel does).
MK_DEV void rope_pair(e16x8& lo, e16x8& hi, const e16x8 cs, const e16x8 sn, const float sgn) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float x1 = (float)lo[i], x2 = (float)hi[i], c = (float)cs[i], s_ = sgn * (float)sn[i];
    lo[i] = (e16)rnd<e16>(rnd<e16>(x1 * c) + rnd<e16>(-x2 * s_));
    hi[i] = (e16)rnd<e16>(rnd<e16>(x2 * c) + rnd<e16>(x1 * s_));
  }
}
// one row held as MFMA fragments: f[kd] = columns 16 kd + 8 half .. + 8; kd and kd + NKD / 2 are partners
template <int NKD>
MK_DEV void rope_row_frags(e16x8 (&f)[NKD], const e16* rcos, const e16* rsin, int p, int half, float sgn) {
  constexpr int HD = NKD * 16, NH = NKD / 2;
  e16x8 cs[NH], sn[NH];
#pragma unroll
  for (int kd = 0; kd < NH; ++kd) {
    cs[kd] = *reinterpret_cast<const e16x8*>(rcos + (long)p * HD + 16 * kd + 8 * half);
    sn[kd] = *reinterpret_cast<const e16x8*>(rsin + (long)p * HD + 16 * kd + 8 * half);
  }
#pragma unroll
  for (int kd = 0; kd < NH; ++kd) rope_pair(f[kd], f[kd + NH], cs[kd], sn[kd], sgn);
}
// stage_seq2 with tensor 0 rotated on its way into the image: a thread takes the chunk pairs (row, ch), (row, ch +
// CPR / 2) of tensor 0 and plain chunks of tensor 1; the positions are requested first, the cos / sin chunks that
// depend on them last, every load before the first LDS write.
template <int HD>
MK_DEV void stage_seq2_rope(const e16* s0, long ld0, char* i0, const e16* s1, long ld1, char* i1, int n, int tid,
                            const e16* rcos, const e16* rsin, const int32_t* rpos) {
  constexpr int CPR = HD / 8, HPR = CPR / 2, MAXC = (160 * CPR + 255) / 256, MAXP = (160 * HPR + 255) / 256;
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  u32x4 lo[MAXP], hi[MAXP], cs[MAXP], sn[MAXP], v1[MAXC];
  int pp[MAXP];
  const int total = n * CPR, totp = n * HPR;
  static_for(std::make_integer_sequence<int, MAXP>{}, [&](auto ic) {
    constexpr int i = decltype(ic)::value;
    pp[i] = rpos[min(tid + 256 * i, totp - 1) / HPR];
  });
  static_for(std::make_integer_sequence<int, MAXP>{}, [&](auto ic) {
    constexpr int i = decltype(ic)::value;
    const int c = min(tid + 256 * i, totp - 1);
    const int row = c / HPR, ch = c % HPR;
    lo[i] = *reinterpret_cast<const u32x4*>(s0 + (long)row * ld0 + ch * 8);
    hi[i] = *reinterpret_cast<const u32x4*>(s0 + (long)row * ld0 + (ch + HPR) * 8);
  });
  static_for(std::make_integer_sequence<int, MAXC>{}, [&](auto ic) {
    constexpr int i = decltype(ic)::value;
    const int c = min(tid + 256 * i, total - 1);
    v1[i] = *reinterpret_cast<const u32x4*>(s1 + (long)(c / CPR) * ld1 + (c % CPR) * 8);
  });
  static_for(std::make_integer_sequence<int, MAXP>{}, [&](auto ic) {
    constexpr int i = decltype(ic)::value;
    const int ch = min(tid + 256 * i, totp - 1) % HPR;
    cs[i] = *reinterpret_cast<const u32x4*>(rcos + (long)pp[i] * HD + ch * 8);
    sn[i] = *reinterpret_cast<const u32x4*>(rsin + (long)pp[i] * HD + ch * 8);
  });
  __builtin_amdgcn_sched_barrier(0);
  static_for(std::make_integer_sequence<int, MAXC>{}, [&](auto ic) {
    constexpr int i = decltype(ic)::value;
    const int c = min(tid + 256 * i, total - 1);
    *reinterpret_cast<u32x4*>(i1 + u_off<HD>(c / CPR, c % CPR)) = v1[i];
  });
  static_for(std::make_integer_sequence<int, MAXP>{}, [&](auto ic) {
    constexpr int i = decltype(ic)::value;
    const int c = min(tid + 256 * i, totp - 1);
    const int row = c / HPR, ch = c % HPR;
    e16x8 l8 = __builtin_bit_cast(e16x8, lo[i]), h8 = __builtin_bit_cast(e16x8, hi[i]);
    rope_pair(l8, h8, __builtin_bit_cast(e16x8, cs[i]), __builtin_bit_cast(e16x8, sn[i]), 1.f);
    *reinterpret_cast<u32x4*>(i0 + u_off<HD>(row, ch)) = __builtin_bit_cast(u32x4, l8);
    *reinterpret_cast<u32x4*>(i0 + u_off<HD>(row, ch + HPR)) = __builtin_bit_cast(u32x4, h8);
  });
}
// store_row16 for a gradient of a ROTATED row: rounded to the element type first (the value the unfused kernel
// stores), rotated back (sgn = -1) with the 16-byte groups of fragments d and d + NDB / 2, which hold partner columns
template <int NDB>
MK_DEV void store_row16_unrope(e16* row, const f32x16 (&acc)[NDB], float mul, int half, bool ok, const e16* cs_row,
                               const e16* sn_row) {
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  constexpr int NH = NDB / 2;
  e16x8 cs[NH][2], sn[NH][2];
#pragma unroll
  for (int d = 0; d < NH; ++d)
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      cs[d][p] = *reinterpret_cast<const e16x8*>(cs_row + d * 32 + 16 * p + 8 * half);
      sn[d][p] = *reinterpret_cast<const e16x8*>(sn_row + d * 32 + 16 * p + 8 * half);
    }
#pragma unroll
  for (int d = 0; d < NH; ++d)
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      e16x8 o2[2];
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
        const int dd = d + hh * NH;
        e16x4 lo, hi;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          lo[e] = (e16)(acc[dd][8 * p + e] * mul);
          hi[e] = (e16)(acc[dd][8 * p + 4 + e] * mul);
        }
        const uint2 a = __builtin_bit_cast(uint2, lo), b = __builtin_bit_cast(uint2, hi);
        const auto sx = __builtin_amdgcn_permlane32_swap(a.x, b.x, false, false);
        const auto sy = __builtin_amdgcn_permlane32_swap(a.y, b.y, false, false);
        u32x4 o;
        o[0] = sx[0]; o[1] = sy[0]; o[2] = sx[1]; o[3] = sy[1];
        o2[hh] = __builtin_bit_cast(e16x8, o);
      }
      rope_pair(o2[0], o2[1], cs[d][p], sn[d][p], -1.f);
      if (ok) {
        *reinterpret_cast<u32x4*>(row + d * 32 + 16 * p + 8 * half) = __builtin_bit_cast(u32x4, o2[0]);
        *reinterpret_cast<u32x4*>(row + (d + NH) * 32 + 16 * p + 8 * half) = __builtin_bit_cast(u32x4, o2[1]);
      }
    }
}

// The forward of the same short sequences: one workgroup per (b, h), K and V of the whole sequence staged once
// (u_off images), a wave owns the 32-row query blocks of the backward's phase 1 and walks the 32-key blocks
// its rows can see in ascending order.  The arithmetic of a row -- exp2 domain, lazy rescale per row, the order of
// the key blocks -- is flash_fwd_kernel's, so o and lse are BIT-IDENTICAL to it (tests/test_kernels_gpu.py checks
// that); what changes is the schedule: 1024 workgroups with one staging step each instead of 2048 (the second of
// every (b, h) holding 16 rows at S = 144) with a barrier pair per 64-key tile.
template <int HD, bool CAUSAL, bool ROPE>
__global__ __launch_bounds__(256, 2) void flash_fwd_short_kernel(FlashArgs a) {
  constexpr int NKD = HD / 16, NDB = HD / 32;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int S = a.Lk;                    // == a.Lq
  char* imgK = lds;
  char* imgV = lds + S * HD * 2;
  int* ldsM = reinterpret_cast<int*>(lds + 2 * S * HD * 2);
  const int b = blockIdx.y, h = blockIdx.x;
  const int l = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int half = l >> 5, lq = l & 31;
  const int lw = (w + h + b) & 3;
  const int nblk = (S + 31) >> 5;
  const e16* Q = a.q + (long)b * a.q_bs + (long)h * HD;
  const e16* K = a.k + (long)b * a.k_bs + (long)h * HD;
  const e16* V = a.v + (long)b * a.v_bs + (long)h * HD;
  const int32_t* km = a.kmask ? a.kmask + (long)b * a.Lk : nullptr;
  const float c2 = a.scale * 1.4426950408889634f;
  if constexpr (ROPE)
    stage_seq2_rope<HD>(K, a.k_ld, imgK, V, a.v_ld, imgV, S, (int)threadIdx.x, a.rcos, a.rsin, a.rpos + (long)b * S);
  else
    stage_seq2<HD>(K, a.k_ld, imgK, V, a.v_ld, imgV, S, (int)threadIdx.x);
  if (threadIdx.x < 160) {
    const int kg = threadIdx.x;
    ldsM[kg] = (kg < S) && (!km || km[min(kg, S - 1)] != 0);
  }
  __syncthreads();
#pragma unroll 1
  for (int t = 0; t < 2; ++t) {
    int blk;
    if (t == 0) blk = CAUSAL ? nblk - 1 - lw : lw;
    else blk = nblk == 5 ? (CAUSAL ? (lw == 2 ? 0 : -1) : (lw == 0 ? 4 : -1)) : -1;
    if (blk < 0 || blk >= nblk) continue;
    const int q0 = blk * 32, qg = q0 + lq;
    e16x8 qf[NKD];
#pragma unroll
    for (int kd = 0; kd < NKD; ++kd)
      qf[kd] = ld8_or_zero(Q + (long)min(qg, S - 1) * a.q_ld + 16 * kd + 8 * half, qg < S);
    if constexpr (ROPE)                  // (rows past the sequence are zero and stay zero)
      rope_row_frags<NKD>(qf, a.rcos, a.rsin, a.rpos[(long)b * S + min(qg, S - 1)], half, 1.f);
    f32x16 oacc[NDB];
#pragma unroll
    for (int d = 0; d < NDB; ++d)
#pragma unroll
      for (int e = 0; e < 16; ++e) oacc[d][e] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;
    const int jend = CAUSAL ? blk + 1 : nblk;
#pragma unroll 1
    for (int j = 0; j < jend; ++j) {
      const int kb = j * 32;
      const int krow = min(kb + lq, S - 1);
      // every key of the block valid and visible to every row of this wave: no mask arithmetic (wave-uniform)
      bool interior = (__builtin_amdgcn_ballot_w64(ldsM[kb + lq] != 0) == ~0ull);
      if (CAUSAL) interior = interior && (kb + 31 <= q0);
      f32x16 s;
#pragma unroll
      for (int e = 0; e < 16; ++e) s[e] = 0.f;
#pragma unroll
      for (int kd = 0; kd < NKD; ++kd)
        s = E16<e16>::mma32(*reinterpret_cast<const e16x8*>(imgK + u_off<HD>(krow, 2 * kd + half)), qf[kd], s);
      uint32_t okbits = 0xffffu;
      if (!interior) {
        okbits = 0;
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
          const int4 m4 = *reinterpret_cast<const int4*>(ldsM + kb + 8 * g4 + 4 * half);
          const int mk[4] = {m4.x, m4.y, m4.z, m4.w};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int kg = kb + e + 8 * g4 + 4 * half;
            bool ok = mk[e] != 0;
            if (CAUSAL) ok = ok && (kg <= qg);
            okbits |= (ok ? 1u : 0u) << (4 * g4 + e);
          }
        }
      }
      e16x8 pf[2];
      softmax_block<NDB>(s, interior, okbits, c2, m_run, l_run, oacc, pf);
#pragma unroll
      for (int d = 0; d < NDB; ++d)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
          oacc[d] = E16<e16>::mma32(tr_frag_u<HD>(imgV, kb + ks * 16, d, S - 1), pf[ks], oacc[d]);
    }
    {
      const float inv = l_run > 0.f ? 1.f / l_run : 0.f;
      store_row16<NDB>(a.o + (long)b * a.o_bs + (long)min(qg, S - 1) * a.o_ld + (long)h * HD, oacc, inv, half, qg < S);
    }
    if (qg < S) {
      if (a.lse && half == 0)
        a.lse[((long)b * a.H + h) * a.Lq + qg] =
            (l_run > 0.f) ? (m_run + __log2f(l_run)) * 0.6931471805599453f : -INFINITY;
    }
  }
}

// ROPE: 0 = q, k, dq, dk as they are; 1 = q, k arrive unrotated (rotated on every load), dq / dk rotated back at the
// store; 2 = q, k arrive ROTATED (mk_rope ran before the forward), only dq / dk are rotated back at the store
template <int HD, bool CAUSAL, int ROPE>
__global__ __launch_bounds__(256, 2) void flash_bwd_short_kernel(FlashBwdArgs a) {
  constexpr int NKD = HD / 16, NDB = HD / 32;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int S = a.Lk;                    // == a.Lq
  char* img0 = lds;                      // K, then Q
  char* img1 = lds + S * HD * 2;         // V, then dO
  float* ldsLse = reinterpret_cast<float*>(lds + 2 * S * HD * 2);
  float* ldsDv = ldsLse + 160;
  int* ldsM = reinterpret_cast<int*>(ldsDv + 160);
  const int b = blockIdx.y, h = blockIdx.x;
  const int l = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int half = l >> 5, ll = l & 31;
  const int lw = (w + h + b) & 3;        // this wave's first 32-row block (rotated per workgroup)
  const int nblk = (S + 31) >> 5;        // <= 5
  const e16* Q = a.q + (long)b * a.q_bs + (long)h * HD;
  const e16* dO = a.dout + (long)b * a.o_bs + (long)h * HD;
  const e16* O = a.o + (long)b * a.o_bs + (long)h * HD;
  const e16* K = a.k + (long)b * a.k_bs + (long)h * HD;
  const e16* V = a.v + (long)b * a.v_bs + (long)h * HD;
  const int32_t* km = a.kmask ? a.kmask + (long)b * a.Lk : nullptr;
  const long rowbase = ((long)b * a.H + h) * a.Lq;
  const float c1 = a.scale * 1.44269504088896341f;
  // bf16: the `scale` of dS multiplies the fp32 accumulators at the store; fp16: dS is scaled before it is rounded
  const float ds_mul = E16<e16>::narrow_exponent ? a.scale : 1.0f;
  const float st_mul = E16<e16>::narrow_exponent ? 1.0f : a.scale;

  // ---------------- phase 1: dQ (lane <-> query) ----------------
  if constexpr (ROPE == 1)
    stage_seq2_rope<HD>(K, a.k_ld, img0, V, a.v_ld, img1, S, (int)threadIdx.x, a.rcos, a.rsin, a.rpos + (long)b * S);
  else
    stage_seq2<HD>(K, a.k_ld, img0, V, a.v_ld, img1, S, (int)threadIdx.x);
  if (threadIdx.x < 160) {
    const int kg = threadIdx.x;
    ldsM[kg] = (kg < S) && (!km || km[min(kg, S - 1)] != 0);
  }
  __syncthreads();
  // blocks -> waves.  Causal work per block is 1..5 block pairs (query block i sees i + 1 key blocks, key block
  // j is seen by nblk - j query blocks): {4}, {3}, {2, 0}, {1} in phase 1 and {0}, {1}, {2, 4}, {3} in phase 2
  // are 5 / 4 / 4 / 2 pairs per wave (w, w + 4 would be 6 / 2 / 3 / 4).
#pragma unroll 1
  for (int t = 0; t < 2; ++t) {
    int blk;
    if (t == 0) blk = CAUSAL ? nblk - 1 - lw : lw;
    else blk = nblk == 5 ? (CAUSAL ? (lw == 2 ? 0 : -1) : (lw == 0 ? 4 : -1)) : -1;
    if (blk < 0 || blk >= nblk) continue;
    const int q0 = blk * 32, qg = q0 + ll, qc = min(qg, S - 1);
    e16x8 qf[NKD], dof[NKD];
    float dv_ = 0.f;
#pragma unroll
    for (int kd = 0; kd < NKD; ++kd) {
      qf[kd] = ld8_or_zero(Q + (long)qc * a.q_ld + 16 * kd + 8 * half, qg < S);
      dof[kd] = ld8_or_zero(dO + (long)qc * a.o_ld + 16 * kd + 8 * half, qg < S);
      const e16x8 of = ld8_or_zero(O + (long)qc * a.o_ld + 16 * kd + 8 * half, qg < S);
#pragma unroll
      for (int e = 0; e < 8; ++e) dv_ += (float)dof[kd][e] * (float)of[e];
    }
    int qpos = 0;
    if constexpr (ROPE != 0) qpos = a.rpos[(long)b * S + qc];
    if constexpr (ROPE == 1) rope_row_frags<NKD>(qf, a.rcos, a.rsin, qpos, half, 1.f);
    dv_ += __shfl_xor(dv_, 32, 64);      // the partner half holds the other 8 of every 16 columns
                                         // (v_permlane32_swap here costs the non-causal instantiation 8 spilled registers)
    // exp2 domain: p = 2^(s * c1 - lse2); masked entries get -inf BEFORE the exponential (valid ones are <= 0
    // up to rounding: lse >= the row maximum); the `scale` of dS = p (dP - D) scale multiplies the accumulators
    // once at the store instead of every element
    const float lse = a.lse[rowbase + qc] * 1.44269504088896341f;
    if (half == 0) { ldsLse[qg] = qg < S ? lse : 0.f; ldsDv[qg] = qg < S ? dv_ : 0.f; }
    f32x16 acc[NDB];
#pragma unroll
    for (int d = 0; d < NDB; ++d)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[d][e] = 0.f;
    const int jend = CAUSAL ? blk + 1 : nblk;
#pragma unroll 1
    for (int j = 0; j < jend; ++j) {
      const int kb = j * 32;
      const int krow = min(kb + ll, S - 1);
      f32x16 s, dp;
#pragma unroll
      for (int e = 0; e < 16; ++e) { s[e] = 0.f; dp[e] = 0.f; }
#pragma unroll
      for (int kd = 0; kd < NKD; ++kd) {
        const e16x8 kf = *reinterpret_cast<const e16x8*>(img0 + u_off<HD>(krow, 2 * kd + half));
        const e16x8 vf = *reinterpret_cast<const e16x8*>(img1 + u_off<HD>(krow, 2 * kd + half));
        s = E16<e16>::mma32(kf, qf[kd], s);
        dp = E16<e16>::mma32(vf, dof[kd], dp);
      }
      e16x8 dsf[2];
      int mk[16];
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const int4 m4 = *reinterpret_cast<const int4*>(ldsM + kb + 8 * g4 + 4 * half);
        mk[4 * g4] = m4.x; mk[4 * g4 + 1] = m4.y; mk[4 * g4 + 2] = m4.z; mk[4 * g4 + 3] = m4.w;
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int kg = kb + (r & 3) + 8 * (r >> 2) + 4 * half;
        bool ok = mk[r] != 0;
        if (CAUSAL) ok = ok && (kg <= qg);
        const float p = __builtin_amdgcn_exp2f(ok ? s[r] * c1 - lse : -1.0e30f);
        dsf[r >> 3][r & 7] = (e16)(p * (dp[r] - dv_) * ds_mul);
      }
#pragma unroll
      for (int d = 0; d < NDB; ++d)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
          acc[d] = E16<e16>::mma32(tr_frag_u<HD>(img0, kb + ks * 16, d, S - 1), dsf[ks], acc[d]);
    }
    if constexpr (ROPE != 0) {
      asm volatile("" : "+v"(qpos));     // (the table addresses are formed HERE, not carried through the key loop)
      store_row16_unrope<NDB>(a.dq + (long)b * a.q_bs + (long)qc * a.q_ld + (long)h * HD, acc, st_mul, half, qg < S,
                              a.rcos + (long)qpos * HD, a.rsin + (long)qpos * HD);
    }
    else
      store_row16<NDB>(a.dq + (long)b * a.q_bs + (long)qc * a.q_ld + (long)h * HD, acc, st_mul, half, qg < S);
  }
  __syncthreads();                       // every wave is done with K / V; lse and D of all rows are in LDS

  // ---------------- phase 2: dK, dV (lane <-> key) ----------------
  // two passes over the query blocks, dV first and dK second (S is recomputed: 8 MFMAs and 16 exponentials per
  // 32 x 32 block): both accumulators beside k, v, S and dP are 280 registers, the two-workgroups-per-CU
  // budget is 256 -- as ONE pass the compiler spilled 64 of them to scratch.
  // (the thread index is laundered: otherwise the compiler keeps the first staging's chunk offsets alive across
  // phase 1 -- in scratch)
  int tid2 = threadIdx.x;
  asm volatile("" : "+v"(tid2));
  if constexpr (ROPE == 1)
    stage_seq2_rope<HD>(Q, a.q_ld, img0, dO, a.o_ld, img1, S, tid2, a.rcos, a.rsin, a.rpos + (long)b * S);
  else
    stage_seq2<HD>(Q, a.q_ld, img0, dO, a.o_ld, img1, S, tid2);
  __syncthreads();
#pragma unroll 1
  for (int t = 0; t < 2; ++t) {
    int blk;
    if (t == 0) blk = lw;
    else blk = nblk == 5 ? (CAUSAL ? (lw == 2 ? 4 : -1) : (lw == 0 ? 4 : -1)) : -1;
    if (blk < 0 || blk >= nblk) continue;
    const int k0 = blk * 32, kg = k0 + ll, kc = min(kg, S - 1);
    e16x8 kf[NKD];                       // B operand: lane holds K[kg][16 kd + 8 half .. + 8]
#pragma unroll
    for (int kd = 0; kd < NKD; ++kd) kf[kd] = ld8_or_zero(K + (long)kc * a.k_ld + 16 * kd + 8 * half, kg < S);
    int kpos = 0;
    if constexpr (ROPE != 0) kpos = a.rpos[(long)b * S + kc];
    if constexpr (ROPE == 1) rope_row_frags<NKD>(kf, a.rcos, a.rsin, kpos, half, 1.f);
    const bool key_ok = ldsM[min(kg, 159)] != 0;
    e16* DK = a.dk + (long)b * a.k_bs + (long)kc * a.k_ld + (long)h * HD;
    e16* DV = a.dv + (long)b * a.v_bs + (long)kc * a.v_ld + (long)h * HD;
    {
      f32x16 dva[NDB];
#pragma unroll
      for (int d = 0; d < NDB; ++d)
#pragma unroll
        for (int e = 0; e < 16; ++e) dva[d][e] = 0.f;
#pragma unroll 1
      for (int i = CAUSAL ? blk : 0; i < nblk; ++i) {
        const int qb = i * 32;
        const int qrow = min(qb + ll, S - 1);
        f32x16 s;
#pragma unroll
        for (int e = 0; e < 16; ++e) s[e] = 0.f;
#pragma unroll
        for (int kd = 0; kd < NKD; ++kd)
          s = E16<e16>::mma32(*reinterpret_cast<const e16x8*>(img0 + u_off<HD>(qrow, 2 * kd + half)), kf[kd], s);
        e16x8 pf[2];
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
          const float4 l4 = *reinterpret_cast<const float4*>(ldsLse + qb + 8 * g4 + 4 * half);
          const float lr[4] = {l4.x, l4.y, l4.z, l4.w};
#pragma unroll
          for (int r4 = 0; r4 < 4; ++r4) {
            const int r = 4 * g4 + r4;
            const int qi = qb + r4 + 8 * g4 + 4 * half;
            bool ok = key_ok & (qi < S);
            if (CAUSAL) ok = ok & (kg <= qi);
            pf[r >> 3][r & 7] = (e16)__builtin_amdgcn_exp2f(ok ? s[r] * c1 - lr[r4] : -1.0e30f);
          }
        }
#pragma unroll
        for (int d = 0; d < NDB; ++d)
#pragma unroll
          for (int ks = 0; ks < 2; ++ks)
            dva[d] = E16<e16>::mma32(tr_frag_u<HD>(img1, qb + ks * 16, d, S - 1), pf[ks], dva[d]);
      }
      store_row16<NDB>(DV, dva, 1.f, half, kg < S);
    }
    {
      e16x8 vf[NKD];
#pragma unroll
      for (int kd = 0; kd < NKD; ++kd) vf[kd] = ld8_or_zero(V + (long)kc * a.v_ld + 16 * kd + 8 * half, kg < S);
      f32x16 dka[NDB];
#pragma unroll
      for (int d = 0; d < NDB; ++d)
#pragma unroll
        for (int e = 0; e < 16; ++e) dka[d][e] = 0.f;
#pragma unroll 1
      for (int i = CAUSAL ? blk : 0; i < nblk; ++i) {
        const int qb = i * 32;
        const int qrow = min(qb + ll, S - 1);
        f32x16 s, dp;
#pragma unroll
        for (int e = 0; e < 16; ++e) { s[e] = 0.f; dp[e] = 0.f; }
#pragma unroll
        for (int kd = 0; kd < NKD; ++kd) {
          const e16x8 qa = *reinterpret_cast<const e16x8*>(img0 + u_off<HD>(qrow, 2 * kd + half));
          const e16x8 da = *reinterpret_cast<const e16x8*>(img1 + u_off<HD>(qrow, 2 * kd + half));
          s = E16<e16>::mma32(qa, kf[kd], s);
          dp = E16<e16>::mma32(da, vf[kd], dp);
        }
        e16x8 dsf[2];
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
          const float4 l4 = *reinterpret_cast<const float4*>(ldsLse + qb + 8 * g4 + 4 * half);
          const float4 d4 = *reinterpret_cast<const float4*>(ldsDv + qb + 8 * g4 + 4 * half);
          const float lr[4] = {l4.x, l4.y, l4.z, l4.w}, dr[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
          for (int r4 = 0; r4 < 4; ++r4) {
            const int r = 4 * g4 + r4;
            const int qi = qb + r4 + 8 * g4 + 4 * half;
            bool ok = key_ok & (qi < S);
            if (CAUSAL) ok = ok & (kg <= qi);
            const float p = __builtin_amdgcn_exp2f(ok ? s[r] * c1 - lr[r4] : -1.0e30f);
            dsf[r >> 3][r & 7] = (e16)(p * (dp[r] - dr[r4]) * ds_mul);
          }
        }
#pragma unroll
        for (int d = 0; d < NDB; ++d)
#pragma unroll
          for (int ks = 0; ks < 2; ++ks)
            dka[d] = E16<e16>::mma32(tr_frag_u<HD>(img0, qb + ks * 16, d, S - 1), dsf[ks], dka[d]);
      }
      if constexpr (ROPE != 0) {
        asm volatile("" : "+v"(kpos));
        store_row16_unrope<NDB>(DK, dka, st_mul, half, kg < S, a.rcos + (long)kpos * HD, a.rsin + (long)kpos * HD);
      }
      else
        store_row16<NDB>(DK, dka, st_mul, half, kg < S);
    }
  }
}

int flash_attn_bwd_impl(const void* q, const void* k, const void* v, const void* o,
                                 const void* dout, const float* lse, float* dvec, void* dq,
                                 void* dk, void* dv, const int32_t* kmask, int32_t B, int32_t H,
                                 int32_t Lq, int32_t Lk, int32_t hd, int64_t q_ld, int64_t q_bs,
                                 int64_t k_ld, int64_t k_bs, int64_t v_ld, int64_t v_bs,
                                 int64_t o_ld, int64_t o_bs, float scale, int32_t causal,
                                 int32_t dtype, void* stream, const void* rope_cos = nullptr,
                                 const void* rope_sin = nullptr, const int32_t* rope_pos = nullptr,
                                 int32_t qk_rotated = 0) {
  if (!q || !k || !v || !o || !dout || !lse || !dvec || !dq || !dk || !dv || B <= 0 || H <= 0 ||
      Lq <= 0 || Lk <= 0)
    return MK_ERR_BAD_ARG;
  const bool rope = rope_cos || rope_sin || rope_pos;
  if (rope && (!rope_cos || !rope_sin || !rope_pos)) return MK_ERR_BAD_ARG;
  if (rope && ((reinterpret_cast<uintptr_t>(rope_cos) | reinterpret_cast<uintptr_t>(rope_sin)) & 15))
    return MK_ERR_UNSUPPORTED;
  if (dtype != E16<e16>::dtype || (hd != 64 && hd != 128)) return MK_ERR_UNSUPPORTED;
  const uintptr_t al = reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k) |
                       reinterpret_cast<uintptr_t>(v) | reinterpret_cast<uintptr_t>(o) |
                       reinterpret_cast<uintptr_t>(dout) | reinterpret_cast<uintptr_t>(dq) |
                       reinterpret_cast<uintptr_t>(dk) | reinterpret_cast<uintptr_t>(dv);
  if ((al & 15) || (q_ld % 8) || (k_ld % 8) || (v_ld % 8) || (o_ld % 8) || (q_bs % 8) ||
      (k_bs % 8) || (v_bs % 8) || (o_bs % 8))
    return MK_ERR_UNSUPPORTED;
  FlashBwdArgs a;
  a.q = (const e16*)q; a.k = (const e16*)k; a.v = (const e16*)v; a.o = (const e16*)o;
  a.dout = (const e16*)dout; a.dq = (e16*)dq; a.dk = (e16*)dk; a.dv = (e16*)dv;
  a.lse = lse; a.dvec = dvec; a.kmask = kmask;
  a.B = B; a.H = H; a.Lq = Lq; a.Lk = Lk;
  a.q_ld = q_ld; a.q_bs = q_bs; a.k_ld = k_ld; a.k_bs = k_bs; a.v_ld = v_ld; a.v_bs = v_bs;
  a.o_ld = o_ld; a.o_bs = o_bs;
  a.scale = scale;
  a.rcos = (const e16*)rope_cos; a.rsin = (const e16*)rope_sin; a.rpos = rope_pos;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const long rows = (long)B * H * Lq;
  dim3 gq(H, B, mk_cdiv(Lq, 128)), gk(H, B, mk_cdiv(Lk, 128)), block(256);
  // backward: dV = P^T dO, dP = dO V^T, dQ = dS K, dK = dS^T Q (4 products) + the recomputed
  // QK^T: counted as the 4 algorithmic ones = 2x the forward
  const double pairs = causal ? ((double)Lq * Lk - 0.5 * (double)min(Lq, Lk) * (min(Lq, Lk) - 1)) : (double)Lq * Lk;
  const int prof = mkp::begin(st, 2, 8.0 * pairs * hd * B * H, Lq, Lk, hd, B * H, causal, 0);
  static const bool dq_sync = getenv("MK_ATTN_DQ_ASYNC") == nullptr;
  static const bool no_short = getenv("MK_ATTN_NO_SHORT_BWD") != nullptr;
  if (hd == 128 && Lq == Lk && Lk <= 160 && !no_short) {
    // one workgroup per (b, h) runs prep + dq + dkv (flash_bwd_short_kernel)
    const int lds_bytes = 2 * Lk * 128 * 2 + 3 * 160 * 4;
    static bool attr_done = false;
    if (!attr_done) {
      const int max_lds = 2 * 160 * 128 * 2 + 3 * 160 * 4;
#define MK_BS_ATTR(CZ, RP)                                                                                  \
  (hipFuncSetAttribute(reinterpret_cast<const void*>(&flash_bwd_short_kernel<128, CZ, RP>),                \
                       hipFuncAttributeMaxDynamicSharedMemorySize, max_lds) != hipSuccess)
      if (MK_BS_ATTR(true, 0) || MK_BS_ATTR(false, 0) || MK_BS_ATTR(true, 1) || MK_BS_ATTR(false, 1) ||
          MK_BS_ATTR(true, 2) || MK_BS_ATTR(false, 2))
        return MK_ERR_LAUNCH;
#undef MK_BS_ATTR
      attr_done = true;
    }
    if (rope && qk_rotated) {
      if (causal) MK_LAUNCH((flash_bwd_short_kernel<128, true, 2>), dim3(H, B), block, lds_bytes, st, a);
      else MK_LAUNCH((flash_bwd_short_kernel<128, false, 2>), dim3(H, B), block, lds_bytes, st, a);
    } else if (rope) {
      if (causal) MK_LAUNCH((flash_bwd_short_kernel<128, true, 1>), dim3(H, B), block, lds_bytes, st, a);
      else MK_LAUNCH((flash_bwd_short_kernel<128, false, 1>), dim3(H, B), block, lds_bytes, st, a);
    } else {
      if (causal) MK_LAUNCH((flash_bwd_short_kernel<128, true, 0>), dim3(H, B), block, lds_bytes, st, a);
      else MK_LAUNCH((flash_bwd_short_kernel<128, false, 0>), dim3(H, B), block, lds_bytes, st, a);
    }
    mkp::end(prof, st);
    return mk_check_launch();
  }
  if (rope) return MK_ERR_UNSUPPORTED;     // the rotation lives in the short-sequence kernel only
#define MK_FB(HDV, CZ)                                                                         \
  do {                                                                                         \
    MK_LAUNCH((flash_bwd_prep_kernel<HDV>), dim3((unsigned)((rows * (HDV / 8) + 255) / 256)), block, 0, st, a); \
    if (dq_sync) MK_LAUNCH((flash_bwd_dq_kernel<HDV, CZ, false>), gq, block, 0, st, a);          \
    else MK_LAUNCH((flash_bwd_dq_kernel<HDV, CZ, true>), gq, block, 0, st, a);                  \
    MK_LAUNCH((flash_bwd_dkv_kernel<HDV, CZ>), gk, block, 0, st, a);                           \
  } while (0)
  if (hd == 128) { if (causal) MK_FB(128, true); else MK_FB(128, false); }
  else { if (causal) MK_FB(64, true); else MK_FB(64, false); }
#undef MK_FB
  mkp::end(prof, st);
  return mk_check_launch();
}
}  // namespace MK_E16_NS
}  // namespace
