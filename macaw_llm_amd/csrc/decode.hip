// Greedy-decode kernels whose per-step position comes from DEVICE memory, so that one decode step
// is a fixed launch sequence and can be captured once in a hipGraph and replayed per token
// (modeling.py:190-195,954-960: the reference appends to the KV cache with torch.cat and re-launches
// the whole eager step from Python for every token).
//
//   mk_kv_append    cache[b][*t_dev][0:cols] = src[b][0:cols]   (post-RoPE keys | values of the new token)
//   mk_decode_attn  one query row per (sample, head) against the first *t_dev + t_add cached keys
//   mk_decode_step_attn  RoPE(q, k_new) + append(k_new, v_new) + that attention in one launch
//   mk_kv_quant_append / mk_decode_step_attn_kv8  the prefill's cache write and the step's attention block over an
//                   e4m3 KV cache (bytes + one fp32 scale per head and position: decode_kv8_impl.inc)
//   mk_decode_step_attn_var / mk_decode_step_attn_kv8_var  the same steps at a position PER SAMPLE, *t_dev + t_off[b]
//   mk_decode_step_attn_beam  the 16-bit step for (sample, beam) rows over a [B][K][t_max][2D] cache read through a beam
//                   indirection table: the prompt's keys once per sample, no cache row ever copied (beam.hip: the emit)
//   mk_decode_step_attn_shared  the 16-bit step for n rows per sample over a prompt cache stored once per sample and a
//                        tail cache per row (parallel sampling): the plain step body per row, a tile of rows per workgroup
//   mk_score_attn   F teacher-forced rows per option over that layout (score()): a RoPE-and-append kernel for every live
//                   row, then the plain step body per row without its append, at a position per row
//   mk_decode_step_attn_multi  the 16-bit step for Q rows per sample at positions pos[b] ... pos[b] + Q - 1 (the verify
//                   pass of prompt-lookup decoding, spec.hip): the plain step body, one workgroup per (head, sample, row)
//   mk_kv_append_rows / mk_kv_quant_append_rows  the prefill's cache write of a padded batch: source row j of sample
//                   b goes to cache row slot[b][j], masked rows (slot < 0) are not written (a compacted, ragged cache)
//
// The fused training / prefill attention (attention.hip) works on 128-row query tiles: at Lq = 1
// it would spend 127 of 128 MFMA rows on padding and, more to the point here, takes its key count
// as a launch argument.
#include "common.h"
#include "../../include/macaw_hip.h"

namespace {

__global__ __launch_bounds__(256) void kv_append_kernel(const char* src, char* dst, long row_bytes,
                                                        long s_src, long s_dst, long ld_dst,
                                                        const int32_t* t_dev, int t_max) {
  const int t = min(max(*t_dev, 0), t_max - 1);
  src += (long)blockIdx.y * s_src;
  dst += (long)blockIdx.y * s_dst + (long)t * ld_dst;
  for (long i = ((long)blockIdx.x * 256 + threadIdx.x) * 16; i < row_bytes; i += (long)gridDim.x * 256 * 16)
    *reinterpret_cast<uint4*>(dst + i) = *reinterpret_cast<const uint4*>(src + i);
}

// cache[b][slot[b][j]] = [k[b][j] | v[b][j]] for slot in [0, t_max): one 16-byte piece per thread, pieces of a
// destination row adjacent (the row is one contiguous 2 * d_bytes run); bytes only, any 16-bit element type.
__global__ __launch_bounds__(256) void kv_append_rows_kernel(const char* k, const char* v, long ld_bytes,
                                                             long in_bs_bytes, char* cache, const int32_t* slot,
                                                             int Sn, int t_max, int d_pieces) {
  const int b = blockIdx.y;
  const long per_row = 2L * d_pieces;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)Sn * per_row) return;
  const int j = (int)(idx / per_row), c = (int)(idx % per_row);
  const int r = slot[(long)b * Sn + j];
  if (r < 0 || r >= t_max) return;
  const char* src = (c < d_pieces ? k + (long)c * 16 : v + (long)(c - d_pieces) * 16) + (long)b * in_bs_bytes +
                    (long)j * ld_bytes;
  char* dst = cache + ((long)b * t_max + r) * per_row * 16 + (long)c * 16;
  *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(src);
}

template <typename T>
__global__ __launch_bounds__(1024) void decode_emit_kernel(const T* logits, long ld, int V, long pad,
                                                           long eos, int64_t* tok, unsigned char* done,
                                                           int64_t* out, long out_ld, int32_t* state) {
  __shared__ float bv[16];
  __shared__ int bi[16];
  const int b = blockIdx.x;
  const T* xr = logits + (long)b * ld;
  float best = -INFINITY;
  int idx = 0x7fffffff;
  for (int c0 = threadIdx.x; c0 < V; c0 += 1024 * 8) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = c0 + j * 1024;
      v[j] = c < V ? (float)xr[c] : -INFINITY;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {                                 // torch.argmax order (common.h)
      const int c = c0 + j * 1024;
      if (c < V && mk_argmax_better(v[j], c, best, idx)) { best = v[j]; idx = c; }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(idx, o, 64);
    if (mk_argmax_better(ov, oi, best, idx)) { best = ov; idx = oi; }
  }
  if ((threadIdx.x & 63) == 0) { bv[threadIdx.x >> 6] = best; bi[threadIdx.x >> 6] = idx; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 16; ++w)
      if (mk_argmax_better(bv[w], bi[w], best, idx)) { best = bv[w]; idx = bi[w]; }
    const int col = state[1];
    const long nxt = done[b] ? pad : (long)idx;
    out[(long)b * out_ld + col] = nxt;
    if (nxt == eos) done[b] = 1;
    tok[b] = nxt;
    __threadfence();
    const int old = __hip_atomic_fetch_add(state + 2, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (old == (int)gridDim.x - 1) {          // every sample has read state[1]: advance the step
      state[0] += 1;
      state[1] = col + 1;
      state[2] = 0;
    }
  }
}

}  // namespace

// the 16-bit kernels: written once over an element type, instantiated for bf16 and f16 (common.h E16<>)
#define MK_E16_T bf16
#define MK_E16_NS e_bf16
#include "decode_impl.inc"
#include "decode_kv8_impl.inc"
#undef MK_E16_T
#undef MK_E16_NS
#define MK_E16_T _Float16
#define MK_E16_NS e_f16
#define decode_attn_kernel decode_attn_f16_kernel
#define decode_step_attn_kernel decode_step_attn_f16_kernel
#define decode_step_attn_multi_kernel decode_step_attn_multi_f16_kernel
#define decode_step_attn4_kernel decode_step_attn4_f16_kernel
#define decode_step_attn_shared_kernel decode_step_attn_shared_f16_kernel
#define score_append_kernel score_append_f16_kernel
#define score_attn_kernel score_attn_f16_kernel
#define kv_quant_append_kernel kv_quant_append_f16_kernel
#define decode_step_attn_kv8_kernel decode_step_attn_kv8_f16_kernel
#include "decode_impl.inc"
#include "decode_kv8_impl.inc"
#undef decode_attn_kernel
#undef decode_step_attn_kernel
#undef decode_step_attn_multi_kernel
#undef decode_step_attn4_kernel
#undef decode_step_attn_shared_kernel
#undef score_append_kernel
#undef score_attn_kernel
#undef kv_quant_append_kernel
#undef decode_step_attn_kv8_kernel
#undef MK_E16_T
#undef MK_E16_NS

extern "C" int mk_decode_step_attn(const void* q, const void* k_new, const void* v_new, int64_t in_bs,
                                   const void* cos_t, const void* sin_t, void* k_cache, void* v_cache,
                                   int64_t kv_ld, int64_t kv_bs, void* o, int64_t o_bs,
                                   const int32_t* t_dev, int32_t t_max, int32_t B, int32_t H,
                                   int32_t hd, float scale, int32_t dtype, void* stream) {
  if (dtype == MK_F16) return e_f16::decode_step_attn_impl(q, k_new, v_new, in_bs, cos_t, sin_t, k_cache, v_cache, kv_ld, kv_bs, o, o_bs, t_dev, t_max, B, H, hd, scale, dtype, stream);
  return e_bf16::decode_step_attn_impl(q, k_new, v_new, in_bs, cos_t, sin_t, k_cache, v_cache, kv_ld, kv_bs, o, o_bs, t_dev, t_max, B, H, hd, scale, dtype, stream);
}

extern "C" int mk_decode_step_attn_var(const void* q, const void* k_new, const void* v_new, int64_t in_bs,
                                       const void* cos_t, const void* sin_t, void* k_cache, void* v_cache,
                                       int64_t kv_ld, int64_t kv_bs, void* o, int64_t o_bs,
                                       const int32_t* t_dev, const int32_t* t_off, int32_t t_max, int32_t B,
                                       int32_t H, int32_t hd, float scale, int32_t dtype, void* stream) {
  if (!t_off) return MK_ERR_BAD_ARG;
  if (reinterpret_cast<uintptr_t>(t_off) & 3) return MK_ERR_UNSUPPORTED;
  if (dtype == MK_F16) return e_f16::decode_step_attn_impl(q, k_new, v_new, in_bs, cos_t, sin_t, k_cache, v_cache, kv_ld, kv_bs, o, o_bs, t_dev, t_max, B, H, hd, scale, dtype, stream, true, t_off);
  return e_bf16::decode_step_attn_impl(q, k_new, v_new, in_bs, cos_t, sin_t, k_cache, v_cache, kv_ld, kv_bs, o, o_bs, t_dev, t_max, B, H, hd, scale, dtype, stream, true, t_off);
}

extern "C" int mk_decode_step_attn_beam(const void* q, const void* k_new, const void* v_new, int64_t in_bs,
                                        const void* cos_t, const void* sin_t, void* k_cache, void* v_cache,
                                        int64_t kv_ld, int64_t kv_bs, void* o, int64_t o_bs, const int32_t* t_dev,
                                        const int32_t* ind, int32_t n_ind, int32_t S0, int32_t t_max, int32_t B,
                                        int32_t K, int32_t H, int32_t hd, float scale, int32_t dtype, void* stream) {
  if (dtype == MK_F16) return e_f16::decode_step_attn_beam_impl(q, k_new, v_new, in_bs, cos_t, sin_t, k_cache, v_cache, kv_ld, kv_bs, o, o_bs, t_dev, ind, n_ind, S0, t_max, B, K, H, hd, scale, dtype, stream);
  return e_bf16::decode_step_attn_beam_impl(q, k_new, v_new, in_bs, cos_t, sin_t, k_cache, v_cache, kv_ld, kv_bs, o, o_bs, t_dev, ind, n_ind, S0, t_max, B, K, H, hd, scale, dtype, stream);
}

extern "C" int mk_decode_step_attn_multi(const void* q, const void* k_new, const void* v_new, int64_t in_bs,
                                         const void* cos_t, const void* sin_t, void* k_cache, void* v_cache,
                                         int64_t kv_ld, int64_t kv_bs, void* o, int64_t o_bs, const int32_t* pos,
                                         int32_t t_max, int32_t B, int32_t Q, int32_t H, int32_t hd, float scale,
                                         int32_t dtype, void* stream) {
  if (dtype == MK_F16) return e_f16::decode_step_attn_multi_impl(q, k_new, v_new, in_bs, cos_t, sin_t, k_cache, v_cache, kv_ld, kv_bs, o, o_bs, pos, t_max, B, Q, H, hd, scale, dtype, stream);
  return e_bf16::decode_step_attn_multi_impl(q, k_new, v_new, in_bs, cos_t, sin_t, k_cache, v_cache, kv_ld, kv_bs, o, o_bs, pos, t_max, B, Q, H, hd, scale, dtype, stream);
}

extern "C" int mk_decode_step_attn_shared(const void* q, const void* k_new, const void* v_new, int64_t in_bs,
                                          const void* cos_t, const void* sin_t, const void* kp, const void* vp,
                                          int64_t p_ld, int64_t p_bs, void* kt, void* vt, int64_t t_ld, int64_t t_bs,
                                          void* o, int64_t o_bs, const int32_t* t_dev, const int32_t* t_off, int32_t S0,
                                          int32_t Tn, int32_t B, int32_t n, int32_t H, int32_t hd, float scale,
                                          int32_t dtype, void* stream) {
  if (dtype == MK_F16) return e_f16::decode_step_attn_shared_impl(q, k_new, v_new, in_bs, cos_t, sin_t, kp, vp, p_ld, p_bs, kt, vt, t_ld, t_bs, o, o_bs, t_dev, t_off, S0, Tn, B, n, H, hd, scale, dtype, stream);
  return e_bf16::decode_step_attn_shared_impl(q, k_new, v_new, in_bs, cos_t, sin_t, kp, vp, p_ld, p_bs, kt, vt, t_ld, t_bs, o, o_bs, t_dev, t_off, S0, Tn, B, n, H, hd, scale, dtype, stream);
}

extern "C" int mk_score_attn(const void* q, const void* k_new, const void* v_new, int64_t in_bs, const void* cos_t,
                             const void* sin_t, const void* kp, const void* vp, int64_t p_ld, int64_t p_bs, void* kt,
                             void* vt, int64_t t_ld, int64_t t_bs, void* o, int64_t o_bs, const int32_t* len,
                             const int32_t* t_off, int32_t S0, int32_t F, int32_t B, int32_t n, int32_t H, int32_t hd,
                             float scale, int32_t dtype, void* stream) {
  if (dtype == MK_F16) return e_f16::score_attn_impl(q, k_new, v_new, in_bs, cos_t, sin_t, kp, vp, p_ld, p_bs, kt, vt, t_ld, t_bs, o, o_bs, len, t_off, S0, F, B, n, H, hd, scale, dtype, stream);
  return e_bf16::score_attn_impl(q, k_new, v_new, in_bs, cos_t, sin_t, kp, vp, p_ld, p_bs, kt, vt, t_ld, t_bs, o, o_bs, len, t_off, S0, F, B, n, H, hd, scale, dtype, stream);
}

extern "C" int mk_decode_step_attn_kv8_var(const void* q, const void* k_new, const void* v_new, int64_t in_bs,
                                           const void* cos_t, const void* sin_t, void* cache, float* scales, void* o,
                                           int64_t o_bs, const int32_t* t_dev, const int32_t* t_off, int32_t t_max,
                                           int32_t B, int32_t H, int32_t hd, float scale, int32_t dtype,
                                           void* stream) {
  if (!t_off) return MK_ERR_BAD_ARG;
  if (reinterpret_cast<uintptr_t>(t_off) & 3) return MK_ERR_UNSUPPORTED;
  if (dtype == MK_F16) return e_f16::decode_step_attn_kv8_impl(q, k_new, v_new, in_bs, cos_t, sin_t, cache, scales, o, o_bs, t_dev, t_max, B, H, hd, scale, dtype, stream, true, t_off);
  return e_bf16::decode_step_attn_kv8_impl(q, k_new, v_new, in_bs, cos_t, sin_t, cache, scales, o, o_bs, t_dev, t_max, B, H, hd, scale, dtype, stream, true, t_off);
}

extern "C" int mk_kv_quant_append_rows(const void* k, const void* v, int64_t ld, int64_t in_bs, void* cache,
                                       float* scales, const int32_t* slot, int32_t Sn, int32_t t_max, int32_t B,
                                       int32_t H, int32_t hd, int32_t dtype, void* stream) {
  if (!slot) return MK_ERR_BAD_ARG;
  if (reinterpret_cast<uintptr_t>(slot) & 3) return MK_ERR_UNSUPPORTED;
  if (dtype == MK_F16) return e_f16::kv_quant_append_impl(k, v, ld, in_bs, cache, scales, 0, Sn, t_max, B, H, hd, dtype, stream, true, slot);
  return e_bf16::kv_quant_append_impl(k, v, ld, in_bs, cache, scales, 0, Sn, t_max, B, H, hd, dtype, stream, true, slot);
}

extern "C" int mk_kv_append_rows(const void* k, const void* v, int64_t ld, int64_t in_bs, void* cache,
                                 const int32_t* slot, int32_t Sn, int32_t t_max, int32_t B, int32_t H, int32_t hd,
                                 int32_t dtype, void* stream) {
  if (!k || !v || !cache || !slot || B <= 0 || H <= 0 || Sn <= 0 || t_max <= 0) return MK_ERR_BAD_ARG;
  if ((dtype != MK_BF16 && dtype != MK_F16) || (hd != 16 && hd != 32 && hd != 64 && hd != 128)) return MK_ERR_UNSUPPORTED;
  const uintptr_t al = reinterpret_cast<uintptr_t>(k) | reinterpret_cast<uintptr_t>(v) |
                       reinterpret_cast<uintptr_t>(cache);
  const int64_t D = (int64_t)H * hd;
  if ((al & 15) || (reinterpret_cast<uintptr_t>(slot) & 3) || (ld % 8) || (in_bs % 8) || ld < D ||
      (B > 1 && in_bs < D))
    return MK_ERR_UNSUPPORTED;
  const int d_pieces = (int)(D / 8);                     // 16-byte pieces of a key (or value) row
  const long n = (long)Sn * 2 * d_pieces;
  dim3 grid((unsigned)mk_cdiv(n, 256), B), block(256);
  MK_LAUNCH(kv_append_rows_kernel, grid, block, 0, reinterpret_cast<hipStream_t>(stream), (const char*)k,
            (const char*)v, (long)ld * 2, (long)in_bs * 2, (char*)cache, slot, Sn, t_max, d_pieces);
  return mk_check_launch();
}

extern "C" int mk_kv_quant_append(const void* k, const void* v, int64_t ld, int64_t in_bs, void* cache, float* scales,
                                  int32_t t0, int32_t Sn, int32_t t_max, int32_t B, int32_t H, int32_t hd,
                                  int32_t dtype, void* stream) {
  if (dtype == MK_F16) return e_f16::kv_quant_append_impl(k, v, ld, in_bs, cache, scales, t0, Sn, t_max, B, H, hd, dtype, stream);
  return e_bf16::kv_quant_append_impl(k, v, ld, in_bs, cache, scales, t0, Sn, t_max, B, H, hd, dtype, stream);
}

extern "C" int mk_decode_step_attn_kv8(const void* q, const void* k_new, const void* v_new, int64_t in_bs,
                                       const void* cos_t, const void* sin_t, void* cache, float* scales, void* o,
                                       int64_t o_bs, const int32_t* t_dev, int32_t t_max, int32_t B, int32_t H,
                                       int32_t hd, float scale, int32_t dtype, void* stream) {
  if (dtype == MK_F16) return e_f16::decode_step_attn_kv8_impl(q, k_new, v_new, in_bs, cos_t, sin_t, cache, scales, o, o_bs, t_dev, t_max, B, H, hd, scale, dtype, stream);
  return e_bf16::decode_step_attn_kv8_impl(q, k_new, v_new, in_bs, cos_t, sin_t, cache, scales, o, o_bs, t_dev, t_max, B, H, hd, scale, dtype, stream);
}

extern "C" int mk_decode_attn(const void* q, const void* k, const void* v, void* o,
                              const int32_t* t_dev, int32_t t_add, int32_t t_max, int32_t B,
                              int32_t H, int32_t hd, int64_t q_bs, int64_t k_ld, int64_t k_bs,
                              int64_t v_ld, int64_t v_bs, int64_t o_bs, float scale, int32_t dtype,
                              void* stream) {
  if (dtype == MK_F16) return e_f16::decode_attn_impl(q, k, v, o, t_dev, t_add, t_max, B, H, hd, q_bs, k_ld, k_bs, v_ld, v_bs, o_bs, scale, dtype, stream);
  return e_bf16::decode_attn_impl(q, k, v, o, t_dev, t_add, t_max, B, H, hd, q_bs, k_ld, k_bs, v_ld, v_bs, o_bs, scale, dtype, stream);
}

extern "C" int mk_decode_emit(const void* logits, int64_t ld, int32_t V, int32_t B, int64_t pad,
                              int64_t eos, int64_t* tok, void* done, int64_t* out, int64_t out_ld,
                              int32_t* state, int32_t dtype, void* stream) {
  if (!logits || !tok || !done || !out || !state || V <= 0 || B <= 0 || ld < V) return MK_ERR_BAD_ARG;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (dtype == MK_BF16)
    MK_LAUNCH((decode_emit_kernel<bf16>), dim3(B), dim3(1024), 0, st, (const bf16*)logits, (long)ld, V,
              (long)pad, (long)eos, tok, (unsigned char*)done, out, (long)out_ld, state);
  else if (dtype == MK_F16)
    MK_LAUNCH((decode_emit_kernel<_Float16>), dim3(B), dim3(1024), 0, st, (const _Float16*)logits, (long)ld, V,
              (long)pad, (long)eos, tok, (unsigned char*)done, out, (long)out_ld, state);
  else if (dtype == MK_F32)
    MK_LAUNCH((decode_emit_kernel<float>), dim3(B), dim3(1024), 0, st, (const float*)logits, (long)ld, V,
              (long)pad, (long)eos, tok, (unsigned char*)done, out, (long)out_ld, state);
  else return MK_ERR_UNSUPPORTED;
  return mk_check_launch();
}


extern "C" int mk_kv_append(const void* src, void* cache, int32_t cols, int32_t batch, int64_t s_src,
                            int64_t s_cache, int64_t ld_cache, const int32_t* t_dev, int32_t t_max,
                            int32_t elem_size, void* stream) {
  if (!src || !cache || !t_dev || cols <= 0 || batch <= 0 || t_max <= 0) return MK_ERR_BAD_ARG;
  if (elem_size != 2 && elem_size != 4) return MK_ERR_UNSUPPORTED;
  const long es = elem_size, row_bytes = (long)cols * es;
  if (((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(cache)) & 15) || (row_bytes % 16) ||
      ((s_src * es) % 16) || ((s_cache * es) % 16) || ((ld_cache * es) % 16))
    return MK_ERR_UNSUPPORTED;
  dim3 grid((unsigned)mk_cdiv(row_bytes, 256L * 16), batch), block(256);
  MK_LAUNCH(kv_append_kernel, grid, block, 0, reinterpret_cast<hipStream_t>(stream), (const char*)src,
            (char*)cache, row_bytes, s_src * es, s_cache * es, ld_cache * es, t_dev, t_max);
  return mk_check_launch();
}

