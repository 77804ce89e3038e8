// Per-request penalties of generate(): frequency_penalty, presence_penalty (OpenAI's and vLLM's additive penalties on the
// GENERATED tokens) and logit_bias, applied in place to the step's logits behind mk_logits_process and in front of
// mk_seq_ban, mk_grammar_mask and every selection, in one launch; the rule is written down in include/macaw_hip.h and
// restated in tests/penalties_ref.py.
//
// One workgroup of 1024 threads per row; f and p are read per row from device arrays, the bias list per row from a CSR
// table.  The generated ids are read from device memory and their count from a device counter (the output column that
// mk_decode_emit advances), so a captured step replays.  Only the columns the generated ids and the bias list name are
// touched, each exactly once:
//   count   the ids are staged in LDS as int32 (-1 for an id outside the vocabulary), PEN_STAGE at a time.  Thread t
//           takes ids t, t + 1024, ...; a V-bit bitmap in LDS marks the ids seen, and the thread whose atomic OR sets an
//           id's bit owns that column: it counts the id over the staged ids (every lane of a wave reads the same four
//           staged ids: an LDS broadcast), looks the column up in the row's sorted bias ids (binary search) and rewrites
//           it once.  The count is a sum of integers: whichever thread owns a column, it computes the same value.
//   bias    thread t takes bias entries t, t + 1024, ...; an entry whose bit is set in the bitmap was folded into its
//           owner's rewrite and is skipped, the others are written here.  The two passes write disjoint columns.
// A history longer than PEN_STAGE is staged in rounds, the owners carrying their count from round to round.
#include "common.h"
#include "../../include/macaw_hip.h"
#include <math.h>

namespace {

constexpr int PNT = 1024;                       // threads per row
constexpr int PEN_MAX_V = 1 << 18;              // the bitmap of the distinct ids: V bits <= 32 KiB of LDS
constexpr int PEN_STAGE = 2048;                 // generated ids staged at a time: 8 KiB
constexpr int PEN_BIAS = 1024;                  // bias ids of a row searched in LDS (a longer list: in global memory)
constexpr int PEN_MAX_N = 1 << 24;              // float(count) is exact

// the index of c in the ascending, distinct ids[0, nb), or -1
MK_DEV int bias_find(const int32_t* ids, int nb, int c) {
  int lo = 0, hi = nb;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (ids[mid] < c) lo = mid + 1; else hi = mid;
  }
  return lo < nb && ids[lo] == c ? lo : -1;
}

template <typename T>
__global__ __launch_bounds__(PNT) void logits_penalize_kernel(T* logits, long ld, int V, const int64_t* out, long out_ld,
                                                              int n_max, const int32_t* n_dev, int n_add,
                                                              const float* freq, const float* pres,
                                                              const int32_t* bias_off, const int32_t* bias_ids,
                                                              const float* bias_val) {
#pragma clang fp contract(off)                  // every fp32 operation below is rounded by itself: no fused multiply-add
  __shared__ uint32_t seen[PEN_MAX_V / 32];
  __shared__ __attribute__((aligned(16))) int32_t ids[PEN_STAGE];
  __shared__ int32_t bid_s[PEN_BIAS];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float f = freq ? freq[b] : 0.f, p = pres ? pres[b] : 0.f;
  const int o0 = bias_off ? bias_off[b] : 0, o1 = bias_off ? bias_off[b + 1] : 0;
  const int nb = o1 > o0 && o0 >= 0 ? o1 - o0 : 0;
  if (f == 0.f && p == 0.f && nb == 0) return;  // (uniform: the row keeps its bits)
  T* row = logits + (long)b * ld;
  const int64_t* gen = out + (long)b * out_ld;
  long nl = (long)(n_dev ? *n_dev : 0) + n_add;
  const int n = (int)(nl < 0 ? 0 : nl > n_max ? n_max : nl);      // generated tokens, inside the output matrix
  const bool pen = (f != 0.f || p != 0.f) && n > 0;

  const int32_t* bid = bias_ids + o0;           // the row's bias ids: from LDS when they fit
  if (nb > 0 && nb <= PEN_BIAS) {
    for (int k = tid; k < nb; k += PNT) bid_s[k] = bias_ids[o0 + k];
    bid = bid_s;
  }
  if (pen) {
    const int words = (V + 31) >> 5;
    for (int w = tid; w < words; w += PNT) seen[w] = 0u;
  }
  __syncthreads();

  if (pen) {
    const int rounds = (n + PEN_STAGE - 1) / PEN_STAGE;
    for (int base = 0; base < n; base += PNT) {                   // (uniform trip counts: the barriers below are reached by all)
      const int i = base + tid;
      const int64_t c64 = i < n ? gen[i] : -1;
      const int c = c64 >= 0 && c64 < V ? (int)c64 : -1;          // an id outside the vocabulary names no column
      bool own = false;
      if (c >= 0) {
        const uint32_t bit = 1u << (c & 31);
        own = !(atomicOr(&seen[c >> 5], bit) & bit);              // counted and rewritten by the thread that came first
      }
      int cnt = 0;
      for (int r = 0; r < rounds; ++r) {
        const int r0 = r * PEN_STAGE, m = n - r0 < PEN_STAGE ? n - r0 : PEN_STAGE, m4 = (m + 3) & ~3;
        if (rounds > 1 || base == 0) {          // one round: staged once, for every base
          if (rounds > 1) __syncthreads();      // the readers of the round before are through
          for (int j = tid; j < m4; j += PNT) {
            const int64_t g = j < m ? gen[r0 + j] : -1;
            ids[j] = g >= 0 && g < V ? (int)g : -1;
          }
          __syncthreads();
        }
        if (own) {
          const int4* q = reinterpret_cast<const int4*>(ids);
          for (int j = 0; j < (m4 >> 2); ++j) {
            const int4 v = q[j];
            cnt += (v.x == c) + (v.y == c) + (v.z == c) + (v.w == c);
          }
        }
      }
      if (own) {
        float x = to_f32<T>(row[c]);
        const int k = nb ? bias_find(bid, nb, c) : -1;
        if (k >= 0) x = x + bias_val[o0 + k];   // (contract(off) above: the product below is rounded by itself)
        const float fc = f * (float)cnt;
        x = x - fc;
        x = x - p;
        row[c] = from_f32<T>(x);
      }
    }
    __syncthreads();                            // the bitmap is complete
  }
  for (int k = tid; k < nb; k += PNT) {
    const int c = bid[k];
    if (c < 0 || c >= V) continue;              // (outside the contract; never outside the row)
    if (pen && (seen[c >> 5] >> (c & 31) & 1u)) continue;         // folded into its owner's rewrite above
    row[c] = from_f32<T>(to_f32<T>(row[c]) + bias_val[o0 + k]);
  }
}

}  // namespace

extern "C" int mk_logits_penalize(void* logits, int64_t ld, int32_t V, int32_t B, const int64_t* out, int64_t out_ld,
                                  int32_t n_max, const int32_t* n_dev, int32_t n_add, const float* frequency,
                                  const float* presence, const int32_t* bias_off, const int32_t* bias_ids,
                                  const float* bias_val, int32_t dtype, void* stream) {
  if (!logits || !out || V <= 0 || B <= 0 || ld < V || n_max < 0 || n_max > PEN_MAX_N || out_ld < n_max ||
      (bias_off && (!bias_ids || !bias_val)))
    return MK_ERR_BAD_ARG;
  if (dtype != MK_BF16 && dtype != MK_F16 && dtype != MK_F32) return MK_ERR_UNSUPPORTED;
  if (V > PEN_MAX_V) return MK_ERR_UNSUPPORTED;
  if (!frequency && !presence && !bias_off) return MK_OK;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (dtype == MK_BF16)
    MK_LAUNCH((logits_penalize_kernel<bf16>), dim3(B), dim3(PNT), 0, st, (bf16*)logits, (long)ld, V, out, (long)out_ld,
              n_max, n_dev, n_add, frequency, presence, bias_off, bias_ids, bias_val);
  else if (dtype == MK_F16)
    MK_LAUNCH((logits_penalize_kernel<_Float16>), dim3(B), dim3(PNT), 0, st, (_Float16*)logits, (long)ld, V, out,
              (long)out_ld, n_max, n_dev, n_add, frequency, presence, bias_off, bias_ids, bias_val);
  else
    MK_LAUNCH((logits_penalize_kernel<float>), dim3(B), dim3(PNT), 0, st, (float*)logits, (long)ld, V, out, (long)out_ld,
              n_max, n_dev, n_add, frequency, presence, bias_off, bias_ids, bias_val);
  return mk_check_launch();
}
