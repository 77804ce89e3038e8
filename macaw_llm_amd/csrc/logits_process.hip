// Logits processors of generate(): repetition_penalty, no_repeat_ngram_size, min_new_tokens (HF's
// RepetitionPenaltyLogitsProcessor -> NoRepeatNGramLogitsProcessor -> MinNewTokensLengthLogitsProcessor), applied in
// place to the step's logits immediately before the emit, in one launch; the rule is written down in
// include/macaw_hip.h and restated in tests/logits_proc_ref.py.
//
// One workgroup of 1024 threads per row.  The history h = prompt ++ generated is read from device memory and its
// generated length from a device counter (the output column that mk_decode_emit advances), so a captured step replays.
// Only the columns the history names are touched, never the V columns of the row:
//   penalty   thread t takes history entries t, t + 1024, ...; a V-bit bitmap in LDS marks the ids seen, and the thread
//             whose atomic OR sets an id's bit is the one that rewrites that column: each distinct id exactly once,
//             whatever the duplicates and the arrival order (the new value depends on the old one only)
//   n-gram    thread t compares windows t, t + 1024, ... with the history's last n - 1 ids; a match stores -inf (stores
//             of the same value to the same column commute)
//   min new   one thread stores -inf at eos
// with a barrier between the three, which orders their stores to a common column.
#include "common.h"
#include "../../include/macaw_hip.h"
#include <math.h>

namespace {

constexpr int LNT = 1024;                       // threads per row
constexpr int LP_MAX_V = 1 << 18;               // the bitmap of the distinct ids: V bits <= 32 KiB of LDS

struct History {
  const int64_t* prompt;                        // row b's prompt ids, or null
  const int64_t* gen;                           // row b's generated ids
  int Lp, L;                                    // prompt ids, all ids
  MK_DEV int64_t at(int i) const { return i < Lp ? prompt[i] : gen[i - Lp]; }
};

template <typename T>
__global__ __launch_bounds__(LNT) void logits_process_kernel(T* logits, long ld, int V, const int64_t* prompt, long p_ld,
                                                             int P, const int32_t* p_len, const int64_t* out,
                                                             long out_ld, int n_max, const int32_t* n_dev, int n_add,
                                                             float theta, int ngram, int min_new, long eos) {
  __shared__ uint32_t seen[LP_MAX_V / 32];
  const int b = blockIdx.x, tid = threadIdx.x;
  T* row = logits + (long)b * ld;
  long nl = (long)(n_dev ? *n_dev : 0) + n_add;
  const int n = (int)(nl < 0 ? 0 : nl > n_max ? n_max : nl);      // generated tokens, inside the output matrix
  History h;
  h.prompt = prompt ? prompt + (long)b * p_ld : nullptr;
  h.gen = out + (long)b * out_ld;
  const int pl = prompt ? p_len[b] : 0;
  h.Lp = pl < 0 ? 0 : pl > P ? P : pl;
  h.L = h.Lp + n;

  if (theta != 1.f) {
    const int words = (V + 31) >> 5;
    for (int w = tid; w < words; w += LNT) seen[w] = 0u;
    __syncthreads();
    for (int i = tid; i < h.L; i += LNT) {
      const int64_t c = h.at(i);
      if (c < 0 || c >= V) continue;            // an id outside the vocabulary names no column
      const uint32_t bit = 1u << (c & 31);
      if (atomicOr(&seen[c >> 5], bit) & bit) continue;           // penalised by the thread that came first
      const float x = to_f32<T>(row[c]);
      row[c] = from_f32<T>(x < 0.f ? x * theta : __fdiv_rn(x, theta));
    }
    __syncthreads();
  }
  if (ngram > 0 && h.L >= ngram) {              // windows i in [0, L - n + 1); the suffix starts at L - n + 1
    const int s0 = h.L - ngram + 1;
    for (int i = tid; i < s0; i += LNT) {
      bool same = true;
      for (int j = 0; j < ngram - 1 && same; ++j) same = h.at(i + j) == h.at(s0 + j);
      if (!same) continue;
      const int64_t c = h.at(i + ngram - 1);
      if (c >= 0 && c < V) row[c] = from_f32<T>(-INFINITY);
    }
    __syncthreads();
  }
  if (tid == 0 && n < min_new && eos >= 0 && eos < V) row[eos] = from_f32<T>(-INFINITY);
}

}  // namespace

extern "C" int mk_logits_process(void* logits, int64_t ld, int32_t V, int32_t B, const int64_t* prompt, int64_t p_ld,
                                 int32_t P, const int32_t* p_len, const int64_t* out, int64_t out_ld, int32_t n_max,
                                 const int32_t* n_dev, int32_t n_add, float repetition_penalty,
                                 int32_t no_repeat_ngram_size, int32_t min_new_tokens, int64_t eos, int32_t dtype,
                                 void* stream) {
  if (!logits || !out || V <= 0 || B <= 0 || ld < V || n_max < 0 || out_ld < n_max || (prompt && (!p_len || P < 0 || p_ld < P)) ||
      !isfinite(repetition_penalty) || repetition_penalty <= 0.f || no_repeat_ngram_size < 0 || min_new_tokens < 0)
    return MK_ERR_BAD_ARG;
  if (dtype != MK_BF16 && dtype != MK_F16 && dtype != MK_F32) return MK_ERR_UNSUPPORTED;
  if (V > LP_MAX_V) return MK_ERR_UNSUPPORTED;
  if (repetition_penalty == 1.f && no_repeat_ngram_size == 0 && (min_new_tokens == 0 || eos < 0)) return MK_OK;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (dtype == MK_BF16)
    MK_LAUNCH((logits_process_kernel<bf16>), dim3(B), dim3(LNT), 0, st, (bf16*)logits, (long)ld, V, prompt, (long)p_ld, P,
              p_len, out, (long)out_ld, n_max, n_dev, n_add, repetition_penalty, no_repeat_ngram_size, min_new_tokens,
              (long)eos);
  else if (dtype == MK_F16)
    MK_LAUNCH((logits_process_kernel<_Float16>), dim3(B), dim3(LNT), 0, st, (_Float16*)logits, (long)ld, V, prompt,
              (long)p_ld, P, p_len, out, (long)out_ld, n_max, n_dev, n_add, repetition_penalty, no_repeat_ngram_size,
              min_new_tokens, (long)eos);
  else
    MK_LAUNCH((logits_process_kernel<float>), dim3(B), dim3(LNT), 0, st, (float*)logits, (long)ld, V, prompt, (long)p_ld,
              P, p_len, out, (long)out_ld, n_max, n_dev, n_add, repetition_penalty, no_repeat_ngram_size, min_new_tokens,
              (long)eos);
  return mk_check_launch();
}
