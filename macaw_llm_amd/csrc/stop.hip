// Token-sequence matching of generate(): bad_words_ids (HF's NoBadWordsLogitsProcessor) and stop_sequences (the stop
// lists of TGI / vLLM, HF's stop_strings at token level).  Both compare the tail of a sample's history with a table of
// token sequences that lives on the device; the rule is written down in include/macaw_hip.h and restated in
// tests/stop_ref.py.
//
// The table: seq_ids int64 [total], the sequences back to back, and seq_off int32 [n_seq + 1], sequence s being
// seq_ids[seq_off[s] .. seq_off[s + 1]).
//   mk_seq_ban     one workgroup of 256 threads per row of logits, in front of the selection: thread t takes sequences
//                  t, t + 256, ...; a sequence whose first m - 1 ids are the history's last m - 1 stores -inf into the
//                  column its last id names (stores of the same value to the same column commute)
//   mk_stop_match  one workgroup of 256 threads per sample, behind the emit: a sequence of m ids that equals the row's
//                  last m generated ids stores 1 into the sample's done byte (likewise)
// The history and its generated length are read from device memory as in logits_process.hip, so a captured step replays.
#include "common.h"
#include "../../include/macaw_hip.h"
#include <math.h>

namespace {

constexpr int SNT = 256;                        // threads per row
constexpr int SEQ_MAX_N = 1 << 16;              // sequences per table
constexpr int SEQ_MAX_LEN = 64;                 // ids per sequence: a longer (or empty) entry of the table matches nothing

MK_DEV int clamp_count(const int32_t* n_dev, int n_add, int n_max) {
  const long nl = (long)(n_dev ? *n_dev : 0) + n_add;
  return (int)(nl < 0 ? 0 : nl > n_max ? n_max : nl);                 // generated tokens, inside the output matrix
}

template <typename T>
__global__ __launch_bounds__(SNT) void seq_ban_kernel(T* logits, long ld, int V, const int64_t* prompt, long p_ld, int P,
                                                      const int32_t* p_len, const int64_t* out, long out_ld, int n_max,
                                                      const int32_t* n_dev, int n_add, const int64_t* seq_ids,
                                                      const int32_t* seq_off, int n_seq) {
  const int b = blockIdx.x;
  T* row = logits + (long)b * ld;
  const int n = clamp_count(n_dev, n_add, n_max);
  const int64_t* hp = prompt ? prompt + (long)b * p_ld : nullptr;     // h = prompt ++ generated
  const int64_t* hg = out + (long)b * out_ld;
  const int pl = prompt ? p_len[b] : 0;
  const int Lp = pl < 0 ? 0 : pl > P ? P : pl;
  const int L = Lp + n;
  for (int s = threadIdx.x; s < n_seq; s += SNT) {
    const int o = seq_off[s], m = seq_off[s + 1] - o;
    if (m < 1 || m > SEQ_MAX_LEN || m - 1 > L) continue;              // the prefix is longer than the history
    const int64_t* q = seq_ids + o;
    const int t0 = L - (m - 1);                                       // the history's last m - 1 ids
    bool same = true;
    for (int j = 0; j < m - 1 && same; ++j) {
      const int i = t0 + j;
      same = (i < Lp ? hp[i] : hg[i - Lp]) == q[j];
    }
    if (!same) continue;
    const int64_t c = q[m - 1];
    if (c >= 0 && c < V) row[c] = from_f32<T>(-INFINITY);             // an id outside the vocabulary names no column
  }
}

__global__ __launch_bounds__(SNT) void stop_match_kernel(const int64_t* out, long out_ld, int n_max, const int32_t* n_dev,
                                                         int n_add, const int64_t* seq_ids, const int32_t* seq_off,
                                                         int n_seq, uint8_t* done) {
  const int b = blockIdx.x;
  // A finished row is not examined.  Another wave of this workgroup may have stored its match already: the only value
  // ever stored is 1, so a thread that sees it and returns loses nothing.
  if (done[b]) return;
  const int n = clamp_count(n_dev, n_add, n_max);
  const int64_t* g = out + (long)b * out_ld;
  for (int s = threadIdx.x; s < n_seq; s += SNT) {
    const int o = seq_off[s], m = seq_off[s + 1] - o;
    if (m < 1 || m > SEQ_MAX_LEN || m > n) continue;                  // the window never reaches into the prompt
    const int64_t* q = seq_ids + o;
    const int64_t* tail = g + (n - m);
    bool same = true;
    for (int j = 0; j < m && same; ++j) same = tail[j] == q[j];
    if (same) done[b] = 1;
  }
}

}  // namespace

extern "C" int mk_seq_ban(void* logits, int64_t ld, int32_t V, int32_t B, const int64_t* prompt, int64_t p_ld, int32_t P,
                          const int32_t* p_len, const int64_t* out, int64_t out_ld, int32_t n_max, const int32_t* n_dev,
                          int32_t n_add, const int64_t* seq_ids, const int32_t* seq_off, int32_t n_seq, int32_t dtype,
                          void* stream) {
  if (!logits || !out || !seq_ids || !seq_off || V <= 0 || B <= 0 || n_seq <= 0 || ld < V || n_max < 0 || out_ld < n_max ||
      (prompt && (!p_len || P < 0 || p_ld < P)))
    return MK_ERR_BAD_ARG;
  if (dtype != MK_BF16 && dtype != MK_F16 && dtype != MK_F32) return MK_ERR_UNSUPPORTED;
  if (n_seq > SEQ_MAX_N) return MK_ERR_UNSUPPORTED;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (dtype == MK_BF16)
    MK_LAUNCH((seq_ban_kernel<bf16>), dim3(B), dim3(SNT), 0, st, (bf16*)logits, (long)ld, V, prompt, (long)p_ld, P, p_len,
              out, (long)out_ld, n_max, n_dev, n_add, seq_ids, seq_off, n_seq);
  else if (dtype == MK_F16)
    MK_LAUNCH((seq_ban_kernel<_Float16>), dim3(B), dim3(SNT), 0, st, (_Float16*)logits, (long)ld, V, prompt, (long)p_ld, P,
              p_len, out, (long)out_ld, n_max, n_dev, n_add, seq_ids, seq_off, n_seq);
  else
    MK_LAUNCH((seq_ban_kernel<float>), dim3(B), dim3(SNT), 0, st, (float*)logits, (long)ld, V, prompt, (long)p_ld, P,
              p_len, out, (long)out_ld, n_max, n_dev, n_add, seq_ids, seq_off, n_seq);
  return mk_check_launch();
}

extern "C" int mk_stop_match(const int64_t* out, int64_t out_ld, int32_t n_max, int32_t B, const int32_t* n_dev,
                             int32_t n_add, const int64_t* seq_ids, const int32_t* seq_off, int32_t n_seq, void* done,
                             void* stream) {
  if (!out || !seq_ids || !seq_off || !done || B <= 0 || n_seq <= 0 || n_max < 0 || out_ld < n_max) return MK_ERR_BAD_ARG;
  if (n_seq > SEQ_MAX_N) return MK_ERR_UNSUPPORTED;
  MK_LAUNCH(stop_match_kernel, dim3(B), dim3(SNT), 0, reinterpret_cast<hipStream_t>(stream), out, (long)out_ld, n_max,
            n_dev, n_add, seq_ids, seq_off, n_seq, (uint8_t*)done);
  return mk_check_launch();
}
