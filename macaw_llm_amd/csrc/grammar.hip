// Grammar-constrained decoding of generate(grammar=): a deterministic automaton over token ids that lives in device
// memory.  The rule is written down in include/macaw_hip.h ("Grammar-constrained decoding") and restated in
// tests/grammar_ref.py.
//
// The table: next int32 [n_states][V] at row pitch ld_next (next[s][t]: the state behind token t in state s, -1 where t
// is not allowed) and flags uint8 [n_states] (bit 0 accepting, bit 1 terminal); per sample state int32 [B] (-1 an
// unconstrained row, -2 a broken one).
//   mk_grammar_mask     in front of the selection: a grid of (chunks of 1024 columns, rows), 256 threads per workgroup,
//                       every thread four columns of its row of the table (one 16-byte load where the pitch allows it);
//                       a column whose entry is negative stores -inf into the logits, nothing else is written.  The
//                       kernel is latency, not traffic: 2.2 - 2.4 us at 1, 8 and 32 rows of 32007 columns.  Variants
//                       with more columns per workgroup, down to one workgroup per row, were measured slower and are
//                       not in the tree (profiles/decode_grammar_generate.txt records them)
//   mk_grammar_advance  behind the emit: one thread per sample moves its state along the token just emitted and sets
//                       the sample's done byte and end column where the new state is terminal (or the row broke)
//   mk_grammar_build    one thread per (state, token): the byte automaton char_next [S][256] walked over the token's bytes
// States and counts are read from device memory, as in stop.hip, so a captured step replays.  Plain loads and stores only.
#include "common.h"
#include "../../include/macaw_hip.h"
#include <math.h>

namespace {

constexpr int GNT = 256;                        // threads per workgroup
constexpr int GCHUNK = GNT * 4;                 // columns per workgroup of the mask: one 16-byte load per thread

typedef int int4v __attribute__((ext_vector_type(4)));

MK_DEV int clamp_count(const int32_t* n_dev, int n_add, int n_max) {
  const long nl = (long)(n_dev ? *n_dev : 0) + n_add;
  return (int)(nl < 0 ? 0 : nl > n_max ? n_max : nl);                 // generated tokens, inside the output matrix
}

// VEC: ld_next % 4 == 0 and a 16-byte aligned table, so every group of four entries of a row is one aligned load (the
// last group of a row may reach into the row's own padding [V, ld_next), which is read and ignored)
template <typename T, bool VEC>
__global__ __launch_bounds__(GNT) void grammar_mask_kernel(T* logits, long ld, int V, const int32_t* next, long ld_next,
                                                           int n_states, const uint8_t* flags, const int32_t* state,
                                                           const uint8_t* done, long eos) {
  const int b = blockIdx.y;
  if (done[b]) return;                                                // a finished row keeps its logits
  const int s = state[b];
  if (s < 0 || s >= n_states) return;                                 // unconstrained (-1), broken (-2), outside the table
  T* row = logits + (long)b * ld;
  const int32_t* nrow = next + (long)s * ld_next;                     // 64-bit: s * ld_next passes 2^31 for large grammars
  const bool eos_ok = (flags[s] & 1) != 0;
  const T ninf = from_f32<T>(-INFINITY);
  const long c = (long)blockIdx.x * GCHUNK + (long)threadIdx.x * 4;    // this thread's four columns
  if (c >= (long)V) return;
  int e[4];
  if (VEC) {
    const int4v v = *reinterpret_cast<const int4v*>(nrow + c);
    e[0] = v.x, e[1] = v.y, e[2] = v.z, e[3] = v.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) e[j] = c + j < (long)V ? nrow[c + j] : 0;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const long cj = c + j;
    if (cj >= (long)V) break;
    const bool banned = cj == eos ? !eos_ok : e[j] < 0;               // the table's own entry in the eos column is ignored
    if (banned) row[cj] = ninf;
  }
}

__global__ __launch_bounds__(GNT) void grammar_advance_kernel(const int64_t* out, long out_ld, int n_max, int B, int V,
                                                              const int32_t* n_dev, int n_add, const int32_t* next,
                                                              long ld_next, int n_states, const uint8_t* flags,
                                                              int32_t* state, uint8_t* done, int32_t* end) {
  const int b = blockIdx.x * GNT + threadIdx.x;
  if (b >= B || done[b]) return;                                      // finished before this launch, by eos too
  const int s = state[b];
  if (s < 0) return;
  const int n = clamp_count(n_dev, n_add, n_max);
  int sn = -1;
  if (n >= 1 && s < n_states) {
    const int64_t t = out[(long)b * out_ld + (n - 1)];
    if (t >= 0 && t < V) sn = next[(long)s * ld_next + t];
    if (sn >= n_states) sn = -1;                                      // a table that names a state it does not hold
  }
  if (sn >= 0) {
    state[b] = sn;
    if (flags[sn] & 2) done[b] = 1, end[b] = n;                       // terminal: accepting and nothing may follow
  } else {
    state[b] = -2, done[b] = 1, end[b] = n;                           // every allowed column was banned by someone else
  }
}

__global__ __launch_bounds__(GNT) void grammar_build_kernel(const int32_t* char_next, const uint8_t* tok_bytes,
                                                            const int32_t* tok_off, int S, int V, int32_t* next,
                                                            long ld_next) {
  const long i = (long)blockIdx.x * GNT + threadIdx.x;
  if (i >= (long)S * V) return;
  const int s = (int)(i / V), t = (int)(i % V);
  const int o = tok_off[t], o1 = tok_off[t + 1];
  int cur = o1 > o && o >= 0 ? s : -1;                                // an empty token is never allowed
  for (int j = o; j < o1 && cur >= 0; ++j) {
    cur = char_next[(long)cur * 256 + tok_bytes[j]];
    if (cur >= S) cur = -1;                                           // a byte table that names a state it does not hold
  }
  next[(long)s * ld_next + t] = cur < 0 ? -1 : cur;
}

template <typename T>
int launch_mask(void* logits, long ld, int V, int B, const int32_t* next, long ld_next, int n_states, const uint8_t* flags,
                const int32_t* state, const uint8_t* done, long eos, hipStream_t st) {
  const dim3 grid((V + GCHUNK - 1) / GCHUNK, B);
  const bool vec = ld_next % 4 == 0 && (reinterpret_cast<uintptr_t>(next) & 15) == 0;
  if (vec)
    MK_LAUNCH((grammar_mask_kernel<T, true>), grid, dim3(GNT), 0, st, (T*)logits, ld, V, next, ld_next, n_states, flags, state,
              done, eos);
  else
    MK_LAUNCH((grammar_mask_kernel<T, false>), grid, dim3(GNT), 0, st, (T*)logits, ld, V, next, ld_next, n_states, flags,
              state, done, eos);
  return mk_check_launch();
}

}  // namespace

extern "C" int mk_grammar_mask(void* logits, int64_t ld, int32_t V, int32_t B, const int32_t* next, int64_t ld_next,
                               int32_t n_states, const void* flags, const int32_t* state, const void* done, int64_t eos,
                               int32_t dtype, void* stream) {
  if (!logits || !next || !flags || !state || !done || V <= 0 || B <= 0 || n_states <= 0 || ld < V || ld_next < V)
    return MK_ERR_BAD_ARG;
  if ((dtype != MK_BF16 && dtype != MK_F16 && dtype != MK_F32) || B > 65535) return MK_ERR_UNSUPPORTED;   // rows: grid.y
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const uint8_t* f = (const uint8_t*)flags;
  const uint8_t* d = (const uint8_t*)done;
  if (dtype == MK_BF16) return launch_mask<bf16>(logits, (long)ld, V, B, next, (long)ld_next, n_states, f, state, d, (long)eos, st);
  if (dtype == MK_F16)
    return launch_mask<_Float16>(logits, (long)ld, V, B, next, (long)ld_next, n_states, f, state, d, (long)eos, st);
  return launch_mask<float>(logits, (long)ld, V, B, next, (long)ld_next, n_states, f, state, d, (long)eos, st);
}

extern "C" int mk_grammar_advance(const int64_t* out, int64_t out_ld, int32_t n_max, int32_t B, int32_t V,
                                  const int32_t* n_dev, int32_t n_add, const int32_t* next, int64_t ld_next,
                                  int32_t n_states, const void* flags, int32_t* state, void* done, int32_t* end,
                                  void* stream) {
  if (!out || !next || !flags || !state || !done || !end || B <= 0 || V <= 0 || n_states <= 0 || ld_next < V || n_max < 0 ||
      out_ld < n_max)
    return MK_ERR_BAD_ARG;
  MK_LAUNCH(grammar_advance_kernel, dim3((B + GNT - 1) / GNT), dim3(GNT), 0, reinterpret_cast<hipStream_t>(stream), out,
            (long)out_ld, n_max, B, V, n_dev, n_add, next, (long)ld_next, n_states, (const uint8_t*)flags, state,
            (uint8_t*)done, end);
  return mk_check_launch();
}

extern "C" int mk_grammar_build(const int32_t* char_next, const void* tok_bytes, const int32_t* tok_off, int32_t S, int32_t V,
                                int32_t* next, int64_t ld_next, void* stream) {
  if (!char_next || !tok_bytes || !tok_off || !next || S <= 0 || V <= 0 || ld_next < V) return MK_ERR_BAD_ARG;
  if ((long)S * V >= (1L << 32)) return MK_ERR_UNSUPPORTED;          // one thread per entry: a launch takes 2^32 threads
  const long blocks = ((long)S * V + GNT - 1) / GNT;
  MK_LAUNCH(grammar_build_kernel, dim3((unsigned)blocks), dim3(GNT), 0, reinterpret_cast<hipStream_t>(stream), char_next,
            (const uint8_t*)tok_bytes, tok_off, S, V, next, (long)ld_next);
  return mk_check_launch();
}
