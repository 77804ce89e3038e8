// Prompt-lookup speculative decoding for generate(prompt_lookup_num_tokens=G): the two bookkeeping launches of a verify
// step, with every piece of state on the device and PER SAMPLE (no batch-wide counter, no arrival counter), so that a
// step -- lookup, embedding of the Q = G + 1 ids per sample, the layers with mk_decode_step_attn_multi (decode.hip), the
// lm_head, verify -- stays a fixed launch sequence that one hipGraph replays (the twin of mk_decode_emit, decode.hip, and
// mk_beam_emit, beam.hip; the rule is written down in include/macaw_hip.h and restated in tests/spec_ref.py).
//
//   mk_spec_lookup       one workgroup of 256 threads per sample.  The history h = prompt ++ emitted ids is read in place
//                        (two pointers, never concatenated).  For n = min(N, L - 1) ... 1 thread t tests the windows i = t,
//                        t + 256, ... against the trailing n ids and keeps its smallest hit; "the smallest i" is decided by
//                        an integer minimum in LDS, never by the order of arrival.  Thread 0 copies the continuation.
//   mk_spec_verify_emit  one workgroup of 1024 threads per sample.  The argmax of each of the sample's R rows is
//                        mk_decode_emit's (thread t owns the columns t, t + 1024, ...; mk_argmax_better decides ties, NaN
//                        and -inf); thread 0 then compares them with the draft and writes the sample's books.
// Plain loads and stores only.
#include "common.h"
#include "../../include/macaw_hip.h"

namespace {

constexpr int SNT = 256;                        // threads per sample of the lookup
constexpr int SQM = 16;                         // most rows per sample: G <= 15

struct LookupArgs {
  const int64_t* prompt; long p_ld; int P; const int32_t* p_len;
  const int64_t* out; long out_ld; int n_max;
  const int32_t* n_out; const unsigned char* done;
  int64_t* tok; int32_t* n_draft;
  int G, N, V;
  long pad, eos;
};

__global__ __launch_bounds__(SNT) void spec_lookup_kernel(LookupArgs a) {
  __shared__ int best;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int Q = a.G + 1;
  int64_t* tok = a.tok + (long)b * Q;
  const int pl = a.prompt ? min(max(a.p_len[b], 0), a.P) : 0;
  const int no = min(max(a.n_out[b], 0), a.n_max);
  const int L = pl + no;
  const int64_t* pr = a.prompt ? a.prompt + (long)b * a.p_ld : nullptr;
  const int64_t* ot = a.out + (long)b * a.out_ld;
  auto h = [&](int i) -> long { return i < pl ? (long)pr[i] : (long)ot[i - pl]; };
  auto in_vocab = [&](long id) { return id >= 0 && id < (long)a.V; };
  int at = -1;                                  // the continuation starts at h[at]
  if (!a.done[b] && L >= 2) {
    for (int n = min(a.N, L - 1); n >= 1; --n) {
      if (tid == 0) best = 0x7fffffff;
      __syncthreads();
      int mine = 0x7fffffff;
      for (int i = tid; i + n < L; i += SNT) {
        bool eq = true;
        for (int j = 0; j < n && eq; ++j) {
          const long x = h(i + j);
          eq = x == h(L - n + j) && in_vocab(x);
        }
        if (eq) { mine = i; break; }            // (this thread's later windows are larger)
      }
      if (mine != 0x7fffffff) atomicMin(&best, mine);
      __syncthreads();
      const int found = best;
      __syncthreads();
      if (found != 0x7fffffff) { at = found + n; break; }
    }
  }
  if (tid == 0) {
    int nd = 0;
    if (at >= 0) {
      const int m = min(a.G, L - at);
      for (; nd < m; ++nd) {
        const long id = h(at + nd);
        if (id == a.eos || !in_vocab(id)) break;
        tok[1 + nd] = id;
      }
    }
    for (int j = nd; j < a.G; ++j) tok[1 + j] = a.pad;
    a.n_draft[b] = nd;
  }
}

struct VerifyArgs {
  const void* logits; long ld; int V, R, Q;
  long eos;
  int64_t* tok; const int32_t* n_draft;
  int32_t* pos; int32_t* n_out; unsigned char* done;
  int64_t* out; long out_ld; int n_max;
  int32_t* steps;
};

template <typename T>
__global__ __launch_bounds__(1024) void spec_verify_emit_kernel(VerifyArgs a) {
  __shared__ float bv[16];
  __shared__ int bi[16];
  __shared__ int am[SQM];
  const int b = blockIdx.x;
  if (a.done[b]) return;                        // a finished sample changes nothing (uniform over the workgroup)
  for (int g = 0; g < a.R; ++g) {
    const T* xr = (const T*)a.logits + ((long)b * a.R + g) * a.ld;
    float best = -INFINITY;
    int idx = 0x7fffffff;
    for (int c0 = threadIdx.x; c0 < a.V; c0 += 1024 * 8) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int c = c0 + j * 1024;
        v[j] = c < a.V ? to_f32<T>(xr[c]) : -INFINITY;
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {                                 // torch.argmax order (common.h)
        const int c = c0 + j * 1024;
        if (c < a.V && mk_argmax_better(v[j], c, best, idx)) { best = v[j]; idx = c; }
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
      am[g] = idx;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    int64_t* tok = a.tok + (long)b * a.Q;
    const int nd = a.R > 1 ? min(max(a.n_draft[b], 0), a.R - 1) : 0;
    int A = 0;
    while (A < nd && tok[1 + A] == (int64_t)am[A]) ++A;
    const int no = min(max(a.n_out[b], 0), a.n_max);
    const int room = a.n_max - no;
    int m = 0;
    bool hit = false;
    long last = tok[0];
    for (; m <= A && m < room && !hit; ++m) {
      last = am[m];
      a.out[(long)b * a.out_ld + no + m] = last;
      hit = last == a.eos;
    }
    a.n_out[b] = no + m;
    a.pos[b] += m;
    a.steps[b] += 1;
    tok[0] = last;
    if (hit || no + m >= a.n_max) a.done[b] = 1;
  }
}

}  // namespace

extern "C" int mk_spec_lookup(const int64_t* prompt, int64_t p_ld, int32_t P, const int32_t* p_len, const int64_t* out,
                              int64_t out_ld, int32_t n_max, const int32_t* n_out, const void* done, int64_t* tok,
                              int32_t* n_draft, int32_t B, int32_t G, int32_t max_matching_ngram_size, int32_t V,
                              int64_t pad, int64_t eos, void* stream) {
  if (!out || !n_out || !done || !tok || !n_draft || B <= 0 || G < 1 || G >= SQM || max_matching_ngram_size < 1 ||
      V <= 0 || n_max < 0 || out_ld < n_max || (prompt && (!p_len || P < 0 || p_ld < P)))
    return MK_ERR_BAD_ARG;
  LookupArgs a;
  a.prompt = prompt; a.p_ld = (long)p_ld; a.P = prompt ? P : 0; a.p_len = p_len;
  a.out = out; a.out_ld = (long)out_ld; a.n_max = n_max; a.n_out = n_out; a.done = (const unsigned char*)done;
  a.tok = tok; a.n_draft = n_draft; a.G = G; a.N = max_matching_ngram_size; a.V = V;
  a.pad = (long)pad; a.eos = (long)eos;
  MK_LAUNCH(spec_lookup_kernel, dim3(B), dim3(SNT), 0, reinterpret_cast<hipStream_t>(stream), a);
  return mk_check_launch();
}

extern "C" int mk_spec_verify_emit(const void* logits, int64_t ld, int32_t V, int32_t B, int32_t R, int32_t Q,
                                   int64_t eos, int64_t* tok, const int32_t* n_draft, int32_t* pos,
                                   int32_t* n_out, void* done, int64_t* out, int64_t out_ld, int32_t n_max,
                                   int32_t* steps, int32_t dtype, void* stream) {
  if (!logits || !tok || !n_draft || !pos || !n_out || !done || !out || !steps || V <= 0 || B <= 0 || ld < V ||
      Q < 1 || Q > SQM || (R != 1 && R != Q) || n_max < 0 || out_ld < n_max)
    return MK_ERR_BAD_ARG;
  VerifyArgs a;
  a.logits = logits; a.ld = (long)ld; a.V = V; a.R = R; a.Q = Q; a.eos = (long)eos;
  a.tok = tok; a.n_draft = n_draft; a.pos = pos; a.n_out = n_out; a.done = (unsigned char*)done;
  a.out = out; a.out_ld = (long)out_ld; a.n_max = n_max; a.steps = steps;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (dtype == MK_BF16) MK_LAUNCH((spec_verify_emit_kernel<bf16>), dim3(B), dim3(1024), 0, st, a);
  else if (dtype == MK_F16) MK_LAUNCH((spec_verify_emit_kernel<_Float16>), dim3(B), dim3(1024), 0, st, a);
  else if (dtype == MK_F32) MK_LAUNCH((spec_verify_emit_kernel<float>), dim3(B), dim3(1024), 0, st, a);
  else return MK_ERR_UNSUPPORTED;
  return mk_check_launch();
}
