/*
 * macaw_hip.h — C ABI of the MI355X-native (gfx950) kernels behind Macaw-LLM's
 * multimodal forward/backward hot path.
 *
 * The reference (lyuchenyang/Macaw-LLM) has no FFI of its own: the hot path is
 * eager PyTorch inside modeling.py.  Each entry point below therefore cites the
 * reference expression (modeling.py:line, or the un-vendored torch/transformers
 * module it calls) whose arithmetic it replaces.  The Python mirror of the
 * reference surface (macaw_llm_amd/modeling.py) calls these through ctypes.
 *
 * Conventions
 *   - plain pointers + sizes, no torch types; all pointers are DEVICE pointers
 *     unless noted; nothing is allocated or retained; asynchronous on `stream`
 *     (a hipStream_t passed as void*).
 *   - return value: 0 on success, <0 on error (MK_ERR_*). Never aborts.
 *   - dtype codes: 0 = f32, 1 = bf16, 2 = f16.  Every kernel exists for all three (the reference's
 *     scripts run fp16: train.sh:36, llm_trainer.py:411-412) except where a comment says otherwise
 *     (fp8 quantisation and the host-input pipeline take bf16 / f32); accumulation is always f32.
 *   - matrices are row-major with an explicit leading dimension (elements).
 */
#ifndef MACAW_HIP_H
#define MACAW_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define MK_OK 0
#define MK_ERR_BAD_ARG (-1)
#define MK_ERR_UNSUPPORTED (-2)
#define MK_ERR_LAUNCH (-3)

#define MK_F32 0
#define MK_BF16 1
#define MK_F16 2
#define MK_FP8 3 /* OCP e4m3fn bytes: mk_gemm operands / mk_fp8_quantize output only */

/* library identification: returns MK_ABI_VERSION */
#define MK_ABI_VERSION 11
int mk_abi_version(void);

/* ------------------------------------------------------------------ GEMM --
 * C[z][M,N] = act(alpha * opA(A[z]) * opB(B[z])^T + bias) + R[z] (+ C[z] if accumulate)
 *
 * Logical operands: A is M x K, B is N x K ("NT": both reduce over their 2nd
 * index).  a_red_major / b_red_major = 1 means the operand is STORED with the
 * reduction index as the row index (i.e. A stored as [K][M], B as [K][N]), so
 * the four BLAS layouts are covered without separate transposes:
 *   nn.Linear forward  y = x W^T        : A=x[M,K]        B=W[N,K]       (0,0)
 *   grad input         dx = dy W        : A=dy[M,N]       B=W[N,K] as [red=N][out=K] (0,1)
 *   grad weight        dW = dy^T x      : A=dy[M,N] as [red=M][out=N], B=x (1,1)
 * Replaces nn.Linear (modeling.py:134-140,159-162,530,912-917), torch.matmul
 * in LlamaAttention (modeling.py:197,215), the packed in-proj / out-proj of
 * nn.MultiheadAttention (modeling.py:882-910) and the HF CLIP / Whisper
 * projections (modeling.py:1073,1082,1092).
 * Batch: grid z = z1*nb2 + z2; pointer offset = z1*s?1 + z2*s?2 (elements).
 */
typedef struct mk_gemm_desc {
  const void* A;
  const void* B;
  void* C;
  const void* R;    /* optional residual added after activation, same dtype as C */
  const void* bias; /* optional, f32 or same dtype as C (see bias_dtype) */
  int32_t M, N, K;
  int64_t lda, ldb, ldc, ldr;
  int32_t a_red_major, b_red_major;
  int32_t nb1, nb2; /* batch = nb1*nb2 (>=1 each) */
  int64_t sA1, sA2, sB1, sB2, sC1, sC2, sR1, sR2;
  float alpha;
  int32_t bias_mode;  /* 0 none, 1 per output column (n), 2 per output row (m) */
  int32_t act;        /* 0 none, 1 gelu(erf), 2 quick_gelu (x*sigmoid(1.702x)) */
  int32_t accumulate; /* 1: C += result */
  int32_t dtype;      /* MK_F32 or MK_BF16: type of A,B,C,R,bias.  MK_FP8: A and B are OCP e4m3 bytes,
                         both K-major (a_red_major = b_red_major = 0), K % 128 == 0, lda / ldb in
                         elements (= bytes) and multiples of 16; C, R, bias are bf16 */
  void* ws;           /* optional device scratch for the stream-K tail (fp32 partial tiles +
                         arrival counters); NULL disables it. Must not be shared by GEMMs that
                         run concurrently on different streams.  Its first 4096 bytes (the
                         counters) must be ZERO before the first use; every launch leaves
                         them zero again (the last arriver of a tile resets its counter).  A
                         workspace too small for a split (4096 + tail tiles x pieces x 64 KiB)
                         runs the tail unsplit.  Pinned by tests/test_gemm_plans_gpu.py. */
  int64_t ws_bytes;
  const float* scale_a; /* optional DEVICE scalars multiplied into alpha in the epilogue (the     */
  const float* scale_b; /* per-tensor de-quantisation scales of fp8 operands; no host sync)       */
  int32_t flags;        /* MK_GEMM_*_KPAD_ZERO: that K-major operand's rows are readable and ZERO from
                           column K up to the next multiple of 64 (a pitched buffer whose pad columns
                           are kept zero, e.g. d(logits) [tokens, 32064] for V = 32007), so a K that
                           is not a multiple of 64 can still take the MFMA tile kernels (the other
                           operand must be reduction-major or padded the same way) */
} mk_gemm_desc;
#define MK_GEMM_SCALE_VEC 4   /* scale_a / scale_b are VECTORS: scale_a[M] per row of A (= output row),
                                 scale_b[N] per row of B (= output column): C = alpha-free
                                 act(acc * scale_a[m] * scale_b[n] + bias) ... (per-row / per-channel
                                 fp8 de-quantisation, mk_fp8_quantize_rows / _cols_t); MK_FP8_E4M3
                                 operands only, MK_ERR_UNSUPPORTED otherwise */
#define MK_GEMM_A_KPAD_ZERO 1
#define MK_GEMM_B_KPAD_ZERO 2
int mk_gemm(const mk_gemm_desc* d, void* stream);
/* Tuning / A-B hook: force the bf16 kernel configuration of the following mk_gemm calls
 * (11 = 256x256 v7 with eight waves, 15 = 256x256 v9: four waves, one per SIMD, hand-placed inline-asm K loop (whole tiles
 * only), 21 = v9's 288x256 tile: both operands K-major, M % 288 == 0, N % 256 == 0, K % 64 == 0, K >= 128, alpha
 * (+ R) only, C / R rows 8-byte aligned -- the same bits as 11 and 15; anywhere else it runs what 11 would,
 * 14 = its hipcc-scheduled predecessor v8 (experiment builds only), 5 = 128x128 v2, 7 = v2 BK32, 0 = generic;
 * -1 = automatic).  A forced configuration is still replaced where it is not legal for the problem.
 * Replaces cuBLAS behind nn.Linear of /root/reference/modeling.py:134-140,159-162,597. */
int mk_gemm_set_cfg(int cfg);
/* 1 if kernel configuration `cfg` is compiled into this library (14 only with MK_EXPERIMENTS=1 at build time). */
int mk_gemm_has_cfg(int cfg);
/* How many CUs the tile kernels may plan for (0 = all of the device, the default).  The 256x256 kernels hold one
 * workgroup per CU with all of its LDS, so a CU occupied by another resident kernel -- an RCCL channel of the
 * gradient reduce-scatter running beside the backward (train.sh:14, configs/deepspeed_config.json:22-41) -- is
 * lost to them: rounds of exactly 256 tiles then take two passes.  The step runtime sets this to
 * (CUs - collective channels) while collectives overlap the backward; round sizes, the spatial tail and the
 * kernel choice follow.  Values at or above the device's CU count mean all as well.  Returns the previous value.
 * Pinned by tests/test_gemm_plans_gpu.py. */
int mk_gemm_set_cus(int n_cus);
/* Grouped launch on the 256 x 256 v9 loop: ONE launch of one persistent workgroup per planned CU (mk_gemm_set_cus is
 * honoured) that runs whole tiles of several GEMMs -- an optional `main` problem, a grad-input GEMM (layout (0,1)), and
 * `n_fill` grad-weight GEMMs (layout (1,1)) whose tiles fill the CUs that the main problem's partial last round leaves
 * idle.  A filler may be consumed over several launches: tiles [0, first_tile) of its tile order are done already, and
 * on return `taken` says how many more this launch ran (they start at first_tile).  drain = 0 takes only what balances
 * the launch and leaves the rest queued; drain = 1 takes everything; drain = MK_GROUP_CARRY (2) is for a queue that
 * outlives the launch (one queue for all layers of a backward pass): the launch ends at the level of least idle time
 * at or above its heaviest workgroup and keeps about one tile per workgroup queued for the launches that follow.
 * main may be NULL (a plain grouped grad-weight
 * launch: whole rounds of the queue, everything with drain).  Every tile is computed exactly as mk_gemm's
 * configuration 15 computes a whole tile, so results do not depend on how the tiles were grouped.
 * The members of one launch run concurrently and in no defined order, so they must be independent: no member's A or B
 * may overlap another member's C (a filler cannot consume the main's output of the same launch), and no two C regions
 * may overlap.  The library does not check this.
 * Every member must be bf16 or f16 (one type for all), unbatched, M % 256 == N % 256 == 0, K % 64 == 0, K >= 128,
 * alpha only (no bias / activation / R / accumulate / scales / flags), operands as configuration 15 needs them
 * (16-byte aligned, pitches % 8 == 0) and C 8-byte aligned with ldc % 4 == 0; at most MK_GROUP_MAX_FILL fillers with
 * fewer than 65536 remaining tiles in all.  Otherwise MK_NOT_GROUPED is returned, nothing is launched or written and
 * the caller runs the members through mk_gemm.  In the profiler a grouped launch is one kind-0 launch with
 * configuration id 16, the main's shape (the first filler's without one) and the FLOPs of the tiles it ran.
 * Replaces cuBLAS behind the backward of nn.Linear (modeling.py:134-140,159-162). */
#define MK_NOT_GROUPED 1
#define MK_GROUP_MAX_FILL 8
#define MK_GROUP_CARRY 2 /* a value of `drain` */
typedef struct mk_gemm_group_fill {
  mk_gemm_desc d;
  int32_t first_tile; /* in: tiles already done */
  int32_t taken;      /* out: tiles this launch ran */
} mk_gemm_group_fill;
int mk_gemm_grouped(const mk_gemm_desc* main, mk_gemm_group_fill* fill, int32_t n_fill, int32_t drain, void* stream);
/* Optional live timing of every mk_gemm launch with HIP events on the launch stream
 * (bench.py roofline): begin, run, then end() synchronises and returns the sums. */
int mk_prof_begin(void);
int mk_prof_end(double* total_ms, double* total_flops, int64_t* launches);
/* the same sums for one launch kind since mk_prof_begin (0 = mk_gemm, 1 = mk_flash_attn_fwd,
 * 2 = mk_flash_attn_bwd; attention FLOPs are algorithmic: causal = lower triangle); call before
 * mk_prof_end */
int mk_prof_sum(int kind, double* total_ms, double* total_flops, int64_t* launches);
/* per-shape CSV breakdown (host path) of the launches since mk_prof_begin; call before end */
int mk_prof_report(const char* path);

/* 2-D (batched) transpose out[z][c][r] = in[z][r][c]; elem_size 2 or 4. */
int mk_transpose(const void* in, void* out, int32_t rows, int32_t cols, int64_t ld_in,
                 int64_t ld_out, int32_t batch, int64_t s_in, int64_t s_out, int32_t elem_size,
                 void* stream);

/* ------------------------------------------------------------ norms ------
 * RMSNorm (modeling.py:311-319): y = w * cast(x * rsqrt(mean(x^2, fp32) + eps)).
 * Optional fused residual: h = x + res is written to h_out and normalised
 * (LlamaDecoderLayer residual adds, modeling.py:283,289). rstd[rows] is f32.
 */
int mk_rmsnorm_fwd(const void* x, const void* res, const void* w, void* h_out, void* y,
                   float* rstd, int32_t rows, int32_t cols, float eps, int32_t dtype, void* stream);
/* dx = dres_in + rmsnorm_bwd(dy; h, rstd, w); dw_partial[nblk][cols] f32 partial
 * column sums (reduced by mk_colsum_partials). dres_in may be NULL. */
int mk_rmsnorm_bwd(const void* dy, const void* h, const void* w, const float* rstd,
                   const void* dres_in, void* dx, float* dw_partial, int32_t nblk, int32_t rows,
                   int32_t cols, int32_t dtype, void* stream);
/* LayerNorm with bias (torch nn.LayerNorm inside HF CLIP / Whisper encoder layers). */
int mk_layernorm_fwd(const void* x, const void* w, const void* b, void* y, float* mean,
                     float* rstd, int32_t rows, int32_t cols, float eps, int32_t dtype,
                     void* stream);
int mk_layernorm_bwd(const void* dy, const void* x, const void* w, const float* mean,
                     const float* rstd, const void* dres_in, void* dx, float* dw_partial,
                     float* db_partial, int32_t nblk, int32_t rows, int32_t cols, int32_t dtype,
                     void* stream);
/* out[c] (+)= sum_b partial[b][c]; out dtype = `dtype`. */
int mk_colsum_partials(const float* partial, void* out, int32_t nblk, int32_t cols,
                       int32_t accumulate, int32_t dtype, void* stream);
/* out[c] (+)= sum_r x[r][c] (bias gradients). ws: f32 [nblk*cols] scratch. */
int mk_colsum(const void* x, int64_t ld, void* out, float* ws, int32_t nblk, int32_t rows,
              int32_t cols, int32_t accumulate, int32_t dtype, void* stream);

/* ----------------------------------------------------------- pointwise ---
 * RoPE (modeling.py:76-123): x layout [B,S,H,hd] (row pitch ld between
 * tokens), half-split rotation, cos/sin tables [max_pos, hd] in `dtype`
 * (already cast as modeling.py:121-122 does); pos[B*S] int32 position ids;
 * inverse=1 applies the transpose rotation (backward).
 */
int mk_rope(void* x, const void* cos_t, const void* sin_t, const int32_t* pos, int32_t tokens,
            int32_t heads, int32_t hd, int64_t ld, int32_t inverse, int32_t dtype, void* stream);
/* SwiGLU (modeling.py:140): a = silu(g) * u ; backward gives dg, du. */
int mk_swiglu_fwd(const void* g, const void* u, void* a, int64_t n, int32_t dtype, void* stream);
int mk_swiglu_bwd(const void* g, const void* u, const void* da, void* dg, void* du, int64_t n,
                  int32_t dtype, void* stream);
/* pitched 2-D forms for the fused gate|up projection buffer [rows, 2*cols] */
int mk_swiglu2d_fwd(const void* g, const void* u, void* a, int64_t rows, int32_t cols,
                    int64_t ld_in, int64_t ld_out, int32_t dtype, void* stream);
int mk_swiglu2d_bwd(const void* g, const void* u, const void* da, void* dg, void* du, int64_t rows,
                    int32_t cols, int64_t ld_gu, int64_t ld_a, int32_t dtype, void* stream);
/* y = act(x): act 1 gelu(erf) (Whisper), 2 quick_gelu (CLIP). */
int mk_act_fwd(const void* x, void* y, int64_t n, int32_t act, int32_t dtype, void* stream);
/* activation backward: dx = dy * act'(x_pre); act 1 gelu(erf), 2 quick_gelu. x_pre is the
 * pre-activation INCLUDING bias. */
int mk_act_bwd(const void* x_pre, const void* dy, void* dx, int64_t n, int32_t act, int32_t dtype,
               void* stream);
/* y = a + b (b may be broadcast over rows with period `period` elements; 0 = none) */
int mk_add(const void* a, const void* b, void* y, int64_t n, int64_t period, int32_t dtype,
           void* stream);
/* dtype conversion (inputs arrive as fp16 from llm_trainer.py:366-368). */
int mk_cast(const void* in, int32_t in_dtype, void* out, int32_t out_dtype, int64_t n,
            void* stream);
int mk_fill(void* p, float v, int64_t n, int32_t dtype, void* stream);
/* out[0] (+)= sum_i x[i]^2 in fp32, deterministic (global gradient norm for clipping: the
 * reference trains with HF max_grad_norm / DeepSpeed gradient_clipping, train.sh + configs/).
 * ws: f32 [1024] scratch; x 16-byte aligned. */
int mk_sumsq(const void* x, int64_t n, float* ws, float* out, int32_t accumulate, int32_t dtype,
             void* stream);
/* dst[z][r][0:cols] = src[z][r][0:cols] (pitched rows, batch strides; s_src = 0 broadcasts):
 * the torch.cat / slice / repeat plumbing of modeling.py:974-1046 without eager kernels. */
int mk_copy2d(const void* src, void* dst, int32_t rows, int32_t cols, int64_t ld_src,
              int64_t ld_dst, int32_t batch, int64_t s_src, int64_t s_dst, int32_t elem_size,
              void* stream);

/* Embedding gather (modeling.py:972,979-980): out[t] = table[ids[t]]; ids int64. */
int mk_embedding_fwd(const void* table, const int64_t* ids, void* out, int32_t tokens,
                     int32_t dim, int64_t ld_out, int32_t vocab, int32_t dtype, void* stream);
/* dtable[ids[t]] += dout[t], deterministic (no atomics): the first occurrence of each id
 * sums all of its occurrences in fp32 and updates the row once. Rows equal to padding_idx
 * (nn.Embedding padding_idx, modeling.py:358) are skipped; pass -1 for none. */
int mk_embedding_bwd(const void* dout, int64_t ld, const int64_t* ids, void* dtable,
                     int32_t tokens, int32_t dim, int32_t vocab, int64_t padding_idx,
                     int32_t dtype, void* stream);

/* Generic strided-window gather ("im2col") used for Conv2d patch embedding
 * (HF CLIPVisionEmbeddings), Whisper conv1/conv2 and the project_* Conv1d
 * (modeling.py:919-924): out[(b,j)][c*kw + t] = x[b*sb + c*sc + (j*stride + t - pad)*st]
 * (zero outside [0,T)), rows padded with zeros up to ld_out. 2-D patches are
 * expressed by the caller as two nested calls or by mk_patchify. */
int mk_im2col1d(const void* x, void* out, int32_t B, int32_t C, int32_t T, int32_t kw,
                int32_t stride, int32_t pad, int32_t Lout, int64_t sb, int64_t sc, int64_t st,
                int64_t ld_out, int32_t dtype, void* stream);
/* adjoint of mk_im2col1d (gather form, no atomics): dx = col2im(dcols). */
int mk_col2im1d(const void* dcols, void* dx, int32_t B, int32_t C, int32_t T, int32_t kw,
                int32_t stride, int32_t pad, int32_t Lout, int64_t sb, int64_t sc, int64_t st,
                int64_t ld_cols, int32_t dtype, void* stream);
/* Non-overlapping 2-D patches: out[(b,py,px)][c*P*P + dy*P + dx] = img[b][c][py*P+dy][px*P+dx] */
int mk_patchify(const void* img, void* out, int32_t B, int32_t C, int32_t H, int32_t W, int32_t P,
                int64_t ld_out, int32_t dtype, void* stream);
int mk_unpatchify(const void* dcols, void* dimg, int32_t B, int32_t C, int32_t H, int32_t W,
                  int32_t P, int64_t ld_cols, int32_t dtype, void* stream);

/* ------------------------------------------------------------- softmax ---
 * Row softmax over scores[z][q][k] with the reference's masking semantics
 * (modeling.py:205-214): causal (k > q + (Lk-Lq) masked) and/or key padding
 * mask kmask[b][Lk] (int32, 0 = masked); masked logits become finfo.min and
 * softmax runs in fp32 then casts.  Optional dropout on the probabilities
 * (nn.MultiheadAttention dropout=0.1, modeling.py:879): keep iff
 * hash(seed, element index) < keep_threshold, kept values scaled by
 * 1/(1-p).  In-place (probs may alias scores).  heads = rows of z per batch
 * element (kmask index = z / heads).
 */
int mk_softmax_fwd(const void* scores, void* probs, void* probs_dropped /* NULL if p == 0 */,
                   const int32_t* kmask, int32_t nz, int32_t heads, int32_t Lq, int32_t Lk,
                   int64_t ld, int32_t causal, float dropout_p, uint64_t seed, int32_t dtype,
                   void* stream);
/* dscores = (P .* (g - rowsum(g .* P))) * scale, g = dP_dropped .* keep/(1-p); in place on
 * dprobs.  probs are the PRE-dropout probabilities; the dropout mask is regenerated from
 * (seed, element index). */
int mk_softmax_bwd(const void* probs, void* dprobs, int32_t nz, int32_t Lq, int32_t Lk,
                   int64_t ld, float scale, float dropout_p, uint64_t seed, int32_t dtype,
                   void* stream);

/* Fused (flash) attention forward, bf16, head_dim 64 or 128: o = softmax(scale q k^T + mask) v
 * per (batch, head) without materialising the scores (modeling.py:197-215 / HF encoder
 * attention).  q/k/v/o are addressed as base + b*bs + token*ld + h*hd (elements); kmask
 * [B, Lk] int32 (0 = masked) optional; causal masks key > query + (Lk - Lq); lse [B, H, Lq]
 * f32 optional (log-sum-exp of the scaled, masked scores).
 * A query row WITHOUT a visible key (every key padded, or causal with Lq > Lk: rows 0 .. Lq - Lk - 1)
 * gets o = 0 and lse = -inf, exactly, and mk_flash_attn_bwd gives it dq = 0 and adds nothing to any
 * dk / dv (a key no query sees gets dk = dv = 0); nothing is NaN.  This deliberately DIFFERS from
 * mk_softmax_fwd, whose finfo.min masking makes such a row uniform over all Lk keys (the reference's
 * eager behaviour): the fused kernels drop masked keys before the exponential, so a row that has none
 * has no weight to spread.  Rows of k / v beyond Lk are never read (a cache with unwritten rows
 * behind T is safe).  Pinned by tests/test_attention_edges_gpu.py. */
int mk_flash_attn_fwd(const void* q, const void* k, const void* v, void* o, float* lse,
                      const int32_t* kmask, int32_t B, int32_t H, int32_t Lq, int32_t Lk,
                      int32_t hd, int64_t q_ld, int64_t q_bs, int64_t k_ld, int64_t k_bs,
                      int64_t v_ld, int64_t v_bs, int64_t o_ld, int64_t o_bs, float scale,
                      int32_t causal, int32_t dtype, void* stream);

/* mk_flash_attn_fwd, always causal, with PER-SAMPLE lengths read on the device: the prefill of several new positions
 * per sample over a KV cache whose length differs per sample (a continued generate() call).  q_len / k_len: int32 [B]
 * device arrays; Lq / Lk are host UPPER BOUNDS that size the grid and the key loop -- the host never synchronises for
 * the lengths.  Addressing is mk_flash_attn_fwd's (base + b*bs + token*ld + h*hd); k and v may be the two halves of a
 * [B][t_max][2D] cache.  The rule, with ql_b = clamp(q_len[b], 0, Lq) and kl_b = clamp(k_len[b], 0, Lk):
 *   - query row i < ql_b of sample b sees key j iff j < kl_b and j <= i + (kl_b - ql_b);
 *   - a row without a visible key -- every row i >= ql_b (up to Lq) and, where kl_b < ql_b, the first ql_b - kl_b rows --
 *     gets o = 0 and lse = -inf, exactly; nothing is NaN (mk_flash_attn_fwd's rule for dead rows);
 *   - no byte of k or v at a row >= kl_b is read, and no byte of q at a row >= ql_b influences any output (a cache with
 *     unwritten rows behind a sample's length, and filler rows behind a sample's new tokens, are safe).
 * A row's result does not depend on the other samples of the launch.  lse [B, H, Lq] f32 optional.
 * Domain: bf16 or f16, hd 64 or 128, the alignment and stride conditions of mk_flash_attn_fwd; otherwise
 * MK_ERR_UNSUPPORTED and nothing is launched.  MK_ERR_BAD_ARG for a null q, k, v, o, q_len or k_len and for B, H, Lq or
 * Lk <= 0.  Inference only: there is no backward.  Pinned by tests/test_flash_varlen_gpu.py.
 * The sessions built on it (generate(return_session=True) / generate(session=), modeling.GenerateSession) keep this
 * rule: a sample's history is built turn by turn -- the valid tokens of the turn's prompt, then the turn's generated tokens
 * up to and including the sample's final token (its eos, the last id of the stop sequence that ended it, or its last
 * token at max_new_tokens; pads behind it never enter).  A continued call returns for every sample what a fresh call would
 * return for that sample alone on history + valid tokens of the new prompt, positions 0 ... len - 1, up to the last bits
 * of its arithmetic.  The final token of a turn was emitted but never fed, so its key is not in the cache: it is the
 * session's pending token and becomes row 0 of the next call's new rows (q_len[b] = 1 + valid new tokens, k_len[b] = cached
 * rows + q_len[b]); no extra step is run for it. */
int mk_flash_attn_varlen_fwd(const void* q, const void* k, const void* v, void* o, float* lse /* optional */,
                             const int32_t* q_len, const int32_t* k_len, int32_t B, int32_t H, int32_t Lq,
                             int32_t Lk, int32_t hd, int64_t q_ld, int64_t q_bs, int64_t k_ld, int64_t k_bs,
                             int64_t v_ld, int64_t v_bs, int64_t o_ld, int64_t o_bs, float scale, int32_t dtype,
                             void* stream);

/* Fused attention backward (recompute form): dq, dk, dv from q, k, v, o, do and the forward's
 * lse; never stores P.  dq/dk/dv/do use the geometry of q/k/v/o.  dvec: f32 [B*H*Lq] scratch. */
int mk_flash_attn_bwd(const void* q, const void* k, const void* v, const void* o, const void* dout,
                      const float* lse, float* dvec, void* dq, void* dk, void* dv,
                      const int32_t* kmask, int32_t B, int32_t H, int32_t Lq, int32_t Lk,
                      int32_t hd, int64_t q_ld, int64_t q_bs, int64_t k_ld, int64_t k_bs,
                      int64_t v_ld, int64_t v_bs, int64_t o_ld, int64_t o_bs, float scale,
                      int32_t causal, int32_t dtype, void* stream);

/* mk_flash_attn_fwd / _bwd with the rotary embedding of q and k (modeling.py:76-91, 167-170) folded in: q and k are
 * the UNROTATED projections, rotated on their way into the kernel with mk_rope's arithmetic (each product and the
 * sum rounded to the element type: q, k as the products see them are bit-identical to mk_rope followed by
 * mk_flash_attn_*); dq and dk come back as gradients of the unrotated tensors (rounded to the element type, then
 * rotated back -- what mk_rope(inverse) after mk_flash_attn_bwd yields).  cos_t / sin_t [positions][hd] of the
 * element type, 16-byte aligned; pos[b * Lq + token] int32.  Only where every q / k element enters the kernel once:
 * hd == 128, Lq == Lk <= 160 (the one-workgroup-per-(b, h) kernels); otherwise MK_ERR_UNSUPPORTED and the caller
 * runs mk_rope itself.  mk_flash_attn_rope_bwd with qk_rotated = 1: q and k ARE the rotated tensors (mk_rope ran
 * before mk_flash_attn_fwd) and only the rotation of dq / dk back is folded into the kernel's stores -- the form the
 * training step uses (one rotation per element instead of three: profiles/r06_rope_fuse.txt). */
int mk_flash_attn_rope_fwd(const void* q, const void* k, const void* v, void* o, float* lse,
                           const int32_t* kmask, const void* cos_t, const void* sin_t,
                           const int32_t* pos, int32_t B, int32_t H, int32_t Lq, int32_t Lk, int32_t hd,
                           int64_t q_ld, int64_t q_bs, int64_t k_ld, int64_t k_bs, int64_t v_ld,
                           int64_t v_bs, int64_t o_ld, int64_t o_bs, float scale, int32_t causal,
                           int32_t dtype, void* stream);
int mk_flash_attn_rope_bwd(const void* q, const void* k, const void* v, const void* o, const void* dout,
                           const float* lse, float* dvec, void* dq, void* dk, void* dv,
                           const int32_t* kmask, const void* cos_t, const void* sin_t,
                           const int32_t* pos, int32_t B, int32_t H, int32_t Lq, int32_t Lk, int32_t hd,
                           int64_t q_ld, int64_t q_bs, int64_t k_ld, int64_t k_bs, int64_t v_ld,
                           int64_t v_bs, int64_t o_ld, int64_t o_bs, float scale, int32_t causal,
                           int32_t qk_rotated, int32_t dtype, void* stream);

/* Shifted cross-entropy (modeling.py:600-610). The caller passes labels already shifted
 * (row r predicts labels[r]; -100 = ignore).  row_loss[r] = lse_r - logit[r][label] (0 when
 * ignored), row_lse[r] kept for backward, loss_sum_cnt = {sum of row losses, number of valid
 * rows, mean loss, 0} (f32[4], reduced deterministically on device). */
int mk_cross_entropy(const void* logits, const int64_t* labels, float* row_loss, float* row_lse,
                     float* loss_sum_cnt, int32_t rows, int32_t V, int64_t ld, int32_t dtype,
                     void* stream);
/* dlogits[r][c] = (softmax(logits[r])[c] - [c == label]) * grad_scale / n_valid, zero for
 * ignored rows and for pad columns c in [V, ld).  dlogits may alias logits. */
int mk_cross_entropy_bwd(const void* logits, void* dlogits, const int64_t* labels,
                         const float* row_lse, const float* loss_sum_cnt, float grad_scale,
                         const float* grad_scale_dev /* optional device scalar multiplied in */,
                         int32_t rows, int32_t V, int64_t ld, int32_t dtype, void* stream);

/* Greedy decoding (modeling.py:959, HF greedy_search): out[r] = index of the first maximum of
 * row r of x[rows][cols] (pitch ld). */
int mk_argmax_rows(const void* x, int64_t ld, int32_t rows, int32_t cols, int64_t* out,
                   int32_t dtype, void* stream);

/* Decode step with the position in DEVICE memory (a fixed launch sequence per token: capturable in
 * a hipGraph; modeling.py:190-195 appends with torch.cat and modeling.py:954-960 re-launches the
 * eager step per token).
 * mk_kv_append: cache[b][t][0:cols] = src[b][0:cols] for b < batch, t = clamp(*t_dev, 0, t_max - 1);
 *   strides in elements: s_src / s_cache between samples, ld_cache between cache rows; 16-byte
 *   aligned rows.
 * mk_decode_attn: o[b][h][:] = softmax(scale * q[b][h] . k[b][0:T][h]) v[b][0:T][h] with
 *   T = clamp(*t_dev + t_add, 1, t_max); one query row per (sample, head); q / o rows are
 *   [H * hd] at batch strides q_bs / o_bs, keys and values [t_max][H * hd] at pitches k_ld / v_ld and
 *   batch strides k_bs / v_bs.  bf16, hd in {16, 32, 64, 128}, t_max <= 15360 (scores in LDS). */
/* mk_decode_linear: y[M][N] = prologue(x) W^T (+ residual) for M <= 16 token rows (M <= 32 without a
 *   prologue; bf16, K % 64 == 0,
 *   16-byte aligned rows), the weight-streaming kernel of mk_gemm's M <= 16 path with the operation
 *   that precedes the linear folded in: prologue 0 = none (x [M][K]); 1 = RMSNorm (x [M][K], norm_w
 *   [K], eps: y = (norm_w * rnd(x * rstd)) W^T, modeling.py:100-105); 2 = SwiGLU (x [M][2K] =
 *   [gate | up]: (rnd(silu(gate)) * up) W^T, modeling.py:140).  With a prologue the prepared token rows
 *   are staged in LDS: M * (K + 8) * 2 bytes <= 40 KiB, else MK_ERR_UNSUPPORTED (use the separate
 *   kernels).  17 <= M <= 32: 32 weight rows x 32 token rows per workgroup where N >= 8192, two
 *   16-token tiles per 16 weight rows below (the same choice mk_gemm makes for M <= 32). */
int mk_decode_linear(const void* x, int64_t ldx, const void* W, int64_t ldw, void* y, int64_t ldy,
                     const void* residual, int64_t ldr, int32_t M, int32_t N, int32_t K,
                     int32_t prologue, const void* norm_w, float eps, int32_t dtype, void* stream);
/* mk_decode_linear_fp8: y[M][N] = prologue(x) (scale * Wq)^T (+ residual), mk_decode_linear with the weight
 *   streamed as OCP e4m3 bytes (W8A16): Wq uint8 [N][K] row-major at pitch ldw BYTES, scale f32[N] one
 *   de-quantisation scale per output channel (the pair mk_fp8_quantize_rows writes for a weight); x,
 *   residual, y bf16 or f16 (dtype), fp32 accumulation.  A lane widens the bytes to the 16-bit type in
 *   registers (exact, subnormals included) and feeds the 16-bit MFMA; tokens are NOT quantised.  The scale
 *   multiplies the fp32 sum before the residual add and the one rounding to the output type.  Prologues
 *   and their rounding points as mk_decode_linear (1: x [M][K], norm_w [K]; 2: x [M][2K]).  Domain,
 *   else MK_ERR_UNSUPPORTED: M <= 16 with a prologue, M <= 32 plain; K % 64 == 0; ldw % 16 == 0 and
 *   ldx % 8 == 0 (elements), pitches not below the row lengths; x, Wq (and norm_w) 16-byte aligned,
 *   scale 4-byte aligned; with a prologue M * (K + 8) * 2 bytes <= 40 KiB of LDS.  Deterministic: the
 *   cross-wave sum has a fixed order. */
int mk_decode_linear_fp8(const void* x, int64_t ldx, const void* Wq, int64_t ldw, const float* scale, void* y,
                         int64_t ldy, const void* residual, int64_t ldr, int32_t M, int32_t N, int32_t K,
                         int32_t prologue, const void* norm_w, float eps, int32_t dtype, void* stream);
/* MXFP4 weight-only decode (generate(decode_weights="mxfp4")): the weight stream of a decode step at 4.25 bits per
 *   element.  ONE format (OCP Microscaling v1.0, MXFP4), for a weight W [N][K], K % 128 == 0:
 *     codes      uint8 [N][K / 2]   row pitch ldw BYTES; element 2 j of a row in the LOW nibble of byte j, element
 *                                   2 j + 1 in the HIGH nibble.  A code is e2m1: a sign bit (bit 3) and 3 bits that
 *                                   index {0, 0.5, 1, 1.5, 2, 3, 4, 6};
 *     exponents  uint8 [N][K / 32]  row pitch lde; one E8M0 byte e per block of 32 elements along K, the scale is
 *                                   2^(e - 127).  The NaN byte 0xFF is never written and not handled.
 *   Quantiser (round to nearest, no calibration), per block: E = clamp(floor(log2(amax)) - 2, EMIN, 125), E = EMIN
 *   for an all-zero block; element = x * 2^-E rounded to the nearest e2m1 value, ties to the even code (0.25 -> 0,
 *   0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4), saturated at +-6; stored byte E + 127.  EMIN is -125
 *   for bf16 and -13 for f16, so every de-quantised value (code * 2^E) is zero or a NORMAL number of the token type:
 *   the widening is exact and no result depends on a denormal mode.  A zero code is written without a sign.
 * mk_mxfp4_quantize_rows: that quantiser for a row-major bf16 / f16 matrix x [rows][cols] at pitch ld (elements;
 *   pitched rows allowed), one block of 32 per thread; deterministic.  cols % 32 == 0, ld % 8 == 0, ldq % 16 == 0,
 *   pitches not below the row lengths, x and q 16-byte aligned, else MK_ERR_UNSUPPORTED.
 * mk_decode_linear_mxfp4: y[M][N] = prologue(x) dequant(Wq, e)^T (+ residual), mk_decode_linear_fp8 with the weight
 *   streamed in that format (W4A16).  A lane's 16-byte load is one MX block; v_cvt_scalef32_pk_{bf16,f16}_fp4 widens
 *   two codes and applies the block scale (built as as_float(e << 23), a normal power of two) in one instruction,
 *   the 16-bit MFMA accumulates in fp32; tokens are NOT quantised.  The residual is added in fp32 before the one
 *   rounding to the output type.  Prologues and their rounding points as mk_decode_linear.  Domain, else
 *   MK_ERR_UNSUPPORTED: bf16 / f16; M <= 16 with a prologue, M <= 32 plain; K % 128 == 0; ldw % 16 == 0, ldw >= K / 2;
 *   lde % 4 == 0, lde >= K / 32; ldx % 8 == 0 (elements), ldx / ldy / ldr not below the row lengths; x, Wq (and
 *   norm_w) 16-byte aligned, e 4-byte aligned; with a prologue M * (K + 8) * 2 bytes <= 40 KiB of LDS.
 *   Deterministic: the cross-wave sum has a fixed order. */
int mk_mxfp4_quantize_rows(const void* x, int32_t rows, int32_t cols, int64_t ld, int32_t dtype, void* q, int64_t ldq,
                           void* e, int64_t lde, void* stream);
int mk_decode_linear_mxfp4(const void* x, int64_t ldx, const void* Wq, int64_t ldw, const void* e, int64_t lde, void* y,
                           int64_t ldy, const void* residual, int64_t ldr, int32_t M, int32_t N, int32_t K,
                           int32_t prologue, const void* norm_w, float eps, int32_t dtype, void* stream);
/* mk_decode_emit: greedy selection + bookkeeping of one decode step (modeling.py:959, HF greedy_search):
 *   for every sample b: nxt = done[b] ? pad : first argmax of logits[b][0:V]; out[b][state[1]] = nxt;
 *   done[b] |= (nxt == eos); tok[b] = nxt.  Then, once: state[0] += 1 (the position the other decode
 *   kernels read), state[1] += 1 (output column); state[2] is an arrival counter that must be zero
 *   before the first launch and is left zero.  done: one byte per sample. */
int mk_decode_emit(const void* logits, int64_t ld, int32_t V, int32_t B, int64_t pad, int64_t eos,
                   int64_t* tok, void* done, int64_t* out, int64_t out_ld, int32_t* state, int32_t dtype,
                   void* stream);
/* Sampled decoding (generate(do_sample=True); HF's temperature -> top-k -> top-p warpers and multinomial draw), one
 *   token per row of logits[rows][V] (pitch ld; columns [V, ld) are never read):
 *   1. x_c = float(logit_c) / temperature in fp32; a NaN or -inf logit is never drawn, and a row without a finite logit
 *      emits what mk_argmax_rows emits.
 *   2. top_k, when 0 < top_k < V: exactly top_k columns stay, the largest values, ties at the k-th value to the LOWER
 *      column (top_k = 1 is greedy; HF keeps the whole tie group).  0 switches it off.
 *   3. top_p, when top_p < 1, over the survivors: with e_c = exp(x_c - x_max) and Z their sum, column c stays iff
 *      sum{e_j : x_j > x_c} < top_p * Z (HF's rule by value: the top value always stays, a tie group stays or goes whole).
 *   4. u = ((mk_hash32(seed, (uint64(step) << 32) | row) >> 8) + 0.5) * 2^-24 (the counter hash of the dropout masks); the
 *      token is the first kept column, in column order, whose inclusive cumulative mass exceeds u * Z_kept.
 *   Selection is an exact radix select; masses are 2^-40 fixed-point integers, so every sum is an integer sum and the
 *   result is bitwise reproducible.  bf16 / f16 / f32.  MK_ERR_BAD_ARG: null pointers, rows <= 0, V <= 0, ld < V,
 *   temperature <= 0 or not finite, top_p outside (0, 1], top_k < 0.  V <= 2^23, else MK_ERR_UNSUPPORTED.
 *   6. The four warpers behind top-p (the _warp entries; HF's MinPLogitsWarper -> TypicalLogitsWarper ->
 *      EpsilonLogitsWarper -> EtaLogitsWarper, min_tokens_to_keep = 1), between rule 3 and the draw of rule 4.  Every stage
 *      works on the survivors of the stages before it, renormalised over them, and keeps at least one column.  With
 *      x_max the largest value of the row (it survives rules 2-3), d_c = x_max - x_c, e_c = exp(-d_c) and Z the sum of e
 *      over the current survivors:
 *      min_p in [0, 1], 0 = off: c stays iff e_c >= min_p (e_c >= min_p * max e, and the maximum is a survivor).
 *      typical_p in (0, 1], 1 = off: survivors whose fixed-point mass is 0 leave first (below V * 2^-40 in all, so a kept
 *        set never has integer mass 0).  D = sum(e_c d_c) / Z, t_c = |d_c - D| (HF's |-log p_c - H|: the log Z terms
 *        cancel); c stays iff the mass of the survivors with t strictly below t_c is below typical_p * Z -- rule 3 on
 *        the key t, ascending: a tie group in t stays or goes whole, the column nearest to D always stays, and the kept
 *        set is a band in d that may leave out the maximum.
 *      epsilon_cutoff in [0, 1), 0 = off: c stays iff e_c / Z >= epsilon_cutoff; when no survivor passes, the survivors
 *        of the largest value stay (a value floor: tie groups whole, as in HF).
 *      eta_cutoff in [0, 1), 0 = off: the same with the threshold min(eta, sqrt(eta) * exp(-H)), H = log Z +
 *        sum(e_c d_c) / Z the entropy of the renormalised survivors.
 *      In the kernel: masses m_c = trunc(e_c * 2^40) as everywhere; Z, sum(trunc(m_c * d_c)) and the largest m_c are
 *      integer reductions; the thresholds are integers (ceil(min_p * 2^40), ceil(typical_p * Z), ceil(threshold * Z)) and
 *      the floors compare m_c against them; D (rounded once to fp32), H and the eta threshold are computed once per row in
 *      fp64 from the integer sums; t_c is fp32 from the fp32 d_c and D, selected by the mass-weighted radix select of
 *      rule 3.  The kept set is: rules 2-3's value prefix, and m_c >= one mass floor, and (typical on) t_c <= one band
 *      edge.  The fall-back of the two cutoffs keeps the survivors of the largest MASS, which is the largest value
 *      wherever two values differ in their fixed-point masses.  No difference to HF beyond rule 2's.
 *      MK_ERR_BAD_ARG for a value outside these ranges or not finite.  All four off (0, 1, 0, 0): the entry without them.
 * mk_sample_rows: out_ids[row] = that token, the sampled twin of mk_argmax_rows.
 * mk_decode_emit_sample: mk_decode_emit with the argmax replaced by that draw for the samples not yet finished, row = b
 *   and step = state[1] (the output column, read on the device: a captured step draws a fresh number on every replay);
 *   pad, eos, tok, done, out and the state hand-off exactly as mk_decode_emit. */
int mk_sample_rows(const void* logits, int64_t ld, int32_t rows, int32_t V, float temperature, int32_t top_k,
                   float top_p, uint64_t seed, int32_t step, int64_t* out_ids, int32_t dtype, void* stream);
int mk_decode_emit_sample(const void* logits, int64_t ld, int32_t V, int32_t B, int64_t pad, int64_t eos,
                          int64_t* tok, void* done, int64_t* out, int64_t out_ld, int32_t* state, float temperature,
                          int32_t top_k, float top_p, uint64_t seed, int32_t dtype, void* stream);
/* mk_sample_rows_warp, mk_decode_emit_sample_warp: the two entries above with rule 6's four values behind top_p.
 * mk_sample_keep_rows: keep[row][c] (one byte, pitch keep_ld >= V) = 1 where the filter of rules 1-3 and 6 keeps column c,
 *   0 elsewhere -- the set the draw of rule 4 lands in, from the same filter code; a row without a finite logit gets an
 *   all-zero mask.  (A top-k survivor whose mass is 0 is kept and never drawn unless typical_p is on.) */
int mk_sample_rows_warp(const void* logits, int64_t ld, int32_t rows, int32_t V, float temperature, int32_t top_k,
                        float top_p, float min_p, float typical_p, float epsilon_cutoff, float eta_cutoff, uint64_t seed,
                        int32_t step, int64_t* out_ids, int32_t dtype, void* stream);
int mk_decode_emit_sample_warp(const void* logits, int64_t ld, int32_t V, int32_t B, int64_t pad, int64_t eos,
                               int64_t* tok, void* done, int64_t* out, int64_t out_ld, int32_t* state, float temperature,
                               int32_t top_k, float top_p, float min_p, float typical_p, float epsilon_cutoff,
                               float eta_cutoff, uint64_t seed, int32_t dtype, void* stream);
int mk_sample_keep_rows(const void* logits, int64_t ld, int32_t rows, int32_t V, float temperature, int32_t top_k,
                        float top_p, float min_p, float typical_p, float epsilon_cutoff, float eta_cutoff, uint8_t* keep,
                        int64_t keep_ld, int32_t dtype, void* stream);
/* Per-row sampling table (generate(sampling_params=[...])): the selection of the entries above with every parameter read
 *   PER ROW from device memory, so one batch mixes greedy and sampled requests, temperatures, filters and seeds (OpenAI's
 *   temperature / top_p / seed per request, vLLM's one SamplingParams per prompt); restated in
 *   tests/sampling_params_ref.py on top of the restatements of rules 1-6.
 *
 * The table: `rows` records of 48 bytes, record r at byte 48 r, the table 16-byte aligned, little endian:
 *     byte  0  float32  temperature        byte 16  float32  typical_p        byte 32  uint64   seed
 *     byte  4  int32    top_k (0 = off)    byte 20  float32  epsilon_cutoff   byte 40  int32    mode: 0 greedy, 1 sampled
 *     byte  8  float32  top_p              byte 24  float32  eta_cutoff       byte 44  int32    reserved, 0
 *     byte 12  float32  min_p              byte 28  uint32   stream
 *
 * The rule for row r with record R:
 *   mode 0 (greedy): the column mk_argmax_rows / mk_decode_emit select for that row -- the first NaN, else the first
 *     maximum, column 0 for a row of -inf -- bit for bit; the other fields are not read.
 *   mode 1 (sampled): rules 1-3 and 6 with R's seven values and the draw of rule 4 with
 *     u = ((mk_hash32(R.seed, (uint64(step) << 32) | R.stream) >> 8) + 0.5) * 2^-24: rule 4 with the record's seed, and
 *     the record's stream where rule 4 has the row index.  So the row's token is exactly what mk_sample_rows (with one of
 *     R's four warpers on: mk_sample_rows_warp) returns at the same step, with R's values and seed, for the same logits
 *     placed at row index R.stream: it does not depend on where the row sits in the batch, nor on the other rows.
 *   A record outside the scalar entries' domain (temperature <= 0 or not finite, top_p outside (0, 1], top_k < 0, a warper
 *     outside its range, another mode) is greedy: the kernel neither refuses nor loops.  Validation belongs where the
 *     table is built.
 *   The record is the workgroup's own, so the choice between the three forms (greedy, without the warpers, with them) is
 *   uniform over the workgroup; the forms are the device functions of the scalar kernels, not copies of them.
 *
 * mk_sample_rows_table: out_ids[r] = that token for every row, the twin of mk_sample_rows / mk_sample_rows_warp.
 * mk_decode_emit_sample_table: the twin of mk_decode_emit_sample / _warp, sample b by table[b] at step = state[1]: a
 *   finished sample emits pad and draws nothing, eos sets done, and the last arriving workgroup advances state[0..2],
 *   exactly as mk_decode_emit.
 * One workgroup of 1024 threads per row; bf16 / f16 / f32.  MK_ERR_BAD_ARG: null pointers (the table included), rows or
 *   B <= 0, V <= 0, ld < V.  MK_ERR_UNSUPPORTED: V > 2^23, a table that is not 16-byte aligned, another dtype. */
int mk_sample_rows_table(const void* logits, int64_t ld, int32_t rows, int32_t V, const void* table, int32_t step,
                         int64_t* out_ids, int32_t dtype, void* stream);
int mk_decode_emit_sample_table(const void* logits, int64_t ld, int32_t V, int32_t B, int64_t pad, int64_t eos,
                                int64_t* tok, void* done, int64_t* out, int64_t out_ld, int32_t* state,
                                const void* table, int32_t dtype, void* stream);
/* Logits processors (generate(repetition_penalty=, no_repeat_ngram_size=, min_new_tokens=)): HF's
 *   RepetitionPenaltyLogitsProcessor -> NoRepeatNGramLogitsProcessor -> MinNewTokensLengthLogitsProcessor, in that
 *   order and with their arithmetic, written down here; restated in torch in tests/logits_proc_ref.py, to which the
 *   kernel is pinned bit for bit.  They rewrite a row of logits IN PLACE, in front of the emit (mk_decode_emit,
 *   mk_decode_emit_sample, mk_argmax_rows, mk_sample_rows): processors first, warpers and the selection behind them.
 *
 * History of row b: h_b = prompt_b ++ generated_b.
 *   prompt     int64 [B][P] at pitch p_ld, the first clamp(p_len[b], 0, P) ids of row b (p_len int32 [B]); a null
 *              pointer means no prompt history (P, p_ld and p_len are then not read).
 *   generated  the step's output matrix, int64 [B][n_max] at pitch out_ld, columns [0, n) of row b, with
 *              n = clamp((n_dev ? *n_dev : 0) + n_add, 0, n_max): n_dev is read on the device (the graph loop passes
 *              state + 1, the output column that mk_decode_emit advances, so a captured step replays); a host loop may
 *              pass n_dev null and its count in n_add.
 *   An id outside [0, V) names no column: it takes part in the n-gram comparison and changes no logit.
 *
 * The rule, L = |h_b|:
 *   1. repetition_penalty theta (1.0 = off): for every DISTINCT id c of h_b, x = float(logit[c]) and
 *      x = x < 0 ? x * theta : x / theta, both in fp32, the division correctly rounded; then one rounding, to nearest
 *      even, to the logits' type.  Each distinct id is penalised once, however often it occurs.  (-0, a NaN and +inf
 *      take the division, -inf stays -inf.)
 *   2. no_repeat_ngram_size n (0 = off): when L + 1 >= n, every i in [0, L - n + 1) with
 *      h[i .. i + n - 1) == h[L - n + 1 .. L) bans h[i + n - 1]: its logit becomes -inf.  n = 1 bans every id of the
 *      history; L < n bans nothing.
 *   3. min_new_tokens m (0 = off): while n < m (generated tokens only), logit[eos] = -inf.  Needs 0 <= eos < V;
 *      eos < 0 (eos_token_id=None) switches it off.
 *
 * mk_logits_process: one workgroup per row; the distinct ids are found with a V-bit bitmap in LDS (atomic OR: the
 *   thread that sets an id's bit rewrites its column), the windows are compared in parallel over i.  Exact and
 *   deterministic whatever the history length and the duplicates.  Only the columns the history and eos name are read
 *   or written: the other columns and the padding [V, ld) keep their bits.  With everything off (theta == 1, n == 0,
 *   and m == 0 or eos < 0) nothing is launched.  Logits bf16 / f16 / f32 [B][V] at pitch ld >= V.
 *   MK_ERR_BAD_ARG: logits or out null, a prompt without p_len, B <= 0, V <= 0, ld < V, n_max < 0, out_ld < n_max,
 *   P < 0, p_ld < P, theta not finite or <= 0, n < 0, m < 0.  The bitmap takes 32 KiB of LDS: V <= 2^18 = 262144, else
 *   MK_ERR_UNSUPPORTED. */
int mk_logits_process(void* logits, int64_t ld, int32_t V, int32_t B, const int64_t* prompt, int64_t p_ld, int32_t P,
                      const int32_t* p_len, const int64_t* out, int64_t out_ld, int32_t n_max, const int32_t* n_dev,
                      int32_t n_add, float repetition_penalty, int32_t no_repeat_ngram_size, int32_t min_new_tokens,
                      int64_t eos, int32_t dtype, void* stream);
/* Per-request penalties (generate(frequency_penalty=, presence_penalty=, logit_bias=)): the additive penalties and the
 *   bias every OpenAI-compatible front end forwards (OpenAI, vLLM, TGI, the llama.cpp server), with OpenAI's and vLLM's
 *   definition, written down here; restated in torch in tests/penalties_ref.py, to which the kernel is pinned bit for
 *   bit.  Unlike repetition_penalty they are additive, proportional to how often a token was generated and blind to the
 *   prompt, and every value is PER ROW: a batch may mix requests.
 *
 * Inputs of row b:
 *   g_b        the GENERATED ids only: the step's output matrix, int64 [B][n_max] at pitch out_ld, columns [0, n) of row
 *              b, with n = clamp((n_dev ? *n_dev : 0) + n_add, 0, n_max), n_dev and n_add exactly as in "Logits
 *              processors" (the graph loop passes state + 1, so a captured step replays).  The prompt is never counted.
 *   cnt_c      the number of positions of g_b that hold id c.  An id outside [0, V) names no column.
 *   f_b, p_b   frequency[b] and presence[b], float32 [B] on the device; a null array is all zeros.
 *   bias       a list per row in CSR form: bias_off int32 [B + 1], ascending from 0; bias_ids int32 [nnz], row b's ids
 *              bias_ids[bias_off[b] .. bias_off[b + 1]) ASCENDING and DISTINCT within the row, all inside [0, V);
 *              bias_val float32 [nnz], finite.  A null bias_off means no bias.
 *
 * The rule.  Column c of row b is TOUCHED iff it has a bias entry beta_c, or cnt_c > 0 and (f_b != 0 or p_b != 0).  For a
 *   touched column, all in fp32, every operation rounded by itself (no fused multiply-add), in this order:
 *     x = float(logit[c])
 *     if it has a bias entry:  x = x + beta_c
 *     if cnt_c > 0:            x = x - (f_b * float(cnt_c));  x = x - p_b      (both steps, also when one of f_b, p_b is 0)
 *     logit[c] = x rounded to nearest even to the logits' type (ONE rounding, also when bias and count meet)
 *   On finite rows this is vLLM's logits -= f * counts; logits -= p * (counts > 0) with the bias added first.
 *   Consequences: -inf stays -inf and a NaN stays NaN, so a ban or min_new_tokens in front cannot be undone (bias values
 *   are finite); +inf stays +inf.  (Which NaN a touched NaN becomes, its sign and payload, is not part of the rule.)  Untouched columns, and the padding [V, ld), keep their bits exactly: -0 and NaN
 *   payloads are not rewritten.  Token 0 (n = 0) sees only the bias.  cnt_c <= n_max <= 2^24, so float(cnt_c) is exact.
 *   Its place in the chain: BEHIND mk_logits_process and in front of mk_seq_ban, mk_grammar_mask, mk_decode_emit_logprobs
 *   and every selection: bans and the grammar have the last word, and log-probabilities are scored on the biased row.
 *   One deliberate difference from vLLM: vLLM adds logit_bias in front of repetition_penalty, here it is added behind
 *   it; the two differ only when both name the same token.
 *
 * mk_logits_penalize: one launch, one workgroup per row.  The generated ids are staged in LDS, the distinct ones found
 *   with the V-bit LDS bitmap of mk_logits_process; the thread whose atomic OR sets an id's bit counts it over the staged
 *   ids, looks its column up in the row's bias ids (binary search) and rewrites it once; the bias entries of columns
 *   that were not generated are written by threads striding over the row's list.  Exact and deterministic whatever the
 *   arrival order: a count is a sum of integers, and every touched column is written exactly once.  A history longer
 *   than the staging buffer (2048 ids) is staged in rounds, not refused.  A row with f_b == 0, p_b == 0 and no bias entry
 *   returns at once and keeps its bits; with frequency, presence and bias_off all null nothing is launched.  Logits
 *   bf16 / f16 / f32 [B][V] at pitch ld >= V, in place.
 *   MK_ERR_BAD_ARG: logits or out null, B <= 0, V <= 0, ld < V, n_max < 0, n_max > 2^24, out_ld < n_max, bias_off
 *   without bias_ids or bias_val.  The bitmap takes 32 KiB of LDS: V <= 2^18 = 262144, else MK_ERR_UNSUPPORTED; another
 *   dtype: MK_ERR_UNSUPPORTED. */
int mk_logits_penalize(void* logits, int64_t ld, int32_t V, int32_t B, const int64_t* out, int64_t out_ld, int32_t n_max,
                       const int32_t* n_dev, int32_t n_add, const float* frequency, const float* presence,
                       const int32_t* bias_off, const int32_t* bias_ids, const float* bias_val, int32_t dtype,
                       void* stream);
/* Token-sequence matching (generate(bad_words_ids=, stop_sequences=)): HF's NoBadWordsLogitsProcessor, and the stop
 *   lists of TGI (stop_sequences) and vLLM (stop) -- HF's stop_strings at token level -- written down here; restated in
 *   torch in tests/stop_ref.py, to which both kernels are pinned exactly (integers and the -inf bit pattern only).
 *
 * The table, on the device, built once per call: seq_ids int64 [total], the sequences back to back, and seq_off int32
 *   [n_seq + 1], ascending from 0: sequence q_s = seq_ids[seq_off[s] .. seq_off[s + 1]).  At most 2^16 = 65536 sequences
 *   of 1 .. 64 ids each; an entry of another length matches nothing.
 * The history h_b = prompt_b ++ generated_b and its arguments (prompt, p_ld, P, p_len, out, out_ld, n_max, n_dev, n_add)
 *   exactly as in "Logits processors": n = clamp((n_dev ? *n_dev : 0) + n_add, 0, n_max) generated tokens, read on the
 *   device, so a captured step replays.
 *
 * The ban rule (mk_seq_ban), L = |h_b|: for every sequence q of m ids, logit[q[m - 1]] = -inf when m == 1, and when
 *   L >= m - 1 and h[L - m + 1 .. L) == q[0 .. m - 1).  A banned sequence is therefore never completed.  Two deliberate
 *   differences from HF: (1) the installed transformers skips a multi-token sequence while L < m, so a banned m-gram can
 *   be emitted as the first m ids of a history (the case of a call on embeddings alone, whose history is the generated
 *   tokens); here L >= m - 1 suffices, and the two agree bit for bit wherever L >= m for every sequence; (2) HF ADDS
 *   a bias row, -inf in the banned columns and 0.0 elsewhere, which turns a banned +inf or NaN logit into NaN and every -0
 *   into +0; here the banned column is SET to -inf whatever it held and no other bit changes.  An id outside
 *   [0, V) names no column: it takes part in the comparison and changes no logit.  Dropping a sequence equal to [eos]
 *   (HF's rule) is the caller's business: the table is taken as it stands.
 *   Its place in the chain: HF runs NoBadWords between the n-gram and the min-length processor.  Every neighbour there
 *   only writes -inf, and the repetition penalty maps -inf to -inf, so a separate launch BEHIND mk_logits_process and in
 *   front of the selection gives HF's chain exactly.
 * mk_seq_ban: one workgroup per row, the threads stride over the sequences and compare each prefix with the history's
 *   tail.  Logits bf16 / f16 / f32 [B][V] at pitch ld >= V.  Only the columns that matching sequences name are written:
 *   every other column and the padding [V, ld) keep their bits.  Several threads may store the same -inf to one column:
 *   plain vector stores, no atomics.
 *
 * The stop rule (mk_stop_match): a sample that has not finished finishes at the step whose token makes its GENERATED
 *   tokens end with one of the sequences: out[b][n - m .. n) == q for a sequence of m <= n ids.  The window is the
 *   generated tokens only: it never reaches into the prompt, and a sequence longer than n cannot match.  The matched
 *   sequence stays in the output, as eos does.
 * mk_stop_match: one workgroup per sample, launched right BEHIND mk_decode_emit / mk_decode_emit_sample and in front of
 *   mk_decode_emit_logprobs (whose latch then gives the last token of a stop sequence its real log-probability and the
 *   columns behind it 0.0); the graph loop passes n_dev = state + 1, which the emit has already advanced.  A row whose
 *   done byte is set is not examined; a match stores 1 into done[b] (uint8 [B]); no other byte is written.
 *
 * Both: MK_ERR_BAD_ARG for a null logits / out / seq_ids / seq_off / done, a prompt without p_len, B <= 0, V <= 0,
 *   n_seq <= 0, ld < V, n_max < 0, out_ld < n_max, P < 0, p_ld < P.  MK_ERR_UNSUPPORTED: n_seq > 65536, another dtype. */
int mk_seq_ban(void* logits, int64_t ld, int32_t V, int32_t B, const int64_t* prompt, int64_t p_ld, int32_t P,
               const int32_t* p_len, const int64_t* out, int64_t out_ld, int32_t n_max, const int32_t* n_dev,
               int32_t n_add, const int64_t* seq_ids, const int32_t* seq_off, int32_t n_seq, int32_t dtype, void* stream);
int mk_stop_match(const int64_t* out, int64_t out_ld, int32_t n_max, int32_t B, const int32_t* n_dev, int32_t n_add,
                  const int64_t* seq_ids, const int32_t* seq_off, int32_t n_seq, void* done, void* stream);
/* Grammar-constrained decoding (generate(grammar=)): a deterministic automaton over token ids held in device memory --
 *   what vLLM (guided_regex, guided_choice), TGI (grammar) and outlines offer, and HF's prefix_allowed_tokens_fn without
 *   its Python callback per token -- written down here; restated in numpy / torch in tests/grammar_ref.py, to which the
 *   three kernels are pinned exactly (integers and the -inf bit pattern only).
 *
 * The device table of a grammar: next int32 [n_states][V] at row pitch ld_next >= V, next[s][t] the state after token t
 *   in state s, or -1 when t is not allowed; flags uint8 [n_states], bit 0 = accepting, bit 1 = terminal, which is
 *   accepting with no allowed token.  The table is token-trimmed: a transition into a state from which no accepting
 *   state can be reached by tokens of this vocabulary is -1 (the table's maker does that; the kernels take the table as
 *   it stands).  Per sample: state int32 [B], -1 an unconstrained row, -2 a broken one.
 *
 * The mask rule (mk_grammar_mask), in place, BEHIND mk_logits_process and mk_seq_ban and in front of every selection
 *   (mk_decode_emit, mk_decode_emit_sample, mk_argmax_rows, mk_sample_rows): nothing is written for a row whose done
 *   byte is set, or whose state is < 0 or >= n_states.  Otherwise every column c in [0, V) with next[s][c] < 0 is set to
 *   -inf, and column eos (when 0 <= eos < V) is set to -inf unless flags[s] & 1: the table's own entry in that column is
 *   ignored.  Every other column keeps its bits, +-0, +-inf and NaN included, and so does the padding [V, ld).  This is
 *   HF's PrefixConstrainedLogitsProcessor with the callback allowed(state) + [eos if accepting], with the two
 *   deliberate differences mk_seq_ban documents: the banned column is SET to -inf whatever it held (HF ADDS -inf, which
 *   turns a banned +inf or NaN into NaN), and -0 stays -0.
 *   One launch of (column chunks of 1024, rows) workgroups of 256 threads; a thread reads four entries of the table's row
 *   -- one 16-byte load where ld_next % 4 == 0 and the table is 16-byte aligned, four 4-byte loads otherwise --
 *   and the row offset state * ld_next is computed in 64 bits.  Only banned columns are written.
 *
 * The advance rule (mk_grammar_advance), right BEHIND the emit and in front of mk_stop_match and
 *   mk_decode_emit_logprobs, with n = clamp((n_dev ? *n_dev : 0) + n_add, 0, n_max) read as mk_stop_match reads it: a
 *   row that was done before this launch is skipped (a row whose emit just took eos included), and so is a row with
 *   state < 0.  Otherwise t = out[b][n - 1] and s' = next[s][t], taken as -1 when t is outside [0, V) (and when n == 0,
 *   s >= n_states or s' >= n_states).  s' >= 0: state[b] = s'; if s' is terminal, done[b] = 1 and end[b] = n.  s' < 0,
 *   reachable only when other processors banned every allowed column: state[b] = -2, done[b] = 1, end[b] = n.  The
 *   completing token stays in the output and pad follows it, as with a stop sequence, and it keeps its real
 *   log-probability.  end int32 [B] starts at -1.  The advance is stateful: it runs exactly once per step.  One thread
 *   per row; no other byte is written; plain vector stores, no atomics.
 *
 * mk_grammar_build makes the table of a byte-level automaton: char_next int32 [S][256] (-1: dead), the vocabulary as
 *   tok_bytes uint8 [total], the tokens' bytes back to back, and tok_off int32 [V + 1] ascending from 0.  Entry (s, t)
 *   is char_next walked over token t's bytes from s: -1 on a dead byte transition or an empty token.  One thread per
 *   (state, token), tokens of any length.  The offsets are device memory and are taken as they stand: the caller
 *   (ops.grammar_build) checks on the host that they ascend from 0 before it uploads them.
 *
 * MK_ERR_BAD_ARG for a null pointer (n_dev may be null), B <= 0, V <= 0, S <= 0, n_states <= 0, ld < V, ld_next < V,
 *   n_max < 0, out_ld < n_max.  MK_ERR_UNSUPPORTED: another dtype, more than 65535 rows, S * V >= 2^32 (mk_grammar_build runs one thread per entry). */
int mk_grammar_mask(void* logits, int64_t ld, int32_t V, int32_t B, const int32_t* next, int64_t ld_next, int32_t n_states,
                    const void* flags, const int32_t* state, const void* done, int64_t eos, int32_t dtype, void* stream);
int mk_grammar_advance(const int64_t* out, int64_t out_ld, int32_t n_max, int32_t B, int32_t V, const int32_t* n_dev,
                       int32_t n_add, const int32_t* next, int64_t ld_next, int32_t n_states, const void* flags,
                       int32_t* state, void* done, int32_t* end, void* stream);
int mk_grammar_build(const int32_t* char_next, const void* tok_bytes, const int32_t* tok_off, int32_t S, int32_t V,
                     int32_t* next, int64_t ld_next, void* stream);
/* Token log-probabilities (generate(return_logprobs=True, top_logprobs=n)): how sure the model was of a token, HF's
 *   compute_transition_scores(normalize_logits=True), written down here; restated in numpy in tests/logprobs_ref.py, to
 *   which the kernels are pinned.  The logits are read as they stand in front of the selection: behind the logits
 *   processors, which rewrite them in place, and in front of temperature / top-k / top-p.  Neither emit writes them.
 *
 * The rule, for a row of logits x[0:V) (bf16 / f16 / f32 at pitch ld >= V; columns [V, ld) are never read):
 *   1. m = the fp32 maximum over the columns that are neither NaN nor -inf; S = sum of expf(x_c - m) over the same columns,
 *      accumulated in fp64 in a fixed order: a thread's own columns, then the lane tree, then wave order (mk_beam_emit's
 *      rule; expf, not a fast intrinsic).  lse = (double)m + log(S), kept in fp64.
 *   2. logprob(c) = (float)((double)x_c - lse): a single rounding.  A -inf column gives -inf, a NaN column gives NaN.
 *   3. A row with no finite logit, or with a +inf in it, is degenerate, as in mk_beam_emit: every log-probability of a
 *      degenerate row is NaN.
 *   4. Top-n, for n = top_logprobs > 0: the n columns with the largest x_c, NaN columns excluded (-inf columns are
 *      columns like any other, and -0 == +0), in descending order; ties go to the LOWER column.  The selection is exact,
 *      by order-preserving integer keys as in mk_sample_rows / mk_beam_emit, never decided by arrival order.  When fewer
 *      than n non-NaN columns exist, the remaining slots are id -1 with log-probability -inf (in a degenerate row too).
 *      In a degenerate row the ids are still the n largest keys and their values are NaN.
 *   Deterministic: the same logits give the same bits.
 *
 * mk_token_logprobs: the stand-alone twin of mk_argmax_rows, one workgroup per row: lp[r] = logprob(ids[r]) of row r, NaN
 *   for an id outside [0, V); with n_top > 0 also top_ids int64 [rows][n_top] and top_lp f32 [rows][n_top], both dense.
 * mk_decode_emit_logprobs: the step form, launched right BEHIND mk_decode_emit / mk_decode_emit_sample, one workgroup per
 *   sample: the token is the one the emit just stored in tok[b], the output column is state[1] - 1, read on the device
 *   (the emit has advanced state[1]), and the kernel fills that column of lp f32 [B][n_max] (pitch lp_ld) and, with
 *   n_top > 0, of top_ids int64 [B][n_max][n_top] and top_lp f32 [B][n_max][n_top] (pitch lp_ld * n_top).  A column
 *   outside [0, n_max) writes nothing to them.  A sample that was finished BEFORE this step gets 0.0, top ids pad and
 *   top values 0.0; the step at which it emits eos still gets eos's real log-probability.  done[b] behind the emit
 *   cannot tell the two apart, so the kernel keeps its own latch fin uint8 [B], zero before the first launch: it reads
 *   fin[b], acts on it, then stores done[b] into it (plain vector stores; the latch follows done whatever the column).
 *   Its values are bit for bit mk_token_logprobs' on the same row.
 *   MK_ERR_BAD_ARG: null pointers (top_ids / top_lp may be null only when n_top == 0), rows / B <= 0, V <= 0, ld < V,
 *   n_top < 0, n_max < 0, lp_ld < n_max.  MK_ERR_UNSUPPORTED: n_top > 20, V > 2^23, another dtype. */
int mk_token_logprobs(const void* logits, int64_t ld, int32_t rows, int32_t V, const int64_t* ids, int32_t n_top,
                      float* lp, int64_t* top_ids, float* top_lp, int32_t dtype, void* stream);
int mk_decode_emit_logprobs(const void* logits, int64_t ld, int32_t V, int32_t B, int64_t pad, const int64_t* tok,
                            const void* done, const int32_t* state, void* fin, int32_t n_max, int32_t n_top, float* lp,
                            int64_t lp_ld, int64_t* top_ids, float* top_lp, int32_t dtype, void* stream);
/* Classifier-free guidance (generate(guidance_scale=s, negative_prompt_ids= / negative_inputs_embeds=)): every step is
 *   scored twice, on the caller's prompt and on a negative prompt, and decodes from the combination of the two rows of
 *   log-probabilities -- HF's UnbatchedClassifierFreeGuidanceLogitsProcessor, the first of its processors, written down
 *   here; restated in numpy in tests/cfg_ref.py, to which the kernel is pinned.
 *
 * The rule.  The step's logits are 2B rows (bf16 / f16 / f32 at pitch ld >= V; columns [V, ld) are never read): for sample
 *   b, c is row b (the prompt) and u is row B + b (the negative prompt); the stored values are widened exactly, s is the
 *   fp32 scale widened exactly.
 *   1. lc = c - lse(c) and lu = u - lse(u), each by rules 1 - 3 of "Token log-probabilities" without the rounding: lse
 *      in fp64 over the columns that are neither NaN nor -inf (expf in fp32, the sum accumulated in fp64 in a fixed order);
 *      a -inf column gives -inf, a NaN column NaN; a row with no finite logit, or with a +inf in it, is all NaN.
 *   2. g = lu + s * (lc - lu), in fp64.
 *   3. Where lc or lu is -inf, g = lc: a masked conditional column stays masked, and a column the negative prompt rules
 *      out is not guided.
 *   4. NaN propagates (rule 3 first: lc = -inf next to lu = NaN is -inf).
 *   5. g is rounded ONCE, to nearest even, to the logits' type and stored into row b, in place.
 *   Rows [B, 2B), the columns [V, ld) and everything outside the 2B rows are not written.  Deterministic: the same logits
 *   give the same bits.  s = 1 gives log_softmax(c); the public surface treats it as OFF and launches nothing.
 *
 * mk_cfg_combine: one workgroup per sample, two passes (an online maximum and sum of both rows; the combine and store,
 *   re-reading the rows from L2), 16-byte accesses where the base and the pitch are multiples of 16 bytes.  It reads
 *   nothing from the host: a captured step replays it.
 *   MK_ERR_BAD_ARG (nothing is launched): logits null, B < 1, V < 1, ld < V, a scale that is not finite, another dtype. */
int mk_cfg_combine(void* logits, int64_t ld, int32_t V, int32_t B, float scale, int32_t dtype, void* stream);
/* mk_decode_step_attn: the attention block of one decode step in one launch: p = clamp(*t_dev, 0,
 *   t_max - 1); q and k_new (rows [H * hd] at batch stride in_bs) are rotated with rows p of the
 *   [positions][hd] cos / sin tables (modeling.py:76-91, rope rounding points of mk_rope); the rotated
 *   key and v_new go to row p of the caches; o = attention of the rotated query over keys 0 ... p.
 *   Pinned by tests/test_decode_attn_edges_gpu.py (fp64 reference at every pass and trip edge of the key -> lane map). */
int mk_decode_step_attn(const void* q, const void* k_new, const void* v_new, int64_t in_bs,
                        const void* cos_t, const void* sin_t, void* k_cache, void* v_cache,
                        int64_t kv_ld, int64_t kv_bs, void* o, int64_t o_bs, const int32_t* t_dev,
                        int32_t t_max, int32_t B, int32_t H, int32_t hd, float scale, int32_t dtype,
                        void* stream);
/* e4m3 KV cache (generate(kv_cache="fp8")): the partner of mk_decode_linear_fp8 for the other stream of a decode
 *   step.  ONE format:
 *     bytes   uint8 [B][t_max][2 * D]  a row = [keys of all heads | values of all heads] (D = H * hd), OCP e4m3fn,
 *                                      the shape of the 16-bit cache; keys are quantised AFTER RoPE;
 *     scales  f32   [B][t_max][2 * H]  a row = [key scale of every head | value scale of every head]: one scale per
 *                                      (sample, position, key or value, head) = amax / 448 over that head's hd
 *                                      elements, 1 for an all-zero head.
 *   Quantisation as mk_fp8_quantize_rows with rows = heads: sc = 448 / amax in fp32, x * sc, clamp to +-448,
 *   round to nearest even.  Scales cost 2H * 4 bytes per 2D cache bytes (3 % at hd = 128): 0.52 of the 16-bit cache.
 * mk_kv_quant_append: the prefill's cache write.  k (already rotated) and v: Sn new rows [H * hd] per sample, bf16
 *   or f16, row pitch ld and sample stride in_bs (elements; two pointers, so slices of a fused [M][3D] buffer and
 *   separate k / v storage both work).  Writes bytes and scales of cache rows [t0, t0 + Sn) of every sample and
 *   touches no other row.  MK_ERR_BAD_ARG unless 0 <= t0 and t0 + Sn <= t_max.
 * mk_decode_step_attn_kv8: mk_decode_step_attn over that cache, one launch: p = clamp(*t_dev, 0, t_max - 1); q and
 *   k_new are rotated with rows p of the cos / sin tables (rounding points of mk_rope); the rotated key and v_new
 *   are quantised per head and their bytes and scales go to cache row p; o = attention of the rotated 16-bit query
 *   over rows 0 ... p of the cache AS STORED AFTER THE APPEND (row p enters as the de-quantised quantised value,
 *   which is what later steps read).  De-quantisation in fp32, the scale applied once per key: s_t = scale *
 *   k_scale[t] * sum(q . e4m3), o += p_t * v_scale[t] * e4m3; nothing is rounded to 16 bits in between.
 * Domain of both, else MK_ERR_UNSUPPORTED and nothing is launched: dtype bf16 / f16; hd in {16, 32, 64, 128}; every
 *   pointer 16-byte aligned (the output excepted); ld % 8 == 0 and in_bs % 8 == 0 (elements), pitches and strides
 *   not below H * hd. */
int mk_kv_quant_append(const void* k, const void* v, int64_t ld, int64_t in_bs, void* cache, float* scales,
                       int32_t t0, int32_t Sn, int32_t t_max, int32_t B, int32_t H, int32_t hd, int32_t dtype,
                       void* stream);
/* Pinned by tests/test_decode_attn_edges_gpu.py. */
int mk_decode_step_attn_kv8(const void* q, const void* k_new, const void* v_new, int64_t in_bs, const void* cos_t,
                            const void* sin_t, void* cache, float* scales, void* o, int64_t o_bs,
                            const int32_t* t_dev, int32_t t_max, int32_t B, int32_t H, int32_t hd, float scale,
                            int32_t dtype, void* stream);
/* Padded batches (generate(attention_mask=)): a ragged, compacted KV cache.  Sample b holds its n_b valid prompt
 *   tokens in cache rows 0 ... n_b - 1 and its new token t in row n_b + t, while the step state keeps ONE device
 *   counter *t_dev for the batch.
 * mk_decode_step_attn_var / mk_decode_step_attn_kv8_var: mk_decode_step_attn / mk_decode_step_attn_kv8 at a position
 *   per sample, p_b = clamp(*t_dev + t_off[b], 0, t_max - 1), t_off int32 [B] on the device: RoPE at table row p_b,
 *   append at cache row p_b, attention over rows 0 ... p_b; no row past p_b is read.  The same kernel bodies and the
 *   same kernel selection: a sample's output and appended row are bit-identical to the plain entry point's at
 *   *t_dev = p_b over the same cache.  Domain of the plain entry points; t_off null is MK_ERR_BAD_ARG.
 * mk_kv_append_rows / mk_kv_quant_append_rows: the prefill's compacting cache write.  k (already rotated) and v: Sn
 *   rows [H * hd] per sample, bf16 or f16, row pitch ld and sample stride in_bs (elements; slices of a fused [M][3D]
 *   buffer work).  Source row j of sample b goes to cache row slot[b * Sn + j] (int32, device); a row whose slot is
 *   negative or >= t_max is skipped, and no other cache byte is touched.  mk_kv_append_rows: the 16-bit cache
 *   [B][t_max][2 * H * hd] = [keys | values], a pure copy in 16-byte pieces.  mk_kv_quant_append_rows: the e4m3 cache
 *   above, bytes and scales of a written row identical to mk_kv_quant_append's for that source row.  Two source rows
 *   of a sample with the same slot: one of them wins.  Domain as mk_kv_quant_append. */
/* Pinned by tests/test_decode_attn_edges_gpu.py. */
int mk_decode_step_attn_var(const void* q, const void* k_new, const void* v_new, int64_t in_bs,
                            const void* cos_t, const void* sin_t, void* k_cache, void* v_cache,
                            int64_t kv_ld, int64_t kv_bs, void* o, int64_t o_bs, const int32_t* t_dev,
                            const int32_t* t_off, int32_t t_max, int32_t B, int32_t H, int32_t hd, float scale,
                            int32_t dtype, void* stream);
/* Pinned by tests/test_decode_attn_edges_gpu.py. */
int mk_decode_step_attn_kv8_var(const void* q, const void* k_new, const void* v_new, int64_t in_bs,
                                const void* cos_t, const void* sin_t, void* cache, float* scales, void* o,
                                int64_t o_bs, const int32_t* t_dev, const int32_t* t_off, int32_t t_max, int32_t B,
                                int32_t H, int32_t hd, float scale, int32_t dtype, void* stream);
int mk_kv_append_rows(const void* k, const void* v, int64_t ld, int64_t in_bs, void* cache, const int32_t* slot,
                      int32_t Sn, int32_t t_max, int32_t B, int32_t H, int32_t hd, int32_t dtype, void* stream);
int mk_kv_quant_append_rows(const void* k, const void* v, int64_t ld, int64_t in_bs, void* cache, float* scales,
                            const int32_t* slot, int32_t Sn, int32_t t_max, int32_t B, int32_t H, int32_t hd,
                            int32_t dtype, void* stream);
/* Beam search (generate(num_beams=K)): classic HF BeamSearchScorer semantics, written down here; restated in pure
 *   numpy in tests/beam_ref.py, to which the kernels are pinned.
 *
 * Per-sample state: K running beams with scores s_k (fp32 sums of log-probabilities), a pool of at most K finished
 *   hypotheses, and a done flag.  The length L used for the penalty counts generated tokens only, the eos included.
 *
 * One step, for a sample that is not done.  K_in rows of logits: 1 for the first token (from the prefill), K afterwards.
 *   L is the output column + 1.
 *   1. cand(k, c) = s_k + (x_kc - lse_k) in fp32.  A NaN or -inf logit gives cand = -inf and is never selected.
 *   2. Take the 2K best candidates by value descending.  Ties go to the lower flat index k * V + c.  The selection is
 *      exact (the radix select of mk_sample_rows).
 *   3. Walk them in rank order r = 0, 1, ...
 *        column == eos and r < K:  insert into the pool with score cand / L^length_penalty.
 *        column == eos and r >= K: skip.
 *        any other column: it becomes the next running beam j = 0, 1, ... with parent k, token c and s_j = cand.
 *      Stop when K running beams are filled.  A beam that cannot be filled because no finite candidate is left gets
 *      s = -inf, token pad and parent 0.
 *   4. Pool insert: append while fewer than K entries; otherwise replace the worst entry if the new score is strictly
 *      greater; among equal worst scores, replace the latest inserted.
 *   5. Done.  early_stopping != 0: the pool holds K.  early_stopping == 0: the pool holds K and
 *      s_0 / L^length_penalty <= worst pool score, s_0 the best running beam after this step.
 *   6. A sample that was already done changes nothing in its books.  Its rows are fed pad.
 *   7. eos < 0 never matches (eos_token_id=None).
 * After the last step (on the host): for every sample not done, each running beam with a finite score enters the pool
 *   in beam order with s_k / L^length_penalty.
 * Result: per sample, the pool sorted by score descending, ties to the earlier insertion, first num_return_sequences
 *   entries.  Sequences are recovered by backtracking the per-step (token, parent) history, which is kept on the device
 *   and never overwritten; a pool entry needs only (score, step, parent beam).
 *
 * State layout (all on the device; B samples, K beams, n_max = the most output columns):
 *   tok        int64 [B * K]             the token each (sample, beam) row is fed next
 *   scores     f32   [B * K]             s_k; before the first step s_0 = 0 (rows k >= K_in are not read)
 *   hist       int32 [n_max][B][K][2]    (token, parent beam) of beam j at output column i
 *   ind        int32 [B * K][n_max]      the indirection table: the cache slot of sample b that holds the key of
 *                                        position S0 + i for row (b, k).  Zero it before the first step.
 *   pool_score f32   [B][K]              scores of the finished hypotheses
 *   pool_info  int32 [B][K + 1][4]       per entry (output column of its eos, parent beam, insertion number, 0);
 *                                        row K = (entries, next insertion number, 0, 0).  Zero it before the first step.
 *   done       one byte per sample;  state: int32 [>= 3] = (position, output column, arrival counter) as mk_decode_emit.
 *
 * mk_beam_emit: that step for every sample, one workgroup per sample, at output column col = state[1]: writes tok,
 *   scores, hist[col], the pool and done; updates ind IN PLACE -- new row j = old row parent[j] over columns 0 ... col - 1
 *   (each column permuted by one thread that reads its K entries before it writes any: columns are independent, so no
 *   second table and no step parity), plus ind[j][col] = j for the token about to be fed.  A done sample writes tok =
 *   pad, hist[col] = (pad, j) and ind[j][col] = j only.  The last workgroup to arrive advances state[0] and state[1]
 *   and leaves state[2] zero, exactly as mk_decode_emit.  A column outside [0, n_max) writes neither hist nor ind.
 *   Logits bf16 / f16 / f32 [B * K_in][V] at pitch ld >= V, sample b's rows b * K_in ... b * K_in + K_in - 1.
 *   MK_ERR_BAD_ARG: null pointers, B <= 0, K outside [1, 16], K_in not in {1, K}, V < 2K, ld < V, n_max <= 0.
 *   V <= 2^23, else MK_ERR_UNSUPPORTED.
 * mk_decode_step_attn_beam: mk_decode_step_attn for row (b, k) of a [B][K][t_max][2D] cache (kv_bs = the stride of one
 *   SLOT; row r = b * K + k of q / k_new / v_new / o).  RoPE, append, attention and rounding points are unchanged.  Key
 *   t < S0 is read from slot 0 of sample b (the prompt is stored once per sample and the prefill runs at batch B);
 *   key S0 <= t < p from slot ind[r][t - S0] (clamped into [0, K)); key p comes from the registers and is appended to
 *   row p of the row's own slot k.  No cache row is ever copied.  Everything after the address of a key is
 *   mk_decode_step_attn's code: a row's output is bit-identical to the plain entry point's on a physically gathered
 *   cache with B * K samples (the same kernel selection on B * K * H).  Domain of mk_decode_step_attn; MK_ERR_BAD_ARG
 *   also for ind null, K outside [1, 16], S0 outside [0, t_max], n_ind < max(t_max - S0, 1). */
int mk_beam_emit(const void* logits, int64_t ld, int32_t V, int32_t B, int32_t K, int32_t K_in, int64_t pad,
                 int64_t eos, float length_penalty, int32_t early_stopping, int64_t* tok, float* scores,
                 int32_t* hist, int32_t* ind, int32_t n_max, float* pool_score, int32_t* pool_info, void* done,
                 int32_t* state, int32_t dtype, void* stream);
/* Pinned by tests/test_decode_attn_edges_gpu.py. */
int mk_decode_step_attn_beam(const void* q, const void* k_new, const void* v_new, int64_t in_bs,
                             const void* cos_t, const void* sin_t, void* k_cache, void* v_cache,
                             int64_t kv_ld, int64_t kv_bs, void* o, int64_t o_bs, const int32_t* t_dev,
                             const int32_t* ind, int32_t n_ind, int32_t S0, int32_t t_max, int32_t B, int32_t K,
                             int32_t H, int32_t hd, float scale, int32_t dtype, void* stream);
/* Prompt-lookup speculative decoding (generate(prompt_lookup_num_tokens=G)): HF's prompt_lookup_num_tokens, greedy.  A
 *   step proposes up to G draft tokens per sample by matching an n-gram in the history and verifies them in ONE pass of
 *   Q = G + 1 token rows per sample over the weights.  The rule is written down here and restated in numpy in
 *   tests/spec_ref.py, to which the kernels are pinned.
 *
 * Per-sample state (all on the device; B samples, Q = G + 1, n_max = max_new_tokens; no batch-wide counter and no
 *   arrival counter):
 *   pos      int32 [B]         position and cache row of the row-0 token of the next step
 *   n_out    int32 [B]         tokens emitted so far
 *   done     one byte per sample
 *   out      int64 [B][n_max]  the emitted ids (pitch out_ld); the host fills it with pad before the first step
 *   tok      int64 [B][Q]      the ids fed to the step: column 0 the last emitted token, columns 1 ... G the draft
 *   n_draft  int32 [B]         draft tokens of the step
 *   steps    int32 [B]         verify steps taken (token 0 included)
 *
 * Draft (mk_spec_lookup, one workgroup per sample).  h = prompt history ++ out[b][:n_out[b]], L = |h|; the prompt history
 *   is the processors': prompt int64 [B][P] at pitch p_ld, the first clamp(p_len[b], 0, P) ids of row b, a null pointer
 *   = empty.  For n = min(max_matching_ngram_size, L - 1) down to 1:
 *   1. take the SMALLEST i with i + n < L and h[i:i+n] == h[L-n:L] (the trailing window itself is never a match);
 *   2. on the first n that has such an i, draft = h[i+n : min(i+n+G, L)];
 *   3. cut the draft BEFORE its first eos;
 *   4. stop after that n: if the cut leaves nothing there is no draft, and no smaller n is tried.
 *   This is transformers' PromptLookupCandidateGenerator.get_candidates without a logits processor.  No match, or L < 2,
 *   gives n_draft = 0.  Draft columns beyond n_draft hold pad.  Ids outside [0, V) never match (a window that holds one
 *   equals nothing) and are never proposed (the draft is cut before the first of them, like an eos).  A finished sample
 *   gets n_draft = 0.  eos < 0 never matches (eos_token_id=None).  tok[b][0] is not written.
 *   MK_ERR_BAD_ARG: out, n_out, done, tok or n_draft null, a prompt without p_len, B <= 0, G outside [1, 15],
 *   max_matching_ngram_size < 1, V <= 0, n_max < 0, out_ld < n_max, P < 0, p_ld < P.
 *
 * Step.  Rows (b, g), g = 0 ... G, at row index b * Q + g, carry tok[b][g] at position pos[b] + g.  Every row runs through
 *   every layer and the lm_head whatever n_draft is: the launch sequence is fixed.
 *
 * Verify and emit (mk_spec_verify_emit, one workgroup per sample).  Logits bf16 / f16 / f32 [B * R][V] at pitch ld >= V,
 *   R rows per sample: R = Q for a step, R = 1 for token 0 (the prefill's [B][V] logits: no draft, n_draft is not read).
 *   a_g = the first argmax of row (b, g) over [0, V), with mk_argmax_rows' treatment of NaN and -inf.
 *   A = the number of leading draft tokens with tok[b][1 + j] == a_j, j < n_draft[b].  The step emits a_0 ... a_A, cut
 *   after the first eos (inclusive) and to n_max - n_out[b] tokens.  With m tokens emitted: out[b][n_out ... n_out + m)
 *   receives them, n_out += m, pos += m, steps += 1, done[b] is set on an emitted eos or when n_out == n_max, and
 *   tok[b][0] becomes the last emitted id.  A finished sample changes nothing; its rows keep running at its frozen pos
 *   and touch only cache rows nobody reads.  Token 0 starts from pos[b] = S0 - 1, so that pos[b] = S0 after it.
 *   MK_ERR_BAD_ARG: a null pointer, V <= 0, B <= 0, ld < V, Q outside [1, 16], R not in {1, Q}, n_max < 0,
 *   out_ld < n_max.  Another dtype: MK_ERR_UNSUPPORTED.
 *
 * Multi-query step attention (mk_decode_step_attn_multi, one workgroup per head, sample and row): mk_decode_step_attn for
 *   the B * Q rows of a step.  q, k_new, v_new: rows [H * hd] at ROW stride in_bs, row b * Q + g; o likewise at row
 *   stride o_bs; the 16-bit cache [B][t_max][2D] (kv_ld, kv_bs as mk_decode_step_attn); pos int32 [B] on the device
 *   (negative values count as 0).  For g = 0 ... Q - 1: p = pos[b] + g; RoPE of q and k at row p of the tables
 *   (mk_rope's rounding points); the rotated key and the value go to cache row p; query g attends over keys 0 ... p --
 *   the cached prefix and the new rows 0 ... g of its own sample, nothing later.  Row (b, g)'s output is BIT FOR BIT what
 *   mk_decode_step_attn writes for a single sample at *t_dev = pos[b] + g on a cache whose rows pos[b] ... pos[b] + g - 1
 *   already hold the rotated keys and values of rows 0 ... g - 1 (the one-workgroup-per-head kernel the plain entry
 *   selects for B * H < 512): the same kernel body with the plain kernel's key -> lane / wave assignment and reduction
 *   order.  The Q rows of a (head, sample) run in Q workgroups side by side, at the latency of one plain launch: row g
 *   rotates the keys of rows 0 ... g - 1 itself (into LDS) and reads their values from v_new -- the bits the cache
 *   will hold -- so no workgroup waits for another, and no cache row >= pos[b] is read.  With H a multiple of 8 the Q
 *   workgroups of a (head, sample) share an XCD: the cached prefix comes from HBM once and from that L2 for the other
 *   rows.  A row with pos[b] + g >= t_max writes nothing to the cache, and its output is zeros.
 *   Domain, else MK_ERR_UNSUPPORTED and nothing is launched: dtype bf16 / f16; hd in {16, 32, 64, 128}; Q <= 16;
 *   alignment and strides as mk_decode_step_attn, pos 4-byte aligned.  The kernel keeps no per-key buffer in LDS, so
 *   t_max does not bound the domain.  MK_ERR_BAD_ARG: a null pointer, B, H or t_max <= 0, Q < 1. */
int mk_spec_lookup(const int64_t* prompt, int64_t p_ld, int32_t P, const int32_t* p_len, const int64_t* out,
                   int64_t out_ld, int32_t n_max, const int32_t* n_out, const void* done, int64_t* tok,
                   int32_t* n_draft, int32_t B, int32_t G, int32_t max_matching_ngram_size, int32_t V, int64_t pad,
                   int64_t eos, void* stream);
int mk_spec_verify_emit(const void* logits, int64_t ld, int32_t V, int32_t B, int32_t R, int32_t Q, int64_t eos,
                        int64_t* tok, const int32_t* n_draft, int32_t* pos, int32_t* n_out, void* done, int64_t* out,
                        int64_t out_ld, int32_t n_max, int32_t* steps, int32_t dtype, void* stream);
/* Pinned by tests/test_decode_attn_edges_gpu.py through mk_decode_step_attn, whose bits it reproduces row by row
 *   (tests/test_prompt_lookup_gpu.py). */
int mk_decode_step_attn_multi(const void* q, const void* k_new, const void* v_new, int64_t in_bs, const void* cos_t,
                              const void* sin_t, void* k_cache, void* v_cache, int64_t kv_ld, int64_t kv_bs, void* o,
                              int64_t o_bs, const int32_t* pos, int32_t t_max, int32_t B, int32_t Q, int32_t H,
                              int32_t hd, float scale, int32_t dtype, void* stream);
/* Parallel sampling (generate(num_samples=n)): n samples drawn from ONE prompt.  The prompt's keys and values are stored
 *   once per prompt, prompt cache [B][S0][2D] (p_ld the row pitch, p_bs the stride of a prompt; kp / vp its key and value
 *   halves), and the rows' own tokens in a tail cache [B * n][Tn][2D] (t_ld, t_bs; kt / vt).  Row r = b * n + j of
 *   q / k_new / v_new (row stride in_bs) and o (row stride o_bs) is sample j of prompt b.
 * mk_decode_step_attn_shared: mk_decode_step_attn for those rows, one launch.  Per step:
 *     i   = clamp(*t_dev - S0, 0, Tn - 1)                      the tail row, the same for every row of the launch
 *     L_b = clamp(S0 + (t_off ? t_off[b] : 0), 0, S0)          the prompt's length (t_off int32 [B] on the device or null:
 *                                                              a padded batch's compacted prompt, engine.Ragged.t_off)
 *     p   = L_b + i                                            the row's position
 *   q and k_new are rotated with table row p (mk_rope's rounding points); the rotated key and v_new go to tail row i of
 *   row r; o = attention of the rotated query over prompt rows 0 ... L_b - 1 of prompt b followed by tail rows 0 ... i of
 *   row r.  No prompt byte is written, no tail byte other than row i of each row is written, no tail row past i and no
 *   prompt row past L_b - 1 is read.
 *   One workgroup per (head, prompt, tile of R rows), R = 1 by default and R = 4 on request.  Each row of a tile runs through mk_decode_step_attn's own
 *   kernel body -- the same key -> lane map, trips, online softmax and merge order, only the address of a key differs -- so
 *   a row's output and appended key are BIT FOR BIT those of mk_decode_step_attn called for the row alone (B = 1, the
 *   one-workgroup-per-head form) at *t_dev = p over a physically gathered cache [prompt rows 0 ... L_b - 1 | tail rows
 *   0 ... i - 1].  The rows of a tile run one after the other in their workgroup and share the prompt's keys through the
 *   cache hierarchy (row 0 brings a key from HBM, the others find it in L1 / L2); they do not share a register copy of it:
 *   a body that applies one loaded key to R queries is other code, in which the compiler contracts other products and
 *   sums, and its fp32 sums differ from the plain kernel's in their last bits.  n need not be a multiple of R.  One form at
 *   every B * n * H (the four-heads-per-workgroup form is not tiled).  MK_SHARED_ATTN_ROWS=1 in the environment (read at
 *   every call) selects the R = 1 instantiation (one workgroup per row, the default: the measured faster one,
 *   profiles/decode_nsample_generate.txt), MK_SHARED_ATTN_ROWS=4 the tiled one; both give the same bits.
 *   Domain, else MK_ERR_UNSUPPORTED and nothing is launched: that of mk_decode_step_attn (dtype bf16 / f16; hd in {16, 32,
 *   64, 128}; alignment and strides), t_dev and t_off 4-byte aligned, n <= 32.  MK_ERR_BAD_ARG: a null pointer (t_off
 *   excepted; kp / vp may be null when S0 == 0), B or H <= 0, n < 1, S0 < 0, Tn < 1.
 *   Pinned by tests/test_shared_attn_gpu.py through mk_decode_step_attn, whose bits it reproduces row by row. */
int mk_decode_step_attn_shared(const void* q, const void* k_new, const void* v_new, int64_t in_bs,
                               const void* cos_t, const void* sin_t, const void* kp, const void* vp, int64_t p_ld,
                               int64_t p_bs, void* kt, void* vt, int64_t t_ld, int64_t t_bs, void* o, int64_t o_bs,
                               const int32_t* t_dev, const int32_t* t_off, int32_t S0, int32_t Tn, int32_t B, int32_t n,
                               int32_t H, int32_t hd, float scale, int32_t dtype, void* stream);
/* Scoring (LlamaForCausalLM.score): the log-likelihood of GIVEN answers over a shared prompt.  The rule, restated in
 *   tests/score_ref.py:
 *   There are B prompts; prompt b has L_b valid tokens and n_b <= n options.  Option (b, j) is a token list
 *   c[0 ... len - 1], len >= 1, and its result is, for g = 0 ... len - 1,
 *     lp[b, j, g] = log_softmax(logits of the model at position L_b + g - 1, given prompt b followed by c[0 ... g - 1])[c[g]]
 *   over positions 0 ... L_b + len - 1: what a fresh call on the concatenation alone computes, and what
 *   generate(return_logprobs=True) reports for a token it emitted itself.  Token 0 of every option of prompt b is predicted
 *   by the prompt's last valid hidden row, computed once per prompt; token g >= 1 by the hidden row of FED token g - 1, so an
 *   option feeds its first len - 1 tokens and the pass has F = (longest option) - 1 rows per option (F = 0: no pass at
 *   all).  The arithmetic of a value is mk_token_logprobs' (fp64 log-sum-exp, one rounding).
 * mk_score_attn: the attention of that pass, F teacher-forced rows per option over mk_decode_step_attn_shared's layout.
 *   Row r = (b * n + j) * F + g of q / k_new / v_new (unrotated, row stride in_bs) and of o (row stride o_bs) is fed token g
 *   of option (b, j).  Prompt cache kp / vp [B][S0][2D] (p_ld, p_bs), read only; L_b = clamp(S0 + (t_off ? t_off[b] : 0),
 *   0, S0), t_off int32 [B] on the device or null.  Tail cache kt / vt [B * n][F][2D] (t_ld, t_bs).  len int32 [B * n] ON
 *   THE DEVICE: option (b, j) feeds f = clamp(len[b * n + j], 0, F) rows; the host never reads it.
 *     g < f (a live row): p = L_b + g; q and k_new are rotated with table row p (mk_rope's rounding points); the rotated
 *       key and v_new go to tail row g of the option; o = attention of the rotated query over prompt rows 0 ... L_b - 1 of
 *       prompt b followed by tail rows 0 ... g of the option.
 *     g >= f (a dead row): o is exactly zero, tail row g is not written, and no byte of the row's q / k_new / v_new
 *       influences anything.
 *   No prompt byte is written, no prompt row >= L_b is read, and for row g no tail row > g is read.
 *   Two kernels on the given stream inside the one call: a RoPE-and-append kernel for every live row (one lane group per
 *   row and head, the step body's own rope8, so its bits), then one workgroup per (head, row) that runs
 *   mk_decode_step_attn's kernel body in its shared-prompt form at the row's position WITHOUT the append -- the same key ->
 *   lane map, trips, online softmax and merge order, only the address of a key differs -- while the tail rows 0 ... g - 1 it
 *   reads are the ones the first kernel stored.  So a live row's output and appended key are BIT FOR BIT those of
 *   mk_decode_step_attn called for the row alone (B = 1, the one-workgroup-per-head form) at *t_dev = p over a physically
 *   gathered cache [prompt rows 0 ... L_b - 1 | tail rows 0 ... g - 1].  Any row count: grid.y carries at most 65535 rows
 *   of a launch, and the attention kernel is launched as often as B * n * F needs.
 *   Domain, else MK_ERR_UNSUPPORTED and nothing is launched: that of mk_decode_step_attn (dtype bf16 / f16; hd in {16, 32,
 *   64, 128}; alignment and strides), len and t_off 4-byte aligned, H <= 65535.  n is not bounded here (score() allows 32).
 *   MK_ERR_BAD_ARG: a null pointer (t_off excepted; kp / vp may be null when S0 == 0), B, n, H or F < 1, S0 < 0.
 *   The tables must hold S0 + F rows (ops.score_attn checks).  Pinned by tests/test_score_attn_gpu.py. */
int mk_score_attn(const void* q, const void* k_new, const void* v_new, int64_t in_bs, const void* cos_t,
                  const void* sin_t, const void* kp, const void* vp, int64_t p_ld, int64_t p_bs, void* kt, void* vt,
                  int64_t t_ld, int64_t t_bs, void* o, int64_t o_bs, const int32_t* len, const int32_t* t_off, int32_t S0,
                  int32_t F, int32_t B, int32_t n, int32_t H, int32_t hd, float scale, int32_t dtype, void* stream);
int mk_kv_append(const void* src, void* cache, int32_t cols, int32_t batch, int64_t s_src,
                 int64_t s_cache, int64_t ld_cache, const int32_t* t_dev, int32_t t_max,
                 int32_t elem_size, void* stream);
/* Pinned by tests/test_decode_attn_edges_gpu.py. */
int mk_decode_attn(const void* q, const void* k, const void* v, void* o, const int32_t* t_dev,
                   int32_t t_add, int32_t t_max, int32_t B, int32_t H, int32_t hd, int64_t q_bs,
                   int64_t k_ld, int64_t k_bs, int64_t v_ld, int64_t v_bs, int64_t o_bs, float scale,
                   int32_t dtype, void* stream);

/* ------------------------------------------------------------ optimizer --
 * Fused AdamW over a flat shard (replaces DeepSpeed CPU-offloaded Adam,
 * configs/deepspeed_config.json:2-13): fp32 master/m/v, `dtype` grads and
 * model weights.  grad_scale multiplies grads first (loss scaling / 1/world). */
int mk_adamw(void* param, float* master, float* m, float* v, const void* grad, int64_t n,
             float lr, float beta1, float beta2, float eps, float weight_decay, int32_t step,
             float grad_scale, int32_t dtype, void* stream);

/* Caps mk_adamw's grid (blocks of 256 threads; 0 = default).  A small grid turns the grid-stride update into a
 * persistent kernel that holds only a few CUs: the per-bucket updates of one rank then run BESIDE the backward's
 * GEMMs (planned for fewer CUs through mk_gemm_set_cus) instead of as a serial tail -- the single-GPU counterpart of
 * overlap_comm (configs/deepspeed_config.json:32).  Process-global like mk_gemm_set_cus; returns the previous cap. */
int mk_adamw_set_max_blocks(int32_t n_blocks);

/* A whole training step replayed from a hipGraph (macaw_llm_amd.train.GraphedStep) cannot change
 * kernel ARGUMENTS between steps; the two per-step scalars of the path live in device memory:
 *  - mk_adamw_multi_dev: mk_adamw_multi with hyper_dev = {lr, 1 - beta1^step, 1 - beta2^step,
 *    grad_scale} (device, f32[4]); mk_adamw_bias_correction fills the two corrections on the HOST
 *    with mk_adamw_multi's own arithmetic (bit-identical updates);
 *  - mk_set_dropout_seed_offset: with a device pointer registered every mk_softmax_fwd / _bwd launch
 *    adds *dev_ptr to its seed when it executes; NULL (default) switches it off. */
int mk_adamw_bias_correction(float beta1, float beta2, int32_t step, float* out2);
int mk_adamw_multi_dev(const void* items, const int64_t* chunk_start, int32_t n_items, int64_t n_chunks,
                       float beta1, float beta2, float eps, float weight_decay, const float* hyper_dev,
                       int32_t dtype, void* stream);
int mk_set_dropout_seed_offset(const uint64_t* dev_ptr);

/* ------------------------------------------------------------------ fp8 --
 * BASELINE cfg 5 ("fp8 MFMA for alignment-attn and QKV GEMMs"): per-tensor scaled OCP e4m3.
 * q[i] = e4m3(clamp(x[i] * 448 / amax(|x|), +-448)); *dequant_scale = amax / 448 (1 if amax == 0),
 * written on the DEVICE and handed to mk_gemm as scale_a / scale_b: no host round trip.
 * amax_ws: device float[1] scratch.  n % 8 == 0, 16-byte aligned x, 8-byte aligned q. */
int mk_fp8_quantize(const void* x, int64_t n, int32_t dtype, uint8_t* q, float* amax_ws,
                    float* dequant_scale, void* stream);
/* Per-ROW scaled e4m3 of a row-major (pitched) [rows, cols] bf16 (or f16) matrix (activations, gradients,
 * K-major weights = one scale per output channel): q[r, c] = e4m3(x[r, c] * 448 / amax_r),
 * scales[r] = amax_r / 448 (1 for a zero row).  cols % 8 == 0; GEMM operands need cols % 128 == 0. */
int mk_fp8_quantize_rows(const void* x, int32_t rows, int32_t cols, int64_t ld, int32_t dtype,
                         uint8_t* q, int64_t ldq, float* scales, void* stream);
/* mk_rmsnorm_fwd (LlamaRMSNorm, modeling.py:311-319) with mk_fp8_quantize_rows of its output y folded in: h_out (with
 * res), y, rstd as mk_rmsnorm_fwd writes them, plus q [rows, cols] e4m3 (pitch ldq) and scales[rows] of y -- the
 * activation operand of the fp8 q|k|v GEMM (BASELINE cfg 5) without a second pass over y.  Bit-identical to the two
 * calls.  bf16, cols % 8 == 0, cols <= 16384, contiguous rows, 16-byte aligned. */
int mk_rmsnorm_fwd_fp8(const void* x, const void* res, const void* w, void* h_out, void* y, float* rstd,
                       uint8_t* q, int64_t ldq, float* scales, int32_t rows, int32_t cols, float eps,
                       int32_t dtype, void* stream);
/* Per-COLUMN scaled e4m3 with TRANSPOSED output: qt[c, r] = e4m3(x[r, c] * 448 / amax_c),
 * scales[c] = amax_c / 448 -- the operand of the fp8 grad-input GEMM dx = dy W (the reduction runs
 * over the rows of W [out, in], modeling.py:159-162: nn.Linear stores [out, in]), i.e. W^T K-major
 * with one scale per input channel.  amax_ws: device float[cols] scratch.  rows, cols % 8 == 0. */
int mk_fp8_quantize_cols_t(const void* x, int32_t rows, int32_t cols, int64_t ld, int32_t dtype,
                           uint8_t* qt, int64_t ldqt, float* scales, float* amax_ws, void* stream);

/* ------------------------------------------------------ host-input pipeline --
 * The per-step CPU work of llm_trainer.py:306-381 (get_self_inputs) moved to the GPU.
 *
 * mk_image_transform = CLIP `_transform(n_px)` (llm_trainer.py:150-157): torchvision
 * Resize(n_px, BICUBIC) on a PIL image -> CenterCrop(n_px) -> ToTensor -> Normalize, for a batch
 * of RGB uint8 HWC images of different sizes packed back to back in `src`.  Bit-exact with
 * Pillow 12.2 ImagingResample (libImaging/Resample.c): the host computes Pillow's 22-bit
 * fixed-point bicubic coefficients (macaw_llm_amd/preprocess.py) for the cropped window only.
 *   descs  : n_images x 12 int64 {src_off, H, W, tmp_off, row0, nrows, hk_off, hb_off, hks,
 *            vk_off, vb_off, vks}  (offsets into src/tmp in bytes, into coef in int32 elements)
 *   coef   : int32 coefficient rows [out_px][ks] and bounds [out_px][2] = {first tap, n taps}
 *   lut    : float[3][256] = ((v / 255) - mean[c]) / std[c] as the reference evaluates it
 *   tmp    : scratch for the horizontally resampled rows (sum of nrows * out_px * 3 bytes)
 *   out    : [n_images][3][out_px][out_px] in `dtype` (MK_F32 / MK_BF16 / MK_F16) */
int mk_image_transform(const uint8_t* src, uint8_t* tmp, const int64_t* descs, const int32_t* coef,
                       const float* lut, void* out, int32_t n_images, int32_t out_px,
                       int64_t max_tmp_rows, int32_t dtype, void* stream);

/* mk_log_mel = whisper.log_mel_spectrogram (llm_trainer.py:343, openai-whisper audio.py):
 * torch.stft(audio, 400, 160, hann, center/reflect) -> |.|^2 without the last frame ->
 * mel_filters[n_mels][201] @ . -> log10(clamp 1e-10) -> max(., per-clip max - 8) -> (. + 4) / 4.
 * audio [n_clips][ld] f32 with n_samples (multiple of 160) valid samples per clip;
 * window f32[400]; twiddle f64[400][2] = (cos, sin)(2 pi j / 400); mel_lo/mel_hi = first / one
 * past last non-zero bin of each filter; ws_logspec f32[n_clips * n_mels * n_samples/160],
 * ws_max int32[n_clips]; out [n_clips][n_mels][n_samples/160] in `dtype`. */
int mk_log_mel(const float* audio, int64_t ld, int32_t n_clips, int32_t n_samples,
               const float* window, const double* twiddle, const float* mel_filters,
               const int32_t* mel_lo, const int32_t* mel_hi, int32_t n_mels, float* ws_logspec,
               int32_t* ws_max, void* out, int32_t dtype, void* stream);

/* Multi-tensor AdamW: one launch for a whole list of tensors (same arithmetic per element as
 * mk_adamw).  items: DEVICE array of n_items records {param, master, m, v, grad, n} (6 x 8 bytes,
 * every pointer 16-byte aligned); chunk_start: DEVICE int64[n_items + 1], prefix sum of
 * ceil(n / mk_adamw_chunk()) per item; n_chunks = chunk_start[n_items] (= grid size).  The gradient is read with the
 * non-temporal hint (touched once per step); every store is a plain one. */
/* elements per workgroup slice of mk_adamw_multi / _dev: chunk_start[i] = sum over items j < i of ceil(n_j / mk_adamw_chunk()) */
int mk_adamw_chunk(void);
int mk_adamw_multi(const void* items, const int64_t* chunk_start, int32_t n_items, int64_t n_chunks,
                   float lr, float beta1, float beta2, float eps, float weight_decay, int32_t step,
                   float grad_scale, int32_t dtype, void* stream);

/* ----------------------------------------------------------------- LoRA --
 * Low-rank adapters of the LLaMA projections (macaw_llm_amd/lora.py, peft LoraLayer semantics):
 * y = x W^T + s (drop(x) A^T) B^T with A [r, K], B [N, r] (row-major, 16-byte aligned), s = lora_alpha / r,
 * r a multiple of 8 in [8, 128].  A GROUP is 1-3 modules that share an input (q|k|v, gate|up); unused
 * pointers of a group may be NULL.  Every product runs on the 16x16x32 MFMA (bf16 / f16, fp32 accumulation);
 * every reduction runs in a fixed order (no float atomics): the backward is bit-reproducible.
 * Dropout (inverted, p in [0, 1)): module i keeps x[m, k] iff mk_hash32(seed + offset, tags[i] << 40 | m K + k)
 * < (1 - p) 2^32, offset = the device value of mk_set_dropout_seed_offset (0 without one); tags: HOST
 * uint64[G] (layer, module) read at the call.  Masks are regenerated, never stored.
 *  - mk_lora_down:   U[m, i r + j] = sum_k drop_i(X)[m, k] A_i[j, k]  ->  U [M, G r] and Ut [G r, ldut]
 *                    (pad8(M) <= ldut <= ceil16(M), a multiple of 8; columns [M, ldut) of Ut are written as 0;
 *                    the same pitch for Ut / dUt in mk_lora_bwd_dy and mk_lora_bwd_x)
 *  - mk_lora_up_add: Y_i[m, n] += s sum_j U[m, i r + j] B_i[n, j], rounded once (Y_i [M, N], pitch ldy)
 *  - mk_lora_bwd_dy: dU = s dY_i B_i -> dU [M, G r], dUt [G r, ldut];  dB_i = s dY_i^T U_i (from Ut)
 *  - mk_lora_bwd_x:  dX += sum_i drop'_i(dU_i A_i);  dA_i = dU_i^T drop_i(X)  (dU, dUt from mk_lora_bwd_dy)
 *  - mk_lora_merge:  W[n, k] += s sum_j B[n, j] A[j, k], fp32, one rounding
 * ws: DEVICE scratch of at least mk_lora_workspace(M, N or K, G, r) bytes (merge: with M = 1, G = 1).
 * Launch kind 4 of the in-library profiler (mk_prof_sum). */
int mk_lora_workspace(int32_t M, int32_t N, int32_t G, int32_t r, int64_t* bytes);
int mk_lora_down(const void* X, int64_t ldx, int32_t M, int32_t K, const void* A0, const void* A1,
                 const void* A2, int32_t G, int32_t r, void* U, void* Ut, int64_t ldut, float p,
                 uint64_t seed, const uint64_t* tags, int32_t dtype, void* stream);
int mk_lora_up_add(const void* U, int32_t M, int32_t r, int32_t G, const void* B0, const void* B1,
                   const void* B2, void* Y0, void* Y1, void* Y2, int64_t ldy, int32_t N, float s,
                   int32_t dtype, void* stream);
int mk_lora_bwd_dy(const void* dY0, const void* dY1, const void* dY2, int64_t ldy, int32_t M, int32_t N,
                   const void* B0, const void* B1, const void* B2, const void* Ut, int64_t ldut, int32_t G,
                   int32_t r, float s, void* dU, void* dUt, void* dB0, void* dB1, void* dB2, void* ws,
                   int64_t ws_bytes, int32_t dtype, void* stream);
int mk_lora_bwd_x(const void* X, int64_t ldx, int32_t M, int32_t K, const void* dU, const void* dUt,
                  int64_t ldut, const void* A0, const void* A1, const void* A2, int32_t G, int32_t r, float p,
                  uint64_t seed, const uint64_t* tags, void* dX, int64_t lddx, void* dA0, void* dA1, void* dA2,
                  void* ws, int64_t ws_bytes, int32_t dtype, void* stream);
int mk_lora_merge(void* W, int64_t ldw, int32_t N, int32_t K, const void* A, const void* B, int32_t r,
                  float s, void* ws, int64_t ws_bytes, int32_t dtype, void* stream);

/* Mixed-adapter LoRA of a decode step (csrc/lora_bgmv.hip; generate(adapter_names=), lora.AdapterBank): token row m
 * uses adapter idx[m] (DEVICE int32 [M], read by the kernels: hipGraph-replayable).  A [n_adapters, G r, K] and
 * B [n_adapters, G N, r] stack the group's matrices row-concatenated, one slab per adapter; s: DEVICE f32 [n_adapters].
 *  - mk_lora_bgmv_shrink: U[m, c] = rnd16(sum_k p(X)[m, k] A[idx[m]][c, k]), c < G r, U [M, G r] at pitch ldu.
 *    p = the token prologue of mk_decode_linear with ITS rounding points (0 none; 1 RMSNorm(X; norm_w, eps),
 *    w * rnd16(x * rstd) as mk_rmsnorm_fwd; 2 SwiGLU of X = [gate | up] [M, 2 K], rnd16(rnd16(silu(gate)) * up) as
 *    mk_swiglu2d_fwd): prologue 1 / 2 on X gives the bits of prologue 0 on the prepared rows.
 *  - mk_lora_bgmv_expand: Y[m, i N + n] = rnd16(Y[m, i N + n] + s[idx[m]] sum_j U[m, i r + j] B[idx[m]][i N + n, j]),
 *    Y [M, >= G N] at pitch ldy, one rounding; a column whose sum is exactly 0 (zero-filled rank / module) is not written.
 * Accumulation is fp32 in an order fixed by (K, r): a row's bits do not depend on M or on the other rows, a row computed
 * in a batch equals the row computed alone, no float atomics.  A row with idx[m] outside [0, n_adapters) reads no adapter
 * memory: shrink writes it as a zero row of U, expand does not touch its row of Y.
 * Domain: bf16 / f16, M <= 32, K % 8 == 0 (K <= 30712: the prepared row sits in LDS), N % 8 == 0, r % 8 == 0 in [8, 128], G in [1, 3], pitches
 * multiples of 8, 16-byte aligned pointers; else MK_ERR_UNSUPPORTED.  Launch kind 4 of the in-library profiler. */
int mk_lora_bgmv_shrink(const void* X, int64_t ldx, int32_t M, int32_t K, const void* A, int32_t n_adapters,
                        int32_t G, int32_t r, const int32_t* idx, int32_t prologue, const void* norm_w, float eps,
                        void* U, int64_t ldu, int32_t dtype, void* stream);
int mk_lora_bgmv_expand(const void* U, int64_t ldu, int32_t M, int32_t G, int32_t r, const void* B, const float* s,
                        int32_t n_adapters, const int32_t* idx, void* Y, int64_t ldy, int32_t N, int32_t dtype,
                        void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MACAW_HIP_H */
