// LoRA adapters of the LLaMA decoder projections (peft LoraLayer semantics, macaw_llm_amd/lora.py):
//   y = x W^T + s * (drop(x) A^T) B^T,   A [r, K], B [N, r], s = lora_alpha / r.
//
// Every product here has one tiny dimension (the rank r), so the kernels are streams over the [M, K] /
// [M, N] activations and HBM bandwidth is their yardstick; the rank-r products run on
// v_mfma_f32_16x16x32 (bf16 / f16) with fp32 accumulation.  Up to three modules that share an input
// (q|k|v on y1, gate|up on y2) form one GROUP: one launch reads the shared operand once.
//
//   rowred   V[m, i*r + j] = scale * sum_k drop_i(X_i)[m, k] Wt_i[j, k]       (down: U = drop(X) A^T;
//            written as V [M, G*r] and as Vt [G*r, ldvt]                       bwd: dU = s dY B)
//   expand   MODE 0: Y_i[m, n] += scale * sum_j V[m, i*r + j] W_i[n, j]       (up-add, merge)
//            MODE 1: Y[m, n]   += sum_i drop'_i(sum_j V[m, i*r + j] W_i[n, j]) (grad-input of the group)
//   colred   P[slab][i][n][j] = sum_{m in slab} drop_i(Y_i)[m, n] Vt[i*r + j, m]   (dB, dA partials)
//   reduce   out_i = scale * sum_slab P  in a fixed order (no float atomics: deterministic)
//
// Dropout masks are never stored: keep(m, k) = mk_hash32(seed, tag_i << 40 | m * K + k) < (1 - p) 2^32, the
// same function in the forward, the backward and a checkpoint recompute.  tag_i = (layer, module) comes from
// the caller, the seed is the step's seed plus the device offset of mk_set_dropout_seed_offset (hipGraph replay).
#include "common.h"
#include "../../include/macaw_hip.h"

const uint64_t* mk_dropout_seed_dev();   // softmax.hip: the registered device seed offset (or NULL)

namespace {

constexpr int LORA_SLAB = 512;   // rows per partial slab of the M reductions (dA, dB)

template <typename T> using x8_t = typename E16<T>::x8;

MK_DEV uint32_t lora_keep_thr(float p) {
  const double k = (1.0 - (double)p) * 4294967296.0;
  return k >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)k;
}

template <typename T> MK_DEV x8_t<T> ld8(const T* p) { return *reinterpret_cast<const x8_t<T>*>(p); }
template <typename T> MK_DEV x8_t<T> zero8() {
  x8_t<T> z;
#pragma unroll
  for (int e = 0; e < 8; ++e) z[e] = (T)0.f;
  return z;
}

// inverted dropout of 8 consecutive elements starting at linear index idx (rounded to T, as the
// dropout output of the 16-bit graph is)
template <typename T>
MK_DEV x8_t<T> drop8(x8_t<T> v, uint64_t seed, uint64_t idx, uint32_t thr, float inv) {
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = (T)(mk_hash32(seed, idx + e) < thr ? (float)v[e] * inv : 0.f);
  return v;
}

struct DropArgs {
  float p;
  uint64_t seed;
  const uint64_t* seed_dev;
  uint64_t tag[3];
};

MK_DEV uint64_t drop_seed(const DropArgs& d) { return d.seed + (d.seed_dev ? *d.seed_dev : 0ull); }

// ------------------------------------------------------------------------------------------ rowred --
template <typename T>
struct RowArgs {
  const T* X[3];
  long ldx;
  int M, K;
  const T* W[3];     // [r, K] row-major each
  int G, r;
  float scale;
  T* V;              // [M, G*r]
  T* Vt;             // [G*r, ldvt]: columns [M, ldvt) are written as 0
  long ldvt;
  DropArgs d;
};

// 16 rows per workgroup, the K loop split over its 4 waves; RT 16-column tiles per module (r <= 16 RT)
template <typename T, int RT, bool DROP>
__global__ __launch_bounds__(256) void lora_rowred_kernel(RowArgs<T> a) {
  __shared__ float red[3 * RT * 256];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int m0 = blockIdx.x * 16;
  const int row = m0 + (lane & 15), kq = 8 * (lane >> 4);
  const bool rok = row < a.M;
  const uint64_t seed = DROP ? drop_seed(a.d) : 0ull;
  const uint32_t thr = lora_keep_thr(a.d.p);
  const float inv = DROP ? 1.f / (1.f - a.d.p) : 1.f;
  const bool shared = a.G == 1 || (a.X[1] == a.X[0] && (a.G < 3 || a.X[2] == a.X[0]));
  f32x4 acc[3][RT];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int t = 0; t < RT; ++t) acc[i][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = w * 32; k0 < a.K; k0 += 128) {
    const int k = k0 + kq;
    const bool kok = k < a.K;
    x8_t<T> x0 = (rok && kok) ? ld8(a.X[0] + (long)row * a.ldx + k) : zero8<T>();
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      if (i >= a.G) break;
      x8_t<T> xi = x0;
      if (i > 0 && !shared) xi = (rok && kok) ? ld8(a.X[i] + (long)row * a.ldx + k) : zero8<T>();
      if (DROP) xi = drop8<T>(xi, seed, (a.d.tag[i] << 40) + (uint64_t)row * a.K + k, thr, inv);
#pragma unroll
      for (int t = 0; t < RT; ++t) {
        const int j = t * 16 + (lane & 15);
        const x8_t<T> wf = (j < a.r && kok) ? ld8(a.W[i] + (long)j * a.K + k) : zero8<T>();
        acc[i][t] = E16<T>::mma16(xi, wf, acc[i][t]);
      }
    }
  }
  // the four K quarters are summed in wave order (fixed: deterministic)
  for (int ww = 0; ww < 4; ++ww) {
    if (w == ww) {
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int t = 0; t < RT; ++t)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            float& dst = red[((i * RT + t) * 64 + lane) * 4 + e];
            dst = ww == 0 ? acc[i][t][e] : dst + acc[i][t][e];
          }
    }
    __syncthreads();
  }
  for (int q = threadIdx.x; q < a.G * RT * 256; q += 256) {
    const int e = q & 3, ln = (q >> 2) & 63, it = q >> 8;
    const int i = it / RT, t = it % RT;
    const int j = t * 16 + (ln & 15), m = m0 + (ln >> 4) * 4 + e;
    if (j >= a.r) continue;
    const T v = (T)(red[q] * a.scale);
    const int c = i * a.r + j;
    if (m < a.M) a.V[(long)m * (a.G * a.r) + c] = v;
    if (m < a.ldvt) a.Vt[(long)c * a.ldvt + m] = m < a.M ? v : (T)0.f;
  }
}

// ------------------------------------------------------------------------------------------ expand --
template <typename T>
struct ExpArgs {
  const T* V;        // [M, ldv], module i at columns [i*r, (i+1)*r)
  long ldv;
  int M, N, G, r;
  const T* W[3];     // [N, r] row-major each
  T* Y[3];           // MODE 0: one output per module; MODE 1: Y[0]
  long ldy;
  float scale;
  DropArgs d;
};

// wave tile: 64 columns n x 32 rows m (4 x 2 MFMA tiles); workgroup: 256 columns.  The MFMA runs as
// Y^T = W V^T so that a lane holds 4 consecutive columns of one row (8-byte read-modify-write).
template <typename T, int MODE, bool DROP>
__global__ __launch_bounds__(256) void lora_expand_kernel(ExpArgs<T> a) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int nb = blockIdx.x * 256 + w * 64, mb = blockIdx.y * 32;
  const int jq = 8 * (lane >> 4);
  const uint64_t seed = DROP ? drop_seed(a.d) : 0ull;
  const uint32_t thr = lora_keep_thr(a.d.p);
  const float inv = DROP ? 1.f / (1.f - a.d.p) : 1.f;
  const int i0 = MODE == 0 ? (int)blockIdx.z : 0, i1 = MODE == 0 ? i0 + 1 : a.G;
  float tot[2][4][4];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
      for (int e = 0; e < 4; ++e) tot[mt][nt][e] = 0.f;
  for (int i = i0; i < i1; ++i) {
    f32x4 acc[2][4];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int j0 = 0; j0 < a.r; j0 += 32) {
      const int j = j0 + jq;
      x8_t<T> vf[2], wf[4];
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) {
        const int m = mb + mt * 16 + (lane & 15);
        vf[mt] = (m < a.M && j < a.r) ? ld8(a.V + (long)m * a.ldv + i * a.r + j) : zero8<T>();
      }
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        const int n = nb + nt * 16 + (lane & 15);
        wf[nt] = (n < a.N && j < a.r) ? ld8(a.W[i] + (long)n * a.r + j) : zero8<T>();
      }
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = E16<T>::mma16(wf[nt], vf[mt], acc[mt][nt]);
    }
    // lane: row m = mb + mt*16 + (lane & 15), columns n = nb + nt*16 + (lane >> 4)*4 + e
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        const int m = mb + mt * 16 + (lane & 15), n = nb + nt * 16 + (lane >> 4) * 4;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float v = acc[mt][nt][e];
          if (DROP && MODE == 1)
            v = mk_hash32(seed, (a.d.tag[i] << 40) + (uint64_t)m * a.N + n + e) < thr ? v * inv : 0.f;
          tot[mt][nt][e] += v;
        }
      }
    if (MODE == 0) {
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
          const int m = mb + mt * 16 + (lane & 15), n = nb + nt * 16 + (lane >> 4) * 4;
          if (m < a.M && n < a.N) {
            T* y = a.Y[i] + (long)m * a.ldy + n;
            typedef T t4 __attribute__((ext_vector_type(4)));
            t4 yv = *reinterpret_cast<t4*>(y);
#pragma unroll
            for (int e = 0; e < 4; ++e) yv[e] = (T)((float)yv[e] + a.scale * tot[mt][nt][e]);
            *reinterpret_cast<t4*>(y) = yv;
          }
#pragma unroll
          for (int e = 0; e < 4; ++e) tot[mt][nt][e] = 0.f;
        }
    }
  }
  if (MODE == 1) {
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        const int m = mb + mt * 16 + (lane & 15), n = nb + nt * 16 + (lane >> 4) * 4;
        if (m < a.M && n < a.N) {
          T* y = a.Y[0] + (long)m * a.ldy + n;
          typedef T t4 __attribute__((ext_vector_type(4)));
          t4 yv = *reinterpret_cast<t4*>(y);
#pragma unroll
          for (int e = 0; e < 4; ++e) yv[e] = (T)((float)yv[e] + a.scale * tot[mt][nt][e]);
          *reinterpret_cast<t4*>(y) = yv;
        }
      }
  }
}

// ------------------------------------------------------------------------------------------ colred --
template <typename T>
struct ColArgs {
  const T* Y[3];     // [M, N] each (pitch ldy)
  long ldy;
  int M, N, G, r;
  const T* Vt;       // [G*r, ldvt]
  long ldvt;
  float* P;          // [nslab][G][N][r]
  DropArgs d;
};

// workgroup: 64 columns n x one slab of LORA_SLAB rows; the [32 x 64] tile of Y goes through LDS so that the
// MFMA's reduction index (m) can be read along a column; wave w owns columns [16 w, 16 w + 16)
template <typename T, int RT, bool DROP>
__global__ __launch_bounds__(256) void lora_colred_kernel(ColArgs<T> a) {
  constexpr int LDT = 64 + 8;
  __shared__ T tile[32 * LDT];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int n0 = blockIdx.x * 64, slab = blockIdx.y, i = blockIdx.z;
  const int mlo = slab * LORA_SLAB, mhi = min(a.M, mlo + LORA_SLAB);
  const uint64_t seed = DROP ? drop_seed(a.d) : 0ull;
  const uint32_t thr = lora_keep_thr(a.d.p);
  const float inv = DROP ? 1.f / (1.f - a.d.p) : 1.f;
  const int lr = threadIdx.x >> 3, lc = (threadIdx.x & 7) * 8;   // loader: row, column of 8 elements
  f32x4 acc[RT];
#pragma unroll
  for (int t = 0; t < RT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int m0 = mlo; m0 < mhi; m0 += 32) {
    const int m = m0 + lr, n = n0 + lc;
    x8_t<T> v = (m < mhi && n < a.N) ? ld8(a.Y[i] + (long)m * a.ldy + n) : zero8<T>();
    if (DROP) v = drop8<T>(v, seed, (a.d.tag[i] << 40) + (uint64_t)m * a.N + n, thr, inv);
    __syncthreads();
    *reinterpret_cast<x8_t<T>*>(&tile[lr * LDT + lc]) = v;
    __syncthreads();
    x8_t<T> af;
    const int kq = 8 * (lane >> 4);
#pragma unroll
    for (int e = 0; e < 8; ++e) af[e] = tile[(kq + e) * LDT + w * 16 + (lane & 15)];
    const int mv = m0 + kq;
#pragma unroll
    for (int t = 0; t < RT; ++t) {
      const int j = t * 16 + (lane & 15);
      const x8_t<T> bf = (j < a.r && mv < mhi) ? ld8(a.Vt + (long)(i * a.r + j) * a.ldvt + mv) : zero8<T>();
      acc[t] = E16<T>::mma16(af, bf, acc[t]);
    }
  }
  // lane: column j = t*16 + (lane & 15), rows n = n0 + 16 w + (lane >> 4)*4 + e
  float* P = a.P + ((long)slab * a.G + i) * (long)a.N * a.r;
#pragma unroll
  for (int t = 0; t < RT; ++t) {
    const int j = t * 16 + (lane & 15);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int n = n0 + w * 16 + (lane >> 4) * 4 + e;
      if (j < a.r && n < a.N) P[(long)n * a.r + j] = acc[t][e];
    }
  }
}

struct RedArgs {
  const float* P;
  int nslab, G, N, r;
  void* out[3];
  int transpose;     // 0: out_i [N, r]; 1: out_i [r, N]
  float scale;
};

template <typename T>
__global__ __launch_bounds__(256) void lora_reduce_kernel(RedArgs a) {
  const long per = (long)a.N * a.r;
  const long q = (long)blockIdx.x * 256 + threadIdx.x;
  if (q >= per * a.G) return;
  const int i = (int)(q / per);
  const long nj = q % per;
  float s = 0.f;
  for (int sl = 0; sl < a.nslab; ++sl) s += a.P[((long)sl * a.G + i) * per + nj];
  const long n = nj / a.r, j = nj % a.r;
  T* o = reinterpret_cast<T*>(a.out[i]);
  o[a.transpose ? j * a.N + n : nj] = (T)(s * a.scale);
}

// out_i[c, r] = in_i[r, c]   (the rank-r operands: tiny)
struct TrArgs {
  const void* in[3];
  int R, C, G;
  void* out;         // [G][C][R]
};
template <typename T>
__global__ __launch_bounds__(256) void lora_transpose_kernel(TrArgs a) {
  const long per = (long)a.R * a.C;
  const long q = (long)blockIdx.x * 256 + threadIdx.x;
  if (q >= per * a.G) return;
  const int i = (int)(q / per);
  const long cr = q % per, c = cr / a.R, rr = cr % a.R;
  reinterpret_cast<T*>(a.out)[q] = reinterpret_cast<const T*>(a.in[i])[rr * a.C + c];
}

// ------------------------------------------------------------------------------------------ host --
bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
int nslab_of(int M) { return (M + LORA_SLAB - 1) / LORA_SLAB; }
long ws_tr(int G, int r, int N) { return ((long)G * r * N * 2 + 255) / 256 * 256; }
long ws_part(int M, int G, int r, int N) { return (long)nslab_of(M) * G * N * r * 4; }

DropArgs mkdrop(float p, uint64_t seed, const uint64_t* tags, int G) {
  DropArgs d{};
  d.p = p;
  d.seed = seed;
  d.seed_dev = mk_dropout_seed_dev();
  for (int i = 0; i < 3; ++i) d.tag[i] = (tags && i < G) ? tags[i] : 0;
  return d;
}

bool rank_ok(int r) { return r >= 8 && r <= 128 && r % 8 == 0; }
bool dtype_ok(int dtype) { return dtype == MK_BF16 || dtype == MK_F16; }
// pitch of Ut / dUt: covers pad8(M) (the column reductions read 8 rows at a time) and stays inside the 16-row
// tiles of the kernel that writes it (columns [M, ldut) are written as 0)
bool ldut_ok(long ldut, int M) { return ldut % 8 == 0 && ldut >= (M + 7) / 8 * 8 && ldut <= (M + 15) / 16 * 16; }

template <typename T>
int transpose_t(const void* const* in, int R, int C, int G, void* out, hipStream_t st) {
  TrArgs a{};
  for (int i = 0; i < G; ++i) a.in[i] = in[i];
  a.R = R; a.C = C; a.G = G; a.out = out;
  const long n = (long)R * C * G;
  MK_LAUNCH((lora_transpose_kernel<T>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a);
  return mk_check_launch();
}

template <typename T, bool DROP>
int rowred_launch(const RowArgs<T>& a, hipStream_t st) {
  const dim3 grid((unsigned)((a.M + 15) / 16)), block(256);
  const int rt = (a.r + 15) / 16;
  if (rt <= 1) MK_LAUNCH((lora_rowred_kernel<T, 1, DROP>), grid, block, 0, st, a);
  else if (rt <= 2) MK_LAUNCH((lora_rowred_kernel<T, 2, DROP>), grid, block, 0, st, a);
  else if (rt <= 4) MK_LAUNCH((lora_rowred_kernel<T, 4, DROP>), grid, block, 0, st, a);
  else MK_LAUNCH((lora_rowred_kernel<T, 8, DROP>), grid, block, 0, st, a);
  return mk_check_launch();
}

template <typename T, bool DROP>
int colred_launch(const ColArgs<T>& a, hipStream_t st) {
  const dim3 grid((unsigned)((a.N + 63) / 64), (unsigned)nslab_of(a.M), (unsigned)a.G), block(256);
  const int rt = (a.r + 15) / 16;
  if (rt <= 1) MK_LAUNCH((lora_colred_kernel<T, 1, DROP>), grid, block, 0, st, a);
  else if (rt <= 2) MK_LAUNCH((lora_colred_kernel<T, 2, DROP>), grid, block, 0, st, a);
  else if (rt <= 4) MK_LAUNCH((lora_colred_kernel<T, 4, DROP>), grid, block, 0, st, a);
  else MK_LAUNCH((lora_colred_kernel<T, 8, DROP>), grid, block, 0, st, a);
  return mk_check_launch();
}

template <typename T>
int reduce_launch(const float* P, int M, int G, int N, int r, void* const* out, int transpose, float scale,
                  hipStream_t st) {
  RedArgs a{};
  a.P = P; a.nslab = nslab_of(M); a.G = G; a.N = N; a.r = r; a.transpose = transpose; a.scale = scale;
  for (int i = 0; i < G; ++i) a.out[i] = out[i];
  const long n = (long)N * r * G;
  MK_LAUNCH((lora_reduce_kernel<T>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a);
  return mk_check_launch();
}

template <typename T>
int expand_launch(const ExpArgs<T>& a, int mode, bool drop, hipStream_t st) {
  const dim3 grid((unsigned)((a.N + 255) / 256), (unsigned)((a.M + 31) / 32), mode == 0 ? (unsigned)a.G : 1u);
  if (mode == 0) MK_LAUNCH((lora_expand_kernel<T, 0, false>), grid, dim3(256), 0, st, a);
  else if (drop) MK_LAUNCH((lora_expand_kernel<T, 1, true>), grid, dim3(256), 0, st, a);
  else MK_LAUNCH((lora_expand_kernel<T, 1, false>), grid, dim3(256), 0, st, a);
  return mk_check_launch();
}

// ---- the five entry points, per element type
template <typename T>
int down_t(const void* X, long ldx, int M, int K, const void* const* A, int G, int r, void* U, void* Ut, long ldut,
           float p, uint64_t seed, const uint64_t* tags, hipStream_t st) {
  RowArgs<T> a{};
  for (int i = 0; i < 3; ++i) { a.X[i] = (const T*)X; a.W[i] = (const T*)A[i < G ? i : 0]; }
  a.ldx = ldx; a.M = M; a.K = K; a.G = G; a.r = r; a.scale = 1.f;
  a.V = (T*)U; a.Vt = (T*)Ut; a.ldvt = ldut;
  a.d = mkdrop(p, seed, tags, G);
  return p > 0.f ? rowred_launch<T, true>(a, st) : rowred_launch<T, false>(a, st);
}

template <typename T>
int up_add_t(const void* U, int M, int r, int G, const void* const* B, void* const* Y, long ldy, int N, float s,
             hipStream_t st) {
  ExpArgs<T> a{};
  a.V = (const T*)U; a.ldv = (long)G * r; a.M = M; a.N = N; a.G = G; a.r = r; a.ldy = ldy; a.scale = s;
  for (int i = 0; i < G; ++i) { a.W[i] = (const T*)B[i]; a.Y[i] = (T*)Y[i]; }
  return expand_launch<T>(a, 0, false, st);
}

template <typename T>
int bwd_dy_t(const void* const* dY, long ldy, int M, int N, const void* const* B, const void* Ut, long ldut, int G,
             int r, float s, void* dU, void* dUt, void* const* dB, char* ws, hipStream_t st) {
  T* Bt = reinterpret_cast<T*>(ws);                                  // [G][r][N]
  float* P = reinterpret_cast<float*>(ws + ws_tr(G, r, N));
  int rc = transpose_t<T>(B, N, r, G, Bt, st);
  if (rc) return rc;
  RowArgs<T> a{};
  for (int i = 0; i < 3; ++i) {
    const int ii = i < G ? i : 0;
    a.X[i] = (const T*)dY[ii];
    a.W[i] = Bt + (long)ii * r * N;
  }
  a.ldx = ldy; a.M = M; a.K = N; a.G = G; a.r = r; a.scale = s;
  a.V = (T*)dU; a.Vt = (T*)dUt; a.ldvt = ldut;
  a.d = mkdrop(0.f, 0, nullptr, G);
  if ((rc = rowred_launch<T, false>(a, st))) return rc;
  ColArgs<T> c{};
  for (int i = 0; i < 3; ++i) c.Y[i] = (const T*)dY[i < G ? i : 0];
  c.ldy = ldy; c.M = M; c.N = N; c.G = G; c.r = r; c.Vt = (const T*)Ut; c.ldvt = ldut; c.P = P;
  c.d = mkdrop(0.f, 0, nullptr, G);
  if ((rc = colred_launch<T, false>(c, st))) return rc;
  return reduce_launch<T>(P, M, G, N, r, dB, 0, s, st);
}

template <typename T>
int bwd_x_t(const void* X, long ldx, int M, int K, const void* dU, const void* dUt, long ldut, const void* const* A,
            int G, int r, float p, uint64_t seed, const uint64_t* tags, void* dX, long lddx, void* const* dA, char* ws,
            hipStream_t st) {
  T* At = reinterpret_cast<T*>(ws);                                  // [G][K][r]
  float* P = reinterpret_cast<float*>(ws + ws_tr(G, r, K));
  int rc = transpose_t<T>(A, r, K, G, At, st);
  if (rc) return rc;
  const DropArgs d = mkdrop(p, seed, tags, G);
  ExpArgs<T> e{};
  e.V = (const T*)dU; e.ldv = (long)G * r; e.M = M; e.N = K; e.G = G; e.r = r; e.ldy = lddx; e.scale = 1.f; e.d = d;
  for (int i = 0; i < G; ++i) e.W[i] = At + (long)i * K * r;
  e.Y[0] = (T*)dX;
  if ((rc = expand_launch<T>(e, 1, p > 0.f, st))) return rc;
  ColArgs<T> c{};
  for (int i = 0; i < 3; ++i) c.Y[i] = (const T*)X;
  c.ldy = ldx; c.M = M; c.N = K; c.G = G; c.r = r; c.Vt = (const T*)dUt; c.ldvt = ldut; c.P = P; c.d = d;
  if ((rc = p > 0.f ? colred_launch<T, true>(c, st) : colred_launch<T, false>(c, st))) return rc;
  return reduce_launch<T>(P, M, G, K, r, dA, 1, 1.f, st);
}

template <typename T>
int merge_t(void* W, long ldw, int N, int K, const void* A, const void* B, int r, float s, char* ws, hipStream_t st) {
  T* At = reinterpret_cast<T*>(ws);                                  // [K][r]
  const void* in[1] = {A};
  int rc = transpose_t<T>(in, r, K, 1, At, st);
  if (rc) return rc;
  ExpArgs<T> e{};
  e.V = (const T*)B; e.ldv = r; e.M = N; e.N = K; e.G = 1; e.r = r; e.ldy = ldw; e.scale = s;
  e.W[0] = At; e.Y[0] = (T*)W;
  return expand_launch<T>(e, 0, false, st);
}

bool ptrs_ok(const void* const* p, int G) {
  for (int i = 0; i < G; ++i)
    if (!p[i] || !al16(p[i])) return false;
  return true;
}

}  // namespace

#define MK_ST reinterpret_cast<hipStream_t>(stream)
#define MK_LORA_DISPATCH(fn, args)                               \
  do {                                                           \
    int rc_;                                                     \
    if (dtype == MK_BF16) rc_ = fn<bf16> args;                   \
    else rc_ = fn<_Float16> args;   /* (dtype_ok: checked before mkp::begin) */ \
    mkp::end(prof, MK_ST);                                       \
    return rc_;                                                  \
  } while (0)

extern "C" int mk_lora_workspace(int32_t M, int32_t N, int32_t G, int32_t r, int64_t* bytes) {
  if (!bytes || M <= 0 || N <= 0 || G < 1 || G > 3 || !rank_ok(r)) return MK_ERR_BAD_ARG;
  *bytes = ws_tr(G, r, N) + ws_part(M, G, r, N);
  return MK_OK;
}

extern "C" int mk_lora_down(const void* X, int64_t ldx, int32_t M, int32_t K, const void* A0, const void* A1,
                            const void* A2, int32_t G, int32_t r, void* U, void* Ut, int64_t ldut, float p,
                            uint64_t seed, const uint64_t* tags, int32_t dtype, void* stream) {
  const void* A[3] = {A0, A1, A2};
  if (!X || !U || !Ut || M <= 0 || K <= 0 || G < 1 || G > 3 || !rank_ok(r) || ldx < K || !ldut_ok(ldut, M) ||
      p < 0.f || p >= 1.f)
    return MK_ERR_BAD_ARG;
  if (!dtype_ok(dtype) || K % 8 || ldx % 8 || !al16(X) || !ptrs_ok(A, G) || (p > 0.f && !tags))
    return MK_ERR_UNSUPPORTED;
  const int prof = mkp::begin(MK_ST, 4, 2.0 * M * K * G * r, M, G * r, K, 1, 0, 0);
  MK_LORA_DISPATCH(down_t, (X, ldx, M, K, A, G, r, U, Ut, ldut, p, seed, tags, MK_ST));
}

extern "C" int mk_lora_up_add(const void* U, int32_t M, int32_t r, int32_t G, const void* B0, const void* B1,
                              const void* B2, void* Y0, void* Y1, void* Y2, int64_t ldy, int32_t N, float s,
                              int32_t dtype, void* stream) {
  const void* B[3] = {B0, B1, B2};
  void* Y[3] = {Y0, Y1, Y2};
  if (!U || M <= 0 || N <= 0 || G < 1 || G > 3 || !rank_ok(r) || ldy < N) return MK_ERR_BAD_ARG;
  if (!dtype_ok(dtype) || N % 8 || ldy % 8 || !al16(U) || !ptrs_ok(B, G) || !ptrs_ok(Y, G)) return MK_ERR_UNSUPPORTED;
  const int prof = mkp::begin(MK_ST, 4, 2.0 * M * N * G * r, M, N * G, r, 1, 1, 0);
  MK_LORA_DISPATCH(up_add_t, (U, M, r, G, B, Y, ldy, N, s, MK_ST));
}

extern "C" int mk_lora_bwd_dy(const void* dY0, const void* dY1, const void* dY2, int64_t ldy, int32_t M, int32_t N,
                              const void* B0, const void* B1, const void* B2, const void* Ut, int64_t ldut, int32_t G,
                              int32_t r, float s, void* dU, void* dUt, void* dB0, void* dB1, void* dB2, void* ws,
                              int64_t ws_bytes, int32_t dtype, void* stream) {
  const void* dY[3] = {dY0, dY1, dY2};
  const void* B[3] = {B0, B1, B2};
  void* dB[3] = {dB0, dB1, dB2};
  if (!Ut || !dU || !dUt || !ws || M <= 0 || N <= 0 || G < 1 || G > 3 || !rank_ok(r) || ldy < N || !ldut_ok(ldut, M))
    return MK_ERR_BAD_ARG;
  if (ws_bytes < ws_tr(G, r, N) + ws_part(M, G, r, N)) return MK_ERR_BAD_ARG;
  if (!dtype_ok(dtype) || N % 8 || ldy % 8 || !al16(Ut) || !al16(ws) || !ptrs_ok(dY, G) || !ptrs_ok(B, G) || !ptrs_ok(dB, G))
    return MK_ERR_UNSUPPORTED;
  const int prof = mkp::begin(MK_ST, 4, 4.0 * M * N * G * r, M, N * G, r, 1, 2, 0);
  MK_LORA_DISPATCH(bwd_dy_t, (dY, ldy, M, N, B, Ut, ldut, G, r, s, dU, dUt, dB, (char*)ws, MK_ST));
}

extern "C" int mk_lora_bwd_x(const void* X, int64_t ldx, int32_t M, int32_t K, const void* dU, const void* dUt,
                             int64_t ldut, const void* A0, const void* A1, const void* A2, int32_t G, int32_t r, float p,
                             uint64_t seed, const uint64_t* tags, void* dX, int64_t lddx, void* dA0, void* dA1, void* dA2,
                             void* ws, int64_t ws_bytes, int32_t dtype, void* stream) {
  const void* A[3] = {A0, A1, A2};
  void* dA[3] = {dA0, dA1, dA2};
  if (!X || !dU || !dUt || !dX || !ws || M <= 0 || K <= 0 || G < 1 || G > 3 || !rank_ok(r) || ldx < K || lddx < K ||
      !ldut_ok(ldut, M) || p < 0.f || p >= 1.f)
    return MK_ERR_BAD_ARG;
  if (ws_bytes < ws_tr(G, r, K) + ws_part(M, G, r, K)) return MK_ERR_BAD_ARG;
  if (!dtype_ok(dtype) || K % 8 || ldx % 8 || lddx % 8 || !al16(X) || !al16(dU) || !al16(dUt) || !al16(dX) || !al16(ws) ||
      !ptrs_ok(A, G) || !ptrs_ok(dA, G) || (p > 0.f && !tags))
    return MK_ERR_UNSUPPORTED;
  const int prof = mkp::begin(MK_ST, 4, 4.0 * M * K * G * r, M, K * G, r, 1, 3, 0);
  MK_LORA_DISPATCH(bwd_x_t, (X, ldx, M, K, dU, dUt, ldut, A, G, r, p, seed, tags, dX, lddx, dA, (char*)ws, MK_ST));
}

extern "C" int mk_lora_merge(void* W, int64_t ldw, int32_t N, int32_t K, const void* A, const void* B, int32_t r,
                             float s, void* ws, int64_t ws_bytes, int32_t dtype, void* stream) {
  if (!W || !A || !B || !ws || N <= 0 || K <= 0 || !rank_ok(r) || ldw < K || ws_bytes < ws_tr(1, r, K))
    return MK_ERR_BAD_ARG;
  if (!dtype_ok(dtype) || K % 8 || ldw % 8 || !al16(W) || !al16(A) || !al16(B) || !al16(ws)) return MK_ERR_UNSUPPORTED;
  const int prof = mkp::begin(MK_ST, 4, 2.0 * N * K * r, N, K, r, 1, 4, 0);
  MK_LORA_DISPATCH(merge_t, (W, ldw, N, K, A, B, r, s, (char*)ws, MK_ST));
}
