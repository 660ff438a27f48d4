// fer_skinny_linear: out[M][N] = act(A' W^T + bias) + R' for M <= 64 rows in bf16 (single-sample / few-sample
// inference, fervit/infer.py), with the LayerNorm of either operand folded in:
//   A' = A or LN(A; gamma_a, beta_a, eps_a)            (normalised on load, row width K)
//   R' = none, res or LN(res; gamma_r, beta_r, eps_r)  (row width N, added in fp32, never rounded to bf16)
//
// Decomposition: at M <= 64 the weight stream is all there is, and it is latency- not bandwidth-bound, so the
// weight is spread over as many CUs as the shape allows: one workgroup per strip of 16 output columns, all M
// rows (N / 16 workgroups: 32 - 128 at the encoder shapes). Inside a workgroup K is split over the 4 waves
// in 32-wide steps, step s to wave s % 4 (neighbouring waves read neighbouring 64-byte halves of a weight line);
// each wave's steps run in increasing order whatever the panel chunking below, so an output element's
// summation order depends on K alone, not on M.
//   * W [N][ldw] goes straight to VGPRs as the MFMA's A operand (v_mfma_f32_16x16x32_bf16: lane l holds W row
//     n0 + (l & 15), k = 8 (l >> 4) ... + 7), read once, a chunk's steps in flight before the first use.
//   * The activation panel goes through LDS (every wave needs every row): chunks of KC columns, 16-byte pieces
//     XOR-swizzled by the row so that the B-operand reads (16 rows at one k) spread over all banks. Rows
//     M .. 16 MT - 1 and columns >= K are zero. With LN-on-load the pieces are normalised on their way in.
//   * The four waves' partial D[n][m] tiles are summed through LDS in wave order 0..3 by the threads that then
//     run the epilogue: lane l holds n = n0 + 4 (l >> 4) ... + 3 of row m = 16 t + (l & 15), one 8-byte store.
//   * Row statistics (fp32, two passes over the stored bf16 values: mean, then centred squares) are recomputed
//     by every workgroup from L2, 16 lanes per row: at most 64 x 768 bf16 = 96 KB per operand. They never
//     go through HBM and there is no LayerNorm launch.
// Workgroups do not communicate: no counters, flags, polling or atomics, so the result is deterministic and
// nothing in the kernel can wait on another workgroup.
#include "common.h"
#include "fervit_internal.h"

namespace fer {

namespace {

constexpr int SK_STRIP = 16;   // output columns per workgroup
constexpr int SK_MAX_M = 64;

struct SkinnyArgs {
  const bf16* A;
  const bf16* W;
  const bf16* res;
  bf16* out;
  const float *bias, *ga, *ba, *gr, *br;
  long lda, ldw, ldr, ldc;
  float eps_a, eps_r;
  int M, N, K, act;
};

// sum over the 16 lanes of a quarter wave, the same bits in each of them
FER_DEV float q16_sum(float v) {
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// st[r] = {mean, rstd} of rows r < M of X [M][ld] over `width` columns; 16 lanes per row, 16 rows per round
FER_DEV void row_stats(const bf16* __restrict__ X, long ld, int M, int width, float eps, float (*st)[2]) {
  const int sub = threadIdx.x & 15, slot = threadIdx.x >> 4;
  for (int r0 = 0; r0 < M; r0 += 16) {
    const int r = r0 + slot;
    const bool live = r < M;
    const bf16* row = X + (long)(live ? r : 0) * ld;  // a slot beyond M reads row 0 (in bounds) and drops it
    float s = 0.f;
    for (int c = sub * 8; c < width; c += 128) {
      float v[8];
      loadp(row + c, v);
      s += ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
    }
    const float mu = q16_sum(s) / (float)width;
    float q = 0.f;
    for (int c = sub * 8; c < width; c += 128) {
      float v[8];
      loadp(row + c, v);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float d = v[i] - mu;
        q = fmaf(d, d, q);
      }
    }
    const float var = q16_sum(q) / (float)width;
    if (live && sub == 0) {
      st[r][0] = mu;
      st[r][1] = 1.0f / sqrtf(var + eps);
    }
  }
}

FER_DEV float skinny_act(int act, float x) {
  if (act == FER_ACT_GELU) return 0.5f * x * (1.0f + erff(x * 0.70710678118654752f));
  return act == FER_ACT_RELU ? fmaxf(x, 0.f) : x;
}

template <int MT> struct SkinnyChunk { static constexpr int KC = MT == 1 ? 1024 : (MT == 2 ? 512 : 256); };

template <int MT>
__global__ __launch_bounds__(256) void skinny_linear_kernel(SkinnyArgs a) {
  constexpr int MP = 16 * MT;             // panel rows
  constexpr int KC = SkinnyChunk<MT>::KC;  // panel columns per chunk: MP * KC * 2 bytes <= 32 KB
  constexpr int PR = KC / 8;              // 16-byte pieces per panel row (>= 16: the swizzle's range)
  constexpr int NS = KC / 128;            // 32-wide k-steps per wave and chunk
  constexpr int FILL = MP * PR / 256;     // pieces per thread and chunk
  __shared__ bf16x8 panel[MP * PR];
  __shared__ f32x4 red[4][MT][64];
  __shared__ float st_a[SK_MAX_M][2], st_r[SK_MAX_M][2];

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 15, q = lane >> 4;
  const int n0 = blockIdx.x * SK_STRIP;
  const bool n_ok = n0 + r < a.N;
  const bf16* wp = a.W + (long)(n_ok ? n0 + r : 0) * a.ldw + q * 8;
  const bf16x8 zero = {};

  // this wave's weight fragments of chunk 0, in flight while the statistics are taken
  bf16x8 wf[NS];
#pragma unroll
  for (int i = 0; i < NS; ++i) {
    const int k = 32 * (wave + 4 * i) + q * 8;
    wf[i] = n_ok && k < a.K ? *(const bf16x8*)(wp + 32 * (wave + 4 * i)) : zero;
  }

  if (a.ga) row_stats(a.A, a.lda, a.M, a.K, a.eps_a, st_a);
  if (a.gr) row_stats(a.res, a.ldr, a.M, a.N, a.eps_r, st_r);
  if (a.ga || a.gr) __syncthreads();

  f32x4 acc[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int kc0 = 0; kc0 < a.K; kc0 += KC) {
    // ---- panel chunk: rows 0 .. MP-1, columns kc0 .. kc0 + KC - 1 (zero beyond M / K)
    bf16x8 pv[FILL];
#pragma unroll
    for (int j = 0; j < FILL; ++j) {
      const int idx = tid + 256 * j, row = idx / PR, k = kc0 + (idx % PR) * 8;
      pv[j] = row < a.M && k < a.K ? *(const bf16x8*)(a.A + (long)row * a.lda + k) : zero;
    }
#pragma unroll
    for (int j = 0; j < FILL; ++j) {
      const int idx = tid + 256 * j, row = idx / PR, p = idx % PR, k = kc0 + p * 8;
      if (a.ga && row < a.M && k < a.K) {
        const float mu = st_a[row][0], rs = st_a[row][1];
        const f32x4 g0 = ldg_f32x4(a.ga + k), g1 = ldg_f32x4(a.ga + k + 4);
        const f32x4 b0 = ldg_f32x4(a.ba + k), b1 = ldg_f32x4(a.ba + k + 4);
        bf16x8 o;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          o[i] = (bf16)fmaf(((float)pv[j][i] - mu) * rs, g0[i], b0[i]);
          o[i + 4] = (bf16)fmaf(((float)pv[j][i + 4] - mu) * rs, g1[i], b1[i]);
        }
        pv[j] = o;
      }
      panel[row * PR + (p ^ (row & 15))] = pv[j];
    }
    __syncthreads();

    // ---- this wave's k-steps of the chunk
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      const int p = 4 * (wave + 4 * i) + q;
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        const bf16x8 x = panel[(16 * t + r) * PR + (p ^ r)];
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[i], x, acc[t], 0, 0, 0);
      }
    }
    // next chunk's weight fragments: in flight during the next panel fill
    if (kc0 + KC < a.K) {
#pragma unroll
      for (int i = 0; i < NS; ++i) {
        const int ks = kc0 + KC + 32 * (wave + 4 * i);
        wf[i] = n_ok && ks + q * 8 < a.K ? *(const bf16x8*)(wp + ks) : zero;
      }
    }
    __syncthreads();  // the panel is rewritten by the next chunk
  }

  // ---- the waves' partial tiles, summed in wave order, and the epilogue
#pragma unroll
  for (int t = 0; t < MT; ++t) red[wave][t][lane] = acc[t];
  __syncthreads();
  if (tid >= 64 * MT) return;
  const int t = wave;  // thread (t, lane): tile t's element set of lane `lane`
  const int m = 16 * t + r, n = n0 + 4 * q;
  if (m >= a.M || n >= a.N) return;
  f32x4 v = ((red[0][t][lane] + red[1][t][lane]) + red[2][t][lane]) + red[3][t][lane];
  if (a.bias) v += ldg_f32x4(a.bias + n);
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = skinny_act(a.act, v[i]);
  if (a.res) {
    const bf16x4 rv = *(const bf16x4*)(a.res + (long)m * a.ldr + n);
    if (a.gr) {
      const float mu = st_r[m][0], rs = st_r[m][1];
      const f32x4 g = ldg_f32x4(a.gr + n), b = ldg_f32x4(a.br + n);
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] += fmaf(((float)rv[i] - mu) * rs, g[i], b[i]);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] += (float)rv[i];
    }
  }
  *(bf16x4*)(a.out + (long)m * a.ldc + n) = bf16x4{(bf16)v[0], (bf16)v[1], (bf16)v[2], (bf16)v[3]};
}

}  // namespace

}  // namespace fer

using namespace fer;

extern "C" int fer_skinny_linear(const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias, int act,
                                 const float* gamma_a, const float* beta_a, float eps_a, const void* res,
                                 int64_t ldr, const float* gamma_r, const float* beta_r, float eps_r, void* out,
                                 int64_t ldc, int M, int N, int K, fer_stream_t stream) {
  if (M < 1 || M > SK_MAX_M) return set_error("skinny_linear: 1 <= M <= 64");
  if (N < 8 || K < 8 || N % 8 || K % 8) return set_error("skinny_linear: N and K must be positive multiples of 8");
  if (act != FER_ACT_NONE && act != FER_ACT_GELU && act != FER_ACT_RELU)
    return set_error("skinny_linear: act must be none, gelu or relu");
  if (!A || !W || !out) return set_error("skinny_linear: A, W and out are required");
  if ((gamma_a == nullptr) != (beta_a == nullptr) || (gamma_r == nullptr) != (beta_r == nullptr))
    return set_error("skinny_linear: a LayerNorm needs both gamma and beta");
  if (gamma_r && !res) return set_error("skinny_linear: gamma_r without res");
  if (lda < K || lda % 8 || ldw < K || ldw % 8 || ldc < N || ldc % 8 || (res && (ldr < N || ldr % 8)))
    return set_error("skinny_linear: every row stride must cover its row and be a multiple of 8");
  if (!al16(A) || !al16(W) || !al16(out) || !al16(res) || !al16(bias) || !al16(gamma_a) || !al16(beta_a) ||
      !al16(gamma_r) || !al16(beta_r))
    return set_error("skinny_linear: every base pointer must be 16-byte aligned");
  SkinnyArgs a;
  a.A = (const bf16*)A, a.W = (const bf16*)W, a.res = (const bf16*)res, a.out = (bf16*)out;
  a.bias = bias, a.ga = gamma_a, a.ba = beta_a, a.gr = gamma_r, a.br = beta_r;
  a.lda = lda, a.ldw = ldw, a.ldr = ldr, a.ldc = ldc;
  a.eps_a = eps_a, a.eps_r = eps_r;
  a.M = M, a.N = N, a.K = K, a.act = act;
  const dim3 grid(ceil_div(N, SK_STRIP));
  dispatch_int<1, 2, 3, 4>(ceil_div(M, 16), [&](auto I) {
    hipLaunchKernelGGL(skinny_linear_kernel<decltype(I)::value>, grid, dim3(256), 0, (hipStream_t)stream, a);
  });
  return hip_check("skinny_linear");
}
