// The two ends of every model around the transformer trunk (HBM-bound kernels): patch im2col,
// token assembly (CLS + pos + dropout) and its gradient, the classification head (LN + Linear on
// the CLS rows) and its gradient, and softmax cross-entropy. The per-chunk / per-sample gradient
// partials are summed by part_reduce (reduce.hip).
#include "common.h"
#include "fervit_internal.h"
#include "step_seed.h"

namespace fer {

// ------------------------------------------------------------------ im2col
template <typename T>
__global__ __launch_bounds__(256) void im2col_kernel(const float* __restrict__ x, int B, int C, int Hh, int Ww, int P,
                                                     T* __restrict__ cols, long ldc) {
  const int gh = Hh / P, gw = Ww / P, K = C * P * P;
  const long total = (long)B * gh * gw * K;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256L) {
    const int k = i % K;
    const long tok = i / K;
    const int gx = tok % gw, gy = (tok / gw) % gh, b = tok / ((long)gw * gh);
    const int c = k / (P * P), kh = (k / P) % P, kw = k % P;
    cols[tok * ldc + k] = from_f<T>(x[(((long)b * C + c) * Hh + gy * P + kh) * Ww + gx * P + kw]);
  }
}

// 4 consecutive kw per thread (P % 4 == 0, Ww % 4 == 0, ldc % 4 == 0): one 16-byte input load
// and one 4-element store, 32-bit index arithmetic (total / 4 < 2^31, checked by the host).
template <typename T>
__global__ __launch_bounds__(256) void im2col4_kernel(const float* __restrict__ x, int B, int C, int Hh, int Ww,
                                                      int P, T* __restrict__ cols, long ldc) {
  const int gh = Hh / P, gw = Ww / P, K = C * P * P, K4 = K >> 2, PP = P * P;
  const int total = B * gh * gw * K4;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    const int k = (i % K4) * 4;
    const int tok = i / K4;
    const int gx = tok % gw, gy = (tok / gw) % gh, b = tok / (gw * gh);
    const int c = k / PP, kh = (k / P) % P, kw = k % P;
    const f32x4 v = *(const f32x4*)(x + (((long)b * C + c) * Hh + gy * P + kh) * Ww + gx * P + kw);
    store4<T>(cols + (long)tok * ldc + k, v);
  }
}

// ------------------------------------------------------------------ tokens
// 4 consecutive d per thread (D % 4 == 0); dropout keep bits identical to the scalar form.
template <typename T>
__global__ __launch_bounds__(256) void tokens_fwd4_kernel(const T* __restrict__ emb, const float* __restrict__ cls,
                                                          const float* __restrict__ pos, T* __restrict__ t, int B,
                                                          int n, int D, uint32_t thr, float dscale, uint64_t seed) {
  seed = step_seed(seed);
  const int N = n + 1, D4 = D >> 2;
  const long total = (long)B * N * D4;
  for (long i4 = blockIdx.x * 256L + threadIdx.x; i4 < total; i4 += (long)gridDim.x * 256L) {
    const int d = (int)(i4 % D4) * 4;
    const long row = i4 / D4;
    const int tk = (int)(row % N), b = (int)(row / N);
    f32x4 v = tk == 0 ? *(const f32x4*)(cls + d) : load4<T>(emb + ((long)b * n + tk - 1) * D + d);
    v += *(const f32x4*)(pos + (long)tk * D + d);
    if (thr) drop4(seed, (uint32_t)(row * D + d), thr, dscale, v);
    store4<T>(t + row * D + d, v);
  }
}

// bf16 with D % 8 == 0 (ViT-B: 256 x 197 x 768): 8 consecutive d per thread (16-byte loads and stores) and
// 32-bit index arithmetic (the 4-wide form's 64-bit divisions per element group were most of its time); the
// same per-element values and keep bits (two keep4 per 8 elements).
__global__ __launch_bounds__(256) void tokens_fwd8_kernel(const bf16* __restrict__ emb, const float* __restrict__ cls,
                                                          const float* __restrict__ pos, bf16* __restrict__ t, int B,
                                                          int n, int D, uint32_t thr, float dscale, uint64_t seed) {
  seed = step_seed(seed);
  const uint32_t N = n + 1, D8 = D >> 3;
  const uint32_t total = (uint32_t)B * N * D8;  // (host: < 2^31)
  for (uint32_t i8 = blockIdx.x * 256u + threadIdx.x; i8 < total; i8 += gridDim.x * 256u) {
    const uint32_t row = i8 / D8, d = (i8 - row * D8) * 8;
    const uint32_t b = row / N, tk = row - b * N;
    f32x4 v0, v1;
    if (tk == 0) {
      v0 = *(const f32x4*)(cls + d);
      v1 = *(const f32x4*)(cls + d + 4);
    } else {
      const bf16x8 e = *(const bf16x8*)(emb + ((long)b * n + tk - 1) * D + d);
      v0 = f32x4{(float)e[0], (float)e[1], (float)e[2], (float)e[3]};
      v1 = f32x4{(float)e[4], (float)e[5], (float)e[6], (float)e[7]};
    }
    v0 += *(const f32x4*)(pos + (long)tk * D + d);
    v1 += *(const f32x4*)(pos + (long)tk * D + d + 4);
    if (thr) {
      const uint32_t idx = row * (uint32_t)D + d;
      drop4(seed, idx, thr, dscale, v0);
      drop4(seed, idx + 4, thr, dscale, v1);
    }
    *(bf16x8*)(t + (long)row * D + d) =
        bf16x8{(bf16)v0[0], (bf16)v0[1], (bf16)v0[2], (bf16)v0[3], (bf16)v1[0], (bf16)v1[1], (bf16)v1[2], (bf16)v1[3]};
  }
}

template <typename T>
__global__ __launch_bounds__(256) void tokens_fwd_kernel(const T* __restrict__ emb, const float* __restrict__ cls,
                                                         const float* __restrict__ pos, T* __restrict__ t, int B,
                                                         int n, int D, uint32_t thr, float dscale, uint64_t seed) {
  seed = step_seed(seed);
  const int N = n + 1;
  const long total = (long)B * N * D;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256L) {
    const int d = i % D;
    const long row = i / D;
    const int tk = row % N, b = row / N;
    float v = tk == 0 ? cls[d] : to_f<T>(emb[((long)b * n + tk - 1) * D + d]);
    v += pos[(long)tk * D + d];
    if (thr) v = drop_keep(seed, (uint32_t)i, thr) ? v * dscale : 0.f;
    t[i] = from_f<T>(v);
  }
}
// dpos partial per b-chunk; demb written directly
template <typename T>
__global__ __launch_bounds__(256) void tokens_bwd_kernel(const T* __restrict__ dt, T* __restrict__ demb, int B, int n,
                                                         int D, uint32_t thr, float dscale, uint64_t seed,
                                                         float* __restrict__ part, int bchunk) {
  seed = step_seed(seed);
  const int N = n + 1;
  const long cols = (long)N * D;
  const long j = blockIdx.x * 256L + threadIdx.x;  // (token, d)
  if (j >= cols) return;
  const int tk = j / D;
  const int b0 = blockIdx.y * bchunk, b1 = min(B, b0 + bchunk);
  float s = 0.f;
  for (int b = b0; b < b1; ++b) {
    const long i = (long)b * cols + j;
    float g = to_f<T>(dt[i]);
    if (thr) g = drop_keep(seed, (uint32_t)i, thr) ? g * dscale : 0.f;
    s += g;
    if (tk > 0 && demb) demb[((long)b * n + tk - 1) * D + (j % D)] = from_f<T>(g);
  }
  part[(long)blockIdx.y * cols + j] = s;
}
// 4 consecutive (token, d) columns per thread (D % 4 == 0: one token): 8/16-byte loads and
// stores and one keep4 per 4 elements instead of a hash per element; same per-element values
// and the same summation order over b as tokens_bwd_kernel (bit-identical partials).
template <typename T>
__global__ __launch_bounds__(256) void tokens_bwd4_kernel(const T* __restrict__ dt, T* __restrict__ demb, int B, int n,
                                                          int D, uint32_t thr, float dscale, uint64_t seed,
                                                          float* __restrict__ part, int bchunk) {
  seed = step_seed(seed);
  const int N = n + 1;
  const long cols = (long)N * D;
  const long j = (blockIdx.x * 256L + threadIdx.x) * 4;  // (token, d), d % 4 == 0
  if (j >= cols) return;
  const int tk = j / D, d = j - (long)tk * D;
  const int b0 = blockIdx.y * bchunk, b1 = min(B, b0 + bchunk);
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  for (int b = b0; b < b1; ++b) {
    const long i = (long)b * cols + j;
    f32x4 g = load4<T>(dt + i);
    if (thr) {
      const uint32_t k = keep4(seed, (uint32_t)i, thr);
#pragma unroll
      for (int r = 0; r < 4; ++r) g[r] = (k >> r) & 1 ? g[r] * dscale : 0.f;
    }
    s += g;
    if (tk > 0 && demb) store4<T>(demb + ((long)b * n + tk - 1) * D + d, g);
  }
  *(f32x4*)(part + (long)blockIdx.y * cols + j) = s;
}
// bf16 with D % 8 == 0 (ViT-B's token gradient, 50,432 x 768): 8 consecutive columns per thread (16-byte
// loads and stores), four batch rows in flight per iteration, and 16 batch chunks instead of 64 (a quarter
// of the fp32 partial slabs the reduction reads: 9.7 instead of 38.7 MB at ViT-B). Per column the batch
// rows of a chunk are summed in ascending order, as in tokens_bwd4_kernel.
__global__ __launch_bounds__(256) void tokens_bwd8_kernel(const bf16* __restrict__ dt, bf16* __restrict__ demb, int B,
                                                          int n, int D, uint32_t thr, float dscale, uint64_t seed,
                                                          float* __restrict__ part, int bchunk) {
  seed = step_seed(seed);
  const int N = n + 1;
  const long cols = (long)N * D;
  const long j = (blockIdx.x * 256L + threadIdx.x) * 8;  // (token, d), d % 8 == 0
  if (j >= cols) return;
  const int tk = j / D, d = j - (long)tk * D;
  const int b0 = blockIdx.y * bchunk, b1 = min(B, b0 + bchunk);
  f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = s0;
  auto one = [&](int b, bf16x8 v) {
    f32x4 g0 = f32x4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
    f32x4 g1 = f32x4{(float)v[4], (float)v[5], (float)v[6], (float)v[7]};
    if (thr) {
      const uint32_t i = (uint32_t)((long)b * cols + j);
      const uint32_t k = keep4(seed, i, thr) | (keep4(seed, i + 4, thr) << 4);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        g0[r] = (k >> r) & 1 ? g0[r] * dscale : 0.f;
        g1[r] = (k >> (4 + r)) & 1 ? g1[r] * dscale : 0.f;
      }
    }
    s0 += g0;
    s1 += g1;
    if (tk > 0 && demb)
      *(bf16x8*)(demb + ((long)b * n + tk - 1) * D + d) =
          bf16x8{(bf16)g0[0], (bf16)g0[1], (bf16)g0[2], (bf16)g0[3], (bf16)g1[0], (bf16)g1[1], (bf16)g1[2], (bf16)g1[3]};
  };
  int b = b0;
  for (; b + 4 <= b1; b += 4) {
    bf16x8 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = *(const bf16x8*)(dt + (long)(b + u) * cols + j);
#pragma unroll
    for (int u = 0; u < 4; ++u) one(b + u, v[u]);
  }
  for (; b < b1; ++b) one(b, *(const bf16x8*)(dt + (long)b * cols + j));
  *(f32x4*)(part + (long)blockIdx.y * cols + j) = s0;
  *(f32x4*)(part + (long)blockIdx.y * cols + j + 4) = s1;
}
__global__ void tokens_bwd_final(const float* __restrict__ part, int nchunk, int N, int D, float* dcls, float* dpos,
                                 int accumulate) {
  const long j = blockIdx.x * 256L + threadIdx.x;
  if (j >= (long)N * D) return;
  float s = 0.f;
  for (int c = 0; c < nchunk; ++c) s += part[(long)c * N * D + j];
  if (dpos) dpos[j] = accumulate ? dpos[j] + s : s;
  if (j < D && dcls) dcls[j] = accumulate ? dcls[j] + s : s;
}

// ------------------------------------------------------------------ head
// One block (256 threads) per sample. stats[b] = {mean, rstd}.
template <typename T>
__global__ __launch_bounds__(256) void head_fwd_kernel(const T* __restrict__ t, long rs, const float* __restrict__ lw,
                                                       const float* __restrict__ lb, float eps,
                                                       const float* __restrict__ W, const float* __restrict__ bias,
                                                       float* __restrict__ logits, float* __restrict__ stats, int D,
                                                       int C, uint32_t thr, float dscale, uint64_t seed) {
  seed = step_seed(seed);
  __shared__ float h[1024];
  __shared__ float red[8];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const T* x = t + (long)b * rs;
  float s = 0.f;
  for (int d = tid; d < D; d += 256) {
    const float v = to_f<T>(x[d]);
    h[d] = v;
    s += v;
  }
  s = wave_sum(s);
  if (lane == 0) red[w] = s;
  __syncthreads();
  const float mu = (red[0] + red[1] + red[2] + red[3]) / D;
  float q = 0.f;
  for (int d = tid; d < D; d += 256) q += (h[d] - mu) * (h[d] - mu);
  q = wave_sum(q);
  __syncthreads();
  if (lane == 0) red[4 + w] = q;
  __syncthreads();
  const float rsd = rsqrtf((red[4] + red[5] + red[6] + red[7]) / D + eps);
  for (int d = tid; d < D; d += 256) {
    float v = (h[d] - mu) * rsd * lw[d] + lb[d];
    if (thr) v = drop_keep(seed, (uint32_t)b * (uint32_t)D + (uint32_t)d, thr) ? v * dscale : 0.f;
    h[d] = v;
  }
  __syncthreads();
  for (int c = w; c < C; c += 4) {
    float a = 0.f;
    for (int d = lane; d < D; d += 64) a += h[d] * W[(long)c * D + d];
    a = wave_sum(a);
    if (lane == 0) logits[(long)b * C + c] = a + bias[c];
  }
  if (tid == 0) {
    stats[2 * b] = mu;
    stats[2 * b + 1] = rsd;
  }
}
// part[b] = [dW (C*D) | dbias (C) | dln_w (D) | dln_b (D)]
template <typename T>
__global__ __launch_bounds__(256) void head_bwd_kernel(const T* __restrict__ t, long rs, const float* __restrict__ lw,
                                                       const float* __restrict__ lb, const float* __restrict__ W,
                                                       const float* __restrict__ stats,
                                                       const float* __restrict__ dlogits, T* __restrict__ dt, int D,
                                                       int C, uint32_t thr, float dscale, uint64_t seed,
                                                       float* __restrict__ part) {
  seed = step_seed(seed);
  __shared__ float xh[1024], gh[1024];
  __shared__ float red[8];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const T* x = t + (long)b * rs;
  const float mu = stats[2 * b], rsd = stats[2 * b + 1];
  const long pstride = (long)C * D + C + 2 * D;
  float* pp = part + (long)b * pstride;
  float s1 = 0.f, s2 = 0.f;
  for (int d = tid; d < D; d += 256) {
    const float xhat = (to_f<T>(x[d]) - mu) * rsd;
    float hv = xhat * lw[d] + lb[d];
    bool keep = true;
    if (thr) keep = drop_keep(seed, (uint32_t)b * (uint32_t)D + (uint32_t)d, thr);
    const float hd = thr ? (keep ? hv * dscale : 0.f) : hv;
    float g = 0.f;
    for (int c = 0; c < C; ++c) {
      const float dl = dlogits[(long)b * C + c];
      g += dl * W[(long)c * D + d];
      pp[(long)c * D + d] = dl * hd;
    }
    if (thr) g = keep ? g * dscale : 0.f;
    pp[(long)C * D + C + d] = g * xhat;  // dln_w
    pp[(long)C * D + C + D + d] = g;     // dln_b
    const float gg = g * lw[d];
    xh[d] = xhat;
    gh[d] = gg;
    s1 += gg;
    s2 += gg * xhat;
  }
  for (int c = tid; c < C; c += 256) pp[(long)C * D + c] = dlogits[(long)b * C + c];  // dbias, any C
  s1 = wave_sum(s1);
  s2 = wave_sum(s2);
  if (lane == 0) {
    red[w] = s1;
    red[4 + w] = s2;
  }
  __syncthreads();
  const float m1 = (red[0] + red[1] + red[2] + red[3]) / D, m2 = (red[4] + red[5] + red[6] + red[7]) / D;
  for (int d = tid; d < D; d += 256) dt[(long)b * rs + d] = from_f<T>((gh[d] - m1 - xh[d] * m2) * rsd);
}
__global__ void head_bwd_final(const float* __restrict__ part, int B, int C, int D, float* dW, float* dbias,
                               float* dlw, float* dlb, int accumulate) {
  const long pstride = (long)C * D + C + 2 * D;
  const long j = blockIdx.x * 256L + threadIdx.x;
  if (j >= pstride) return;
  float s = 0.f;
  for (int b = 0; b < B; ++b) s += part[(long)b * pstride + j];
  float* o;
  long k;
  if (j < (long)C * D) { o = dW; k = j; }
  else if (j < (long)C * D + C) { o = dbias; k = j - (long)C * D; }
  else if (j < (long)C * D + C + D) { o = dlw; k = j - (long)C * D - C; }
  else { o = dlb; k = j - (long)C * D - C - D; }
  if (!o) return;
  o[k] = accumulate ? o[k] + s : s;
}
template <typename T>
__global__ void zero_rows4_kernel(T* __restrict__ dt, long rows, int D_ld, int D, long stride_keep) {
  const int D4 = D >> 2;
  const long total = rows * (long)D4;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256L) {
    const long r = i / D4;
    if (r % stride_keep) store4<T>(dt + r * D_ld + (i % D4) * 4, f32x4{0.f, 0.f, 0.f, 0.f});
  }
}
template <typename T>
__global__ void zero_rows_kernel(T* __restrict__ dt, long rows, int D_ld, int D, long stride_keep) {
  const long total = rows * (long)D;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256L) {
    const long r = i / D;
    if (r % stride_keep) dt[r * D_ld + (i % D)] = from_f<T>(0.f);
  }
}

// ------------------------------------------------------------------ cross entropy
__global__ __launch_bounds__(256) void ce_kernel(const float* __restrict__ logits, const int64_t* __restrict__ y,
                                                 const float* __restrict__ wt, int B, int C, float ls, float gscale,
                                                 float* loss, float* dlogits) {
  // single block; pass 1: per-sample terms; pass 2: normalise
  __shared__ float red[2][4];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  float num = 0.f, den = 0.f;
  for (int b = tid; b < B; b += 256) {
    const float* z = logits + (long)b * C;
    float m = -INFINITY;
    for (int c = 0; c < C; ++c) m = fmaxf(m, z[c]);
    float se = 0.f;
    for (int c = 0; c < C; ++c) se += expf(z[c] - m);
    // -log p_c = log(se) + (m - z_c): the difference first (exact for nearby logits), so the term keeps
    // its own precision; (m + log(se)) - z_c rounds the sum to an ulp of |m| (5e-4 at logits ~1e4)
    const float lg = logf(se);
    const int yb = (int)y[b];
    const float wy = wt ? wt[yb] : 1.f;
    float sm = 0.f;
    for (int c = 0; c < C; ++c) sm += (wt ? wt[c] : 1.f) * (lg + (m - z[c]));
    num += (1.f - ls) * wy * (lg + (m - z[yb])) + ls / C * sm;
    den += wy;
  }
  num = wave_sum(num);
  den = wave_sum(den);
  if (lane == 0) {
    red[0][w] = num;
    red[1][w] = den;
  }
  __syncthreads();
  const float N = red[0][0] + red[0][1] + red[0][2] + red[0][3];
  const float Dn = red[1][0] + red[1][1] + red[1][2] + red[1][3];
  if (tid == 0 && loss) *loss = N / Dn;
  if (!dlogits) return;
  for (int b = tid; b < B; b += 256) {
    const float* z = logits + (long)b * C;
    float m = -INFINITY;
    for (int c = 0; c < C; ++c) m = fmaxf(m, z[c]);
    float se = 0.f;
    for (int c = 0; c < C; ++c) se += expf(z[c] - m);
    const int yb = (int)y[b];
    const float wy = wt ? wt[yb] : 1.f;
    float wsum = 0.f;
    for (int c = 0; c < C; ++c) wsum += wt ? wt[c] : 1.f;
    for (int c = 0; c < C; ++c) {
      const float p = expf(z[c] - m) / se;
      // d/dz_c of (1-ls) wy (lse - z_y) + ls/C sum_k w_k (lse - z_k)
      float g = (1.f - ls) * wy * (p - (c == yb ? 1.f : 0.f)) + ls / C * (wsum * p - (wt ? wt[c] : 1.f));
      dlogits[(long)b * C + c] = g * gscale / Dn;
    }
  }
}

}  // namespace fer

using namespace fer;

extern "C" int fer_im2col_patch(int dtype, const float* x, int B, int C, int Hh, int Ww, int P, void* cols,
                                int64_t ldc, fer_stream_t stream) {
  if (check_dtype(dtype, "im2col_patch: unknown dtype")) return -1;
  const long total = (long)B * (Hh / P) * (Ww / P) * C * P * P;
  if (total <= 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  if (P % 4 == 0 && Ww % 4 == 0 && ldc % 4 == 0 && total / 4 < 0x7FFFFFFFL && (uintptr_t)x % 16 == 0) {
    with_dtype(dtype, [&](auto tag) {
      using T = typename decltype(tag)::type;
      hipLaunchKernelGGL(im2col4_kernel<T>, dim3(grid_for(total / 4)), dim3(256), 0, st, x, B, C, Hh, Ww, P, (T*)cols,
                         (long)ldc);
    });
    return hip_check("im2col_patch");
  }
  with_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(im2col_kernel<T>, dim3(grid_for(total)), dim3(256), 0, st, x, B, C, Hh, Ww, P, (T*)cols,
                       (long)ldc);
  });
  return hip_check("im2col_patch");
}

extern "C" int fer_tokens_fwd(int dtype, const void* emb, const float* cls, const float* pos, void* t, int B, int n,
                              int D, uint32_t drop_thresh, float drop_scale, uint64_t seed, fer_stream_t stream) {
  if (check_dtype(dtype, "tokens_fwd: unknown dtype")) return -1;
  const long total = (long)B * (n + 1) * D;
  if (total <= 0) return 0;
  if (check_drop_range(drop_thresh, total, "tokens_fwd: dropout over >= 2^32 elements")) return -1;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == FER_BF16 && D % 8 == 0 && total < (1L << 31)) {
    hipLaunchKernelGGL(tokens_fwd8_kernel, dim3(grid_for(total / 8)), dim3(256), 0, st, (const bf16*)emb, cls, pos,
                       (bf16*)t, B, n, D, drop_thresh, drop_scale, seed);
    return hip_check("tokens_fwd8");
  }
  if (D % 4 == 0) {
    with_dtype(dtype, [&](auto tag) {
      using T = typename decltype(tag)::type;
      hipLaunchKernelGGL(tokens_fwd4_kernel<T>, dim3(grid_for(total / 4)), dim3(256), 0, st, (const T*)emb, cls, pos,
                         (T*)t, B, n, D, drop_thresh, drop_scale, seed);
    });
    return hip_check("tokens_fwd");
  }
  with_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(tokens_fwd_kernel<T>, dim3(grid_for(total)), dim3(256), 0, st, (const T*)emb, cls, pos, (T*)t,
                       B, n, D, drop_thresh, drop_scale, seed);
  });
  return hip_check("tokens_fwd");
}

static int tokens_chunks(int B) { return std::max(1, std::min(B, 64)); }
extern "C" int64_t fer_tokens_bwd_ws(int B, int N, int D) { return (int64_t)tokens_chunks(B) * N * D * 4; }

extern "C" int fer_tokens_bwd(int dtype, const void* dt, void* demb, float* dcls, float* dpos, int accumulate, int B,
                              int n, int D, uint32_t drop_thresh, float drop_scale, uint64_t seed, float* ws,
                              int64_t ws_bytes, fer_stream_t stream) {
  if (check_dtype(dtype, "tokens_bwd: unknown dtype")) return -1;
  const int N = n + 1;
  if (B <= 0) return 0;
  const int nch = tokens_chunks(B);
  if (!ws || ws_bytes < fer_tokens_bwd_ws(B, N, D)) return set_error("tokens_bwd: workspace too small");
  if (check_drop_range(drop_thresh, (long)B * N * D, "tokens_bwd: dropout over >= 2^32 elements")) return -1;
  int bchunk = ceil_div(B, nch);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == FER_BF16 && D % 8 == 0) {
    const int nch8 = std::min(nch, 16);  // (the workspace is sized for tokens_chunks(B) >= nch8 slabs)
    bchunk = ceil_div(B, nch8);
    dim3 grid8(ceil_div((long)N * D / 8, 256), nch8);
    hipLaunchKernelGGL(tokens_bwd8_kernel, grid8, dim3(256), 0, st, (const bf16*)dt, (bf16*)demb, B, n, D, drop_thresh,
                       drop_scale, seed, ws, bchunk);
    if (dpos) part_reduce(ws, nch8, (long)N * D, N * D, N * D, dpos, nullptr, nullptr, accumulate, nullptr, st);
    if (dcls) part_reduce(ws, nch8, (long)N * D, D, D, dcls, nullptr, nullptr, accumulate, nullptr, st);
    return hip_check("tokens_bwd8");
  }
  if (D % 4 == 0) {
    dim3 grid4(ceil_div((long)N * D / 4, 256), nch);
    with_dtype(dtype, [&](auto tag) {
      using T = typename decltype(tag)::type;
      hipLaunchKernelGGL(tokens_bwd4_kernel<T>, grid4, dim3(256), 0, st, (const T*)dt, (T*)demb, B, n, D, drop_thresh,
                         drop_scale, seed, ws, bchunk);
    });
  } else {
    dim3 grid(ceil_div((long)N * D, 256), nch);
    with_dtype(dtype, [&](auto tag) {
      using T = typename decltype(tag)::type;
      hipLaunchKernelGGL(tokens_bwd_kernel<T>, grid, dim3(256), 0, st, (const T*)dt, (T*)demb, B, n, D, drop_thresh,
                         drop_scale, seed, ws, bchunk);
    });
  }
  if (dpos) part_reduce(ws, nch, (long)N * D, N * D, N * D, dpos, nullptr, nullptr, accumulate, nullptr, st);
  if (dcls) part_reduce(ws, nch, (long)N * D, D, D, dcls, nullptr, nullptr, accumulate, nullptr, st);
  return hip_check("tokens_bwd");
}

extern "C" int fer_head_fwd(int dtype, const void* t, int64_t row_stride, const float* ln_w, const float* ln_b,
                            float eps, const float* W, const float* bias, float* logits, float* stats, int B, int D,
                            int C, uint32_t drop_thresh, float drop_scale, uint64_t seed, fer_stream_t stream) {
  if (check_dtype(dtype, "head_fwd: unknown dtype")) return -1;
  if (B <= 0) return 0;
  if (D > 1024) return set_error("head_fwd: D <= 1024");
  hipStream_t st = (hipStream_t)stream;
  with_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(head_fwd_kernel<T>, dim3(B), dim3(256), 0, st, (const T*)t, (long)row_stride, ln_w, ln_b, eps,
                       W, bias, logits, stats, D, C, drop_thresh, drop_scale, seed);
  });
  return hip_check("head_fwd");
}

extern "C" int64_t fer_head_bwd_ws(int B, int D, int C) { return (int64_t)B * ((int64_t)C * D + C + 2 * D) * 4; }

extern "C" int fer_head_bwd(int dtype, const void* t, int64_t row_stride, const float* ln_w, const float* ln_b,
                            const float* W, const float* stats, const float* dlogits, void* dt, int zero_rest,
                            int rows_total, int D_ld, float* dln_w, float* dln_b, float* dW, float* dbias,
                            int accumulate, int B, int D, int C, uint32_t drop_thresh, float drop_scale,
                            uint64_t seed, float* ws, int64_t ws_bytes, fer_stream_t stream) {
  if (check_dtype(dtype, "head_bwd: unknown dtype")) return -1;
  if (B <= 0) return 0;
  if (D > 1024) return set_error("head_bwd: D <= 1024");
  if (!ws || ws_bytes < fer_head_bwd_ws(B, D, C)) return set_error("head_bwd: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  if (zero_rest && D % 4 == 0 && D_ld % 4 == 0) {
    const long total = (long)rows_total * D / 4;
    with_dtype(dtype, [&](auto tag) {
      using T = typename decltype(tag)::type;
      hipLaunchKernelGGL(zero_rows4_kernel<T>, dim3(grid_for(total)), dim3(256), 0, st, (T*)dt, (long)rows_total,
                         D_ld, D, (long)(row_stride / D_ld));
    });
  } else if (zero_rest) {
    const long total = (long)rows_total * D;
    with_dtype(dtype, [&](auto tag) {
      using T = typename decltype(tag)::type;
      hipLaunchKernelGGL(zero_rows_kernel<T>, dim3(grid_for(total)), dim3(256), 0, st, (T*)dt, (long)rows_total, D_ld,
                         D, (long)(row_stride / D_ld));
    });
  }
  with_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(head_bwd_kernel<T>, dim3(B), dim3(256), 0, st, (const T*)t, (long)row_stride, ln_w, ln_b, W,
                       stats, dlogits, (T*)dt, D, C, drop_thresh, drop_scale, seed, ws);
  });
  const long ps = (long)C * D + C + 2 * D;
  if (dW) part_reduce(ws, B, ps, C * D, C * D, dW, nullptr, nullptr, accumulate, nullptr, st);
  if (dbias) part_reduce(ws + (long)C * D, B, ps, C, C, dbias, nullptr, nullptr, accumulate, nullptr, st);
  if (dln_w || dln_b) part_reduce(ws + (long)C * D + C, B, ps, 2 * D, D, dln_w, dln_b, nullptr, accumulate, nullptr, st);
  return hip_check("head_bwd");
}

extern "C" int fer_cross_entropy(const float* logits, const int64_t* labels, const float* weight, int B, int C,
                                 float label_smoothing, float grad_scale, float* loss, float* dlogits,
                                 fer_stream_t stream) {
  if (B <= 0) return 0;
  hipLaunchKernelGGL(ce_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, logits, labels, weight, B, C,
                     label_smoothing, grad_scale, loss, dlogits);
  return hip_check("cross_entropy");
}
