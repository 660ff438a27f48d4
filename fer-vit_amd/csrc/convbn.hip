// LatentCNN operators (reference `models_fer_vit/latent_cnn.py`): the k = 3 Conv1d as im2col around
// fer_gemm, BatchNorm1d with its ReLU / residual / dropout epilogue, the sequence mean pool and the
// small-N classifier. Token-major [M = B*L][C] throughout, so the reference's transpose(1, 2) is
// free and BatchNorm's channel axis is the column axis.
//
// All of them are latency- and HBM-bound at the model's sizes (M = 1,152 rows at batch 64, 1.2 MB
// per activation: resident in L2). Memory pieces are 16 bytes (8 bf16 / 4 fp32 columns), as in
// layernorm.hip.
//
// BatchNorm runs one workgroup per 16-byte column slab: its 256 threads walk the M rows of the slab
// three times (sum -> mean, sum of squared deviations -> variance, normalise + epilogue; the second
// and third walk hit L2), so the statistics are a true two-pass mean / variance, every reduction
// stays inside one workgroup in a fixed order (wave butterflies, then the four waves in order), and
// the whole layer is one launch with no partial slabs, no second reduction launch and no atomics.
// The backward has the same shape: dgamma / dbeta are complete inside the workgroup before dx needs
// them. Repeat calls are bit-identical. C = 512 gives 64 (bf16) or 128 (fp32) workgroups.
#include "common.h"
#include "fervit_internal.h"
#include "step_seed.h"

namespace fer {

// ---------------------------------------------------------------- conv1d im2col
// cols[m][c*3 + k] = x[m + k - 1][c] inside the sample, 0 outside: a gather, values copied bit for bit.
template <typename T>
__global__ __launch_bounds__(256) void conv1d_cols_kernel(const T* __restrict__ x, long ldx, T* __restrict__ cols,
                                                          long ldc, int L, int C, long M) {
  constexpr int V = Pc<T>::V;
  const int pieces = 3 * C / V;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= M * pieces) return;
  const long m = i / pieces;
  const int j0 = (int)(i - m * pieces) * V;
  const int l = (int)(m % L);
  typename Pc<T>::vec out;
#pragma unroll
  for (int r = 0; r < V; ++r) {
    const int j = j0 + r, c = j / 3, k = j - 3 * c;
    const int ll = l + k - 1;
    out[r] = (ll >= 0 && ll < L) ? x[(m + k - 1) * ldx + c] : (T)0.f;
  }
  *(typename Pc<T>::vec*)(cols + m * ldc + j0) = out;
}

// dx[m][c] = (res[m][c] +) dcols[m+1][3c] + dcols[m][3c+1] + dcols[m-1][3c+2] (k = 0, 1, 2 in that
// order), rows outside the sample left out. res: the gradient arriving over a residual connection.
template <typename T>
__global__ __launch_bounds__(256) void conv1d_cols_bwd_kernel(const T* __restrict__ dcols, long ldd,
                                                              const T* __restrict__ res, long ldr,
                                                              T* __restrict__ dx, long lddx, int L, int C, long M) {
  constexpr int V = Pc<T>::V;
  const int pieces = C / V;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= M * pieces) return;
  const long m = i / pieces;
  const int c0 = (int)(i - m * pieces) * V;
  const int l = (int)(m % L);
  float s[V];
#pragma unroll
  for (int r = 0; r < V; ++r) s[r] = 0.f;
  if (res) loadp(res + m * ldr + c0, s);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int ll = l - k + 1;
    if (ll < 0 || ll >= L) continue;
    const T* row = dcols + (m - k + 1) * ldd + 3 * c0;  // 3*V consecutive elements, 16-byte aligned
    float a[3][V];
    loadp(row, a[0]);
    loadp(row + V, a[1]);
    loadp(row + 2 * V, a[2]);
#pragma unroll
    for (int r = 0; r < V; ++r) {
      const int j = 3 * r + k;
      s[r] += a[j / V][j % V];
    }
  }
  storep(dx + m * lddx + c0, s);
}

// ---------------------------------------------------------------- BatchNorm
FER_DEV float bn_val(float x, float mu, float rs, float g, float b) { return fmaf((x - mu) * rs, g, b); }

template <typename T>
__global__ __launch_bounds__(256) void bn_fwd_kernel(const T* __restrict__ x, long ldx, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, float* rmean, float* rvar,
                                                     long long* nbt, int train, float momentum, float eps,
                                                     const T* __restrict__ res, long ldr, int relu, uint32_t thr,
                                                     float dscale, uint64_t seed, T* __restrict__ y, long ldy,
                                                     float* __restrict__ mean_out, float* __restrict__ rstd_out, int M,
                                                     int C) {
  constexpr int V = Pc<T>::V;
  seed = step_seed(seed);
  __shared__ float red[4][V];
  const int c0 = blockIdx.x * V;
  float mu[V], rs[V];
  if (train) {
    float s[V], q[V];
#pragma unroll
    for (int i = 0; i < V; ++i) s[i] = q[i] = 0.f;
    for (int r = threadIdx.x; r < M; r += 256) {
      float v[V];
      loadp(x + (long)r * ldx + c0, v);
#pragma unroll
      for (int i = 0; i < V; ++i) s[i] += v[i];
    }
    block_sum<V>(s, red);
#pragma unroll
    for (int i = 0; i < V; ++i) mu[i] = s[i] / (float)M;
    for (int r = threadIdx.x; r < M; r += 256) {
      float v[V];
      loadp(x + (long)r * ldx + c0, v);
#pragma unroll
      for (int i = 0; i < V; ++i) {
        const float d = v[i] - mu[i];
        q[i] = fmaf(d, d, q[i]);
      }
    }
    block_sum<V>(q, red);
#pragma unroll
    for (int i = 0; i < V; ++i) rs[i] = 1.0f / sqrtf(q[i] / (float)M + eps);
    if (threadIdx.x == 0) {
#pragma unroll
      for (int i = 0; i < V; ++i) {
        if (rmean) rmean[c0 + i] = (1.0f - momentum) * rmean[c0 + i] + momentum * mu[i];
        if (rvar) rvar[c0 + i] = (1.0f - momentum) * rvar[c0 + i] + momentum * (q[i] / (float)(M - 1));
      }
      if (nbt && blockIdx.x == 0) *nbt += 1;
    }
  } else {
#pragma unroll
    for (int i = 0; i < V; ++i) {
      mu[i] = rmean[c0 + i];
      rs[i] = 1.0f / sqrtf(rvar[c0 + i] + eps);
    }
  }
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < V; ++i) {
      if (mean_out) mean_out[c0 + i] = mu[i];
      if (rstd_out) rstd_out[c0 + i] = rs[i];
    }
  }
  float g[V], b[V];
#pragma unroll
  for (int i = 0; i < V; ++i) {
    g[i] = gamma[c0 + i];
    b[i] = beta[c0 + i];
  }
  for (int r = threadIdx.x; r < M; r += 256) {
    float v[V];
    loadp(x + (long)r * ldx + c0, v);
#pragma unroll
    for (int i = 0; i < V; ++i) v[i] = bn_val(v[i], mu[i], rs[i], g[i], b[i]);
    if (res) {
      float t[V];
      loadp(res + (long)r * ldr + c0, t);
#pragma unroll
      for (int i = 0; i < V; ++i) v[i] += t[i];
    }
    if (relu) {
#pragma unroll
      for (int i = 0; i < V; ++i) v[i] = fmaxf(v[i], 0.f);
    }
    if (thr) {
      const uint32_t k = keep_piece<V>(seed, (uint32_t)r * (uint32_t)C + (uint32_t)c0, thr);
#pragma unroll
      for (int i = 0; i < V; ++i) v[i] = (k >> i) & 1 ? v[i] * dscale : 0.f;
    }
    storep(y + (long)r * ldy + c0, v);
  }
}

// g = dy * [v > 0] * keep * dscale, the gradient at the BatchNorm output (also the residual branch's);
// dbeta = sum g, dgamma = sum g * xhat, dx = gamma * rstd * (g - dbeta / M - xhat * dgamma / M) in train
// mode, gamma * rstd * g with running statistics. The gate and the keep bits are recomputed.
template <typename T>
__global__ __launch_bounds__(256) void bn_bwd_kernel(const T* __restrict__ dy, long lddy, const T* __restrict__ x,
                                                     long ldx, const float* __restrict__ mean,
                                                     const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, const T* __restrict__ res,
                                                     long ldr, int relu, uint32_t thr, float dscale, uint64_t seed,
                                                     int train, T* __restrict__ dx, long lddx, T* __restrict__ dres,
                                                     long lddr, float* dgamma, float* dbeta, int accumulate, int M,
                                                     int C) {
  constexpr int V = Pc<T>::V;
  seed = step_seed(seed);
  __shared__ float red[4][V];
  const int c0 = blockIdx.x * V;
  float mu[V], rs[V], g[V], b[V];
#pragma unroll
  for (int i = 0; i < V; ++i) {
    mu[i] = mean[c0 + i];
    rs[i] = rstd[c0 + i];
    g[i] = gamma[c0 + i];
    b[i] = beta[c0 + i];
  }
  // gated gradient and xhat of row r
  auto gated = [&](int r, float (&gd)[V], float (&xh)[V]) {
    float xv[V];
    loadp(dy + (long)r * lddy + c0, gd);
    loadp(x + (long)r * ldx + c0, xv);
#pragma unroll
    for (int i = 0; i < V; ++i) xh[i] = (xv[i] - mu[i]) * rs[i];
    if (relu) {
      float v[V];
#pragma unroll
      for (int i = 0; i < V; ++i) v[i] = bn_val(xv[i], mu[i], rs[i], g[i], b[i]);
      if (res) {
        float t[V];
        loadp(res + (long)r * ldr + c0, t);
#pragma unroll
        for (int i = 0; i < V; ++i) v[i] += t[i];
      }
#pragma unroll
      for (int i = 0; i < V; ++i) gd[i] = v[i] > 0.f ? gd[i] : 0.f;
    }
    if (thr) {
      const uint32_t k = keep_piece<V>(seed, (uint32_t)r * (uint32_t)C + (uint32_t)c0, thr);
#pragma unroll
      for (int i = 0; i < V; ++i) gd[i] = (k >> i) & 1 ? gd[i] * dscale : 0.f;
    }
  };
  float sb[V], sg[V];
#pragma unroll
  for (int i = 0; i < V; ++i) sb[i] = sg[i] = 0.f;
  for (int r = threadIdx.x; r < M; r += 256) {
    float gd[V], xh[V];
    gated(r, gd, xh);
#pragma unroll
    for (int i = 0; i < V; ++i) {
      sb[i] += gd[i];
      sg[i] = fmaf(gd[i], xh[i], sg[i]);
    }
    if (dres) storep(dres + (long)r * lddr + c0, gd);
  }
  block_sum<V>(sb, red);
  block_sum<V>(sg, red);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < V; ++i) {
      if (dgamma) dgamma[c0 + i] = accumulate ? dgamma[c0 + i] + sg[i] : sg[i];
      if (dbeta) dbeta[c0 + i] = accumulate ? dbeta[c0 + i] + sb[i] : sb[i];
    }
  }
  if (!dx) return;
  float mb[V], mg[V];
#pragma unroll
  for (int i = 0; i < V; ++i) {
    mb[i] = train ? sb[i] / (float)M : 0.f;
    mg[i] = train ? sg[i] / (float)M : 0.f;
  }
  for (int r = threadIdx.x; r < M; r += 256) {
    float gd[V], xh[V];
    gated(r, gd, xh);
#pragma unroll
    for (int i = 0; i < V; ++i) gd[i] = g[i] * rs[i] * ((gd[i] - mb[i]) - xh[i] * mg[i]);
    storep(dx + (long)r * lddx + c0, gd);
  }
}

// ---------------------------------------------------------------- sequence mean
template <typename T>
__global__ __launch_bounds__(256) void seq_mean_fwd_kernel(const T* __restrict__ x, long ldx, T* __restrict__ y,
                                                           long ldy, int B, int L, int C) {
  constexpr int V = Pc<T>::V;
  const int pieces = C / V;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)B * pieces) return;
  const long b = i / pieces;
  const int c0 = (int)(i - b * pieces) * V;
  float s[V];
#pragma unroll
  for (int r = 0; r < V; ++r) s[r] = 0.f;
  for (int l = 0; l < L; ++l) {
    float v[V];
    loadp(x + (b * L + l) * ldx + c0, v);
#pragma unroll
    for (int r = 0; r < V; ++r) s[r] += v[r];
  }
#pragma unroll
  for (int r = 0; r < V; ++r) s[r] /= (float)L;
  storep(y + b * ldy + c0, s);
}

template <typename T>
__global__ __launch_bounds__(256) void seq_mean_bwd_kernel(const T* __restrict__ dy, long lddy, T* __restrict__ dx,
                                                           long lddx, int B, int L, int C) {
  constexpr int V = Pc<T>::V;
  const int pieces = C / V;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)B * L * pieces) return;
  const long m = i / pieces;
  const int c0 = (int)(i - m * pieces) * V;
  float v[V];
  loadp(dy + (m / L) * lddy + c0, v);
#pragma unroll
  for (int r = 0; r < V; ++r) v[r] /= (float)L;
  storep(dx + m * lddx + c0, v);
}

// ---------------------------------------------------------------- small-N classifier
// logits[b][c] = sum_d x[b][d] W[c][d] + bias[c]: one wave per (b, c), lanes stride D, butterfly sum.
template <typename T>
__global__ __launch_bounds__(256) void logits_fwd_kernel(const T* __restrict__ x, long ldx, const float* __restrict__ W,
                                                         const float* __restrict__ bias, float* __restrict__ out, int B,
                                                         int D, int Cc) {
  const int lane = threadIdx.x & 63;
  const long wid = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (wid >= (long)B * Cc) return;
  const long b = wid / Cc;
  const int c = (int)(wid - b * Cc);
  float s = 0.f;
  for (int d = lane; d < D; d += 64) s = fmaf(to_f<T>(x[b * ldx + d]), W[(long)c * D + d], s);
  s = wave_sum(s);
  if (lane == 0) out[b * Cc + c] = s + (bias ? bias[c] : 0.f);
}

// One thread per output element, each a fixed-order loop: dx[b][d] = (sum_c dl[b][c] W[c][d]) * gate[b][d],
// dW[c][d] (+)= sum_b dl[b][c] x[b][d], dbias[c] (+)= sum_b dl[b][c].
template <typename T>
__global__ __launch_bounds__(256) void logits_bwd_kernel(const T* __restrict__ x, long ldx, const float* __restrict__ W,
                                                         const float* __restrict__ dl, const T* __restrict__ gate,
                                                         long ldg, T* __restrict__ dx, long lddx, float* dW,
                                                         float* dbias, int accumulate, int B, int D, int Cc) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const long ndx = dx ? (long)B * D : 0, nw = dW ? (long)Cc * D : 0, nb = dbias ? Cc : 0;
  if (i < ndx) {
    const long b = i / D;
    const int d = (int)(i - b * D);
    float s = 0.f;
    for (int c = 0; c < Cc; ++c) s = fmaf(dl[b * Cc + c], W[(long)c * D + d], s);
    if (gate) s *= to_f<T>(gate[b * ldg + d]);
    dx[b * lddx + d] = from_f<T>(s);
  } else if (i < ndx + nw) {
    const long j = i - ndx;
    const int c = (int)(j / D), d = (int)(j - (long)c * D);
    float s = 0.f;
    for (long b = 0; b < B; ++b) s = fmaf(dl[b * Cc + c], to_f<T>(x[b * ldx + d]), s);
    dW[j] = accumulate ? dW[j] + s : s;
  } else if (i < ndx + nw + nb) {
    const int c = (int)(i - ndx - nw);
    float s = 0.f;
    for (long b = 0; b < B; ++b) s += dl[b * Cc + c];
    dbias[c] = accumulate ? dbias[c] + s : s;
  }
}

}  // namespace fer

using namespace fer;

extern "C" int fer_conv1d_cols(int dtype, const void* x, int64_t ldx, void* cols, int64_t ldc, int B, int L, int C,
                               fer_stream_t stream) {
  if (check_dtype(dtype, "conv1d_cols: unknown dtype")) return -1;
  const int V = piece_len(dtype);
  if (B < 1 || L < 1 || C < 1) return set_error("conv1d_cols: B, L, C must be >= 1");
  if ((3 * C) % V) return set_error("conv1d_cols: 3*C must be a multiple of the 16-byte piece (8 bf16 / 4 fp32)");
  if (!x || ldx < C) return set_error("conv1d_cols: x is null or its row stride is below C");
  if (!piece_ok(cols, ldc, 3 * C, V)) return set_error("conv1d_cols: cols needs 16-byte aligned rows of stride >= 3*C");
  const long M = (long)B * L, n = M * (3 * C / V);
  if (too_many(n)) return set_error("conv1d_cols: too many elements for one launch");
  hipStream_t st = (hipStream_t)stream;
  with_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(conv1d_cols_kernel<T>, dim3(blocks_for(n)), dim3(256), 0, st, (const T*)x, (long)ldx,
                       (T*)cols, (long)ldc, L, C, M);
  });
  return hip_check("conv1d_cols");
}

extern "C" int fer_conv1d_cols_bwd(int dtype, const void* dcols, int64_t ldd, const void* res, int64_t ldr, void* dx,
                                   int64_t lddx, int B, int L, int C, fer_stream_t stream) {
  if (check_dtype(dtype, "conv1d_cols_bwd: unknown dtype")) return -1;
  const int V = piece_len(dtype);
  if (B < 1 || L < 1 || C < 1) return set_error("conv1d_cols_bwd: B, L, C must be >= 1");
  if (C % V) return set_error("conv1d_cols_bwd: C must be a multiple of the 16-byte piece (8 bf16 / 4 fp32)");
  if (!piece_ok(dcols, ldd, 3 * C, V))
    return set_error("conv1d_cols_bwd: dcols needs 16-byte aligned rows of stride >= 3*C");
  if (!piece_ok(dx, lddx, C, V) || (res && !piece_ok(res, ldr, C, V)))
    return set_error("conv1d_cols_bwd: dx, res need 16-byte aligned rows of stride >= C");
  const long M = (long)B * L, n = M * (C / V);
  if (too_many(n)) return set_error("conv1d_cols_bwd: too many elements for one launch");
  hipStream_t st = (hipStream_t)stream;
  with_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(conv1d_cols_bwd_kernel<T>, dim3(blocks_for(n)), dim3(256), 0, st, (const T*)dcols, (long)ldd,
                       (const T*)res, (long)ldr, (T*)dx, (long)lddx, L, C, M);
  });
  return hip_check("conv1d_cols_bwd");
}

extern "C" int fer_batchnorm_fwd(int dtype, const void* x, int64_t ldx, const float* gamma, const float* beta,
                                 float* running_mean, float* running_var, int64_t* num_batches_tracked, int train,
                                 float momentum, float eps, const void* res, int64_t ldr, int relu,
                                 uint32_t drop_thresh, float drop_scale, uint64_t seed, void* y, int64_t ldy,
                                 float* mean, float* rstd, int M, int C, fer_stream_t stream) {
  if (check_dtype(dtype, "batchnorm_fwd: unknown dtype")) return -1;
  const int V = piece_len(dtype);
  if (M < 1 || C < 1) return set_error("batchnorm_fwd: M and C must be >= 1");
  if (C % V) return set_error("batchnorm_fwd: C must be a multiple of the 16-byte piece (8 bf16 / 4 fp32)");
  if (train && M < 2) return set_error("batchnorm_fwd: train mode needs more than 1 value per channel");
  if (!train && (!running_mean || !running_var)) return set_error("batchnorm_fwd: eval mode needs the running statistics");
  if (!gamma || !beta) return set_error("batchnorm_fwd: gamma / beta are null");
  if (!piece_ok(x, ldx, C, V) || !piece_ok(y, ldy, C, V) || (res && !piece_ok(res, ldr, C, V)))
    return set_error("batchnorm_fwd: x, y, res need 16-byte aligned rows of stride >= C");
  if (!(eps >= 0.f) || !(momentum >= 0.f && momentum <= 1.f)) return set_error("batchnorm_fwd: bad eps or momentum");
  if (check_drop_range(drop_thresh, (long)M * C, "batchnorm_fwd: dropout over >= 2^32 elements")) return -1;
  hipStream_t st = (hipStream_t)stream;
  with_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(bn_fwd_kernel<T>, dim3(C / V), dim3(256), 0, st, (const T*)x, (long)ldx, gamma, beta,
                       running_mean, running_var, (long long*)num_batches_tracked, train, momentum, eps,
                       (const T*)res, (long)ldr, relu, drop_thresh, drop_scale, seed, (T*)y, (long)ldy, mean, rstd,
                       M, C);
  });
  return hip_check("batchnorm_fwd");
}

extern "C" int fer_batchnorm_bwd(int dtype, const void* dy, int64_t lddy, const void* x, int64_t ldx,
                                 const float* mean, const float* rstd, const float* gamma, const float* beta,
                                 const void* res, int64_t ldr, int relu, uint32_t drop_thresh, float drop_scale,
                                 uint64_t seed, int train, void* dx, int64_t lddx, void* dres, int64_t lddr,
                                 float* dgamma, float* dbeta, int accumulate, int M, int C, fer_stream_t stream) {
  if (check_dtype(dtype, "batchnorm_bwd: unknown dtype")) return -1;
  const int V = piece_len(dtype);
  if (M < 1 || C < 1) return set_error("batchnorm_bwd: M and C must be >= 1");
  if (C % V) return set_error("batchnorm_bwd: C must be a multiple of the 16-byte piece (8 bf16 / 4 fp32)");
  if (!mean || !rstd || !gamma || !beta) return set_error("batchnorm_bwd: mean, rstd, gamma, beta are required");
  if (!dx && !dres && !dgamma && !dbeta) return set_error("batchnorm_bwd: no output requested");
  if (!piece_ok(dy, lddy, C, V) || !piece_ok(x, ldx, C, V) || (res && !piece_ok(res, ldr, C, V)) ||
      (dx && !piece_ok(dx, lddx, C, V)) || (dres && !piece_ok(dres, lddr, C, V)))
    return set_error("batchnorm_bwd: dy, x, res, dx, dres need 16-byte aligned rows of stride >= C");
  if (check_drop_range(drop_thresh, (long)M * C, "batchnorm_bwd: dropout over >= 2^32 elements")) return -1;
  hipStream_t st = (hipStream_t)stream;
  with_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(bn_bwd_kernel<T>, dim3(C / V), dim3(256), 0, st, (const T*)dy, (long)lddy, (const T*)x,
                       (long)ldx, mean, rstd, gamma, beta, (const T*)res, (long)ldr, relu, drop_thresh, drop_scale,
                       seed, train, (T*)dx, (long)lddx, (T*)dres, (long)lddr, dgamma, dbeta, accumulate, M, C);
  });
  return hip_check("batchnorm_bwd");
}

extern "C" int fer_seq_mean_fwd(int dtype, const void* x, int64_t ldx, void* y, int64_t ldy, int B, int L, int C,
                                fer_stream_t stream) {
  if (check_dtype(dtype, "seq_mean_fwd: unknown dtype")) return -1;
  const int V = piece_len(dtype);
  if (B < 1 || L < 1 || C < 1) return set_error("seq_mean_fwd: B, L, C must be >= 1");
  if (C % V) return set_error("seq_mean_fwd: C must be a multiple of the 16-byte piece (8 bf16 / 4 fp32)");
  if (!piece_ok(x, ldx, C, V) || !piece_ok(y, ldy, C, V))
    return set_error("seq_mean_fwd: x, y need 16-byte aligned rows of stride >= C");
  const long n = (long)B * (C / V);
  if (too_many(n)) return set_error("seq_mean_fwd: too many elements for one launch");
  hipStream_t st = (hipStream_t)stream;
  with_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(seq_mean_fwd_kernel<T>, dim3(blocks_for(n)), dim3(256), 0, st, (const T*)x, (long)ldx, (T*)y,
                       (long)ldy, B, L, C);
  });
  return hip_check("seq_mean_fwd");
}

extern "C" int fer_seq_mean_bwd(int dtype, const void* dy, int64_t lddy, void* dx, int64_t lddx, int B, int L, int C,
                                fer_stream_t stream) {
  if (check_dtype(dtype, "seq_mean_bwd: unknown dtype")) return -1;
  const int V = piece_len(dtype);
  if (B < 1 || L < 1 || C < 1) return set_error("seq_mean_bwd: B, L, C must be >= 1");
  if (C % V) return set_error("seq_mean_bwd: C must be a multiple of the 16-byte piece (8 bf16 / 4 fp32)");
  if (!piece_ok(dy, lddy, C, V) || !piece_ok(dx, lddx, C, V))
    return set_error("seq_mean_bwd: dy, dx need 16-byte aligned rows of stride >= C");
  const long n = (long)B * L * (C / V);
  if (too_many(n)) return set_error("seq_mean_bwd: too many elements for one launch");
  hipStream_t st = (hipStream_t)stream;
  with_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(seq_mean_bwd_kernel<T>, dim3(blocks_for(n)), dim3(256), 0, st, (const T*)dy, (long)lddy,
                       (T*)dx, (long)lddx, B, L, C);
  });
  return hip_check("seq_mean_bwd");
}

extern "C" int fer_logits_fwd(int dtype, const void* x, int64_t ldx, const float* W, const float* bias, float* logits,
                              int B, int D, int C, fer_stream_t stream) {
  if (check_dtype(dtype, "logits_fwd: unknown dtype")) return -1;
  if (B < 1 || D < 1 || C < 1) return set_error("logits_fwd: B, D, C must be >= 1");
  if (!x || ldx < D || !W || !logits) return set_error("logits_fwd: null operand or row stride below D");
  const long waves = (long)B * C;
  if (waves > 0x7FFFFFFFL * 4) return set_error("logits_fwd: too many elements for one launch");
  hipStream_t st = (hipStream_t)stream;
  with_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(logits_fwd_kernel<T>, dim3((int)((waves + 3) / 4)), dim3(256), 0, st, (const T*)x, (long)ldx, W,
                       bias, logits, B, D, C);
  });
  return hip_check("logits_fwd");
}

extern "C" int fer_logits_bwd(int dtype, const void* x, int64_t ldx, const float* W, const float* dlogits,
                              const void* gate, int64_t ldg, void* dx, int64_t lddx, float* dW, float* dbias,
                              int accumulate, int B, int D, int C, fer_stream_t stream) {
  if (check_dtype(dtype, "logits_bwd: unknown dtype")) return -1;
  if (B < 1 || D < 1 || C < 1) return set_error("logits_bwd: B, D, C must be >= 1");
  if (!dlogits || !W) return set_error("logits_bwd: dlogits and W are required");
  if (!dx && !dW && !dbias) return set_error("logits_bwd: no output requested");
  if (dW && (!x || ldx < D)) return set_error("logits_bwd: dW needs x with a row stride >= D");
  if ((dx && lddx < D) || (gate && ldg < D)) return set_error("logits_bwd: dx / gate row stride below D");
  const long n = (dx ? (long)B * D : 0) + (dW ? (long)C * D : 0) + (dbias ? C : 0);
  if (too_many(n)) return set_error("logits_bwd: too many elements for one launch");
  hipStream_t st = (hipStream_t)stream;
  with_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(logits_bwd_kernel<T>, dim3(blocks_for(n)), dim3(256), 0, st, (const T*)x, (long)ldx, W, dlogits,
                       (const T*)gate, (long)ldg, (T*)dx, (long)lddx, dW, dbias, accumulate, B, D, C);
  });
  return hip_check("logits_bwd");
}
