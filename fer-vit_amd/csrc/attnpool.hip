// LatentCNNDeep operators (reference `models_fer_vit/latent_cnn.py:164-261`) that convbn.hip does not
// have: the softmax attention pooling over the sequence (`:207-211, 256-257`) and the ReLU -> Dropout
// step behind the LayerNorm of input_proj (`:183-188`). Token-major [M = B*L][C], 16-byte pieces
// (8 bf16 / 4 fp32 columns), wave64, fp32 arithmetic, as convbn.hip.
//
// The pooling runs one 256-thread workgroup per sample: the four waves take the rows l = wave, wave + 4,
// ... (each lane dots 16-byte pieces of the row with the weight, then a wave butterfly), the L scores go
// to LDS, every thread forms their max and the sum of the exponentials in one fixed order (the same bits
// in every thread), and thread t then owns the pieces t, t + 256, ... of the output and walks the L rows
// a second time (18 KB per sample at the model's size: the second read hits cache). The backward has the
// same shape. No atomics, nothing crosses a workgroup inside a kernel: the parameter gradients leave as
// per-sample partials dw_part [B][C] / dbias_part [B] that the caller sums with fer_colsum. Repeat calls
// are bit-identical. L is limited by the LDS arrays (FER_ATTNPOOL_MAX_L).
#include "common.h"
#include "fervit_internal.h"
#include "step_seed.h"

namespace fer {

constexpr int APL = FER_ATTNPOOL_MAX_L;

// V consecutive fp32 values (a parameter row; 16-byte aligned)
template <int V>
FER_DEV void loadw(const float* p, float (&v)[V]) {
#pragma unroll
  for (int i = 0; i < V; i += 4) {
    const f32x4 t = *(const f32x4*)(p + i);
    v[i] = t[0], v[i + 1] = t[1], v[i + 2] = t[2], v[i + 3] = t[3];
  }
}

// sum_c row[c] * (float)vec[c] over the C / V pieces, lanes striding the pieces, V partial sums per lane
// combined as a tree, then the wave butterfly: the same bits in all 64 lanes.
template <typename T, typename W>
FER_DEV float wave_dot(const T* __restrict__ row, const W* __restrict__ vec, int pieces, int lane) {
  constexpr int V = Pc<T>::V;
  float acc[V];
#pragma unroll
  for (int i = 0; i < V; ++i) acc[i] = 0.f;
  for (int p = lane; p < pieces; p += 64) {
    float a[V], b[V];
    loadp(row + p * V, a);
    if constexpr (sizeof(W) == sizeof(T)) loadp(vec + p * V, b);
    else loadw<V>(vec + p * V, b);
#pragma unroll
    for (int i = 0; i < V; ++i) acc[i] = fmaf(a[i], b[i], acc[i]);
  }
#pragma unroll
  for (int h = V / 2; h > 0; h >>= 1) {
#pragma unroll
    for (int i = 0; i < h; ++i) acc[i] += acc[i + h];
  }
  return wave_sum(acc[0]);
}

// ---------------------------------------------------------------- attention pooling
template <typename T>
__global__ __launch_bounds__(256) void attnpool_fwd_kernel(const T* __restrict__ x, long ldx,
                                                           const float* __restrict__ w,
                                                           const float* __restrict__ bias, T* __restrict__ y,
                                                           long ldy, float* __restrict__ probs, int L, int C) {
  constexpr int V = Pc<T>::V;
  __shared__ float a[APL];
  const int pieces = C / V, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const T* xb = x + (long)blockIdx.x * L * ldx;
  const float bv = bias ? *bias : 0.f;
  for (int l = wave; l < L; l += 4) {
    const float s = wave_dot<T, float>(xb + (long)l * ldx, w, pieces, lane);
    if (lane == 0) a[l] = s + bv;
  }
  __syncthreads();
  float mx = a[0];
  for (int l = 1; l < L; ++l) mx = fmaxf(mx, a[l]);
  __syncthreads();  // every thread has read the scores
  for (int l = threadIdx.x; l < L; l += 256) a[l] = expf(a[l] - mx);
  __syncthreads();
  float sum = 0.f;
  for (int l = 0; l < L; ++l) sum += a[l];
  __syncthreads();
  for (int l = threadIdx.x; l < L; l += 256) {
    const float p = a[l] / sum;
    a[l] = p;
    if (probs) probs[(long)blockIdx.x * L + l] = p;
  }
  __syncthreads();
  for (int p = threadIdx.x; p < pieces; p += 256) {
    float acc[V];
#pragma unroll
    for (int i = 0; i < V; ++i) acc[i] = 0.f;
    for (int l = 0; l < L; ++l) {
      float v[V];
      loadp(xb + (long)l * ldx + p * V, v);
      const float al = a[l];
#pragma unroll
      for (int i = 0; i < V; ++i) acc[i] = fmaf(al, v[i], acc[i]);
    }
    storep(y + (long)blockIdx.x * ldy + p * V, acc);
  }
}

// da_l = sum_c dy_c x_lc, ds_l = a_l (da_l - sum_l' a_l' da_l'), dx_lc = a_l dy_c + ds_l w_c,
// dw_part[b][c] = sum_l ds_l x_lc, dbias_part[b] = sum_l ds_l.
template <typename T>
__global__ __launch_bounds__(256) void attnpool_bwd_kernel(const T* __restrict__ dy, long lddy,
                                                           const T* __restrict__ x, long ldx,
                                                           const float* __restrict__ w,
                                                           const float* __restrict__ probs, T* __restrict__ dx,
                                                           long lddx, float* __restrict__ dw_part,
                                                           float* __restrict__ dbias_part, int L, int C) {
  constexpr int V = Pc<T>::V;
  __shared__ float a[APL];
  __shared__ float ds[APL];  // da first
  const int pieces = C / V, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long b = blockIdx.x;
  const T* xb = x + b * L * ldx;
  const T* dyb = dy + b * lddy;
  for (int l = threadIdx.x; l < L; l += 256) a[l] = probs[b * L + l];
  for (int l = wave; l < L; l += 4) {
    const float s = wave_dot<T, T>(xb + (long)l * ldx, dyb, pieces, lane);
    if (lane == 0) ds[l] = s;
  }
  __syncthreads();
  float dot = 0.f;
  for (int l = 0; l < L; ++l) dot = fmaf(a[l], ds[l], dot);
  __syncthreads();  // every thread has read da
  for (int l = threadIdx.x; l < L; l += 256) ds[l] = a[l] * (ds[l] - dot);
  __syncthreads();
  if (dbias_part && threadIdx.x == 0) {
    float s = 0.f;
    for (int l = 0; l < L; ++l) s += ds[l];
    dbias_part[b] = s;
  }
  if (!dx && !dw_part) return;
  for (int p = threadIdx.x; p < pieces; p += 256) {
    float g[V], wv[V], acc[V];
    loadp(dyb + p * V, g);
    loadw<V>(w + p * V, wv);
#pragma unroll
    for (int i = 0; i < V; ++i) acc[i] = 0.f;
    for (int l = 0; l < L; ++l) {
      float v[V], o[V];
      loadp(xb + (long)l * ldx + p * V, v);
      const float al = a[l], dl = ds[l];
#pragma unroll
      for (int i = 0; i < V; ++i) {
        o[i] = fmaf(dl, wv[i], al * g[i]);
        acc[i] = fmaf(dl, v[i], acc[i]);
      }
      if (dx) storep(dx + (b * L + l) * lddx + p * V, o);
    }
    if (dw_part) {
#pragma unroll
      for (int i = 0; i < V; i += 4)
        *(f32x4*)(dw_part + b * C + p * V + i) = f32x4{acc[i], acc[i + 1], acc[i + 2], acc[i + 3]};
    }
  }
}

// ---------------------------------------------------------------- ReLU + dropout
// y = keep * scale * max(x, 0); dx = dy * [x > 0] * keep * scale with the gate and the keep bits
// recomputed from x and the seed. One thread per 16-byte piece; keep bits at linear index r * C + c0,
// as bn_fwd_kernel draws them.
template <typename T>
__global__ __launch_bounds__(256) void relu_dropout_kernel(const T* __restrict__ g, long ldg,
                                                           const T* __restrict__ x, long ldx, T* __restrict__ y,
                                                           long ldy, long M, int C, uint32_t thr, float dscale,
                                                           uint64_t seed) {
  constexpr int V = Pc<T>::V;
  const int pieces = C / V;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= M * pieces) return;
  const long r = i / pieces;
  const int c0 = (int)(i - r * pieces) * V;
  float v[V], o[V];
  loadp(x + r * ldx + c0, v);
  if (g) {  // backward: the gradient passes where the forward value did
    loadp(g + r * ldg + c0, o);
#pragma unroll
    for (int k = 0; k < V; ++k) o[k] = v[k] > 0.f ? o[k] : 0.f;
  } else {
#pragma unroll
    for (int k = 0; k < V; ++k) o[k] = v[k] > 0.f ? v[k] : 0.f;
  }
  if (thr) {
    const uint32_t k = keep_piece<V>(step_seed(seed), (uint32_t)r * (uint32_t)C + (uint32_t)c0, thr);
#pragma unroll
    for (int j = 0; j < V; ++j) o[j] = (k >> j) & 1 ? o[j] * dscale : 0.f;
  }
  storep(y + r * ldy + c0, o);
}

}  // namespace fer

using namespace fer;

extern "C" int fer_attnpool_fwd(int dtype, const void* x, int64_t ldx, const float* w, const float* bias, void* y,
                                int64_t ldy, float* probs, int B, int L, int C, fer_stream_t stream) {
  if (check_dtype(dtype, "attnpool_fwd: unknown dtype")) return -1;
  const int V = piece_len(dtype);
  if (B < 1 || L < 1 || C < 1) return set_error("attnpool_fwd: B, L, C must be >= 1");
  if (C % V) return set_error("attnpool_fwd: C must be a multiple of the 16-byte piece (8 bf16 / 4 fp32)");
  if (L > FER_ATTNPOOL_MAX_L) return set_error("attnpool_fwd: L is above FER_ATTNPOOL_MAX_L (the LDS score array)");
  if (!piece_ok(x, ldx, C, V) || !piece_ok(y, ldy, C, V))
    return set_error("attnpool_fwd: x, y need 16-byte aligned rows of stride >= C");
  if (!w || !al16(w)) return set_error("attnpool_fwd: w is null or not 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  with_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(attnpool_fwd_kernel<T>, dim3(B), dim3(256), 0, st, (const T*)x, (long)ldx, w, bias, (T*)y,
                       (long)ldy, probs, L, C);
  });
  return hip_check("attnpool_fwd");
}

extern "C" int fer_attnpool_bwd(int dtype, const void* dy, int64_t lddy, const void* x, int64_t ldx, const float* w,
                                const float* probs, void* dx, int64_t lddx, float* dw_part, float* dbias_part, int B,
                                int L, int C, fer_stream_t stream) {
  if (check_dtype(dtype, "attnpool_bwd: unknown dtype")) return -1;
  const int V = piece_len(dtype);
  if (B < 1 || L < 1 || C < 1) return set_error("attnpool_bwd: B, L, C must be >= 1");
  if (C % V) return set_error("attnpool_bwd: C must be a multiple of the 16-byte piece (8 bf16 / 4 fp32)");
  if (L > FER_ATTNPOOL_MAX_L) return set_error("attnpool_bwd: L is above FER_ATTNPOOL_MAX_L (the LDS score array)");
  if (!dx && !dw_part && !dbias_part) return set_error("attnpool_bwd: no output requested");
  if (!piece_ok(dy, lddy, C, V) || !piece_ok(x, ldx, C, V) || (dx && !piece_ok(dx, lddx, C, V)))
    return set_error("attnpool_bwd: dy, x, dx need 16-byte aligned rows of stride >= C");
  if (!w || !al16(w) || !probs) return set_error("attnpool_bwd: w (16-byte aligned) and probs are required");
  if (dw_part && !al16(dw_part)) return set_error("attnpool_bwd: dw_part is not 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  with_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(attnpool_bwd_kernel<T>, dim3(B), dim3(256), 0, st, (const T*)dy, (long)lddy, (const T*)x,
                       (long)ldx, w, probs, (T*)dx, (long)lddx, dw_part, dbias_part, L, C);
  });
  return hip_check("attnpool_bwd");
}

// g = null: the forward
static int relu_dropout_launch(const char* name, int dtype, const void* g, int64_t ldg, const void* x, int64_t ldx,
                               void* y, int64_t ldy, int M, int C, uint32_t thr, float sc, uint64_t seed,
                               hipStream_t st) {
  const long n = (long)M * (C / piece_len(dtype));
  with_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(relu_dropout_kernel<T>, dim3(blocks_for(n)), dim3(256), 0, st, (const T*)g, (long)ldg,
                       (const T*)x, (long)ldx, (T*)y, (long)ldy, (long)M, C, thr, sc, seed);
  });
  return hip_check(name);
}

extern "C" int fer_relu_dropout_fwd(int dtype, const void* x, int64_t ldx, void* y, int64_t ldy, int M, int C,
                                    uint32_t drop_thresh, float drop_scale, uint64_t seed, fer_stream_t stream) {
  if (check_dtype(dtype, "relu_dropout_fwd: unknown dtype")) return -1;
  const int V = piece_len(dtype);
  if (M < 1 || C < 1) return set_error("relu_dropout_fwd: M and C must be >= 1");
  if (C % V) return set_error("relu_dropout_fwd: C must be a multiple of the 16-byte piece (8 bf16 / 4 fp32)");
  if (!piece_ok(x, ldx, C, V) || !piece_ok(y, ldy, C, V))
    return set_error("relu_dropout_fwd: x, y need 16-byte aligned rows of stride >= C");
  if (check_drop_range(drop_thresh, (long)M * C, "relu_dropout_fwd: dropout over >= 2^32 elements")) return -1;
  if (too_many((long)M * (C / V))) return set_error("relu_dropout_fwd: too many elements for one launch");
  return relu_dropout_launch("relu_dropout_fwd", dtype, nullptr, 0, x, ldx, y, ldy, M, C, drop_thresh, drop_scale,
                             seed, (hipStream_t)stream);
}

extern "C" int fer_relu_dropout_bwd(int dtype, const void* dy, int64_t lddy, const void* x, int64_t ldx, void* dx,
                                    int64_t lddx, int M, int C, uint32_t drop_thresh, float drop_scale, uint64_t seed,
                                    fer_stream_t stream) {
  if (check_dtype(dtype, "relu_dropout_bwd: unknown dtype")) return -1;
  const int V = piece_len(dtype);
  if (M < 1 || C < 1) return set_error("relu_dropout_bwd: M and C must be >= 1");
  if (C % V) return set_error("relu_dropout_bwd: C must be a multiple of the 16-byte piece (8 bf16 / 4 fp32)");
  if (!piece_ok(dy, lddy, C, V) || !piece_ok(x, ldx, C, V) || !piece_ok(dx, lddx, C, V))
    return set_error("relu_dropout_bwd: dy, x, dx need 16-byte aligned rows of stride >= C");
  if (check_drop_range(drop_thresh, (long)M * C, "relu_dropout_bwd: dropout over >= 2^32 elements")) return -1;
  if (too_many((long)M * (C / V))) return set_error("relu_dropout_bwd: too many elements for one launch");
  return relu_dropout_launch("relu_dropout_bwd", dtype, dy, lddy, x, ldx, dx, lddx, M, C, drop_thresh, drop_scale,
                             seed, (hipStream_t)stream);
}
