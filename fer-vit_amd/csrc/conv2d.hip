// LatentCNN2D operators (reference `models_fer_vit/latent_cnn.py:333-409`): the w+ code (18, 512) as a
// one-channel image. Pixel-major [M = B*H*W][C] (NHWC) throughout, the 2-D form of convbn.hip's
// [B*L][C]: BatchNorm2d's channel axis is the column axis (fer_batchnorm_* serve as they are) and
// AdaptiveAvgPool2d(1) is fer_seq_mean_* with L = H*W.
//
//   conv2d_cols / _bwd     im2col of Conv2d(3x3, stride 1, padding 1) in (cin, kh, kw) column order --
//                          the memory order of nn.Conv2d.weight [Cout][Cin][3][3], so the parameter is
//                          fer_gemm's B operand with K = 9*Cin as it stands -- and its adjoint
//   conv2d_c1_fwd / _bwd   the first layer Conv2d(1, Cout, 3, padding 1) + bias, direct (K = 9 is
//                          nothing for an MFMA; the layer is bound by writing M x Cout outputs)
//   pool2_chdrop_fwd/_bwd  MaxPool2d((2, 2)) (optional) then Dropout2d, one launch
//
// Memory pieces are 16 bytes (8 bf16 / 4 fp32 channels), as in convbn.hip. No atomics, no stored masks
// or indices: the keep bits and the pooling argmax are recomputed in the backward. Every sum is a
// fixed-order loop, so repeat calls are bit-identical.
#include "common.h"
#include "fervit_internal.h"
#include "step_seed.h"

namespace fer {

// pixel m -> (h, w) inside its image
struct Pix {
  int h, w;
};
FER_DEV Pix pix_of(long m, int H, int W) {
  const long r = m / W;
  return Pix{(int)(r % H), (int)(m - r * W)};
}

// ---------------------------------------------------------------- conv2d im2col
// One thread per (pixel, 16-byte channel piece): the nine neighbour pieces x[m + (kh-1)*W + (kw-1)][c0..c0+V)
// are loaded whole (zeros outside the image: never the neighbouring row's or sample's pixel) and
// leave as cols[m][c0*9 .. (c0+V)*9), which is 9 consecutive pieces: element (c0 + r)*9 + k is tap k of
// channel r, a V x 9 transpose in registers. Values are copied bit for bit.
template <typename T>
__global__ __launch_bounds__(256) void conv2d_cols_kernel(const T* __restrict__ x, long ldx, T* __restrict__ cols,
                                                          long ldc, int H, int W, int C, long M) {
  constexpr int V = Pc<T>::V;
  typedef typename Pc<T>::vec vec;
  const int pieces = C / V;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= M * pieces) return;
  const long m = i / pieces;
  const int c0 = (int)(i - m * pieces) * V;
  const Pix p = pix_of(m, H, W);
  vec a[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const int dh = k / 3 - 1, dw = k % 3 - 1;
    const int hh = p.h + dh, ww = p.w + dw;
    vec z;
#pragma unroll
    for (int r = 0; r < V; ++r) z[r] = (T)0.f;
    a[k] = (hh >= 0 && hh < H && ww >= 0 && ww < W) ? *(const vec*)(x + (m + (long)dh * W + dw) * ldx + c0) : z;
  }
  T* out = cols + m * ldc + (long)c0 * 9;
#pragma unroll
  for (int q = 0; q < 9; ++q) {
    vec o;
#pragma unroll
    for (int e = 0; e < V; ++e) {
      const int j = q * V + e;  // = r * 9 + k
      o[e] = a[j % 9][j / 9];
    }
    *(vec*)(out + q * V) = o;
  }
}

// dx[m][c] = sum over (kh, kw) in scan order of dcols[m - (kh-1)*W - (kw-1)][c*9 + kh*3 + kw], the
// pixels outside the image left out: the up to nine contributions added in a fixed order in fp32.
template <typename T>
__global__ __launch_bounds__(256) void conv2d_cols_bwd_kernel(const T* __restrict__ dcols, long ldd,
                                                              T* __restrict__ dx, long lddx, int H, int W, int C,
                                                              long M) {
  constexpr int V = Pc<T>::V;
  const int pieces = C / V;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= M * pieces) return;
  const long m = i / pieces;
  const int c0 = (int)(i - m * pieces) * V;
  const Pix p = pix_of(m, H, W);
  float s[V];
#pragma unroll
  for (int r = 0; r < V; ++r) s[r] = 0.f;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const int dh = k / 3 - 1, dw = k % 3 - 1;
    const int hh = p.h - dh, ww = p.w - dw;  // the output pixel whose tap k reads this pixel
    if (hh < 0 || hh >= H || ww < 0 || ww >= W) continue;
    const T* row = dcols + (m - (long)dh * W - dw) * ldd + (long)c0 * 9;
#pragma unroll
    for (int r = 0; r < V; ++r) s[r] += to_f<T>(row[r * 9 + k]);
  }
  storep(dx + m * lddx + c0, s);
}

// ---------------------------------------------------------------- first layer, Cin = 1
// y[m][co] = bias[co] + sum_k x9[m][k] w[co][k], k = kh*3 + kw in order, fmaf in fp32. The weights are
// the fp32 master parameter on both paths (the bf16 path rounds only x on input and y on output); they
// sit in LDS transposed, wl[k][co], so a thread's V output channels are consecutive words.
constexpr int C1_MAX_COUT = FER_CONV2D_C1_MAX_COUT;

FER_DEV void load_w_lds(float* wl, const float* __restrict__ w, int Cout) {
  for (int j = threadIdx.x; j < Cout * 9; j += 256) {
    const int co = j / 9, k = j - co * 9;
    wl[k * Cout + co] = w[j];
  }
  __syncthreads();
}

// the 3x3 neighbourhood of pixel m of the one-channel image, zeros outside
template <typename T>
FER_DEV void taps9(const T* __restrict__ x, long ldx, long m, Pix p, int H, int W, float (&t)[9]) {
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const int dh = k / 3 - 1, dw = k % 3 - 1;
    const int hh = p.h + dh, ww = p.w + dw;
    t[k] = (hh >= 0 && hh < H && ww >= 0 && ww < W) ? to_f<T>(x[(m + (long)dh * W + dw) * ldx]) : 0.f;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void conv2d_c1_fwd_kernel(const T* __restrict__ x, long ldx,
                                                            const float* __restrict__ w,
                                                            const float* __restrict__ bias, T* __restrict__ y,
                                                            long ldy, int H, int W, int Cout, long M) {
  constexpr int V = Pc<T>::V;
  extern __shared__ float wl[];
  load_w_lds(wl, w, Cout);
  const int pieces = Cout / V;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= M * pieces) return;
  const long m = i / pieces;
  const int c0 = (int)(i - m * pieces) * V;
  float t[9];
  taps9(x, ldx, m, pix_of(m, H, W), H, W, t);
  float s[V];
#pragma unroll
  for (int r = 0; r < V; ++r) s[r] = bias ? bias[c0 + r] : 0.f;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
#pragma unroll
    for (int r = 0; r < V; ++r) s[r] = fmaf(t[k], wl[k * Cout + c0 + r], s[r]);
  }
  storep(y + m * ldy + c0, s);
}

// dw_part[g][co*9 + k] = sum over the pixels m of workgroup g's strip of dy[m][co] x9[m][k]. The 256
// threads are `lanes` pixel lanes x `pieces` channel pieces; a thread walks its lane's pixels of the strip
// in order, then the lanes are added in order through LDS, one tap at a time. A strip without pixels
// writes zeros. The caller sums the n_parts rows (fer_colsum).
template <typename T>
__global__ __launch_bounds__(256) void conv2d_c1_dw_kernel(const T* __restrict__ dy, long lddy,
                                                           const T* __restrict__ x, long ldx,
                                                           float* __restrict__ dw_part, int H, int W, int Cout,
                                                           long M, long chunk) {
  constexpr int V = Pc<T>::V;
  __shared__ float red[256 * V];
  const int pieces = Cout / V, lanes = 256 / pieces;
  const int lane = threadIdx.x / pieces, c0 = (threadIdx.x - lane * pieces) * V;
  const long m0 = (long)blockIdx.x * chunk, m1 = m0 + chunk < M ? m0 + chunk : M;
  float acc[9][V];
#pragma unroll
  for (int k = 0; k < 9; ++k)
#pragma unroll
    for (int r = 0; r < V; ++r) acc[k][r] = 0.f;
  if (lane < lanes) {
    for (long m = m0 + lane; m < m1; m += lanes) {
      float t[9], g[V];
      taps9(x, ldx, m, pix_of(m, H, W), H, W, t);
      loadp(dy + m * lddy + c0, g);
#pragma unroll
      for (int k = 0; k < 9; ++k)
#pragma unroll
        for (int r = 0; r < V; ++r) acc[k][r] = fmaf(g[r], t[k], acc[k][r]);
    }
  }
  float* out = dw_part + (long)blockIdx.x * Cout * 9;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    __syncthreads();
    if (lane < lanes) {
#pragma unroll
      for (int r = 0; r < V; ++r) red[lane * Cout + c0 + r] = acc[k][r];
    }
    __syncthreads();
    for (int co = threadIdx.x; co < Cout; co += 256) {
      float s = 0.f;
      for (int l = 0; l < lanes; ++l) s += red[l * Cout + co];
      out[co * 9 + k] = s;
    }
  }
}

// dx[m] = sum_k sum_co dy[m - (kh-1)*W - (kw-1)][co] w[co][k], taps in scan order, channels in order.
template <typename T>
__global__ __launch_bounds__(256) void conv2d_c1_dx_kernel(const T* __restrict__ dy, long lddy,
                                                           const float* __restrict__ w, T* __restrict__ dx,
                                                           long lddx, int H, int W, int Cout, long M) {
  constexpr int V = Pc<T>::V;
  extern __shared__ float wl[];
  load_w_lds(wl, w, Cout);
  const long m = (long)blockIdx.x * 256 + threadIdx.x;
  if (m >= M) return;
  const Pix p = pix_of(m, H, W);
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const int dh = k / 3 - 1, dw = k % 3 - 1;
    const int hh = p.h - dh, ww = p.w - dw;
    if (hh < 0 || hh >= H || ww < 0 || ww >= W) continue;
    const T* row = dy + (m - (long)dh * W - dw) * lddy;
    for (int c0 = 0; c0 < Cout; c0 += V) {
      float g[V];
      loadp(row + c0, g);
#pragma unroll
      for (int r = 0; r < V; ++r) s = fmaf(g[r], wl[k * Cout + c0 + r], s);
    }
  }
  dx[m * lddx] = from_f<T>(s);
}

// ---------------------------------------------------------------- MaxPool2d((2, 2)) + Dropout2d
// The window's first maximum in (kh, kw) scan order with a strict >, PyTorch's rule: ties (zeros behind the
// ReLU, bf16 duplicates) go to the earliest pixel. amax[r] = its position 0..3.
template <int V>
FER_DEV void window_max(const float (&a)[4][V], float (&best)[V], int (&amax)[V]) {
#pragma unroll
  for (int r = 0; r < V; ++r) {
    best[r] = a[0][r];
    amax[r] = 0;
#pragma unroll
    for (int q = 1; q < 4; ++q) {
      if (a[q][r] > best[r]) {
        best[r] = a[q][r];
        amax[r] = q;
      }
    }
  }
}

// One thread per (output pixel, channel piece). Dropout2d drops whole (sample, channel) planes: the keep
// bit is the library's hash at element index b*C + c. thr = 0: the values pass bit for bit.
template <typename T>
__global__ __launch_bounds__(256) void pool2_chdrop_fwd_kernel(const T* __restrict__ x, long ldx, T* __restrict__ y,
                                                               long ldy, int H, int W, int C, int pool, uint32_t thr,
                                                               float dscale, uint64_t seed, long Mo) {
  constexpr int V = Pc<T>::V;
  seed = step_seed(seed);
  const int pieces = C / V;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= Mo * pieces) return;
  const long mo = i / pieces;
  const int c0 = (int)(i - mo * pieces) * V;
  const int Ho = pool ? H / 2 : H, Wo = pool ? W / 2 : W;
  const long b = mo / ((long)Ho * Wo);
  float v[V];
  if (pool) {
    const Pix p = pix_of(mo, Ho, Wo);
    const T* base = x + ((b * H + 2 * p.h) * W + 2 * p.w) * ldx + c0;
    float a[4][V];
    int amax[V];
    loadp(base, a[0]);
    loadp(base + ldx, a[1]);
    loadp(base + (long)W * ldx, a[2]);
    loadp(base + ((long)W + 1) * ldx, a[3]);
    window_max<V>(a, v, amax);
  } else {
    loadp(x + mo * ldx + c0, v);
  }
  if (thr) {
    const uint32_t k = keep_piece<V>(seed, (uint32_t)b * (uint32_t)C + (uint32_t)c0, thr);
#pragma unroll
    for (int r = 0; r < V; ++r) v[r] = (k >> r) & 1 ? v[r] * dscale : 0.f;
  }
  storep(y + mo * ldy + c0, v);
}

// One thread per (input pixel, channel piece): dx = dy * keep * dscale where this pixel is its window's
// argmax (recomputed from the forward's x), exactly 0 elsewhere, the rows and columns floor division
// leaves out included. Every dx element is written once.
template <typename T>
__global__ __launch_bounds__(256) void pool2_chdrop_bwd_kernel(const T* __restrict__ dy, long lddy,
                                                               const T* __restrict__ x, long ldx, T* __restrict__ dx,
                                                               long lddx, int H, int W, int C, int pool, uint32_t thr,
                                                               float dscale, uint64_t seed, long M) {
  constexpr int V = Pc<T>::V;
  seed = step_seed(seed);
  const int pieces = C / V;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= M * pieces) return;
  const long m = i / pieces;
  const int c0 = (int)(i - m * pieces) * V;
  const long b = m / ((long)H * W);
  float g[V];
  if (pool) {
    const int Ho = H / 2, Wo = W / 2;
    const Pix p = pix_of(m, H, W);
    const int ho = p.h >> 1, wo = p.w >> 1;
    if (ho >= Ho || wo >= Wo) {
#pragma unroll
      for (int r = 0; r < V; ++r) g[r] = 0.f;
      storep(dx + m * lddx + c0, g);
      return;
    }
    const T* base = x + ((b * H + 2 * ho) * W + 2 * wo) * ldx + c0;
    float a[4][V], best[V];
    int amax[V];
    loadp(base, a[0]);
    loadp(base + ldx, a[1]);
    loadp(base + (long)W * ldx, a[2]);
    loadp(base + ((long)W + 1) * ldx, a[3]);
    window_max<V>(a, best, amax);
    const int me = (p.h & 1) * 2 + (p.w & 1);
    loadp(dy + ((b * Ho + ho) * Wo + wo) * lddy + c0, g);
#pragma unroll
    for (int r = 0; r < V; ++r) g[r] = amax[r] == me ? g[r] : 0.f;
  } else {
    loadp(dy + m * lddy + c0, g);
  }
  if (thr) {
    const uint32_t k = keep_piece<V>(seed, (uint32_t)b * (uint32_t)C + (uint32_t)c0, thr);
#pragma unroll
    for (int r = 0; r < V; ++r) g[r] = (k >> r) & 1 ? g[r] * dscale : 0.f;
  }
  storep(dx + m * lddx + c0, g);
}

}  // namespace fer

using namespace fer;

// B*H*W as a long, or -1 when a factor is < 1 or the product leaves 2^40 (far beyond any operand)
static long pixels(int B, int H, int W) {
  if (B < 1 || H < 1 || W < 1) return -1;
  const long m = (long)B * H * W;
  return m > (1L << 40) ? -1 : m;
}

extern "C" int fer_conv2d_cols(int dtype, const void* x, int64_t ldx, void* cols, int64_t ldc, int B, int H, int W,
                               int C, fer_stream_t stream) {
  if (check_dtype(dtype, "conv2d_cols: unknown dtype")) return -1;
  const int V = piece_len(dtype);
  const long M = pixels(B, H, W);
  if (M < 0 || C < 1) return set_error("conv2d_cols: B, H, W, C must be >= 1");
  if (C % V) return set_error("conv2d_cols: C must be a multiple of the 16-byte piece (8 bf16 / 4 fp32)");
  if (!piece_ok(x, ldx, C, V)) return set_error("conv2d_cols: x needs 16-byte aligned rows of stride >= C");
  if (!piece_ok(cols, ldc, 9 * C, V)) return set_error("conv2d_cols: cols needs 16-byte aligned rows of stride >= 9*C");
  const long n = M * (C / V);
  if (too_many(n)) return set_error("conv2d_cols: too many elements for one launch");
  hipStream_t st = (hipStream_t)stream;
  with_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(conv2d_cols_kernel<T>, dim3(blocks_for(n)), dim3(256), 0, st, (const T*)x, (long)ldx, (T*)cols,
                       (long)ldc, H, W, C, M);
  });
  return hip_check("conv2d_cols");
}

extern "C" int fer_conv2d_cols_bwd(int dtype, const void* dcols, int64_t ldd, void* dx, int64_t lddx, int B, int H,
                                   int W, int C, fer_stream_t stream) {
  if (check_dtype(dtype, "conv2d_cols_bwd: unknown dtype")) return -1;
  const int V = piece_len(dtype);
  const long M = pixels(B, H, W);
  if (M < 0 || C < 1) return set_error("conv2d_cols_bwd: B, H, W, C must be >= 1");
  if (C % V) return set_error("conv2d_cols_bwd: C must be a multiple of the 16-byte piece (8 bf16 / 4 fp32)");
  if (!piece_ok(dcols, ldd, 9 * C, V))
    return set_error("conv2d_cols_bwd: dcols needs 16-byte aligned rows of stride >= 9*C");
  if (!piece_ok(dx, lddx, C, V)) return set_error("conv2d_cols_bwd: dx needs 16-byte aligned rows of stride >= C");
  const long n = M * (C / V);
  if (too_many(n)) return set_error("conv2d_cols_bwd: too many elements for one launch");
  hipStream_t st = (hipStream_t)stream;
  with_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(conv2d_cols_bwd_kernel<T>, dim3(blocks_for(n)), dim3(256), 0, st, (const T*)dcols, (long)ldd,
                       (T*)dx, (long)lddx, H, W, C, M);
  });
  return hip_check("conv2d_cols_bwd");
}

extern "C" int fer_conv2d_c1_fwd(int dtype, const void* x, int64_t ldx, const float* w, const float* bias, void* y,
                                 int64_t ldy, int B, int H, int W, int Cout, fer_stream_t stream) {
  if (check_dtype(dtype, "conv2d_c1_fwd: unknown dtype")) return -1;
  const int V = piece_len(dtype);
  const long M = pixels(B, H, W);
  if (M < 0 || Cout < 1) return set_error("conv2d_c1_fwd: B, H, W, Cout must be >= 1");
  if (Cout % V || Cout > C1_MAX_COUT)
    return set_error("conv2d_c1_fwd: Cout must be a multiple of the 16-byte piece (8 bf16 / 4 fp32), at most "
                     "FER_CONV2D_C1_MAX_COUT");
  if (!x || ldx < 1 || !w) return set_error("conv2d_c1_fwd: x or w is null, or x's stride is below 1");
  if (!piece_ok(y, ldy, Cout, V)) return set_error("conv2d_c1_fwd: y needs 16-byte aligned rows of stride >= Cout");
  const long n = M * (Cout / V);
  if (too_many(n)) return set_error("conv2d_c1_fwd: too many elements for one launch");
  hipStream_t st = (hipStream_t)stream;
  with_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(conv2d_c1_fwd_kernel<T>, dim3(blocks_for(n)), dim3(256), (size_t)Cout * 9 * sizeof(float), st,
                       (const T*)x, (long)ldx, w, bias, (T*)y, (long)ldy, H, W, Cout, M);
  });
  return hip_check("conv2d_c1_fwd");
}

extern "C" int fer_conv2d_c1_bwd(int dtype, const void* dy, int64_t lddy, const void* x, int64_t ldx, const float* w,
                                 float* dw_part, int n_parts, void* dx, int64_t lddx, int B, int H, int W, int Cout,
                                 fer_stream_t stream) {
  if (check_dtype(dtype, "conv2d_c1_bwd: unknown dtype")) return -1;
  const int V = piece_len(dtype);
  const long M = pixels(B, H, W);
  if (M < 0 || Cout < 1) return set_error("conv2d_c1_bwd: B, H, W, Cout must be >= 1");
  if (Cout % V || Cout > C1_MAX_COUT)
    return set_error("conv2d_c1_bwd: Cout must be a multiple of the 16-byte piece (8 bf16 / 4 fp32), at most "
                     "FER_CONV2D_C1_MAX_COUT");
  if (!dw_part && !dx) return set_error("conv2d_c1_bwd: no output requested");
  if (!piece_ok(dy, lddy, Cout, V)) return set_error("conv2d_c1_bwd: dy needs 16-byte aligned rows of stride >= Cout");
  if (dw_part && (!x || ldx < 1 || n_parts < 1 || !al16(dw_part)))
    return set_error("conv2d_c1_bwd: dw_part needs x (stride >= 1), n_parts >= 1 and a 16-byte aligned buffer");
  if (dx && (!w || lddx < 1)) return set_error("conv2d_c1_bwd: dx needs w and a stride >= 1");
  if (too_many(M)) return set_error("conv2d_c1_bwd: too many elements for one launch");
  hipStream_t st = (hipStream_t)stream;
  with_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    if (dw_part)
      hipLaunchKernelGGL(conv2d_c1_dw_kernel<T>, dim3(n_parts), dim3(256), 0, st, (const T*)dy, (long)lddy,
                         (const T*)x, (long)ldx, dw_part, H, W, Cout, M, (M + n_parts - 1) / n_parts);
    if (dx)
      hipLaunchKernelGGL(conv2d_c1_dx_kernel<T>, dim3(blocks_for(M)), dim3(256), (size_t)Cout * 9 * sizeof(float), st,
                         (const T*)dy, (long)lddy, w, (T*)dx, (long)lddx, H, W, Cout, M);
  });
  return hip_check("conv2d_c1_bwd");
}

// shared argument checks of the two pool entry points; returns M (input pixels) or -1 with the error set
static long pool_check(const char* who, int V, int B, int H, int W, int C, int pool, uint32_t thr, char* msg,
                       size_t len) {
  const long M = pixels(B, H, W);
  const char* why = nullptr;
  if (M < 0 || C < 1) why = "B, H, W, C must be >= 1";
  else if (C % V) why = "C must be a multiple of the 16-byte piece (8 bf16 / 4 fp32)";
  else if (pool != 0 && pool != 1) why = "pool must be 0 or 1";
  else if (pool && (H < 2 || W < 2)) why = "MaxPool2d((2, 2)) needs H >= 2 and W >= 2";
  else if (thr > 65536u) why = "drop_thresh above 65536";
  else if (thr && (long)B * C > 0xFFFFFFFFL) why = "dropout over >= 2^32 planes";
  if (!why) return M;
  snprintf(msg, len, "%s: %s", who, why);
  set_error(msg);
  return -1;
}

extern "C" int fer_pool2_chdrop_fwd(int dtype, const void* x, int64_t ldx, void* y, int64_t ldy, int B, int H, int W,
                                    int C, int pool, uint32_t drop_thresh, float drop_scale, uint64_t seed,
                                    fer_stream_t stream) {
  if (check_dtype(dtype, "pool2_chdrop_fwd: unknown dtype")) return -1;
  const int V = piece_len(dtype);
  char msg[160];
  const long M = pool_check("pool2_chdrop_fwd", V, B, H, W, C, pool, drop_thresh, msg, sizeof(msg));
  if (M < 0) return -1;
  if (!piece_ok(x, ldx, C, V) || !piece_ok(y, ldy, C, V))
    return set_error("pool2_chdrop_fwd: x, y need 16-byte aligned rows of stride >= C");
  const long Mo = pool ? (long)B * (H / 2) * (W / 2) : M, n = Mo * (C / V);
  if (too_many(n)) return set_error("pool2_chdrop_fwd: too many elements for one launch");
  hipStream_t st = (hipStream_t)stream;
  with_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(pool2_chdrop_fwd_kernel<T>, dim3(blocks_for(n)), dim3(256), 0, st, (const T*)x, (long)ldx,
                       (T*)y, (long)ldy, H, W, C, pool, drop_thresh, drop_scale, seed, Mo);
  });
  return hip_check("pool2_chdrop_fwd");
}

extern "C" int fer_pool2_chdrop_bwd(int dtype, const void* dy, int64_t lddy, const void* x, int64_t ldx, void* dx,
                                    int64_t lddx, int B, int H, int W, int C, int pool, uint32_t drop_thresh,
                                    float drop_scale, uint64_t seed, fer_stream_t stream) {
  if (check_dtype(dtype, "pool2_chdrop_bwd: unknown dtype")) return -1;
  const int V = piece_len(dtype);
  char msg[160];
  const long M = pool_check("pool2_chdrop_bwd", V, B, H, W, C, pool, drop_thresh, msg, sizeof(msg));
  if (M < 0) return -1;
  if (!piece_ok(dy, lddy, C, V) || !piece_ok(dx, lddx, C, V))
    return set_error("pool2_chdrop_bwd: dy, dx need 16-byte aligned rows of stride >= C");
  if (pool && !piece_ok(x, ldx, C, V))
    return set_error("pool2_chdrop_bwd: pooling needs the forward's x, 16-byte aligned rows of stride >= C");
  const long n = M * (C / V);
  if (too_many(n)) return set_error("pool2_chdrop_bwd: too many elements for one launch");
  hipStream_t st = (hipStream_t)stream;
  with_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(pool2_chdrop_bwd_kernel<T>, dim3(blocks_for(n)), dim3(256), 0, st, (const T*)dy, (long)lddy,
                       (const T*)x, (long)ldx, (T*)dx, (long)lddx, H, W, C, pool, drop_thresh, drop_scale, seed, M);
  });
  return hip_check("pool2_chdrop_bwd");
}
