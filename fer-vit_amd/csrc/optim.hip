// The training step outside the model: fused AdamW over FlatParams segments, the device step
// counter's advance, the transposed bf16 weight shadow, the gradient-clip coefficient, and the
// flat element-wise kernels (casts, axpy, stand-alone dropout).
#include "common.h"
#include "fervit_internal.h"
#include "step_seed.h"

namespace fer {

// ------------------------------------------------------------------ elementwise
__global__ void cast_f32_bf16_kernel(const float* __restrict__ x, bf16* __restrict__ y, long n) {
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256L) y[i] = (bf16)x[i];
}
__global__ void cast_bf16_f32_kernel(const bf16* __restrict__ x, float* __restrict__ y, long n) {
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256L) y[i] = (float)x[i];
}
template <typename T>
__global__ void axpy_kernel(const T* __restrict__ x, const T* __restrict__ t, const float* __restrict__ s,
                            T* __restrict__ y, long n) {
  const float a = *s;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256L)
    y[i] = from_f<T>(to_f<T>(x[i]) + a * to_f<T>(t[i]));
}
template <typename T>
__global__ void dropout_kernel(const T* __restrict__ x, T* __restrict__ y, long n, uint32_t thr, float sc,
                               uint64_t seed) {
  seed = step_seed(seed);
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256L)
    y[i] = from_f<T>(drop_keep(seed, (uint32_t)i, thr) ? to_f<T>(x[i]) * sc : 0.f);
}
__global__ void clip_coef_kernel(const float* sumsq, float sq_scale, float max_norm, float* coef) {
  if (threadIdx.x) return;
  const float nrm = sqrtf(*sumsq * sq_scale);
  *coef = fminf(1.f, max_norm / (nrm + 1e-6f));
}

// ------------------------------------------------------------------ AdamW
__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                    float* __restrict__ m, float* __restrict__ v, bf16* __restrict__ pb,
                                                    const fer_adamw_segment* __restrict__ segs, float gscale,
                                                    const float* __restrict__ clip,
                                                    const uint64_t* __restrict__ step_add) {
  const fer_adamw_segment sg = segs[blockIdx.y];
  const float sc = gscale * (clip ? *clip : 1.f);
  const float t = (float)(sg.step + (step_add ? (long)*step_add : 0L));  // + graph replays
  const float bc1 = 1.f - powf(sg.beta1, t);
  const float bc2 = 1.f - powf(sg.beta2, t);
  const float step_size = sg.lr / bc1;
  const float bc2s = sqrtf(bc2);
  const float decay = 1.f - sg.lr * sg.weight_decay;
  // 16-byte accesses over the segment's multiple-of-4 head (segment offsets are 64-element aligned
  // in FlatParams; checked per segment), then the per-element loop over the tail -- the same
  // arithmetic per element either way
  long j0 = 0;
  if ((sg.offset & 3) == 0) {
    j0 = sg.numel & ~3L;
    for (long j = (blockIdx.x * 256L + threadIdx.x) * 4; j < j0; j += (long)gridDim.x * 1024L) {
      const long i = sg.offset + j;
      const f32x4 g4 = *(const f32x4*)(g + i);
      f32x4 p4 = *(const f32x4*)(p + i), m4 = *(const f32x4*)(m + i), v4 = *(const f32x4*)(v + i);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float gr = g4[e] * sc;
        float pv = p4[e] * decay;
        const float mv = sg.beta1 * m4[e] + (1.f - sg.beta1) * gr;
        const float vv = sg.beta2 * v4[e] + (1.f - sg.beta2) * gr * gr;
        m4[e] = mv;
        v4[e] = vv;
        pv -= step_size * mv / (sqrtf(vv) / bc2s + sg.eps);
        p4[e] = pv;
      }
      *(f32x4*)(m + i) = m4;
      *(f32x4*)(v + i) = v4;
      *(f32x4*)(p + i) = p4;
      if (pb) *(bf16x4*)(pb + i) = bf16x4{(bf16)p4[0], (bf16)p4[1], (bf16)p4[2], (bf16)p4[3]};
    }
  }
  for (long j = j0 + blockIdx.x * 256L + threadIdx.x; j < sg.numel; j += (long)gridDim.x * 256L) {
    const long i = sg.offset + j;
    const float gr = g[i] * sc;
    float pv = p[i] * decay;
    const float mv = sg.beta1 * m[i] + (1.f - sg.beta1) * gr;
    const float vv = sg.beta2 * v[i] + (1.f - sg.beta2) * gr * gr;
    m[i] = mv;
    v[i] = vv;
    pv -= step_size * mv / (sqrtf(vv) / bc2s + sg.eps);
    p[i] = pv;
    if (pb) pb[i] = (bf16)pv;
  }
}

// Transposed bf16 weight shadow: for each 2-D segment {off, rows, cols, first_tile} of a flat
// buffer, dst[off + c*rows + r] = src[off + r*cols + c]. One launch over all segments (64x64
// tiles through LDS, block -> segment by binary search on first_tile). The dgrad GEMMs read the
// result as a K-contiguous operand (dX = dY W = dY (W^T)^T), which streams through the
// 16-byte-row DMA path instead of the transposed-LDS-read path of an MN operand.
__global__ __launch_bounds__(256) void transpose_segs_kernel(const uint16_t* __restrict__ src,
                                                             uint16_t* __restrict__ dst,
                                                             const int64_t* __restrict__ segs, int nseg) {
  __shared__ uint32_t tile[64][33];  // 64 rows x 64 bf16 (as 32 pairs), +1 word pad
  __shared__ __attribute__((aligned(16))) uint16_t t16x[64 * 72];  // fast path: rows padded by 16 B
  const long t = blockIdx.x;
  int lo = 0, hi = nseg - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (segs[mid * 4 + 3] <= t) lo = mid;
    else hi = mid - 1;
  }
  const long off = segs[lo * 4], rows = segs[lo * 4 + 1], cols = segs[lo * 4 + 2];
  const long lt = t - segs[lo * 4 + 3], tc = (cols + 63) / 64;
  const long r0 = (lt / tc) * 64, c0 = (lt % tc) * 64;
  const uint16_t* s = src + off;
  uint16_t* d = dst + off;
  const int tid = threadIdx.x;
  if (r0 + 64 <= rows && c0 + 64 <= cols && rows % 8 == 0 && cols % 8 == 0 && off % 8 == 0) {
    // full, 16-byte aligned tile: 16-byte loads along input rows, 16-byte stores along output rows
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int i = tid + k * 256, r = i >> 3, ch = i & 7;
      const uint4 v = *(const uint4*)(s + (r0 + r) * cols + c0 + ch * 8);
      *(uint4*)(t16x + r * 72 + ch * 8) = v;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int i = tid + k * 256, c = i >> 3, rc = i & 7;  // output row c, 8 input rows from rc*8
      uint16_t e[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) e[j] = t16x[(rc * 8 + j) * 72 + c];
      uint4 o;
      o.x = e[0] | ((uint32_t)e[1] << 16);
      o.y = e[2] | ((uint32_t)e[3] << 16);
      o.z = e[4] | ((uint32_t)e[5] << 16);
      o.w = e[6] | ((uint32_t)e[7] << 16);
      *(uint4*)(d + (c0 + c) * rows + r0 + rc * 8) = o;
    }
    return;
  }
  // load: row r, column pair cp (2 bf16); 64 x 32 pairs = 2048 / 256 threads
  for (int i = tid; i < 64 * 32; i += 256) {
    const int r = i >> 5, cp = i & 31;
    const long gr = r0 + r, gc = c0 + cp * 2;
    uint32_t v = 0;
    if (gr < rows) {
      const uint16_t lo16 = gc < cols ? s[gr * cols + gc] : 0;
      const uint16_t hi16 = gc + 1 < cols ? s[gr * cols + gc + 1] : 0;
      v = lo16 | ((uint32_t)hi16 << 16);
    }
    tile[r][cp] = v;
  }
  __syncthreads();
  // store: output row c (= input column), pair of input rows rp
  for (int i = tid; i < 64 * 32; i += 256) {
    const int c = i >> 5, rp = i & 31;
    const long gc = c0 + c, gr = r0 + rp * 2;
    if (gc >= cols) continue;
    const uint32_t a = tile[rp * 2][c >> 1], b = tile[rp * 2 + 1][c >> 1];
    const uint16_t x0 = (c & 1) ? (uint16_t)(a >> 16) : (uint16_t)a;
    const uint16_t x1 = (c & 1) ? (uint16_t)(b >> 16) : (uint16_t)b;
    if (gr + 1 < rows && ((off + gc * rows + gr) & 1) == 0) {
      *(uint32_t*)(d + gc * rows + gr) = x0 | ((uint32_t)x1 << 16);
    } else {
      if (gr < rows) d[gc * rows + gr] = x0;
      if (gr + 1 < rows) d[gc * rows + gr + 1] = x1;
    }
  }
}

}  // namespace fer

using namespace fer;

extern "C" int fer_cast_f32_bf16(const float* x, void* y, int64_t n, fer_stream_t stream) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(cast_f32_bf16_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, x, (bf16*)y, (long)n);
  return hip_check("cast_f32_bf16");
}
extern "C" int fer_cast_bf16_f32(const void* x, float* y, int64_t n, fer_stream_t stream) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(cast_bf16_f32_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, (const bf16*)x, y,
                     (long)n);
  return hip_check("cast_bf16_f32");
}
extern "C" int fer_axpy(int dtype, const void* x, const void* t, const float* scale_ptr, void* y, int64_t n,
                        fer_stream_t stream) {
  if (check_dtype(dtype, "axpy: unknown dtype")) return -1;
  if (n <= 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  with_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(axpy_kernel<T>, dim3(grid_for(n)), dim3(256), 0, st, (const T*)x, (const T*)t, scale_ptr,
                       (T*)y, (long)n);
  });
  return hip_check("axpy");
}
extern "C" int fer_clip_coef(const float* sumsq, float sq_scale, float max_norm, float* coef, fer_stream_t stream) {
  hipLaunchKernelGGL(clip_coef_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, sumsq, sq_scale, max_norm, coef);
  return hip_check("clip_coef");
}
extern "C" int fer_dropout(int dtype, const void* x, void* y, int64_t n, uint32_t drop_thresh, float drop_scale,
                           uint64_t seed, fer_stream_t stream) {
  if (check_dtype(dtype, "dropout: unknown dtype")) return -1;
  if (n <= 0) return 0;
  if (check_drop_range(drop_thresh, n, "dropout: >= 2^32 elements")) return -1;
  hipStream_t st = (hipStream_t)stream;
  with_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(dropout_kernel<T>, dim3(grid_for(n)), dim3(256), 0, st, (const T*)x, (T*)y, (long)n,
                       drop_thresh, drop_scale, seed);
  });
  return hip_check("dropout");
}

extern "C" int fer_transpose_bf16_segments(const void* src, void* dst, const int64_t* segs, int nseg,
                                          int64_t total_tiles, fer_stream_t stream) {
  if (nseg <= 0 || total_tiles <= 0) return 0;
  if (!src || !dst || !segs || src == dst) return set_error("transpose_bf16_segments: bad pointers (in-place is not supported)");
  hipLaunchKernelGGL(transpose_segs_kernel, dim3((unsigned)total_tiles), dim3(256), 0, (hipStream_t)stream,
                     (const uint16_t*)src, (uint16_t*)dst, segs, nseg);
  return hip_check("transpose_bf16_segments");
}

__global__ void step_advance_kernel(uint64_t* counter) {
  if (threadIdx.x == 0) *counter += 1;
}

extern "C" int fer_step_advance(uint64_t* counter, fer_stream_t stream) {
  hipLaunchKernelGGL(step_advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, counter);
  return hip_check("step_advance");
}

extern "C" int fer_adamw(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, void* param_bf16,
                         const fer_adamw_segment* segs_device, int nsegs, int64_t max_seg_numel, float grad_scale,
                         const float* clip_coef, const uint64_t* step_add, fer_stream_t stream) {
  if (nsegs <= 0) return 0;
  // blocks per segment: enough for the largest one to stream at full rate (the grid-stride loop
  // covers the rest); every block of a smaller segment past its end exits at once, and with one
  // block per 1024 elements of the largest segment those empty blocks (~80 % of a latent-ViT
  // launch's 82 k blocks) cost more than the update itself
  const long per_seg = std::max<long>(8, std::min<long>(256, 32768 / std::max(1, nsegs)));
  dim3 grid((unsigned)std::max<long>(1, std::min<long>((max_seg_numel + 1023) / 1024, per_seg)), nsegs);
  hipLaunchKernelGGL(adamw_kernel, grid, dim3(256), 0, (hipStream_t)stream, param, grad, exp_avg, exp_avg_sq,
                     (bf16*)param_bf16, segs_device, grad_scale, clip_coef, step_add);
  return hip_check("adamw");
}
