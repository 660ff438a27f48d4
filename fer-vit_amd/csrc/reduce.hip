// Deterministic reductions: the second pass over per-block partial sums (part_reduce, which every
// other translation unit calls through fervit_internal.h), its process-wide deferral window
// (fer_reduce_defer / fer_reduce_flush), bias-gradient column sums (fer_colsum) and dot / sumsq.
// All cross-row reductions are two-pass (per-block partials, then a fixed-order sum),
// so every result is bitwise reproducible run to run.
#include <mutex>

#include "common.h"
#include "fervit_internal.h"

namespace fer {

// ------------------------------------------------------------------ reductions
// Deterministic second pass: out_k[c % seg] (+)= scale * sum_{b<nb} part[b*ld + c],
// k = c / seg selects one of three outputs.
// CB columns per block x (256 / CB) row phases, 8 independent accumulators per thread (8 loads in
// flight; the partial slabs are read once and the sum is latency-bound otherwise). CB is picked so
// that the grid covers the CUs (ViT-B: 2304 columns -> 288 blocks of 8 columns instead of 72 of
// 32). Fixed association order for a given shape -> deterministic.
template <int CB>
__device__ __forceinline__ void part_reduce_body(const float* __restrict__ part, int nb, long ld, int ncols, int seg,
                                                 float* o0, float* o1, float* o2, int accumulate,
                                                 const float* __restrict__ scale, int bx) {
  constexpr int RP = 256 / CB;
  __shared__ float red[RP][CB + 1];
  const int cx = threadIdx.x % CB, j = threadIdx.x / CB;
  const int c = bx * CB + cx;
  float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (c < ncols) {
    int b = j;
    for (; b + 7 * RP < nb; b += 8 * RP) {
#pragma unroll
      for (int u = 0; u < 8; ++u) s[u] += part[(long)(b + RP * u) * ld + c];
    }
    for (int u = 0; b < nb; b += RP, ++u) s[u] += part[(long)b * ld + c];
  }
  red[j][cx] = ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
  __syncthreads();
  if (j == 0 && c < ncols) {
    float t = 0.f;
#pragma unroll 8
    for (int i = 0; i < RP; ++i) t += red[i][cx];
    if (scale) t *= *scale;
    const int k = c / seg, col = c - k * seg;
    float* o = k == 0 ? o0 : (k == 1 ? o1 : o2);
    if (o) o[col] = accumulate ? o[col] + t : t;
  }
}
template <int CB>
__global__ __launch_bounds__(256) void part_reduce_kernel(const float* __restrict__ part, int nb, long ld, int ncols,
                                                          int seg, float* o0, float* o1, float* o2, int accumulate,
                                                          const float* __restrict__ scale) {
  part_reduce_body<CB>(part, nb, ld, ncols, seg, o0, o1, o2, accumulate, scale, blockIdx.x);
}

// Deferred reductions (fer_reduce_defer): inside a backward pass the column partials of the bias /
// LayerNorm / attention-bias gradients are written into an arena instead of the shared scratch and
// their part_reduce launches are queued; fer_reduce_flush (the end of the backward, or before a
// gradient-ready hook such as the DDP bucket all-reduce reads them) runs them all as ONE launch.
// Same per-column arithmetic as part_reduce_kernel<8> (the batch only takes shapes that would use
// the 8-column kernel), so bit-identical results; only their time on the compute stream moves.
struct RedDesc {
  const float* part;
  long ld;
  float* o[3];
  int nb, ncols, seg, accumulate, blk0;
};
constexpr int kRedMax = 56;  // kernel-argument budget (64 bytes each)
struct RedBatch {
  RedDesc d[kRedMax];
  int n;
};
// The batch kernel: 64 columns per block (a wave reads 256 contiguous bytes of a partial row,
// where part_reduce_kernel<8>'s 8-column blocks read 32-byte pieces -- it needs narrow blocks to
// spread one small reduction over the CUs; a batch has blocks enough). Lane = column, wave w owns
// the row phases j = 8w .. 8w+7 of part_reduce_kernel<8> (RP = 32) and runs each with the same
// eight accumulators in the same order, then the phases are summed in order j = 0..31: the same
// float operations per column as the immediate kernel, so bit-identical.
__global__ __launch_bounds__(256) void part_reduce_multi_kernel(const RedBatch b) {
  constexpr int RP = 32;
  __shared__ float red[RP][65];
  int i = 0;
  while (i + 1 < b.n && (int)blockIdx.x >= b.d[i + 1].blk0) ++i;
  const RedDesc& d = b.d[i];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int c = (blockIdx.x - d.blk0) * 64 + lane;
  const float* __restrict__ part = d.part;
  const int nb = d.nb;
  const long ld = d.ld;
  for (int jj = 0; jj < 8; ++jj) {
    const int j = w * 8 + jj;
    float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (c < d.ncols) {
      int bb = j;
      for (; bb + 7 * RP < nb; bb += 8 * RP) {
#pragma unroll
        for (int u = 0; u < 8; ++u) s[u] += part[(long)(bb + RP * u) * ld + c];
      }
      for (int u = 0; bb < nb; bb += RP, ++u) s[u] += part[(long)bb * ld + c];
    }
    red[j][lane] = ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
  }
  __syncthreads();
  if (w == 0 && c < d.ncols) {
    float t = 0.f;
#pragma unroll 8
    for (int k = 0; k < RP; ++k) t += red[k][lane];
    const int k = c / d.seg, col = c - k * d.seg;
    float* o = k == 0 ? d.o[0] : (k == 1 ? d.o[1] : d.o[2]);
    if (o) o[col] = d.accumulate ? o[col] + t : t;
  }
}
// One window per process, on one device (fer_reduce_defer rejects a second device while open); the
// state is guarded by g_red_mu (part_reduce / reduction_ws are reached from every host entry point).
static std::mutex g_red_mu;
static struct {
  bool on = false, take = false;  // window open (queue valid) / taking new reductions
  int dev = -1;
  char* arena = nullptr;
  size_t cap = 0, used = 0;
  hipStream_t st = nullptr;
  RedBatch b;
  int blocks = 0;
} g_red;
static bool red_batchable(int ncols) { return ceil_div(ncols, 16) < 256; }
static int red_flush() {
  if (g_red.b.n) {
    hipLaunchKernelGGL(part_reduce_multi_kernel, dim3(g_red.blocks), dim3(256), 0, g_red.st, g_red.b);
    g_red.b.n = 0;
    g_red.blocks = 0;
  }
  g_red.used = 0;
  return hip_check("reduce_flush");
}
// Only partial sets up to 2 MB are deferred: the small-token
// configurations' (latent w+ 1.5-1.9 MB per LayerNorm / attention bias) gain one launch each
// (latent ViT 2.22 -> 2.16 ms), while ViT-B's (4.7-16.5 MB, 52 per step) measured 35.62 -> 35.75
// ms deferred (their sums then re-read from HBM at the end of the backward instead of from the
// last-level cache right after the producer; profiles/r03am_reduce_defer_ab.txt).
float* reduction_ws(float* ws, size_t bytes, int ncols, hipStream_t st) {
  constexpr size_t max_b = 2048 * 1024L;
  std::lock_guard<std::mutex> lk(g_red_mu);
  if (!g_red.take || st != g_red.st || !red_batchable(ncols) || bytes > g_red.cap || bytes > max_b) return ws;
  bytes = (bytes + 255) & ~(size_t)255;
  if (g_red.used + bytes > g_red.cap || g_red.b.n == kRedMax) red_flush();
  float* p = (float*)(g_red.arena + g_red.used);
  g_red.used += bytes;
  return p;
}

void part_reduce(const float* part, int nb, long ld, int ncols, int seg, float* o0, float* o1, float* o2,
                 int accumulate, const float* scale, hipStream_t st) {
  std::lock_guard<std::mutex> lk(g_red_mu);
  const bool in_arena = g_red.take && st == g_red.st && (const char*)part >= g_red.arena &&
                        (const char*)part < g_red.arena + g_red.cap;
  // an output range overlapping a queued one (any base pointer: segmented o0/o1/o2 outputs vs a
  // whole-buffer output): run the queue first, keeping the two updates in stream order
  auto span = [](float* const (&o)[3], int k, int ncols, int seg) -> std::pair<const float*, const float*> {
    const int n = std::min(seg, ncols - k * seg);
    return o[k] && n > 0 ? std::make_pair((const float*)o[k], (const float*)o[k] + n)
                         : std::make_pair((const float*)nullptr, (const float*)nullptr);
  };
  float* const mine[3] = {o0, o1, o2};
  bool dup = false;
  for (int i = 0; i < g_red.b.n && !dup; ++i)
    for (int k = 0; k < 3 && !dup; ++k) {
      const auto q = span(g_red.b.d[i].o, k, g_red.b.d[i].ncols, g_red.b.d[i].seg);
      if (!q.first) continue;
      for (int j = 0; j < 3 && !dup; ++j) {
        const auto m = span(mine, j, ncols, seg);
        dup = m.first && m.first < q.second && q.first < m.second;
      }
    }
  if (in_arena && !scale && red_batchable(ncols) && g_red.b.n < kRedMax && !dup) {
    g_red.b.d[g_red.b.n++] = RedDesc{part, ld, {o0, o1, o2}, nb, ncols, seg, accumulate, g_red.blocks};
    g_red.blocks += ceil_div(ncols, 64);
    return;
  }
  if (g_red.b.n && (in_arena || dup)) {  // run the queue first; this call's partials stay valid
    const size_t keep = g_red.used;
    red_flush();
    g_red.used = keep;
  }
  if (ceil_div(ncols, 16) >= 256)
    hipLaunchKernelGGL(part_reduce_kernel<16>, dim3(ceil_div(ncols, 16)), dim3(256), 0, st, part, nb, ld, ncols, seg,
                       o0, o1, o2, accumulate, scale);
  else
    hipLaunchKernelGGL(part_reduce_kernel<8>, dim3(ceil_div(ncols, 8)), dim3(256), 0, st, part, nb, ld, ncols, seg,
                       o0, o1, o2, accumulate, scale);
  if (in_arena && !g_red.b.n) g_red.used = 0;
}

// ------------------------------------------------------------------ colsum
// part[rb][n] = sum over row chunk rb of x[m][n]; block = 64 vec4 columns x 4 row phases.
constexpr int CS_ROWBLK = 256;
template <typename T>
__global__ __launch_bounds__(256) void colsum_part_kernel(const T* __restrict__ x, long ldx, int M, int N,
                                                          float* __restrict__ part, int rows_per_blk) {
  __shared__ f32x4 red[4][64];
  const int c4 = blockIdx.x * 64 + (threadIdx.x & 63);
  const int j = threadIdx.x >> 6;
  const int r0 = blockIdx.y * rows_per_blk, r1 = min(M, r0 + rows_per_blk);
  f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = s0;
  if (c4 * 4 < N) {
    int r = r0 + j;
    for (; r + 4 < r1; r += 8) {
      s0 += load4<T>(x + (long)r * ldx + c4 * 4);
      s1 += load4<T>(x + (long)(r + 4) * ldx + c4 * 4);
    }
    if (r < r1) s0 += load4<T>(x + (long)r * ldx + c4 * 4);
  }
  red[j][threadIdx.x & 63] = s0 + s1;
  __syncthreads();
  if (j == 0 && c4 * 4 < N) {
    const int t = threadIdx.x & 63;
    *(f32x4*)(part + (long)blockIdx.y * N + c4 * 4) = red[0][t] + red[1][t] + red[2][t] + red[3][t];
  }
}
// row blocks of 32 rows (up to 256): a 4,864-row colsum (hybrid adapters' bias gradients) was
// 38 x 3 = 114 workgroups of 128 rows, 7.6 us for 7.5 MB
static int colsum_nblk(int M) { return std::max(1, std::min(ceil_div(M, 32), CS_ROWBLK)); }

// ------------------------------------------------------------------ dot / sumsq
template <typename T>
__global__ __launch_bounds__(256) void dot_part_kernel(const T* __restrict__ a, const T* __restrict__ b, long n,
                                                       float* __restrict__ part) {
  __shared__ float red[4];
  float s = 0.f;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256L)
    s += to_f<T>(a[i]) * (b ? to_f<T>(b[i]) : to_f<T>(a[i]));
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}
// Fixed-order (deterministic) sum of the partials: thread t adds partials t, t+256, ... in order,
// then a butterfly per wave and the four wave sums in order. (One thread walking up to 1024 partials
// was a chain of dependent L2 loads: 46 us per call, the hybrid adapters' alpha gradients 0.5 ms
// per step.)
__global__ __launch_bounds__(256) void sum_final_kernel(const float* __restrict__ part, int n, float* out,
                                                        int accumulate) {
  __shared__ float red[4];
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) s += part[i];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float t = (red[0] + red[1]) + (red[2] + red[3]);
    *out = accumulate ? *out + t : t;
  }
}

}  // namespace fer

using namespace fer;

extern "C" int64_t fer_colsum_ws(int M, int N) { return (int64_t)colsum_nblk(M) * N * 4; }

extern "C" int fer_reduce_defer(int mode, void* arena, int64_t arena_bytes, fer_stream_t stream) {
  std::lock_guard<std::mutex> lk(g_red_mu);
  if (mode == 2) {  // pause: keep the queue, stop taking new reductions
    g_red.take = false;
    return 0;
  }
  if (mode != 0 && mode != 1) return set_error("reduce_defer: mode must be 0, 1 or 2");
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess) return set_error("reduce_defer: hipGetDevice failed");
  if (mode == 1 && g_red.on && dev != g_red.dev)
    return set_error("reduce_defer: a window is open on another device (one window per process)");
  const bool same = g_red.on && g_red.arena == (char*)arena && g_red.cap == (size_t)arena_bytes &&
                    g_red.st == (hipStream_t)stream;
  if (g_red.on && (mode == 0 || !same)) {
    const int rc = red_flush();
    g_red.on = g_red.take = false;
    if (rc) return rc;
  }
  if (mode == 0) return 0;
  if (!arena || arena_bytes < 65536) return set_error("reduce_defer: arena too small");
  if (!same) {
    g_red.arena = (char*)arena;
    g_red.cap = (size_t)arena_bytes;
    g_red.st = (hipStream_t)stream;
    g_red.used = 0;
  }
  g_red.dev = dev;
  g_red.on = g_red.take = true;
  return 0;
}

extern "C" int fer_reduce_flush(void) {
  std::lock_guard<std::mutex> lk(g_red_mu);
  return g_red.on ? red_flush() : 0;
}

extern "C" int fer_colsum(int dtype, const void* x, int64_t ldx, int M, int N, float* out, int accumulate,
                          const float* scale_ptr, float* ws, int64_t ws_bytes, fer_stream_t stream) {
  if (check_dtype(dtype, "colsum: unknown dtype")) return -1;
  if (N <= 0) return 0;
  if (N % 4 || ldx % 4) return set_error("colsum: N and ld must be multiples of 4");
  const int nblk = colsum_nblk(M);
  if (!ws || ws_bytes < fer_colsum_ws(M, N)) return set_error("colsum: workspace too small");
  const int rpb = ceil_div(std::max(M, 1), nblk);
  hipStream_t st = (hipStream_t)stream;
  ws = reduction_ws(ws, (size_t)fer_colsum_ws(M, N), N, st);
  dim3 grid(ceil_div(N / 4, 64), nblk);
  with_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(colsum_part_kernel<T>, grid, dim3(256), 0, st, (const T*)x, (long)ldx, M, N, ws, rpb);
  });
  part_reduce(ws, nblk, N, N, N, out, nullptr, nullptr, accumulate, scale_ptr, st);
  return hip_check("colsum");
}

static int dot_blocks(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>((n + 1023) / 1024, 1024)); }
extern "C" int fer_dot(int dtype, const void* a, const void* b, int64_t n, float* out, int accumulate, float* ws,
                       int64_t ws_bytes, fer_stream_t stream) {
  if (check_dtype(dtype, "dot: unknown dtype")) return -1;
  const int nb = dot_blocks(n);
  if (!ws || ws_bytes < nb * 4) return set_error("dot: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  with_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(dot_part_kernel<T>, dim3(nb), dim3(256), 0, st, (const T*)a, (const T*)b, (long)n, ws);
  });
  hipLaunchKernelGGL(sum_final_kernel, dim3(1), dim3(256), 0, st, ws, nb, out, accumulate);
  return hip_check("dot");
}
extern "C" int fer_sumsq(const float* x, int64_t n, float* out, float* ws, int64_t ws_bytes, fer_stream_t stream) {
  return fer_dot(FER_F32, x, nullptr, n, out, 0, ws, ws_bytes, stream);
}
