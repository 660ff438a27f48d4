// Grouped linear layers and the highway mix of the AFS style extractor (reference `afs/style_extractor.py`:
// 18 independent StyleBlocks, one per w+ layer: Linear(512, 256) -> 2 x HighwayLayer(256) -> Linear(256, 512)).
// One launch covers one stage of all G blocks: every operand of group g is `base + g * group_stride` with
// its own row stride, so the [B][G][K] input is read in place, the last stage writes [B][G][N] in place,
// and the weights are read where the flat parameter store keeps them (the blocks are structurally
// identical, hence at a constant stride).
//
//   forward  Y_s[g] = X[g] W_s[g]^T + b_s[g]        up to three weight sets s on one input (a highway
//                                                   layer's nonlinear / linear / gate pre-activations)
//   dgrad    dX[g]  = sum_s dY_s[g] W_s[g]
//   wgrad    dW_s[g] (+)= dY_s[g]^T X[g], db_s[g] (+)= column sums of dY_s[g]     (fp32 outputs)
//
// The model's M is its batch (8 by default): the work of every stage is moving the weights (or their
// gradients), not arithmetic. The bf16 forward is v_mfma_f32_16x16x32_bf16 with both operands straight from global
// memory (W and X are K-contiguous: a lane's 8 k-values are one 16-byte load), one wave per 16 output
// columns, K kept inside the wave, rows beyond M zero-filled by masked loads. dgrad and wgrad contract
// over the ROW index of their K-contiguous operands (n of W [N][K], m of dY / X), where an MFMA
// operand would need transposed 2-byte gathers; they are FMA kernels that move 16-byte pieces with fp32
// accumulation in a fixed order: wgrad writes every gradient once; dgrad reads the weights once per block
// of MB rows (4 bf16 / 8 fp32 rows: twice at M = 8 in bf16, the repeats from L2). fp32 (parity mode) is FMA
// throughout. No atomics, nothing crosses a workgroup: repeat calls are bit-identical.
//
// Highway forward / backward: y = g n + (1 - g) l, n = act(BN(pn)), l = pl, g = sigmoid(pg), BatchNorm
// per (group, channel) over the B rows. One thread owns a channel for all rows of a group (B is small),
// so the statistics are plain two-pass sums in one thread: no cancellation on a large mean, no
// reduction across threads.
#include <stdio.h>

#include "common.h"
#include "fervit_internal.h"

namespace fer {

struct GlinArgs {
  const void* a[3];  // forward: unused; dgrad / wgrad: dY_s
  const void* w[3];  // forward / dgrad: W_s
  const float* b[3];
  void* y[3];        // forward: Y_s; wgrad: dW_s (fp32)
  float* db[3];
  const void* x;     // forward / wgrad: X; dgrad: unused
  void* dx;
  long ldx, gsx, ldw, gsw, gsb, ldy, gsy, lda, gsa;
  int M, N, K, nsets, accumulate;
  unsigned long long skip;
};

// ---------------------------------------------------------------- forward, bf16 MFMA
// grid (ceil(N / 64), sets, G), 4 waves, wave w: output columns n0 = 16 (4 blockIdx.x + w) ... + 15.
// A = W rows n0 + (l & 15), B = X rows m0 + (l & 15), both k = 8 (l >> 4) + j: D[n][m], lane l holds
// n = n0 + 4 (l >> 4) + i (i = 0..3) of row m = m0 + (l & 15): one 8-byte store.
__global__ __launch_bounds__(256) void glin_fwd_mfma_kernel(GlinArgs a) {
  const int lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
  const int n0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 16;
  if (n0 >= a.N) return;
  const int s = blockIdx.y;
  const long g = blockIdx.z;
  const bf16* wp = (const bf16*)a.w[s] + g * a.gsw + (long)(n0 + r) * a.ldw + q * 8;
  const float* bp = a.b[s] ? a.b[s] + g * a.gsb + n0 + 4 * q : nullptr;
  float bv[4] = {0.f, 0.f, 0.f, 0.f};
  if (bp) {
#pragma unroll
    for (int i = 0; i < 4; ++i) bv[i] = bp[i];
  }
  const bf16x8 zero = {};
  for (int m0 = 0; m0 < a.M; m0 += 16) {
    const bool ok = m0 + r < a.M;
    const bf16* xp = (const bf16*)a.x + g * a.gsx + (long)(ok ? m0 + r : 0) * a.ldx + q * 8;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    // four k-steps' operands (8 x 16 bytes per lane) are in flight before the first MFMA of a round
    int k = 0;
    for (; k + 128 <= a.K; k += 128) {
      bf16x8 av[4], xv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        av[u] = *(const bf16x8*)(wp + k + 32 * u);
        xv[u] = *(const bf16x8*)(xp + k + 32 * u);  // a lane beyond M reads row 0 (in bounds) and drops it
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[u], ok ? xv[u] : zero, acc, 0, 0, 0);
    }
    for (; k < a.K; k += 32) {
      const bf16x8 av = *(const bf16x8*)(wp + k);
      const bf16x8 ld = *(const bf16x8*)(xp + k);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, ok ? ld : zero, acc, 0, 0, 0);
    }
    if (ok) {
      bf16* yp = (bf16*)a.y[s] + g * a.gsy + (long)(m0 + r) * a.ldy + n0 + 4 * q;
      *(bf16x4*)yp = bf16x4{(bf16)(acc[0] + bv[0]), (bf16)(acc[1] + bv[1]), (bf16)(acc[2] + bv[2]),
                            (bf16)(acc[3] + bv[3])};
    }
  }
}

// ---------------------------------------------------------------- forward, FMA (fp32 parity mode)
// grid (ceil(N / 4), sets, G): one wave per output column n, lanes striding the K / V pieces of the
// weight row, 8 rows of X at a time against it, wave butterflies.
template <typename T>
__global__ __launch_bounds__(256) void glin_fwd_fma_kernel(GlinArgs a) {
  constexpr int V = Pc<T>::V, MB = 8;
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= a.N) return;
  const int s = blockIdx.y;
  const long g = blockIdx.z;
  const T* wp = (const T*)a.w[s] + g * a.gsw + (long)n * a.ldw;
  const float bv = a.b[s] ? a.b[s][g * a.gsb + n] : 0.f;
  const int pieces = a.K / V;
  for (int m0 = 0; m0 < a.M; m0 += MB) {
    float acc[MB];
#pragma unroll
    for (int i = 0; i < MB; ++i) acc[i] = 0.f;
    for (int p = lane; p < pieces; p += 64) {
      float wv[V];
      loadp(wp + p * V, wv);
#pragma unroll
      for (int i = 0; i < MB; ++i) {
        if (m0 + i < a.M) {
          float xv[V];
          loadp((const T*)a.x + g * a.gsx + (long)(m0 + i) * a.ldx + p * V, xv);
#pragma unroll
          for (int j = 0; j < V; ++j) acc[i] = fmaf(xv[j], wv[j], acc[i]);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < MB; ++i) {
      const float t = wave_sum(acc[i]);
      if (lane == i && m0 + i < a.M) ((T*)a.y[s])[g * a.gsy + (long)(m0 + i) * a.ldy + n] = from_f<T>(t + bv);
    }
  }
}

// ---------------------------------------------------------------- dgrad
// grid (ceil(K / V / 16), ceil(M / MB), G), 256 threads: thread t owns piece t & 15 of the block's 16
// pieces of dX columns for MB rows, over the slice n = (t >> 4), (t >> 4) + 16, ... of every set; the 16
// slices are then added in a fixed order through LDS. MB * V = 32: 32 KB of LDS.
template <typename T>
__global__ __launch_bounds__(256) void glin_dgrad_kernel(GlinArgs a) {
  constexpr int V = Pc<T>::V, MB = 32 / V;
  __shared__ float red[16][MB][16 * V];
  const int pl = threadIdx.x & 15, sl = threadIdx.x >> 4;
  const int piece = blockIdx.x * 16 + pl, pieces = a.K / V;
  const int m0 = blockIdx.y * MB;
  const long g = blockIdx.z;
  float acc[MB][V];
#pragma unroll
  for (int i = 0; i < MB; ++i)
#pragma unroll
    for (int j = 0; j < V; ++j) acc[i][j] = 0.f;
  if (piece < pieces) {
    for (int s = 0; s < a.nsets; ++s) {
      const T* wp = (const T*)a.w[s] + g * a.gsw + piece * V;
      const T* dyp = (const T*)a.a[s] + g * a.gsa + (long)m0 * a.lda;
      for (int n = sl; n < a.N; n += 16) {
        float wv[V];
        loadp(wp + (long)n * a.ldw, wv);
#pragma unroll
        for (int i = 0; i < MB; ++i) {
          const float d = m0 + i < a.M ? to_f<T>(dyp[(long)i * a.lda + n]) : 0.f;
#pragma unroll
          for (int j = 0; j < V; ++j) acc[i][j] = fmaf(d, wv[j], acc[i][j]);
        }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < MB; ++i)
#pragma unroll
    for (int j = 0; j < V; ++j) red[sl][i][pl * V + j] = acc[i][j];
  __syncthreads();
  // MB rows x 16 pieces of V values leave the block: threads 0 .. 16 MB - 1 take one (row, piece) each
  for (int o = threadIdx.x; o < MB * 16; o += 256) {
    const int i = o >> 4, p = o & 15;
    const int pc = blockIdx.x * 16 + p;
    if (m0 + i >= a.M || pc >= pieces) continue;
    float v[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
      float t = 0.f;
#pragma unroll
      for (int k = 0; k < 16; ++k) t += red[k][i][p * V + j];
      v[j] = t;
    }
    storep((T*)a.dx + g * a.gsx + (long)(m0 + i) * a.ldx + pc * V, v);
  }
}

// ---------------------------------------------------------------- wgrad
// One thread per (n, piece of V columns of k): dW[n][k..] (+)= sum_m dY[m][n] X[m][k..] in row order, the
// thread of piece 0 also sums db[n]. grid (ceil(N * K / V / 256), sets, G).
template <typename T>
__global__ __launch_bounds__(256) void glin_wgrad_kernel(GlinArgs a) {
  constexpr int V = Pc<T>::V;
  const long g = blockIdx.z;
  if (g < 64 && ((a.skip >> g) & 1ull)) return;
  const int s = blockIdx.y;
  const int pieces = a.K / V;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  const int n = (int)(idx / pieces), p = (int)(idx - (long)n * pieces);
  if (n >= a.N) return;
  const T* dyp = (const T*)a.a[s] + g * a.gsa + n;
  const T* xp = (const T*)a.x + g * a.gsx + p * V;
  float acc[V], sum = 0.f;
#pragma unroll
  for (int j = 0; j < V; ++j) acc[j] = 0.f;
  for (int m = 0; m < a.M; ++m) {
    const float d = to_f<T>(dyp[(long)m * a.lda]);
    float xv[V];
    loadp(xp + (long)m * a.ldx, xv);
    sum += d;
#pragma unroll
    for (int j = 0; j < V; ++j) acc[j] = fmaf(d, xv[j], acc[j]);
  }
  if (a.y[s]) {
    float* o = (float*)a.y[s] + g * a.gsy + (long)n * a.ldy + p * V;
#pragma unroll
    for (int j = 0; j < V; j += 4) {
      f32x4 t = {acc[j], acc[j + 1], acc[j + 2], acc[j + 3]};
      if (a.accumulate) t += *(const f32x4*)(o + j);
      *(f32x4*)(o + j) = t;
    }
  }
  if (p == 0 && a.db[s]) {
    float* o = a.db[s] + g * a.gsb + n;
    *o = a.accumulate ? *o + sum : sum;
  }
}

// ---------------------------------------------------------------- highway
struct HwArgs {
  const void *pn, *pl, *pg, *dy;
  void *y, *dpn, *dpl, *dpg;
  const float *gamma, *beta;
  float *rmean, *rvar, *mean, *rstd, *dgamma, *dbeta;
  long long* nbt;
  long ldp, gsp, ldy, gsy, lddp, gsdp, gs_par, gs_stat, gs_nbt;
  float momentum, eps;
  int train, act, accumulate, B, C;
  unsigned long long skip;
};

FER_DEV float hw_act(int act, float v) { return v > 0.f ? v : (act == FER_HIGHWAY_LRELU ? 0.2f * v : 0.f); }
FER_DEV float hw_act_grad(int act, float v) { return v > 0.f ? 1.f : (act == FER_HIGHWAY_LRELU ? 0.2f : 0.f); }

// grid (ceil(C / 64), G), 64 threads: thread = channel c of group g, all B rows.
template <typename T>
__global__ __launch_bounds__(64) void highway_fwd_kernel(HwArgs a) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  const long g = blockIdx.y;
  if (c == 0 && a.train && a.nbt) a.nbt[g * a.gs_nbt] += 1;
  if (c >= a.C) return;
  const T* pn = (const T*)a.pn + g * a.gsp + c;
  const T* pl = (const T*)a.pl + g * a.gsp + c;
  const T* pg = (const T*)a.pg + g * a.gsp + c;
  float mean, var;
  if (a.train) {
    float s = 0.f;
    for (int b = 0; b < a.B; ++b) s += to_f<T>(pn[(long)b * a.ldp]);
    mean = s / (float)a.B;
    float s2 = 0.f;
    for (int b = 0; b < a.B; ++b) {
      const float d = to_f<T>(pn[(long)b * a.ldp]) - mean;
      s2 = fmaf(d, d, s2);
    }
    var = s2 / (float)a.B;
    if (a.rmean) {
      float* rm = a.rmean + g * a.gs_stat + c;
      float* rv = a.rvar + g * a.gs_stat + c;
      *rm = (1.f - a.momentum) * *rm + a.momentum * mean;
      *rv = (1.f - a.momentum) * *rv + a.momentum * (s2 / (float)(a.B - 1));
    }
  } else {
    mean = a.rmean[g * a.gs_stat + c];
    var = a.rvar[g * a.gs_stat + c];
  }
  const float rstd = 1.f / sqrtf(var + a.eps);
  if (a.mean) {
    a.mean[g * a.C + c] = mean;
    a.rstd[g * a.C + c] = rstd;
  }
  const float gam = a.gamma[g * a.gs_par + c], bet = a.beta[g * a.gs_par + c];
  T* y = (T*)a.y + g * a.gsy + c;
  for (int b = 0; b < a.B; ++b) {
    const float v = fmaf((to_f<T>(pn[(long)b * a.ldp]) - mean) * rstd, gam, bet);
    const float z = to_f<T>(pg[(long)b * a.ldp]);
    const float gt = 1.f / (1.f + expf(-z)), gc = 1.f / (1.f + expf(z));  // gc = 1 - gt without cancellation
    y[(long)b * a.ldy] = from_f<T>(fmaf(gt, hw_act(a.act, v), gc * to_f<T>(pl[(long)b * a.ldp])));
  }
}

// dg = dy (n - l) g (1 - g), dl = dy (1 - g), dn = dy g through the activation and the BatchNorm adjoint
// (train: dpn = gamma rstd (dv - mean_b dv - xh mean_b (dv xh)); eval: gamma rstd dv).
template <typename T>
__global__ __launch_bounds__(64) void highway_bwd_kernel(HwArgs a) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  const long g = blockIdx.y;
  if (c >= a.C) return;
  const T* pn = (const T*)a.pn + g * a.gsp + c;
  const T* pl = (const T*)a.pl + g * a.gsp + c;
  const T* pg = (const T*)a.pg + g * a.gsp + c;
  const T* dy = (const T*)a.dy + g * a.gsy + c;
  T* dpn = (T*)a.dpn + g * a.gsdp + c;
  T* dpl = (T*)a.dpl + g * a.gsdp + c;
  T* dpg = (T*)a.dpg + g * a.gsdp + c;
  const float mean = a.mean[g * a.C + c], rstd = a.rstd[g * a.C + c];
  const float gam = a.gamma[g * a.gs_par + c], bet = a.beta[g * a.gs_par + c];
  float sb = 0.f, sg = 0.f;
  for (int b = 0; b < a.B; ++b) {
    const float xh = (to_f<T>(pn[(long)b * a.ldp]) - mean) * rstd;
    const float v = fmaf(xh, gam, bet);
    const float z = to_f<T>(pg[(long)b * a.ldp]), l = to_f<T>(pl[(long)b * a.ldp]);
    const float d = to_f<T>(dy[(long)b * a.ldy]);
    const float gt = 1.f / (1.f + expf(-z)), gc = 1.f / (1.f + expf(z));
    const float dv = d * gt * hw_act_grad(a.act, v);
    sb += dv;
    sg = fmaf(dv, xh, sg);
    dpl[(long)b * a.lddp] = from_f<T>(d * gc);
    dpg[(long)b * a.lddp] = from_f<T>(d * (hw_act(a.act, v) - l) * (gt * gc));
  }
  const float mb = a.train ? sb / (float)a.B : 0.f, mg = a.train ? sg / (float)a.B : 0.f;
  for (int b = 0; b < a.B; ++b) {
    const float xh = (to_f<T>(pn[(long)b * a.ldp]) - mean) * rstd;
    const float v = fmaf(xh, gam, bet);
    const float z = to_f<T>(pg[(long)b * a.ldp]);
    const float gt = 1.f / (1.f + expf(-z));
    const float dv = to_f<T>(dy[(long)b * a.ldy]) * gt * hw_act_grad(a.act, v);
    dpn[(long)b * a.lddp] = from_f<T>(gam * rstd * (dv - mb - xh * mg));
  }
  if (g < 64 && ((a.skip >> g) & 1ull)) return;
  if (a.dgamma) {
    float* o = a.dgamma + g * a.gs_par + c;
    *o = a.accumulate ? *o + sg : sg;
  }
  if (a.dbeta) {
    float* o = a.dbeta + g * a.gs_par + c;
    *o = a.accumulate ? *o + sb : sb;
  }
}

}  // namespace fer

using namespace fer;

// ---------------------------------------------------------------- host checks
// An operand of `rows` x `cols` per group, moved in 16-byte pieces: 16-byte aligned base, row and group
// strides multiples of 8 elements, rows at least `cols` long.
static bool glin_operand_ok(const void* p, int64_t ld, int64_t gs, int cols) {
  return p && al16(p) && ld >= cols && ld % 8 == 0 && gs % 8 == 0 && gs >= 0;
}

static int glin_shape(const char* name, int G, int M, int N, int K, char* msg, size_t len) {
  if (N < 1 || K < 1) return snprintf(msg, len, "%s: N and K must be >= 1", name), 1;
  if (K % 32) return snprintf(msg, len, "%s: K must be a multiple of 32 (one MFMA step, whole 16-byte pieces)", name), 1;
  if (N % 16) return snprintf(msg, len, "%s: N must be a multiple of 16 (one MFMA tile of output columns)", name), 1;
  if (G > 65535 || M > 65535 * 4) return snprintf(msg, len, "%s: G or M is above the launch grid's limit", name), 1;
  return 0;
}

// sets are given from 0 upwards: returns their number, 0 when the pattern is broken
static int glin_sets(const void* p0, const void* p1, const void* p2) {
  if (!p0 || (!p1 && p2)) return 0;
  return 1 + (p1 ? 1 : 0) + (p2 ? 1 : 0);
}

extern "C" int fer_grouped_linear_fwd(int dtype, const void* x, int64_t ldx, int64_t gsx, const void* w0,
                                      const void* w1, const void* w2, int64_t ldw, int64_t gsw, const float* b0,
                                      const float* b1, const float* b2, int64_t gsb, void* y0, void* y1, void* y2,
                                      int64_t ldy, int64_t gsy, int G, int M, int N, int K, fer_stream_t stream) {
  if (check_dtype(dtype, "grouped_linear_fwd: unknown dtype")) return -1;
  if (G <= 0 || M <= 0) return 0;
  char msg[160];
  if (glin_shape("grouped_linear_fwd", G, M, N, K, msg, sizeof msg)) return set_error(msg);
  const int ns = glin_sets(w0, w1, w2);
  if (!ns || ns != glin_sets(y0, y1, y2))
    return set_error("grouped_linear_fwd: weight sets and outputs must be given together, from set 0 upwards");
  const void* w[3] = {w0, w1, w2};
  const float* b[3] = {b0, b1, b2};
  void* y[3] = {y0, y1, y2};
  if (!glin_operand_ok(x, ldx, gsx, K)) return set_error("grouped_linear_fwd: x needs 16-byte aligned rows (stride >= K, strides multiples of 8)");
  for (int s = 0; s < ns; ++s) {
    if (!glin_operand_ok(w[s], ldw, gsw, K) || !glin_operand_ok(y[s], ldy, gsy, N))
      return set_error("grouped_linear_fwd: w, y need 16-byte aligned rows (stride >= K / N, strides multiples of 8)");
  }
  GlinArgs a{};
  for (int s = 0; s < ns; ++s) a.w[s] = w[s], a.b[s] = b[s], a.y[s] = y[s];
  a.x = x, a.ldx = ldx, a.gsx = gsx, a.ldw = ldw, a.gsw = gsw, a.gsb = gsb, a.ldy = ldy, a.gsy = gsy;
  a.M = M, a.N = N, a.K = K, a.nsets = ns;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == FER_BF16)
    hipLaunchKernelGGL(glin_fwd_mfma_kernel, dim3(ceil_div(N, 64), ns, G), dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL(glin_fwd_fma_kernel<float>, dim3(ceil_div(N, 4), ns, G), dim3(256), 0, st, a);
  return hip_check("grouped_linear_fwd");
}

extern "C" int fer_grouped_linear_dgrad(int dtype, const void* dy0, const void* dy1, const void* dy2, int64_t lddy,
                                        int64_t gsdy, const void* w0, const void* w1, const void* w2, int64_t ldw,
                                        int64_t gsw, void* dx, int64_t lddx, int64_t gsdx, int G, int M, int N, int K,
                                        fer_stream_t stream) {
  if (check_dtype(dtype, "grouped_linear_dgrad: unknown dtype")) return -1;
  if (G <= 0 || M <= 0) return 0;
  char msg[160];
  if (glin_shape("grouped_linear_dgrad", G, M, N, K, msg, sizeof msg)) return set_error(msg);
  const int ns = glin_sets(w0, w1, w2);
  if (!ns || ns != glin_sets(dy0, dy1, dy2))
    return set_error("grouped_linear_dgrad: weight sets and gradients must be given together, from set 0 upwards");
  const void* w[3] = {w0, w1, w2};
  const void* dy[3] = {dy0, dy1, dy2};
  if (!glin_operand_ok(dx, lddx, gsdx, K)) return set_error("grouped_linear_dgrad: dx needs 16-byte aligned rows (stride >= K, strides multiples of 8)");
  for (int s = 0; s < ns; ++s) {
    if (!glin_operand_ok(w[s], ldw, gsw, K) || !glin_operand_ok(dy[s], lddy, gsdy, N))
      return set_error("grouped_linear_dgrad: w, dy need 16-byte aligned rows (stride >= K / N, strides multiples of 8)");
  }
  GlinArgs a{};
  for (int s = 0; s < ns; ++s) a.w[s] = w[s], a.a[s] = dy[s];
  a.dx = dx, a.ldx = lddx, a.gsx = gsdx, a.ldw = ldw, a.gsw = gsw, a.lda = lddy, a.gsa = gsdy;
  a.M = M, a.N = N, a.K = K, a.nsets = ns;
  hipStream_t st = (hipStream_t)stream;
  with_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    constexpr int V = Pc<T>::V, MB = 32 / V;
    hipLaunchKernelGGL(glin_dgrad_kernel<T>, dim3(ceil_div(K / V, 16), ceil_div(M, MB), G), dim3(256), 0, st, a);
  });
  return hip_check("grouped_linear_dgrad");
}

extern "C" int fer_grouped_linear_wgrad(int dtype, const void* dy0, const void* dy1, const void* dy2, int64_t lddy,
                                        int64_t gsdy, const void* x, int64_t ldx, int64_t gsx, float* dw0, float* dw1,
                                        float* dw2, int64_t lddw, int64_t gsdw, float* db0, float* db1, float* db2,
                                        int64_t gsdb, int accumulate, uint64_t skip_mask, int G, int M, int N, int K,
                                        fer_stream_t stream) {
  if (check_dtype(dtype, "grouped_linear_wgrad: unknown dtype")) return -1;
  if (G <= 0 || M <= 0) return 0;
  char msg[160];
  if (glin_shape("grouped_linear_wgrad", G, M, N, K, msg, sizeof msg)) return set_error(msg);
  const int ns = glin_sets(dy0, dy1, dy2);
  if (!ns) return set_error("grouped_linear_wgrad: gradients must be given from set 0 upwards");
  if (skip_mask && G > 64) return set_error("grouped_linear_wgrad: skip_mask covers at most 64 groups");
  const void* dy[3] = {dy0, dy1, dy2};
  float* dw[3] = {dw0, dw1, dw2};
  float* db[3] = {db0, db1, db2};
  if (!glin_operand_ok(x, ldx, gsx, K)) return set_error("grouped_linear_wgrad: x needs 16-byte aligned rows (stride >= K, strides multiples of 8)");
  bool any = false;
  for (int s = 0; s < ns; ++s) {
    if (!glin_operand_ok(dy[s], lddy, gsdy, N))
      return set_error("grouped_linear_wgrad: dy needs 16-byte aligned rows (stride >= N, strides multiples of 8)");
    if (dw[s] && (!al16(dw[s]) || lddw < K || lddw % 4 || gsdw % 4))
      return set_error("grouped_linear_wgrad: dw needs 16-byte aligned fp32 rows (stride >= K, strides multiples of 4)");
    any = any || dw[s] || db[s];
  }
  for (int s = ns; s < 3; ++s)
    if (dw[s] || db[s]) return set_error("grouped_linear_wgrad: an output without its gradient set");
  if (!any) return set_error("grouped_linear_wgrad: no output requested");
  if (too_many((long)N * (K / piece_len(dtype)))) return set_error("grouped_linear_wgrad: N * K is too large for one launch");
  GlinArgs a{};
  for (int s = 0; s < ns; ++s) a.a[s] = dy[s], a.y[s] = dw[s], a.db[s] = db[s];
  a.x = x, a.ldx = ldx, a.gsx = gsx, a.lda = lddy, a.gsa = gsdy, a.ldy = lddw, a.gsy = gsdw, a.gsb = gsdb;
  a.M = M, a.N = N, a.K = K, a.nsets = ns, a.accumulate = accumulate, a.skip = skip_mask;
  hipStream_t st = (hipStream_t)stream;
  with_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    const long n = (long)N * (K / Pc<T>::V);
    hipLaunchKernelGGL(glin_wgrad_kernel<T>, dim3(blocks_for(n), ns, G), dim3(256), 0, st, a);
  });
  return hip_check("grouped_linear_wgrad");
}

// ---------------------------------------------------------------- highway entry points
static bool hw_operand_ok(const void* p, int64_t ld, int64_t gs, int C) { return p && ld >= C && gs >= 0; }

extern "C" int fer_highway_fwd(int dtype, const void* pn, const void* pl, const void* pg, int64_t ldp, int64_t gsp,
                               const float* gamma, const float* beta, int64_t gs_par, float* running_mean,
                               float* running_var, int64_t gs_stat, int64_t* num_batches_tracked, int64_t gs_nbt,
                               int train, float momentum, float eps, int act, void* y, int64_t ldy, int64_t gsy,
                               float* mean, float* rstd, int G, int B, int C, fer_stream_t stream) {
  if (check_dtype(dtype, "highway_fwd: unknown dtype")) return -1;
  if (G <= 0 || B <= 0 || C <= 0) return 0;
  if (G > 65535) return set_error("highway_fwd: G is above the launch grid's limit");
  if (act != FER_HIGHWAY_LRELU && act != FER_HIGHWAY_RELU) return set_error("highway_fwd: unknown activation");
  if (train && B < 2) return set_error("highway_fwd: training needs more than 1 row per channel");
  if (!train && (!running_mean || !running_var)) return set_error("highway_fwd: eval needs the running statistics");
  if ((running_mean == nullptr) != (running_var == nullptr))
    return set_error("highway_fwd: running_mean and running_var go together");
  if ((mean == nullptr) != (rstd == nullptr)) return set_error("highway_fwd: mean and rstd go together");
  if (!gamma || !beta) return set_error("highway_fwd: gamma and beta are required");
  if (!hw_operand_ok(pn, ldp, gsp, C) || !hw_operand_ok(pl, ldp, gsp, C) || !hw_operand_ok(pg, ldp, gsp, C) ||
      !hw_operand_ok(y, ldy, gsy, C))
    return set_error("highway_fwd: pn, pl, pg, y need rows of stride >= C");
  HwArgs a{};
  a.pn = pn, a.pl = pl, a.pg = pg, a.ldp = ldp, a.gsp = gsp, a.gamma = gamma, a.beta = beta, a.gs_par = gs_par;
  a.rmean = running_mean, a.rvar = running_var, a.gs_stat = gs_stat, a.nbt = (long long*)num_batches_tracked;
  a.gs_nbt = gs_nbt, a.train = train, a.momentum = momentum, a.eps = eps, a.act = act, a.y = y, a.ldy = ldy;
  a.gsy = gsy, a.mean = mean, a.rstd = rstd, a.B = B, a.C = C;
  hipStream_t st = (hipStream_t)stream;
  with_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(highway_fwd_kernel<T>, dim3(ceil_div(C, 64), G), dim3(64), 0, st, a);
  });
  return hip_check("highway_fwd");
}

extern "C" int fer_highway_bwd(int dtype, const void* dy, int64_t lddy, int64_t gsdy, const void* pn, const void* pl,
                               const void* pg, int64_t ldp, int64_t gsp, const float* mean, const float* rstd,
                               const float* gamma, const float* beta, int64_t gs_par, int train, int act, void* dpn,
                               void* dpl, void* dpg, int64_t lddp, int64_t gsdp, float* dgamma, float* dbeta,
                               int accumulate, uint64_t skip_mask, int G, int B, int C, fer_stream_t stream) {
  if (check_dtype(dtype, "highway_bwd: unknown dtype")) return -1;
  if (G <= 0 || B <= 0 || C <= 0) return 0;
  if (G > 65535) return set_error("highway_bwd: G is above the launch grid's limit");
  if (act != FER_HIGHWAY_LRELU && act != FER_HIGHWAY_RELU) return set_error("highway_bwd: unknown activation");
  if (skip_mask && G > 64) return set_error("highway_bwd: skip_mask covers at most 64 groups");
  if (!mean || !rstd || !gamma || !beta) return set_error("highway_bwd: mean, rstd, gamma and beta are required");
  if (!hw_operand_ok(pn, ldp, gsp, C) || !hw_operand_ok(pl, ldp, gsp, C) || !hw_operand_ok(pg, ldp, gsp, C) ||
      !hw_operand_ok(dy, lddy, gsdy, C) || !hw_operand_ok(dpn, lddp, gsdp, C) || !hw_operand_ok(dpl, lddp, gsdp, C) ||
      !hw_operand_ok(dpg, lddp, gsdp, C))
    return set_error("highway_bwd: dy, pn, pl, pg, dpn, dpl, dpg need rows of stride >= C");
  HwArgs a{};
  a.dy = dy, a.ldy = lddy, a.gsy = gsdy, a.pn = pn, a.pl = pl, a.pg = pg, a.ldp = ldp, a.gsp = gsp;
  a.mean = (float*)mean, a.rstd = (float*)rstd, a.gamma = gamma, a.beta = beta, a.gs_par = gs_par, a.train = train;
  a.act = act, a.dpn = dpn, a.dpl = dpl, a.dpg = dpg, a.lddp = lddp, a.gsdp = gsdp, a.dgamma = dgamma;
  a.dbeta = dbeta, a.accumulate = accumulate, a.skip = skip_mask, a.B = B, a.C = C;
  hipStream_t st = (hipStream_t)stream;
  with_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(highway_bwd_kernel<T>, dim3(ceil_div(C, 64), G), dim3(64), 0, st, a);
  });
  return hip_check("highway_bwd");
}
