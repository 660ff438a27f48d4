// Evaluation metrics on the device (reference `eval/evaluate_model.py:135-159, 231-296`: argmax, softmax,
// sklearn's confusion matrix and classification report on the host, torch.cosine_similarity of the final
// tokens; `sefa/verify_directions.py:48-69`: did a shift along a direction change the prediction). Four
// launches, each one kernel, none reads the host or allocates, so all are capturable:
//
//   cls_stats     one wave per row of fp32 logits [B][C]: argmax by torch's CPU rule (lowest index of the
//                 maximum, a NaN counts as the maximum, the first NaN wins), fp32 softmax, confidence, and
//                 one 64-bit atomic add into confusion[label][pred] (integer adds: any order, same bits).
//                 One kernel for every B and C: lanes stride the row, so there is no dispatch threshold.
//   cls_report    one workgroup over confusion [C][C]: integer row / column sums, then fp64 precision,
//                 recall, f1 and support per class, accuracy, macro and weighted f1, in a fixed order.
//   token_cosine  cos(x, y) = x.y / (max(|x|, eps) max(|y|, eps)) of row 0 against rows 1..N-1 (cls_sim) and
//                 of rows 1..N-1 against each other (tok_sim). bf16: the Gram tile is
//                 v_mfma_f32_16x16x32_bf16 with both operands K-contiguous straight from global memory
//                 (the access pattern of grouped.hip glin_fwd_mfma_kernel: token rows are K-contiguous for
//                 both sides of X X^T), rows beyond N zero-filled by masked loads, squared norms summed in
//                 fp32 from the operands already in registers, the division in the epilogue. fp32: FMA, one
//                 wave per (row i, 8 rows j). A row's squared norm is summed by the same procedure on
//                 either side, and an element's arithmetic does not depend on which outputs were asked
//                 for: each output requested alone or both together give the same bits.
//   label_change  one wave per (direction k, sample i): cls_stats' argmax of the sample's base logits and of
//                 its S shifted rows, changed = any step's prediction differs, 64-bit atomic adds into
//                 counts[k] and step_counts[k][s].
#include "common.h"
#include "fervit_internal.h"

namespace fer {

// ---------------------------------------------------------------- cls_stats
struct ClsArgs {
  const float* z;
  const long long* labels;
  long long* preds;
  float* conf;
  float* probs;
  unsigned long long* confusion;
  unsigned long long* counters;
  long ld, ldp;
  int B, C;
};

constexpr int ARG_EMPTY = 0x7FFFFFFF;  // index of a lane that holds no element yet

// (v, i) comes before (bv, bi) in torch.argmax's order: NaN above everything, then the larger value, ties
// to the lower index. A total order, so the butterfly below ends with the same winner in every lane.
FER_DEV bool arg_better(float v, int i, float bv, int bi) {
  if (bi == ARG_EMPTY) return true;
  if (i == ARG_EMPTY) return false;
  const bool an = v != v, bn = bv != bv;
  if (an || bn) return an && (!bn || i < bi);
  return v > bv || (v == bv && i < bi);
}

// grid ceil(B / 4), 256 threads: wave = row.
__global__ __launch_bounds__(256) void cls_stats_kernel(ClsArgs a) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= a.B) return;
  const float* z = a.z + row * a.ld;
  float bv = 0.f;
  int bi = ARG_EMPTY;
  for (int i = lane; i < a.C; i += 64) {
    const float v = z[i];
    if (arg_better(v, i, bv, bi)) bv = v, bi = i;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (arg_better(ov, oi, bv, bi)) bv = ov, bi = oi;
  }
  const float m = bv;
  const int pred = bi;
  if (a.conf || a.probs) {
    // sum_j exp(z_j - m): each lane its elements in index order, then the xor butterfly
    float s = 0.f;
    for (int i = lane; i < a.C; i += 64) s += expf(z[i] - m);
    s = wave_sum(s);
    if (a.probs) {
      float* p = a.probs + row * a.ldp;
      for (int i = lane; i < a.C; i += 64) p[i] = expf(z[i] - m) / s;
    }
    if (lane == 0 && a.conf) a.conf[row] = expf(z[pred] - m) / s;
  }
  if (lane == 0) {
    if (a.preds) a.preds[row] = pred;
    const long long y = a.labels[row];
    const bool ok = y >= 0 && y < a.C;
    if (ok && a.confusion) atomicAdd(a.confusion + y * a.C + pred, 1ull);
    if (a.counters) atomicAdd(a.counters + (ok ? 0 : 1), 1ull);
  }
}

// ---------------------------------------------------------------- cls_report
// One workgroup. Thread t owns classes t, t + 256, ...: integer row and column sums (exact), the class's
// four fp64 figures, and its partial sums; thread 0 then adds the 256 partials in thread order.
__global__ __launch_bounds__(256) void cls_report_kernel(const long long* cm, int C, double* out) {
  __shared__ double s_f1[256], s_f1w[256];
  __shared__ long long s_n[256], s_hit[256];
  __shared__ int s_present[256];
  const int t = threadIdx.x;
  double f1s = 0.0, f1w = 0.0;
  long long n = 0, hit = 0;
  int present = 0;
  for (int c = t; c < C; c += 256) {
    long long rs = 0, cs = 0;
    for (int j = 0; j < C; ++j) {
      rs += cm[(long)c * C + j];
      cs += cm[(long)j * C + c];
    }
    const long long tp = cm[(long)c * C + c];
    const double prec = cs > 0 ? (double)tp / (double)cs : 0.0;
    const double rec = rs > 0 ? (double)tp / (double)rs : 0.0;
    const double f1 = rs + cs > 0 ? 2.0 * (double)tp / (double)(rs + cs) : 0.0;
    double* o = out + 4 + 4 * (long)c;
    o[0] = prec, o[1] = rec, o[2] = f1, o[3] = (double)rs;
    f1s += f1;
    f1w += f1 * (double)rs;
    n += rs;
    hit += tp;
    present += rs + cs > 0 ? 1 : 0;
  }
  s_f1[t] = f1s, s_f1w[t] = f1w, s_n[t] = n, s_hit[t] = hit, s_present[t] = present;
  __syncthreads();
  if (t == 0) {
    for (int k = 1; k < 256; ++k) f1s += s_f1[k], f1w += s_f1w[k], n += s_n[k], hit += s_hit[k], present += s_present[k];
    out[0] = n > 0 ? (double)hit / (double)n : 0.0;
    out[1] = present > 0 ? f1s / (double)present : 0.0;
    out[2] = n > 0 ? f1w / (double)n : 0.0;
    out[3] = (double)n;
  }
}

// ---------------------------------------------------------------- token_cosine
struct CosArgs {
  const void* x;
  float* cls;
  float* tok;
  long ld, ldc, ldt;
  int N, D, i_first;
  float eps;
};

// cos of rows (i, j) into whichever output holds it: i = 0 -> cls_sim[j - 1], i >= 1 -> tok_sim[i - 1][j - 1]
FER_DEV void cos_store(const CosArgs& a, long b, int i, int j, float v) {
  if (i >= a.N || j < 1 || j >= a.N) return;
  if (i == 0) {
    if (a.cls) a.cls[b * a.ldc + (j - 1)] = v;
  } else if (a.tok) {
    a.tok[(b * (a.N - 1) + (i - 1)) * a.ldt + (j - 1)] = v;
  }
}

// sum of the squares of a lane's 8 operand elements, as a fixed pairwise tree
FER_DEV float sumsq8(bf16x8 v) {
  float f[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) f[k] = (float)v[k];
  const float p0 = fmaf(f[1], f[1], f[0] * f[0]), p1 = fmaf(f[3], f[3], f[2] * f[2]);
  const float p2 = fmaf(f[5], f[5], f[4] * f[4]), p3 = fmaf(f[7], f[7], f[6] * f[6]);
  return (p0 + p1) + (p2 + p3);
}

// grid (ceil(ceil(N / 16) / 4), row tiles, B), 4 waves, wave w: the 16 x 16 Gram tile of rows
// i0 = 16 blockIdx.y against rows j0 = 16 (4 blockIdx.x + w). A = rows i0 + (l & 15), B = rows j0 + (l & 15),
// both k = 8 (l >> 4) + e: lane l holds G[i0 + 4 (l >> 4) + reg][j0 + (l & 15)], reg = 0..3. Four
// accumulators take the k-steps round robin (short dependent chains), added pairwise at the end. A lane's
// squared-norm share is summed over its k-steps in order, then over the four lanes of a row (xor 16, 32).
__global__ __launch_bounds__(256) void token_cosine_mfma_kernel(CosArgs a) {
  const int lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
  const int j0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 16;
  if (j0 >= a.N) return;
  const int i0 = blockIdx.y * 16;
  const long b = blockIdx.z;
  const bf16* xb = (const bf16*)a.x + b * a.N * a.ld;
  const bool oki = i0 + r < a.N, okj = j0 + r < a.N;
  // a lane beyond N reads row 0 (in bounds) and drops it
  const bf16* ap = xb + (long)(oki ? i0 + r : 0) * a.ld + q * 8;
  const bf16* bp = xb + (long)(okj ? j0 + r : 0) * a.ld + q * 8;
  const bf16x8 zero = {};
  f32x4 acc[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
  float na = 0.f, nb = 0.f;
  int k = 0;
  for (; k + 128 <= a.D; k += 128) {
    bf16x8 av[4], bv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      av[u] = *(const bf16x8*)(ap + k + 32 * u);
      bv[u] = *(const bf16x8*)(bp + k + 32 * u);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const bf16x8 x = oki ? av[u] : zero, y = okj ? bv[u] : zero;
      acc[u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(x, y, acc[u], 0, 0, 0);
      na += sumsq8(x);
      nb += sumsq8(y);
    }
  }
#pragma unroll
  for (int u = 0; u < 3; ++u) {
    if (k + 32 * u < a.D) {
      const bf16x8 ld_a = *(const bf16x8*)(ap + k + 32 * u), ld_b = *(const bf16x8*)(bp + k + 32 * u);
      const bf16x8 x = oki ? ld_a : zero, y = okj ? ld_b : zero;
      acc[u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(x, y, acc[u], 0, 0, 0);
      na += sumsq8(x);
      nb += sumsq8(y);
    }
  }
  na += __shfl_xor(na, 16, 64);
  na += __shfl_xor(na, 32, 64);
  nb += __shfl_xor(nb, 16, 64);
  nb += __shfl_xor(nb, 32, 64);
  const float da = fmaxf(sqrtf(na), a.eps), db = fmaxf(sqrtf(nb), a.eps);
  const f32x4 g = (acc[0] + acc[1]) + (acc[2] + acc[3]);
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const float dai = __shfl(da, 4 * q + reg, 64);  // the lane whose row (l & 15) is this element's row
    cos_store(a, b, i0 + 4 * q + reg, j0 + r, g[reg] / (dai * db));
  }
}

// grid (ceil(N / 32), rows i, B), 4 waves, wave w: row i = i_first + blockIdx.y against the 8 rows from
// j0 = 8 (4 blockIdx.x + w); lanes stride the 16-byte pieces of the rows, wave butterflies.
__global__ __launch_bounds__(256) void token_cosine_fma_kernel(CosArgs a) {
  constexpr int JB = 8;
  const int lane = threadIdx.x & 63;
  const int j0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * JB;
  if (j0 >= a.N) return;
  const int i = a.i_first + blockIdx.y;
  const long b = blockIdx.z;
  const float* xb = (const float*)a.x + b * a.N * a.ld;
  const float* xi = xb + (long)i * a.ld;
  float dot[JB], nb[JB], na = 0.f;
#pragma unroll
  for (int jj = 0; jj < JB; ++jj) dot[jj] = 0.f, nb[jj] = 0.f;
  const int pieces = a.D / 4;
  for (int p = lane; p < pieces; p += 64) {
    const f32x4 xv = *(const f32x4*)(xi + 4 * p);
#pragma unroll
    for (int e = 0; e < 4; ++e) na = fmaf(xv[e], xv[e], na);
#pragma unroll
    for (int jj = 0; jj < JB; ++jj) {
      if (j0 + jj < a.N) {
        const f32x4 yv = *(const f32x4*)(xb + (long)(j0 + jj) * a.ld + 4 * p);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          dot[jj] = fmaf(xv[e], yv[e], dot[jj]);
          nb[jj] = fmaf(yv[e], yv[e], nb[jj]);
        }
      }
    }
  }
  const float da = fmaxf(sqrtf(wave_sum(na)), a.eps);
#pragma unroll
  for (int jj = 0; jj < JB; ++jj) {
    const float d = wave_sum(dot[jj]);
    const float db = fmaxf(sqrtf(wave_sum(nb[jj])), a.eps);
    if (lane == jj) cos_store(a, b, i, j0 + jj, d / (da * db));
  }
}

// ---------------------------------------------------------------- label_change
// `sefa/verify_directions.py:48-69` on logits already computed: does any of the S shifted copies of sample i
// along direction k change the model's prediction? shifted holds the rows in fer_latent_shift's grid order,
// row (k*S + s)*n + i.
struct LabelChangeArgs {
  const float* base;
  const float* shifted;
  long long* preds;
  unsigned char* changed;
  unsigned long long* counts;
  unsigned long long* step_counts;
  long ldb, lds;
  int K, S, n, C;
};

// argmax of one row by the whole wave (cls_stats' rule and reduction): the same index in every lane
FER_DEV int wave_argmax(const float* z, int C, int lane) {
  float bv = 0.f;
  int bi = ARG_EMPTY;
  for (int i = lane; i < C; i += 64) {
    const float v = z[i];
    if (arg_better(v, i, bv, bi)) bv = v, bi = i;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (arg_better(ov, oi, bv, bi)) bv = ov, bi = oi;
  }
  return bi;
}

// grid ceil(K*n / 4), 256 threads: wave = (k, i).
__global__ __launch_bounds__(256) void label_change_kernel(LabelChangeArgs a) {
  const int lane = threadIdx.x & 63;
  const long w = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= (long)a.K * a.n) return;
  const int k = (int)(w / a.n), i = (int)(w - (long)k * a.n);
  const int base = wave_argmax(a.base + (long)i * a.ldb, a.C, lane);
  bool any = false;
  for (int s = 0; s < a.S; ++s) {
    const long ks = (long)k * a.S + s;
    const int pred = wave_argmax(a.shifted + (ks * a.n + i) * a.lds, a.C, lane);
    if (lane == 0) {
      if (a.preds) a.preds[ks * a.n + i] = pred;
      if (pred != base && a.step_counts) atomicAdd(a.step_counts + ks, 1ull);
    }
    any |= pred != base;
  }
  if (lane == 0) {
    if (a.changed) a.changed[w] = any ? 1 : 0;
    if (any) atomicAdd(a.counts + k, 1ull);
  }
}

}  // namespace fer

using namespace fer;

// ---------------------------------------------------------------- entry points
extern "C" int fer_cls_stats(const float* logits, int64_t ld, const int64_t* labels, int B, int C, int64_t* preds,
                             float* conf, float* probs, int64_t ld_probs, int64_t* confusion, int64_t* counters,
                             fer_stream_t stream) {
  if (C < 1) return set_error("cls_stats: C must be >= 1");
  if (!logits || !labels) return set_error("cls_stats: logits and labels are required");
  if (ld < C) return set_error("cls_stats: the logits' row stride must be >= C");
  if (probs && ld_probs < C) return set_error("cls_stats: the probabilities' row stride must be >= C");
  if (B <= 0) return 0;
  if (too_many((long)B * 64)) return set_error("cls_stats: B is too large for one launch");
  ClsArgs a{};
  a.z = logits, a.ld = ld, a.labels = (const long long*)labels, a.B = B, a.C = C, a.preds = (long long*)preds;
  a.conf = conf, a.probs = probs, a.ldp = ld_probs, a.confusion = (unsigned long long*)confusion;
  a.counters = (unsigned long long*)counters;
  hipLaunchKernelGGL(cls_stats_kernel, dim3(ceil_div(B, 4)), dim3(256), 0, (hipStream_t)stream, a);
  return hip_check("cls_stats");
}

extern "C" int fer_cls_report(const int64_t* confusion, int C, double* out, fer_stream_t stream) {
  if (C < 1) return set_error("cls_report: C must be >= 1");
  if (!confusion || !out) return set_error("cls_report: confusion and out are required");
  hipLaunchKernelGGL(cls_report_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const long long*)confusion, C, out);
  return hip_check("cls_report");
}

extern "C" int fer_token_cosine(int dtype, const void* tokens, int64_t ld, int B, int N, int D, float eps,
                                float* cls_sim, int64_t ld_cls, float* tok_sim, int64_t ld_tok, fer_stream_t stream) {
  if (check_dtype(dtype, "token_cosine: unknown dtype")) return -1;
  if (N < 2) return set_error("token_cosine: N must be >= 2 (row 0 and at least one more token)");
  const int V = piece_len(dtype);
  if (D < 1 || D % (dtype == FER_BF16 ? 32 : 4))
    return set_error("token_cosine: D must be a positive multiple of 32 (bf16: one MFMA step) or 4 (fp32)");
  if (!piece_ok(tokens, ld, D, V))
    return set_error("token_cosine: tokens need 16-byte aligned rows (stride >= D, a multiple of 8 bf16 / 4 fp32)");
  if (!cls_sim && !tok_sim) return set_error("token_cosine: no output requested");
  if ((cls_sim && ld_cls < N - 1) || (tok_sim && ld_tok < N - 1))
    return set_error("token_cosine: an output's row stride must be >= N - 1");
  if (!(eps >= 0.f)) return set_error("token_cosine: eps must be >= 0");
  if (B <= 0) return 0;
  if (B > 65535 || N > 65535) return set_error("token_cosine: B or N is above the launch grid's limit");
  hipStream_t st = (hipStream_t)stream;
  CosArgs a{};
  a.x = tokens, a.ld = ld, a.N = N, a.D = D, a.eps = eps, a.cls = cls_sim, a.ldc = ld_cls, a.tok = tok_sim;
  a.ldt = ld_tok;
  if (dtype == FER_BF16) {
    const int tiles = ceil_div(N, 16);
    // cls_sim alone lives in the first row tile
    hipLaunchKernelGGL(token_cosine_mfma_kernel, dim3(ceil_div(tiles, 4), tok_sim ? tiles : 1, B), dim3(256), 0, st, a);
  } else {
    a.i_first = cls_sim ? 0 : 1;
    const int rows = tok_sim ? N - a.i_first : 1;
    hipLaunchKernelGGL(token_cosine_fma_kernel, dim3(ceil_div(N, 32), rows, B), dim3(256), 0, st, a);
  }
  return hip_check("token_cosine");
}

extern "C" int fer_label_change(const float* base, int64_t ld_base, const float* shifted, int64_t ld_shifted, int K,
                                int S, int n, int C, int64_t* preds, uint8_t* changed, int64_t* counts,
                                int64_t* step_counts, fer_stream_t stream) {
  if (K < 1 || S < 1) return set_error("label_change: K and S must be >= 1");
  if (C < 1) return set_error("label_change: C must be >= 1");
  if (!base || !shifted || !counts) return set_error("label_change: base, shifted and counts are required");
  if (ld_base < C || ld_shifted < C) return set_error("label_change: a row stride must be >= C");
  if (n <= 0) return 0;
  if ((long)K * S * n > 0x7FFFFFFFL) return set_error("label_change: K * S * n is too large for one launch");
  LabelChangeArgs a{};
  a.base = base, a.ldb = ld_base, a.shifted = shifted, a.lds = ld_shifted, a.K = K, a.S = S, a.n = n, a.C = C;
  a.preds = (long long*)preds, a.changed = changed, a.counts = (unsigned long long*)counts;
  a.step_counts = (unsigned long long*)step_counts;
  hipLaunchKernelGGL(label_change_kernel, dim3(ceil_div((long)K * n, 4)), dim3(256), 0, (hipStream_t)stream, a);
  return hip_check("label_change");
}
