// Attention maps: the softmax probabilities the fused attention forward never materialises
// (fer_attention_probs), and the CLS row of the attention rollout over layers
// (fer_attention_rollout_cls). Eval semantics: no dropout, fp32 output.
//
// fer_attention_probs, bf16: one workgroup per (batch element, block of 32 x waves selected query
// rows), four waves, wave w = 32 queries (a wave without a tile, e.g. three of four when only the
// CLS row is asked for, does no MFMA work and only helps to stage the keys). Keys stream through LDS in chunks of 128 rows as
// swizzled [rows][64 col] images (the layout of attention.hip's generic kernels). No O(N^2)
// workspace: Q K^T is computed twice.
//   pass 1 (per head): S^T = K Q^T -- lane = query, the 16 accumulator registers = keys -- so the
//     running max / sum of a query is lane-local plus one 32-lane swap; (max, 1 / sum) of every
//     (head, query) goes to a small LDS table.
//   pass 2 (per key chunk, heads inside): S = Q K^T -- lane = key, registers = queries -- so one
//     store instruction writes 32 consecutive keys (128 B) of a query row. Per head the tile is
//     stored at once; head-averaged it is summed in registers over heads 0..H-1 (fixed order, one
//     workgroup, no atomics) and stored once per chunk: the per-head tensor never exists.
// A probability depends only on its own query's scores and the key blocking, never on where the
// query sits in a tile: a row-selected call returns the bits of the full call's rows.
//
// fp32 (parity path): one workgroup per (batch, query row), plain FMA, scores recomputed for the
// max, the sum and the final value.
//
// fer_attention_rollout_cls: one workgroup per batch element, r double-buffered in LDS; thread
// (g, k) sums r[q] * A[q][k] over the g-th contiguous slice of q (reads of A coalesced along k),
// the slices are combined in slice order.
#include "common.h"
#include "fervit_internal.h"

namespace fer {
namespace {

constexpr float LOG2E = 1.4426950408889634f;
constexpr int PR_ROWS = 128;            // keys per LDS chunk
constexpr int PR_IMG = PR_ROWS * 128;   // one 64-column half of a chunk
constexpr int PR_LDS_MAX = 64 * 1024;   // dynamic LDS without an opt-in attribute

FER_DEV int swz(int r) { return (((r >> 1) & 1) << 2) | ((r >> 2) & 3); }
FER_DEV int img_off(int r, int c) { return r * 128 + ((c ^ swz(r)) << 4); }
FER_DEV bf16x8 rd_row(const char* img, int r, int c) { return *(const bf16x8*)(img + img_off(r, c)); }
FER_DEV f32x16 mfma32(bf16x8 a, bf16x8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
// accumulator register -> row within the 32-row tile
FER_DEV int acc_row(int reg, int hh) { return (reg & 3) + 8 * (reg >> 2) + 4 * hh; }
FER_DEV float ex2(float x) { return __builtin_amdgcn_exp2f(x); }

// Key rows [0, 32 * nkb) of one head's K column block (src = its first row, row stride ld) -> DH2
// images; rows >= nrows and columns >= dh are zero.
template <int DH2>
FER_DEV void load_keys(char* img, const bf16* src, long ld, int nrows, int dh, int nkb) {
#pragma unroll
  for (int hf = 0; hf < DH2; ++hf)
    for (int idx = threadIdx.x; idx < nkb * 32 * 8; idx += blockDim.x) {
      const int r = idx >> 3, c = idx & 7, d0 = hf * 64 + c * 8;
      bf16x8 v = {};
      if (r < nrows && d0 < dh) v = *(const bf16x8*)(src + (long)r * ld + d0);
      *(bf16x8*)(img + hf * PR_IMG + img_off(r, c)) = v;
    }
}

template <int DH2>
FER_DEV void load_q(bf16x8 (&qf)[4 * DH2], const bf16* qrow, bool qv, int dh, int hh) {
#pragma unroll
  for (int s = 0; s < 4 * DH2; ++s) {
    const int d0 = 16 * s + 8 * hh;
    qf[s] = (qv && d0 < dh) ? *(const bf16x8*)(qrow + d0) : bf16x8{};
  }
}

template <int DH2>
__global__ __launch_bounds__(256) void attn_probs_bf16(const bf16* __restrict__ qkv, long ldq,
                                                       float* __restrict__ probs, int N, int H, int dh, float sl2,
                                                       int head_avg, int q0, int nq, int qw) {
  extern __shared__ __attribute__((aligned(1024))) char lds[];
  char* Ki = lds;
  float2* ml = (float2*)(lds + DH2 * PR_IMG);  // [H][QR]: (max in the exp2 domain, 1 / sum)
  const int QR = qw * 32;  // query rows of this workgroup: waves 0 .. qw-1 hold a tile, the rest only load keys
  const int b = blockIdx.x, D = H * dh;
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), hh = lane >> 5;
  const bool act = w < qw;
  const int qb = blockIdx.y * QR + w * 32;  // first selected row of this wave's tile
  const int qi = qb + (lane & 31);
  const bool qv = act && qi < nq;
  const bf16* base = qkv + (long)b * N * ldq;
  const bf16* qrow = base + (long)(q0 + (qv ? qi : 0)) * ldq;
  bf16x8 qf[4 * DH2];

  // ---- pass 1: (max, 1 / sum) per (head, query)
#pragma unroll 1
  for (int h = 0; h < H; ++h) {
    load_q<DH2>(qf, qrow + h * dh, qv, dh, hh);
    float m = -INFINITY, l = 0.f;
#pragma unroll 1
    for (int c0 = 0; c0 < N; c0 += PR_ROWS) {
      const int nkb = min(PR_ROWS / 32, (N - c0 + 31) / 32);
      __syncthreads();  // every wave is done with the previous image
      load_keys<DH2>(Ki, base + (long)c0 * ldq + D + h * dh, ldq, N - c0, dh, nkb);
      __syncthreads();
#pragma unroll 1
      for (int kb = 0; act && kb < nkb; ++kb) {
        f32x16 st = {};
#pragma unroll
        for (int hf = 0; hf < DH2; ++hf)
#pragma unroll
          for (int s = 0; s < 4; ++s)
            st = mfma32(rd_row(Ki + hf * PR_IMG, kb * 32 + (lane & 31), 2 * s + hh), qf[4 * hf + s], st);
        const int k0 = c0 + kb * 32;
        float bm = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (k0 + acc_row(r, hh) < N) bm = fmaxf(bm, st[r] * sl2);
        bm = xhalf_max(bm);  // key 0 of every block is a real key: bm is finite
        const float mn = fmaxf(m, bm);
        l *= ex2(m - mn);
        m = mn;
        // the exponent exactly as pass 2 forms it; padding keys contribute exactly zero
#pragma unroll
        for (int r = 0; r < 16; ++r) l += (k0 + acc_row(r, hh) < N) ? ex2(fmaf(st[r], sl2, -mn)) : 0.f;
      }
    }
    l = xhalf_sum(l);
    if (act && hh == 0) ml[h * QR + w * 32 + (lane & 31)] = float2{m, 1.f / l};
  }

  // ---- pass 2: normalise and store (or sum over heads, then store)
  const float inv_h = 1.f / (float)H;
#pragma unroll 1
  for (int c0 = 0; c0 < N; c0 += PR_ROWS) {
    const int nkb = min(PR_ROWS / 32, (N - c0 + 31) / 32);
    f32x16 acc[PR_ROWS / 32];
#pragma unroll
    for (int kb = 0; kb < PR_ROWS / 32; ++kb) acc[kb] = f32x16{};
#pragma unroll 1
    for (int h = 0; h < H; ++h) {
      load_q<DH2>(qf, qrow + h * dh, qv, dh, hh);
      __syncthreads();
      load_keys<DH2>(Ki, base + (long)c0 * ldq + D + h * dh, ldq, N - c0, dh, nkb);
      __syncthreads();  // (also orders pass 1's table writes before the reads below)
      if (!act) continue;
      float mr[16], ir[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float2 t = ml[h * QR + w * 32 + acc_row(r, hh)];
        mr[r] = t.x;
        ir[r] = t.y;
      }
#pragma unroll
      for (int kb = 0; kb < PR_ROWS / 32; ++kb) {
        if (kb < nkb) {
          f32x16 st = {};
#pragma unroll
          for (int hf = 0; hf < DH2; ++hf)
#pragma unroll
            for (int s = 0; s < 4; ++s)
              st = mfma32(qf[4 * hf + s], rd_row(Ki + hf * PR_IMG, kb * 32 + (lane & 31), 2 * s + hh), st);
#pragma unroll
          for (int r = 0; r < 16; ++r) st[r] = ex2(fmaf(st[r], sl2, -mr[r])) * ir[r];
          if (head_avg) {
            acc[kb] += st;
          } else {
            const int k = c0 + kb * 32 + (lane & 31);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const int row = qb + acc_row(r, hh);
              if (row < nq && k < N) probs[(((long)b * H + h) * nq + row) * N + k] = st[r];
            }
          }
        }
      }
    }
    if (head_avg && act) {
#pragma unroll
      for (int kb = 0; kb < PR_ROWS / 32; ++kb) {
        if (kb < nkb) {
          const int k = c0 + kb * 32 + (lane & 31);
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int row = qb + acc_row(r, hh);
            if (row < nq && k < N) probs[((long)b * nq + row) * N + k] = acc[kb][r] * inv_h;
          }
        }
      }
    }
  }
}

// Fixed-order tree over the 256 threads' values (red: 256 floats of LDS); every thread gets the result.
template <bool MAX>
FER_DEV float block_reduce256(float v, float* red) {
  __syncthreads();  // earlier readers of red are done
  red[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      const float a = red[threadIdx.x], c = red[threadIdx.x + o];
      red[threadIdx.x] = MAX ? fmaxf(a, c) : a + c;
    }
    __syncthreads();
  }
  return red[0];
}

FER_DEV float dot_f32(const float* a, const float* b, int n) {
  float s = 0.f;
  for (int d = 0; d < n; ++d) s = fmaf(a[d], b[d], s);
  return s;
}

// fp32 parity path: workgroup = (batch, selected query row), thread t owns keys t, t + 256, ...
__global__ __launch_bounds__(256) void attn_probs_f32(const float* __restrict__ qkv, long ldq, float* __restrict__ probs,
                                                      int N, int H, int dh, float scale, int head_avg, int q0, int nq) {
  extern __shared__ float smem[];
  float* red = smem;        // [256]
  float* mh = smem + 256;   // [H] row max
  float* lh = mh + H;       // [H] row sum
  const int b = blockIdx.x / nq, qi = blockIdx.x - b * nq, D = H * dh;
  const float* base = qkv + (long)b * N * ldq;
  const float* qr = base + (long)(q0 + qi) * ldq;
  for (int h = 0; h < H; ++h) {
    const float* kc = base + D + h * dh;
    float m = -INFINITY;
    for (int k = threadIdx.x; k < N; k += 256) m = fmaxf(m, dot_f32(qr + h * dh, kc + (long)k * ldq, dh) * scale);
    m = block_reduce256<true>(m, red);
    float l = 0.f;
    for (int k = threadIdx.x; k < N; k += 256) l += expf(dot_f32(qr + h * dh, kc + (long)k * ldq, dh) * scale - m);
    l = block_reduce256<false>(l, red);
    if (threadIdx.x == 0) {
      mh[h] = m;
      lh[h] = l;
    }
  }
  __syncthreads();
  const float inv_h = 1.f / (float)H;
  for (int k = threadIdx.x; k < N; k += 256) {
    float acc = 0.f;
    for (int h = 0; h < H; ++h) {
      const float p = expf(dot_f32(qr + h * dh, base + (long)k * ldq + D + h * dh, dh) * scale - mh[h]) / lh[h];
      if (head_avg)
        acc += p;
      else
        probs[(((long)b * H + h) * nq + qi) * N + k] = p;
    }
    if (head_avg) probs[((long)b * nq + qi) * N + k] = acc * inv_h;
  }
}

// CLS row of the rollout. LDS: r ping / pong [2][N], slice partials [1024].
constexpr int RO_THREADS = 1024;
__global__ __launch_bounds__(RO_THREADS) void rollout_cls_kernel(const float* __restrict__ maps, int L, int B, int N,
                                                                 float residual, float* __restrict__ out) {
  extern __shared__ float smem[];
  float* rbuf = smem;            // [2][N]
  float* part = smem + 2 * (long)N;  // [G][KT]
  const int b = blockIdx.x, t = threadIdx.x;
  const int KT = min(RO_THREADS, (N + 63) / 64 * 64);  // key columns per sweep
  const int G = RO_THREADS / KT;                       // q slices summed side by side
  const int g = t / KT, kk = t - g * KT;
  const int qs = (N + G - 1) / G;  // slice length
  const int qlo = min(N, g * qs), qhi = min(N, qlo + qs);
  for (int k = t; k < N; k += RO_THREADS) rbuf[k] = k == 0 ? 1.f : 0.f;
  __syncthreads();
  int cur = 0;
  const float keep = 1.f - residual;
  for (int l = L - 1; l >= 0; --l) {
    const float* A = maps + ((long)l * B + b) * N * N;
    const float* r = rbuf + (long)cur * N;
    float* rn = rbuf + (long)(cur ^ 1) * N;
    for (int k0 = 0; k0 < N; k0 += KT) {
      const int k = k0 + kk;
      float s = 0.f;
      if (g < G && k < N)
        for (int q = qlo; q < qhi; ++q) s = fmaf(r[q], A[(long)q * N + k], s);
      if (g < G) part[g * KT + kk] = s;
      __syncthreads();
      if (g == 0 && k < N) {
        float tot = part[kk];
        for (int j = 1; j < G; ++j) tot += part[j * KT + kk];
        rn[k] = residual * r[k] + keep * tot;
      }
      __syncthreads();
    }
    cur ^= 1;
  }
  for (int k = t; k < N; k += RO_THREADS) out[(long)b * N + k] = rbuf[(long)cur * N + k];
}

}  // namespace
}  // namespace fer

using namespace fer;

extern "C" int fer_attention_probs(int dtype, const void* qkv, int64_t ld_qkv, int B, int N, int H, int dh, float scale,
                                   int head_avg, int q0, int nq, float* probs, int64_t probs_floats,
                                   fer_stream_t stream) {
  if (check_dtype(dtype, "attention_probs: unknown dtype")) return -1;
  hipStream_t st = (hipStream_t)stream;
  if (B < 0 || N < 1 || H < 1 || dh < 1) return set_error("attention_probs: needs B >= 0, N >= 1, H >= 1, dh >= 1");
  if (q0 < 0 || nq < 1 || (int64_t)q0 + nq > N) return set_error("attention_probs: query rows q0 .. q0+nq-1 outside [0, N)");
  if (!qkv || !probs) return set_error("attention_probs: null pointer");
  if (ld_qkv < (int64_t)3 * H * dh) return set_error("attention_probs: ld_qkv smaller than 3*H*dh");
  const int64_t need = (int64_t)B * (head_avg ? 1 : H) * nq * N;
  if (probs_floats < need) return set_error("attention_probs: probs buffer smaller than B*(H)*nq*N floats");
  if (B == 0) return 0;
  if (dtype == FER_F32) {
    const size_t lds = (size_t)(256 + 2 * (int64_t)H) * 4;
    if (lds > (size_t)PR_LDS_MAX) return set_error("attention_probs(fp32): too many heads");
    if ((int64_t)B * nq > 0x7FFFFFFFL) return set_error("attention_probs(fp32): B*nq exceeds the grid limit");
    hipLaunchKernelGGL(attn_probs_f32, dim3((unsigned)((int64_t)B * nq)), dim3(256), lds, st, (const float*)qkv,
                       (long)ld_qkv, probs, N, H, dh, scale, head_avg ? 1 : 0, q0, nq);
    return hip_check("attention_probs_f32");
  }
  if (dh > 128 || dh % 8) return set_error("attention_probs(bf16): needs dh <= 128, dh % 8 == 0");
  if (ld_qkv % 8 || ((uintptr_t)qkv & 15)) return set_error("attention_probs(bf16): misaligned qkv or leading dimension");
  const int dh2 = dh <= 64 ? 1 : 2;
  // tile waves: nq = 1 (CLS only) computes one tile per head and key block; the workgroup still has four
  // waves, the others only help to stage the keys
  int waves = std::min(4, (nq + 31) / 32);
  while (waves > 1 && (size_t)dh2 * PR_IMG + (size_t)H * waves * 32 * 8 > (size_t)PR_LDS_MAX) waves >>= 1;
  const size_t lds = (size_t)dh2 * PR_IMG + (size_t)H * waves * 32 * 8;
  if (lds > (size_t)PR_LDS_MAX) return set_error("attention_probs(bf16): too many heads");
  const int64_t qblocks = ((int64_t)nq + waves * 32 - 1) / (waves * 32);
  if (qblocks > 65535) return set_error("attention_probs(bf16): more than 65535 query blocks");
  const dim3 grid((unsigned)B, (unsigned)qblocks);
  const float sl2 = scale * LOG2E;
  if (dh2 == 1)
    hipLaunchKernelGGL(attn_probs_bf16<1>, grid, dim3(256), lds, st, (const bf16*)qkv, (long)ld_qkv, probs, N, H,
                       dh, sl2, head_avg ? 1 : 0, q0, nq, waves);
  else
    hipLaunchKernelGGL(attn_probs_bf16<2>, grid, dim3(256), lds, st, (const bf16*)qkv, (long)ld_qkv, probs, N, H,
                       dh, sl2, head_avg ? 1 : 0, q0, nq, waves);
  return hip_check("attention_probs_bf16");
}

extern "C" int fer_attention_rollout_cls(const float* maps, int L, int B, int N, float residual, float* r,
                                         fer_stream_t stream) {
  if (L < 1 || N < 1 || B < 0) return set_error("attention_rollout_cls: needs L >= 1, N >= 1, B >= 0");
  if (!(residual >= 0.f && residual < 1.f)) return set_error("attention_rollout_cls: residual must be in [0, 1)");
  if (!maps || !r) return set_error("attention_rollout_cls: null pointer");
  const size_t lds = ((size_t)2 * N + RO_THREADS) * 4;
  if (lds > (size_t)PR_LDS_MAX) return set_error("attention_rollout_cls: N too large for the LDS row buffers");
  if (B == 0) return 0;
  hipLaunchKernelGGL(rollout_cls_kernel, dim3((unsigned)B), dim3(RO_THREADS), lds, (hipStream_t)stream, maps, L, B, N,
                     residual, r);
  return hip_check("attention_rollout_cls");
}
