// Mixup on the device (`train/train_latent_vit_v2.py:118-130`: lam ~ Beta(a, a), a batch permutation, the mixed
// batch and the two-target loss), so that a captured training step draws afresh on every replay: the draw kernel
// mixes the device step counter into its seed (step_seed.h), and the mixing and loss kernels read lam and the
// permutation from device memory. DESIGN.md section 2.14; host mirror of the draw: tests/mixup_ref.py.
#include "common.h"
#include "fervit_internal.h"
#include "step_seed.h"

namespace fer {

constexpr int MIXUP_MAX_B = 2048;
// Marsaglia-Tsang attempts per Gamma draw. One attempt accepts with probability >= 0.95 for every shape >= 1
// (Marsaglia & Tsang 2000, section 6: 0.9516 at shape 1, rising with the shape), and a shape below 1 is drawn at
// shape + 1, so all 16 attempts of one draw fail with probability <= 0.05^16 = 1.6e-21; a lam takes two draws:
// <= 3.1e-21 per launch, below 1e-18 (even at a rejection rate of 0.07: 2 * 0.07^16 = 6.7e-19). A draw that
// does exhaust them takes d = shape - 1/3, the value the proposal gives at x = 0 (the bulk of the density).
constexpr int MIXUP_ATTEMPTS = 16;
// streams of one set's seed: the permutation keys and the two Gamma draws
constexpr uint64_t MIXUP_PERM_XOR = 0x2545F4914F6CDD1Dull;
constexpr uint64_t MIXUP_GAMMA1_XOR = 0x9FB21C651E98DF25ull, MIXUP_GAMMA2_XOR = 0xD6E8FEB86659FD93ull;

// (0, 1]: ((float)(h >> 8) + 0.5f) * 2^-24, as wplus.hip's u01
FER_DEV float mixup_u01(uint32_t h) { return ((float)(h >> 8) + 0.5f) * (1.0f / 16777216.0f); }

// log of a Gamma(alpha, 1) draw, alpha > 0. Attempt t takes the uniforms 3t, 3t+1 (Box-Muller normal) and 3t+2
// (the acceptance test) of the stream; a shape below 1 is Gamma(alpha + 1) * U^(1/alpha) with uniform
// 3 * MIXUP_ATTEMPTS, applied in the log so that a tiny alpha cannot underflow to 0 / 0.
FER_DEV float mixup_log_gamma(float alpha, uint64_t seed) {
  const float a = alpha < 1.f ? alpha + 1.f : alpha;
  const float d = a - 1.f / 3.f, c = 1.f / sqrtf(9.f * d);
  float g = d;
  for (int t = 0; t < MIXUP_ATTEMPTS; ++t) {
    const float u1 = mixup_u01(fer_hash(seed, 3u * t)), u2 = mixup_u01(fer_hash(seed, 3u * t + 1u));
    const float u = mixup_u01(fer_hash(seed, 3u * t + 2u));
    const float x = sqrtf(-2.f * logf(u1)) * cospif(2.f * u2);
    const float w = 1.f + c * x;
    if (w <= 0.f) continue;
    const float v = w * w * w;
    if (logf(u) < 0.5f * x * x + d - d * v + d * logf(v)) {
      g = d * v;
      break;
    }
  }
  float lg = logf(g);
  if (alpha < 1.f) lg += logf(mixup_u01(fer_hash(seed, 3u * MIXUP_ATTEMPTS))) / alpha;
  return lg;
}

// One workgroup per set. perm[i] = rank of (key_i, i), key_i = fer_hash(perm seed, i): the keys go to LDS, each
// thread counts the smaller ones for its elements (four keys per 16-byte LDS read, the same address in every
// lane). The padding keys up to a multiple of 4 are 0xFFFFFFFF at indices >= B: never smaller than a real pair.
__global__ __launch_bounds__(256) void mixup_draw_kernel(float alpha, int B, uint64_t seed, float* __restrict__ lam,
                                                         int32_t* __restrict__ perm) {
  __shared__ __attribute__((aligned(16))) uint32_t keys[MIXUP_MAX_B];
  const int s = blockIdx.x, tid = threadIdx.x;
  const uint64_t ss = step_stream_seed(seed, (uint64_t)s);
  const uint64_t sp = ss ^ MIXUP_PERM_XOR;
  const int B4 = (B + 3) & ~3;
  for (int i = tid; i < B4; i += 256) keys[i] = i < B ? fer_hash(sp, (uint32_t)i) : 0xFFFFFFFFu;
  __syncthreads();
  for (int i = tid; i < B; i += 256) {
    const uint32_t k = keys[i];
    int r = 0;
    for (int j = 0; j < B4; j += 4) {
      const uint4 q = *(const uint4*)(keys + j);
      r += (q.x < k || (q.x == k && j < i)) + (q.y < k || (q.y == k && j + 1 < i)) +
           (q.z < k || (q.z == k && j + 2 < i)) + (q.w < k || (q.w == k && j + 3 < i));
    }
    perm[(long)s * B + i] = r;
  }
  if (tid == 255) {  // one lane (of the wave with the least permutation work)
    float l = 1.f;
    if (alpha > 0.f) {
      const float lg1 = mixup_log_gamma(alpha, ss ^ MIXUP_GAMMA1_XOR);
      const float lg2 = mixup_log_gamma(alpha, ss ^ MIXUP_GAMMA2_XOR);
      l = 1.f / (1.f + expf(lg2 - lg1));  // g1 / (g1 + g2)
    }
    lam[s] = l;
  }
}

// out[b] = lam * x[b] + (1 - lam) * x[perm[b]], one row per blockIdx.y, a grid-stride loop over the row.
// A perm entry outside [0, B) takes the row itself (never an address outside x).
template <typename V>
__global__ __launch_bounds__(256) void mixup_apply_kernel(const V* __restrict__ x, const int32_t* __restrict__ perm,
                                                          const float* __restrict__ lam, V* __restrict__ out, int B,
                                                          long n) {
  const int b = blockIdx.y;
  int p = perm[b];
  if ((unsigned)p >= (unsigned)B) p = b;
  const float l = *lam, m = 1.f - l;
  const V* xa = x + (long)b * n;
  const V* xb = x + (long)p * n;
  V* o = out + (long)b * n;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256L) o[i] = l * xa[i] + m * xb[i];
}

// ce_kernel (vit_edge.hip) with two targets per row, y[b] and y[perm[b]]: one block, one log-sum-exp per row.
__global__ __launch_bounds__(256) void ce_mix_kernel(const float* __restrict__ logits, const int64_t* __restrict__ y,
                                                     const int32_t* __restrict__ perm, const float* __restrict__ lamp,
                                                     const float* __restrict__ wt, int B, int C, float ls,
                                                     float gscale, float* loss, float* dlogits) {
  __shared__ float red[4][4];
  const int tid = threadIdx.x;
  float s[4] = {0.f, 0.f, 0.f, 0.f};  // num, den of the first target; num, den of the second
  auto second = [&](int b) {
    const int p = perm ? perm[b] : b;
    return (int)y[(unsigned)p < (unsigned)B ? p : b];
  };
  for (int b = tid; b < B; b += 256) {
    const float* z = logits + (long)b * C;
    float m = -INFINITY;
    for (int c = 0; c < C; ++c) m = fmaxf(m, z[c]);
    float se = 0.f;
    for (int c = 0; c < C; ++c) se += expf(z[c] - m);
    // -log p_c = log(se) + (m - z_c), the difference first (ce_kernel)
    const float lg = logf(se);
    const int y1 = (int)y[b], y2 = second(b);
    const float w1 = wt ? wt[y1] : 1.f, w2 = wt ? wt[y2] : 1.f;
    float sm = 0.f;
    for (int c = 0; c < C; ++c) sm += (wt ? wt[c] : 1.f) * (lg + (m - z[c]));
    s[0] += (1.f - ls) * w1 * (lg + (m - z[y1])) + ls / C * sm;
    s[1] += w1;
    s[2] += (1.f - ls) * w2 * (lg + (m - z[y2])) + ls / C * sm;
    s[3] += w2;
  }
  block_sum<4>(s, red);
  const float lam = *lamp;
  if (tid == 0 && loss) *loss = lam * (s[0] / s[1]) + (1.f - lam) * (s[2] / s[3]);
  if (!dlogits) return;
  const float a1 = lam * gscale / s[1], a2 = (1.f - lam) * gscale / s[3];
  for (int b = tid; b < B; b += 256) {
    const float* z = logits + (long)b * C;
    float m = -INFINITY;
    for (int c = 0; c < C; ++c) m = fmaxf(m, z[c]);
    float se = 0.f;
    for (int c = 0; c < C; ++c) se += expf(z[c] - m);
    const int y1 = (int)y[b], y2 = second(b);
    const float w1 = wt ? wt[y1] : 1.f, w2 = wt ? wt[y2] : 1.f;
    float wsum = 0.f;
    for (int c = 0; c < C; ++c) wsum += wt ? wt[c] : 1.f;
    for (int c = 0; c < C; ++c) {
      const float p = expf(z[c] - m) / se;
      // a1 d/dz_c [(1-ls) w1 (lse - z_y1) + ls/C sum_k w_k (lse - z_k)] + a2 [the same with y2]
      const float hard = a1 * w1 * (p - (c == y1 ? 1.f : 0.f)) + a2 * w2 * (p - (c == y2 ? 1.f : 0.f));
      dlogits[(long)b * C + c] = (1.f - ls) * hard + ls / C * (a1 + a2) * (wsum * p - (wt ? wt[c] : 1.f));
    }
  }
}

}  // namespace fer

using namespace fer;

extern "C" int fer_mixup_draw(float alpha, int B, uint64_t seed, int n_sets, float* lam, int32_t* perm,
                              fer_stream_t stream) {
  if (B < 1 || B > MIXUP_MAX_B) return set_error("mixup_draw: 1 <= B <= 2048");
  if (n_sets < 1) return set_error("mixup_draw: n_sets >= 1");
  if (!lam || !perm) return set_error("mixup_draw: null output");
  hipLaunchKernelGGL(mixup_draw_kernel, dim3(n_sets), dim3(256), 0, (hipStream_t)stream, alpha, B, seed, lam, perm);
  return hip_check("mixup_draw");
}

extern "C" int fer_mixup_apply(const float* x, const int32_t* perm, const float* lam, float* out, int B, int64_t L,
                               fer_stream_t stream) {
  if (B <= 0 || L <= 0) return 0;
  if (!x || !perm || !lam || !out) return set_error("mixup_apply: null operand");
  if (B > 65535) return set_error("mixup_apply: B <= 65535");
  const int64_t n = (int64_t)B * L;
  // (the gather reads rows an in-place mix would have overwritten already)
  if (out < x + n && x < out + n) return set_error("mixup_apply: out must not overlap x");
  hipStream_t st = (hipStream_t)stream;
  // memory-bound: 16 bytes per lane where the rows allow it, at most ~2048 blocks (256 CUs x 8) and a
  // grid-stride loop for the rest
  const int per_row = std::max(1, 2048 / B);
  if (L % 4 == 0 && al16(x) && al16(out)) {
    const dim3 grid(std::min<int64_t>(ceil_div(L / 4, 256), per_row), B);
    hipLaunchKernelGGL(mixup_apply_kernel<f32x4>, grid, dim3(256), 0, st, (const f32x4*)x, perm, lam, (f32x4*)out, B,
                       (long)(L / 4));
  } else {
    const dim3 grid(std::min<int64_t>(ceil_div(L, 256), per_row), B);
    hipLaunchKernelGGL(mixup_apply_kernel<float>, grid, dim3(256), 0, st, x, perm, lam, out, B, (long)L);
  }
  return hip_check("mixup_apply");
}

extern "C" int fer_cross_entropy_mix(const float* logits, const int64_t* labels, const int32_t* perm, const float* lam,
                                     const float* weight, int B, int C, float label_smoothing, float grad_scale,
                                     float* loss, float* dlogits, fer_stream_t stream) {
  if (B <= 0) return 0;
  if (!logits || !labels || !lam) return set_error("cross_entropy_mix: null operand");
  hipLaunchKernelGGL(ce_mix_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, logits, labels, perm, lam, weight, B, C,
                     label_smoothing, grad_scale, loss, dlogits);
  return hip_check("cross_entropy_mix");
}
