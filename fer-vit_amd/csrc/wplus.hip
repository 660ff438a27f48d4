// Latent (w+) models' own kernels: the fused w+ prologue (SemanticPE / LayerWiseNorm / LEAM,
// forward and backward with its chunked parameter-gradient sums), the LatentDecomposer projection
// and the on-device latent augmentation.
#include "common.h"
#include "fervit_internal.h"
#include "step_seed.h"

namespace fer {

// ------------------------------------------------------------------ w+ prologue
// Block per (row r = b*L + l); 256 threads; D <= 1024. saved[r] = {mean, rstd}.
__global__ __launch_bounds__(256) void wplus_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, int L,
                                                        int D, const float* sg, const float* sl, const int64_t* grp,
                                                        const float* lw, const float* lb, const float* gate,
                                                        const float* lm, float eps, float* saved) {
  __shared__ float red[8];
  const long r = blockIdx.x;
  const int l = r % L, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  float v[4];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int d = tid + i * 256;
    float a = 0.f;
    if (d < D) {
      a = x[r * D + d];
      if (sg) a += sg[grp[l] * D + d] + sl[(long)l * D + d];
    }
    v[i] = a;
    s += a;
  }
  float mu = 0.f, rs = 0.f;
  if (lw) {
    s = wave_sum(s);
    if (lane == 0) red[w] = s;
    __syncthreads();
    mu = (red[0] + red[1] + red[2] + red[3]) / D;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (tid + i * 256 < D) q += (v[i] - mu) * (v[i] - mu);
    q = wave_sum(q);
    if (lane == 0) red[4 + w] = q;
    __syncthreads();
    rs = rsqrtf((red[4] + red[5] + red[6] + red[7]) / D + eps);
  }
  const float sgate = gate ? 1.f / (1.f + __expf(-gate[l])) : 0.f;
  const float slm = lm ? 1.f / (1.f + __expf(-lm[l])) : 1.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int d = tid + i * 256;
    if (d >= D) continue;
    float u = v[i];
    if (lw) {
      const float n = (v[i] - mu) * rs * lw[(long)l * D + d] + lb[(long)l * D + d];
      u = gate ? v[i] + sgate * (n - v[i]) : n;
    }
    y[r * D + d] = u * slm;
  }
  if (tid == 0 && saved) {
    saved[2 * r] = mu;
    saved[2 * r + 1] = rs;
  }
}
// Block per (l, b-chunk). part layout per (chunk, l): [dlw D | dlb D | dsl D | dgate 1 | dleam 1]
__global__ __launch_bounds__(256) void wplus_bwd_kernel(const float* __restrict__ x, const float* __restrict__ saved,
                                                        const float* __restrict__ dy, float* __restrict__ dx, int B,
                                                        int L, int D, int bchunk, const float* sg, const float* sl,
                                                        const int64_t* grp, const float* lw, const float* lb,
                                                        const float* gate, const float* lm,
                                                        float* __restrict__ part) {
  __shared__ float red[3][4];
  const int l = blockIdx.x, ch = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int b0 = ch * bchunk, b1 = min(B, b0 + bchunk);
  const float sgate = gate ? 1.f / (1.f + __expf(-gate[l])) : 0.f;
  const float slm = lm ? 1.f / (1.f + __expf(-lm[l])) : 1.f;
  float plw[4] = {}, plb[4] = {}, psl[4] = {};
  float pgate = 0.f, pleam = 0.f;
  for (int b = b0; b < b1; ++b) {
    const long r = (long)b * L + l;
    const float mu = saved ? saved[2 * r] : 0.f, rs = saved ? saved[2 * r + 1] : 0.f;
    float v[4], xh[4], n[4], du[4];
    float a1 = 0.f, a2 = 0.f, ag = 0.f, al = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int d = tid + i * 256;
      v[i] = xh[i] = n[i] = du[i] = 0.f;
      if (d >= D) continue;
      float a = x[r * D + d];
      if (sg) a += sg[grp[l] * D + d] + sl[(long)l * D + d];
      v[i] = a;
      float u = a;
      if (lw) {
        xh[i] = (a - mu) * rs;
        n[i] = xh[i] * lw[(long)l * D + d] + lb[(long)l * D + d];
        u = gate ? a + sgate * (n[i] - a) : n[i];
      }
      const float g = dy[r * D + d];
      al += g * u;
      du[i] = g * slm;
    }
    // through LWN
    float dv[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int d = tid + i * 256;
      dv[i] = du[i];
      if (d >= D || !lw) continue;
      const float dn = gate ? du[i] * sgate : du[i];
      if (gate) {
        ag += du[i] * (n[i] - v[i]);
        dv[i] = du[i] * (1.f - sgate);
      } else {
        dv[i] = 0.f;
      }
      plw[i] += dn * xh[i];
      plb[i] += dn;
      const float gg = dn * lw[(long)l * D + d];
      n[i] = gg;  // reuse: g*gamma
      a1 += gg;
      a2 += gg * xh[i];
    }
    if (lw) {
      a1 = wave_sum(a1);
      a2 = wave_sum(a2);
      ag = wave_sum(ag);
      __syncthreads();
      if (lane == 0) {
        red[0][w] = a1;
        red[1][w] = a2;
        red[2][w] = ag;
      }
      __syncthreads();
      const float m1 = (red[0][0] + red[0][1] + red[0][2] + red[0][3]) / D;
      const float m2 = (red[1][0] + red[1][1] + red[1][2] + red[1][3]) / D;
      if (tid == 0) pgate += red[2][0] + red[2][1] + red[2][2] + red[2][3];
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (tid + i * 256 < D) dv[i] += (n[i] - m1 - xh[i] * m2) * rs;
    }
    al = wave_sum(al);
    __syncthreads();
    if (lane == 0) red[0][w] = al;
    __syncthreads();
    if (tid == 0) pleam += red[0][0] + red[0][1] + red[0][2] + red[0][3];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int d = tid + i * 256;
      if (d >= D) continue;
      dx[r * D + d] = dv[i];
      psl[i] += dv[i];
    }
  }
  const long ps = 3L * D + 2;
  float* pp = part + ((long)ch * L + l) * ps;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int d = tid + i * 256;
    if (d >= D) continue;
    pp[d] = plw[i];
    pp[D + d] = plb[i];
    pp[2 * D + d] = psl[i];
  }
  if (tid == 0) {
    pp[3 * D] = pgate * sgate * (1.f - sgate);
    pp[3 * D + 1] = pleam * slm * (1.f - slm);
  }
}
// reduce chunks; group embedding grad = sum of layer-embedding grads over its layers
__global__ void wplus_bwd_final(const float* __restrict__ part, int nch, int L, int D, const int64_t* grp, float* dsg,
                                float* dsl, float* dlw, float* dlb, float* dgate, float* dleam, int accumulate) {
  const long ps = 3L * D + 2;
  const long j = blockIdx.x * 256L + threadIdx.x;
  if (j >= (long)L * ps) return;
  const int l = j / ps;
  const long k = j - (long)l * ps;
  float s = 0.f;
  for (int c = 0; c < nch; ++c) s += part[((long)c * L + l) * ps + k];
  float* o = nullptr;
  long oi = 0;
  if (k < D) { o = dlw; oi = (long)l * D + k; }
  else if (k < 2 * D) { o = dlb; oi = (long)l * D + k - D; }
  else if (k < 3 * D) { o = dsl; oi = (long)l * D + k - 2 * D; }
  else if (k == 3 * D) { o = dgate; oi = l; }
  else { o = dleam; oi = l; }
  if (o) o[oi] = accumulate ? o[oi] + s : s;
  if (k >= 2 * D && k < 3 * D && dsg && l == 0) {
    // group sums computed by the l == 0 thread of each column: fixed order over layers
    const int d = k - 2 * D;
    float gsum[3] = {0.f, 0.f, 0.f};
    for (int ll = 0; ll < L; ++ll) {
      float t = 0.f;
      for (int c = 0; c < nch; ++c) t += part[((long)c * L + ll) * ps + 2 * D + d];
      gsum[grp[ll]] += t;
    }
    for (int g = 0; g < 3; ++g) dsg[(long)g * D + d] = accumulate ? dsg[(long)g * D + d] + gsum[g] : gsum[g];
  }
}

// ------------------------------------------------------------------ decomposer
__global__ __launch_bounds__(256) void decomp_scores_kernel(const float* __restrict__ w, const float* __restrict__ dirs,
                                                            int C, int LD, float* __restrict__ scores) {
  __shared__ float red[16][4];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  float acc[16] = {};
  for (int i = tid; i < LD; i += 256) {
    const float x = w[(long)b * LD + i];
    for (int c = 0; c < C; ++c) acc[c] += x * dirs[(long)c * LD + i];
  }
  for (int c = 0; c < C; ++c) {
    const float s = wave_sum(acc[c]);
    if (lane == 0) red[c][wv] = s;
  }
  __syncthreads();
  if (tid < C) scores[(long)b * C + tid] = red[tid][0] + red[tid][1] + red[tid][2] + red[tid][3];
}
__global__ __launch_bounds__(256) void decomp_out_kernel(const float* __restrict__ w, const float* __restrict__ dirs,
                                                         const float* __restrict__ scores, int C, int LD, int omode,
                                                         float alpha, int dmode, float* __restrict__ y) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= LD) return;
  const float* sc = scores + (long)b * C;
  float e = 0.f;
  if (dmode == 0) {
    for (int c = 0; c < C; ++c) e += sc[c] * dirs[(long)c * LD + i];
  } else {
    int best = 0;
    float bv = fabsf(sc[0]);
    for (int c = 1; c < C; ++c)
      if (fabsf(sc[c]) > bv) { bv = fabsf(sc[c]); best = c; }
    e = sc[best] * dirs[(long)best * LD + i];
  }
  const float x = w[(long)b * LD + i];
  const float idv = x - e;
  if (omode == 3) {
    y[(long)b * 2 * LD + i] = e;
    y[(long)b * 2 * LD + LD + i] = idv;
  } else {
    y[(long)b * LD + i] = omode == 0 ? e : (omode == 1 ? idv : idv + alpha * e);
  }
}

}  // namespace fer

using namespace fer;

static int wplus_chunks(int B) { return std::max(1, std::min(B, 32)); }
extern "C" int64_t fer_wplus_ws(int B, int L, int D) { return (int64_t)wplus_chunks(B) * L * (3L * D + 2) * 4; }

extern "C" int fer_wplus_fwd(const float* x, float* y, int B, int L, int D, const float* spe_group,
                             const float* spe_layer, const int64_t* groups, const float* lwn_w, const float* lwn_b,
                             const float* lwn_gate, const float* leam_w, float eps, float* saved,
                             fer_stream_t stream) {
  if (B <= 0) return 0;
  if (D > 1024) return set_error("wplus_fwd: D <= 1024");
  hipLaunchKernelGGL(wplus_fwd_kernel, dim3(B * L), dim3(256), 0, (hipStream_t)stream, x, y, L, D, spe_group,
                     spe_layer, groups, lwn_w, lwn_b, lwn_gate, leam_w, eps, saved);
  return hip_check("wplus_fwd");
}

extern "C" int fer_wplus_bwd(const float* x, const float* saved, const float* dy, float* dx, int B, int L, int D,
                             const float* spe_group, const float* spe_layer, const int64_t* groups,
                             const float* lwn_w, const float* lwn_b, const float* lwn_gate, const float* leam_w,
                             float eps, float* d_spe_group, float* d_spe_layer, float* d_lwn_w, float* d_lwn_b,
                             float* d_lwn_gate, float* d_leam_w, int accumulate, float* ws, int64_t ws_bytes,
                             fer_stream_t stream) {
  (void)eps;
  if (B <= 0) return 0;
  if (D > 1024) return set_error("wplus_bwd: D <= 1024");  // 4 x 256 columns per row, as the forward
  if (!ws || ws_bytes < fer_wplus_ws(B, L, D)) return set_error("wplus_bwd: workspace too small");
  const int nch = wplus_chunks(B);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(wplus_bwd_kernel, dim3(L, nch), dim3(256), 0, st, x, saved, dy, dx, B, L, D, ceil_div(B, nch),
                     spe_group, spe_layer, groups, lwn_w, lwn_b, lwn_gate, leam_w, ws);
  const long tot = (long)L * (3L * D + 2);
  hipLaunchKernelGGL(wplus_bwd_final, dim3(ceil_div(tot, 256)), dim3(256), 0, st, ws, nch, L, D, groups, d_spe_group,
                     d_spe_layer, d_lwn_w, d_lwn_b, d_lwn_gate, d_leam_w, accumulate);
  return hip_check("wplus_bwd");
}

extern "C" int fer_decompose(const float* w, const float* dirs, int B, int C, int LD, int output_mode, float alpha,
                             int decompose_mode, float* y, float* scores, fer_stream_t stream) {
  if (B <= 0) return 0;
  if (C > 16) return set_error("decompose: at most 16 directions");
  if (!scores) return set_error("decompose: scores buffer required");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(decomp_scores_kernel, dim3(B), dim3(256), 0, st, w, dirs, C, LD, scores);
  if (y)
    hipLaunchKernelGGL(decomp_out_kernel, dim3(ceil_div(LD, 256), B), dim3(256), 0, st, w, dirs, (const float*)scores,
                       C, LD, output_mode, alpha, decompose_mode, y);
  return hip_check("decompose");
}

// ------------------------------------------------------------------ latent augmentation
// LatentAugment (`data/latent_dataset.py:6-49`) on device, in the reference's order:
// x += N(0, noise_std) (Box-Muller on two 32-bit hashes), x *= U(scale_lo, scale_hi) drawn once
// per sample, x *= (U(0,1) > mask_prob). Same distributions as the reference's torch RNG calls
// (not the same stream). Counter-based like the dropout masks: element i of the batch.
FER_DEV float u01(uint32_t h) { return ((float)(h >> 8) + 0.5f) * (1.f / 16777216.f); }
__global__ void latent_augment_kernel(float* __restrict__ x, long n, int LD, float noise_std, float scale_lo,
                                      float scale_hi, float mask_prob, uint64_t seed) {
  seed = step_seed(seed);
  const uint64_t s_noise = seed, s_scale = seed ^ 0x5851F42D4C957F2Dull, s_mask = seed ^ 0x14057B7EF767814Full;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256L) {
    float v = x[i];
    if (noise_std > 0.f) {
      const uint32_t e = (uint32_t)i;
      const float u1 = u01(fer_hash(s_noise, 2u * e)), u2 = u01(fer_hash(s_noise, 2u * e + 1u));
      v += noise_std * sqrtf(-2.f * logf(u1)) * cosf(6.28318530717958648f * u2);
    }
    if (scale_hi > scale_lo || scale_lo != 1.f) {
      const uint32_t b = (uint32_t)(i / LD);
      v *= scale_lo + (scale_hi - scale_lo) * u01(fer_hash(s_scale, b));
    }
    if (mask_prob > 0.f && !(u01(fer_hash(s_mask, (uint32_t)i)) > mask_prob)) v = 0.f;
    x[i] = v;
  }
}

extern "C" int fer_latent_augment(float* x, int64_t B, int LD, float noise_std, float scale_lo, float scale_hi,
                                  float mask_prob, uint64_t seed, fer_stream_t stream) {
  const long n = (long)B * LD;
  if (n <= 0) return 0;
  if (n > 0x7FFFFFFFL) return set_error("latent_augment: more than 2^31 elements per call");
  hipLaunchKernelGGL(latent_augment_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, x, n, LD,
                     noise_std, scale_lo, scale_hi, mask_prob, seed);
  return hip_check("latent_augment");
}

// ------------------------------------------------------------------ direction draw
// The per-sample draw behind direction augmentation (fer_latent_shift in choice mode): sample i is left
// unchanged (choice -1) with probability p_keep, else takes one of n_choices (direction, step) pairs with
// equal probability. That is the per-sample distribution of drawing uniformly from the reference's expanded
// directory (`data/augment_latents.py:47-71`: 1 original + K*S variants per sample) when p_keep =
// 1 / (1 + K*S). Two hashes per sample, counters 2i and 2i + 1; the pair index is the high word of
// hash * n_choices (integers only: a host replica gives the same values).
constexpr uint64_t DIR_XOR = 0xD1B54A32D192ED03ull;
__global__ void latent_dir_draw_kernel(int* __restrict__ choice, long n, uint32_t n_choices, float p_keep,
                                       uint64_t seed) {
  seed = step_seed(seed) ^ DIR_XOR;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256L) {
    const uint32_t e = (uint32_t)i;
    const float u = u01(fer_hash(seed, 2u * e));
    choice[i] = u <= p_keep ? -1 : (int)(((uint64_t)fer_hash(seed, 2u * e + 1u) * n_choices) >> 32);
  }
}

extern "C" int fer_latent_dir_draw(int32_t* choice, int64_t n, int n_choices, float p_keep, uint64_t seed,
                                   fer_stream_t stream) {
  if (n_choices < 1) return set_error("latent_dir_draw: n_choices must be >= 1");
  if (!(p_keep >= 0.f && p_keep <= 1.f)) return set_error("latent_dir_draw: p_keep must be in [0, 1]");
  if (n <= 0) return 0;
  if (!choice) return set_error("latent_dir_draw: choice is required");
  if (n > 0x7FFFFFFFL) return set_error("latent_dir_draw: more than 2^31 samples per call");
  hipLaunchKernelGGL(latent_dir_draw_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, choice, (long)n,
                     (uint32_t)n_choices, p_keep, seed);
  return hip_check("latent_dir_draw");
}
