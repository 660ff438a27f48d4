// fer_skinny_adapter: out[M][D] = X + alpha * (GELU_erf(X W1^T + b1) W2^T + b2) for M <= 64 rows in bf16: the
// AdapterModule of the pre-norm models (fervit/blocks.py) as one launch of the skinny inference plan
// (fervit/infer.py). alpha is read from device memory by the kernel, never by the host.
//
// Decomposition, by fer_skinny_linear's rules (skinny.hip): one workgroup per strip of 16 output columns, all M
// rows (D / 16 workgroups), and workgroups never communicate: no counters, flags, polling or atomics.
//   * Every workgroup computes the whole hidden tile H = GELU(X W1^T + b1) [M][R] itself. Sharing it would need
//     either a second launch with an R-wide middle (R / 16 <= 8 workgroups on the machine) or a hand-over between
//     workgroups; recomputing it is M * R * D MACs (6 MFLOP at 64 x 128 x 768) against W1's R * D * 2 bytes
//     (at most 192 KB) out of L2.
//   * Phase 1: wave w owns the hidden column tiles w and w + 4 (16 columns each, R <= 128) for every row tile
//     and runs the whole K = D loop for them in increasing k, so there is no cross-wave reduction. W1 rows go
//     straight to VGPRs as the MFMA's A operand (v_mfma_f32_16x16x32_bf16: lane l holds W1 row h0 + (l & 15),
//     k = 8 (l >> 4) ... + 7), a 256-column chunk's fragments in flight before their first use. The X panel
//     goes through LDS in 256-column chunks, 16-byte pieces XOR-swizzled by the row as in skinny.hip; rows
//     M .. 16 MT - 1 and columns >= D are zero.
//   * H is rounded to bf16 once, into LDS, as the second product's matrix operand (the eager path stores it to
//     memory in bf16 at the same point). Columns R .. 31 of a half-used last k-step are zero.
//   * Phase 2: wave t takes row tile t: out^T tile [16 columns][16 rows] = W2 strip (A operand, from L2) times
//     H (B operand, from LDS), K = R in increasing k. Lane l holds columns n0 + 4 (l >> 4) ... + 3 of row
//     16 t + (l & 15): b2 is added, then x + alpha * (.) in fp32, one rounding, one 8-byte vector store.
// An element's summation order depends on D and R alone, not on M or on the other rows.
#include "common.h"
#include "fervit_internal.h"

namespace fer {

namespace {

constexpr int AD_STRIP = 16;    // output columns per workgroup
constexpr int AD_MAX_M = 64;
constexpr int AD_MAX_R = 128;
constexpr int AD_KC = 256;      // X panel columns per chunk: 64 * 256 * 2 bytes = 32 KB at four row tiles
constexpr int AD_PR = AD_KC / 8;   // 16-byte pieces per panel row
constexpr int AD_NS = AD_KC / 32;  // k-steps per chunk
constexpr int AD_HS = AD_MAX_R + 8;  // H row stride in LDS: 272 bytes, 16 rows at one k cover all 64 banks

struct AdapterArgs {
  const bf16* X;
  const bf16* W1;
  const bf16* W2;
  bf16* out;
  const float *b1, *b2, *alpha;
  long ldx, ldw1, ldw2, ldc;
  int M, D, R;
};

FER_DEV float adapter_gelu(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752f)); }

template <int MT>
__global__ __launch_bounds__(256) void skinny_adapter_kernel(AdapterArgs a) {
  constexpr int MP = 16 * MT;              // panel rows
  constexpr int FILL = MP * AD_PR / 256;   // pieces per thread and chunk
  __shared__ bf16x8 panel[MP * AD_PR];
  __shared__ __attribute__((aligned(16))) bf16 hid[MP * AD_HS];

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 15, q = lane >> 4;
  const int n0 = blockIdx.x * AD_STRIP;
  const int RT = a.R >> 4;  // hidden column tiles
  const bf16x8 zero = {};
  const float alpha = *a.alpha;

  // the second product's weight fragments (this workgroup's 16 rows of W2), in flight from the start
  bf16x8 w2f[AD_MAX_R / 32];
#pragma unroll
  for (int s = 0; s < AD_MAX_R / 32; ++s) {
    const int k = 32 * s + 8 * q;
    w2f[s] = k < a.R ? *(const bf16x8*)(a.W2 + (long)(n0 + r) * a.ldw2 + k) : zero;
  }

  // this wave's hidden column tiles j = wave and wave + 4, and their W1 fragments of chunk 0
  bool on[2];
  const bf16* wp[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int j = wave + 4 * i;
    on[i] = j < RT;
    wp[i] = a.W1 + (long)(on[i] ? 16 * j + r : 0) * a.ldw1 + 8 * q;
  }
  bf16x8 wf[AD_NS][2];
#pragma unroll
  for (int s = 0; s < AD_NS; ++s)
#pragma unroll
    for (int i = 0; i < 2; ++i) wf[s][i] = on[i] && 32 * s + 8 * q < a.D ? *(const bf16x8*)(wp[i] + 32 * s) : zero;

  // zero columns R .. R + 15 of H where the last k-step of the second product is half used
  if ((a.R & 16) && tid < 2 * MP) *(bf16x8*)(hid + (tid >> 1) * AD_HS + a.R + 8 * (tid & 1)) = zero;

  f32x4 acc[2][MT];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[i][t] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int kc0 = 0; kc0 < a.D; kc0 += AD_KC) {
    // ---- panel chunk: rows 0 .. MP-1, columns kc0 .. kc0 + 255 (zero beyond M / D)
    bf16x8 pv[FILL];
#pragma unroll
    for (int j = 0; j < FILL; ++j) {
      const int idx = tid + 256 * j, row = idx / AD_PR, k = kc0 + (idx % AD_PR) * 8;
      pv[j] = row < a.M && k < a.D ? *(const bf16x8*)(a.X + (long)row * a.ldx + k) : zero;
    }
#pragma unroll
    for (int j = 0; j < FILL; ++j) {
      const int idx = tid + 256 * j, row = idx / AD_PR, p = idx % AD_PR;
      panel[row * AD_PR + (p ^ (row & 15))] = pv[j];
    }
    __syncthreads();

    // ---- this wave's hidden tiles over the chunk's k-steps
    if (on[0]) {
#pragma unroll
      for (int s = 0; s < AD_NS; ++s) {
        const int p = 4 * s + q;
#pragma unroll
        for (int t = 0; t < MT; ++t) {
          const bf16x8 x = panel[(16 * t + r) * AD_PR + (p ^ r)];
          acc[0][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[s][0], x, acc[0][t], 0, 0, 0);
          if (on[1]) acc[1][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[s][1], x, acc[1][t], 0, 0, 0);
        }
      }
    }
    // next chunk's W1 fragments: in flight during the next panel fill
    if (kc0 + AD_KC < a.D) {
#pragma unroll
      for (int s = 0; s < AD_NS; ++s) {
        const int ks = kc0 + AD_KC + 32 * s;
#pragma unroll
        for (int i = 0; i < 2; ++i) wf[s][i] = on[i] && ks + 8 * q < a.D ? *(const bf16x8*)(wp[i] + ks) : zero;
      }
    }
    __syncthreads();  // the panel is rewritten by the next chunk
  }

  // ---- H = GELU(. + b1), rounded to bf16 once: lane l holds columns 16 j + 4 q ... + 3 of row 16 t + r
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    if (!on[i]) continue;
    const int h = 16 * (wave + 4 * i) + 4 * q;
    const f32x4 b = ldg_f32x4(a.b1 + h);
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      const f32x4 v = acc[i][t] + b;
      *(bf16x4*)(hid + (16 * t + r) * AD_HS + h) = bf16x4{(bf16)adapter_gelu(v[0]), (bf16)adapter_gelu(v[1]),
                                                          (bf16)adapter_gelu(v[2]), (bf16)adapter_gelu(v[3])};
    }
  }
  __syncthreads();

  // ---- wave t: row tile t of this workgroup's 16 output columns
  if (wave >= MT) return;
  f32x4 o = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < AD_MAX_R / 32; ++s) {
    if (32 * s < a.R) {
      const bf16x8 hf = *(const bf16x8*)(hid + (16 * wave + r) * AD_HS + 32 * s + 8 * q);
      o = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w2f[s], hf, o, 0, 0, 0);
    }
  }
  const int m = 16 * wave + r, n = n0 + 4 * q;
  if (m >= a.M) return;
  o += ldg_f32x4(a.b2 + n);
  const bf16x4 xv = *(const bf16x4*)(a.X + (long)m * a.ldx + n);
#pragma unroll
  for (int i = 0; i < 4; ++i) o[i] = fmaf(alpha, o[i], (float)xv[i]);
  *(bf16x4*)(a.out + (long)m * a.ldc + n) = bf16x4{(bf16)o[0], (bf16)o[1], (bf16)o[2], (bf16)o[3]};
}

}  // namespace

}  // namespace fer

using namespace fer;

extern "C" int fer_skinny_adapter(const void* X, int64_t ldx, const void* W1, int64_t ldw1, const float* b1,
                                  const void* W2, int64_t ldw2, const float* b2, const float* alpha, void* out,
                                  int64_t ldc, int M, int D, int R, fer_stream_t stream) {
  if (M < 1 || M > AD_MAX_M) return set_error("skinny_adapter: 1 <= M <= 64");
  if (D < 16 || D % 16) return set_error("skinny_adapter: D must be a positive multiple of 16");
  if (R < 16 || R > AD_MAX_R || R % 16)
    return set_error("skinny_adapter: the adapter width R must be a multiple of 16, 16 <= R <= 128");
  if (!X || !W1 || !b1 || !W2 || !b2 || !out)
    return set_error("skinny_adapter: X, W1, b1, W2, b2 and out are required");
  if (!alpha) return set_error("skinny_adapter: alpha is a device pointer to one float and is required");
  if (ldx < D || ldx % 8 || ldw1 < D || ldw1 % 8 || ldw2 < R || ldw2 % 8 || ldc < D || ldc % 8)
    return set_error("skinny_adapter: every row stride must cover its row and be a multiple of 8");
  if (!al16(X) || !al16(W1) || !al16(b1) || !al16(W2) || !al16(b2) || !al16(out) || ((uintptr_t)alpha & 3))
    return set_error("skinny_adapter: every base pointer must be 16-byte aligned (alpha: 4-byte)");
  const uintptr_t x0 = (uintptr_t)X, x1 = x0 + ((uintptr_t)(M - 1) * ldx + D) * sizeof(bf16);
  const uintptr_t o0 = (uintptr_t)out, o1 = o0 + ((uintptr_t)(M - 1) * ldc + D) * sizeof(bf16);
  if (x0 < o1 && o0 < x1) return set_error("skinny_adapter: out must not overlap X (every workgroup reads all of X)");
  AdapterArgs a;
  a.X = (const bf16*)X, a.W1 = (const bf16*)W1, a.W2 = (const bf16*)W2, a.out = (bf16*)out;
  a.b1 = b1, a.b2 = b2, a.alpha = alpha;
  a.ldx = ldx, a.ldw1 = ldw1, a.ldw2 = ldw2, a.ldc = ldc;
  a.M = M, a.D = D, a.R = R;
  const dim3 grid(D / AD_STRIP);
  dispatch_int<1, 2, 3, 4>(ceil_div(M, 16), [&](auto I) {
    hipLaunchKernelGGL(skinny_adapter_kernel<decltype(I)::value>, grid, dim3(256), 0, (hipStream_t)stream, a);
  });
  return hip_check("skinny_adapter");
}
