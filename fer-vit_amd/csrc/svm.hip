// Batched linear-SVM passes (reference `latent_analysis/compute_expression_direction.py:58-116`: LinearSVC on the
// flattened w+ latents, one-vs-rest). All P <= 8 one-vs-rest problems share X [N][F] fp32, so a solver step is a
// pass over X with P right-hand sides, bound by the N F 4 bytes of X. Two passes, each deterministic (fixed
// partition, fixed order, no floating-point atomics), neither reads the host nor allocates:
//
//   forward  Z = X W^T + bias, then an epilogue per element.
//            svm_dot_kernel      one wave per (8 rows, F chunk): lanes stride the 16-byte pieces of the chunk, a
//                                W piece is loaded once for the 8 rows (W is re-read from L2: P F 4 bytes per
//                                wave, as many bytes as the wave's 8 rows of X when P = 8), 64 fp32 FMA chains
//                                per lane, xor butterflies, row r's 8 partial dot products stored by lane r.
//                                F is cut into `splits` chunks (a multiple of 64 pieces each) only as far as the
//                                row blocks alone leave compute units idle: N = 256 runs 32 x 12 waves,
//                                N = 28,709 runs 3,589 x 1.
//            svm_epilogue_kernel a thread per row: the chunks' partials added in chunk order, + bias, then
//                                hinge: s = +-1, m = 1 - s z, a = [m > 0]: R = c a s m, Dw = c a, and the
//                                       workgroup's loss sums of c a m^2 (butterfly, then the four waves in order)
//                                scale: R = Dw * Z (the inner half of a Hessian-vector product)
//            svm_loss_kernel     the workgroups' loss sums added in workgroup order.
//   xtr      G = R^T X, gb = column sums of R.
//            svm_xtr_kernel      rows are cut into slabs of 32. One wave per (64 pieces of F, group of `gs`
//                                consecutive slabs): a lane owns one piece, walks a slab's rows in order with
//                                32 FMA chains (R's row is wave-uniform: scalar loads), adds the slab's sum to
//                                the group's sum, slab after slab. gs = ceil(slabs / 128): N = 256 runs 36 x 8
//                                waves; N = 28,709 runs 36 x 113 and writes 113 partials (29 MB, read once
//                                more: 5.5 % of X).
//            svm_xtr_reduce_kernel  a thread per (column, piece): the groups' sums added in group order.
//            So G[p][f] = sum over groups in order of (sum over the group's slabs in order of (sum over the
//            slab's rows in order)): a function of the input and of N alone.
//
// Rows of X, W and G need no alignment: a row operand whose base is 16-byte aligned and whose stride is a
// multiple of 4 moves in 16-byte pieces, any other one element by element, and the last F % 4 elements always
// do. Which lane owns which element, and so every sum's order, is the same on both paths.
#include "common.h"
#include "fervit_internal.h"

namespace fer {

constexpr int SVM_P = 8;           // columns per launch
constexpr int SVM_ROWS = 8;        // rows per wave of svm_dot_kernel
constexpr int SVM_EPI_ROWS = 256;  // rows per workgroup of svm_epilogue_kernel
constexpr int SVM_WAVES = 512;     // svm_dot_kernel cuts F until it runs this many waves (2 per CU)

// 4 consecutive floats from p of which the first `valid` exist (the rest, and all of them for valid <= 0, read
// as 0 without a load); vec: p is 16-byte aligned
FER_DEV f32x4 ld_piece(const float* p, int valid, bool vec) {
  if (vec && valid >= 4) return *(const f32x4*)p;
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (valid > 0) v[0] = p[0];
  if (valid > 1) v[1] = p[1];
  if (valid > 2) v[2] = p[2];
  if (valid > 3) v[3] = p[3];
  return v;
}
FER_DEV void st_piece(float* p, f32x4 v, int valid, bool vec) {
  if (vec && valid >= 4) {
    *(f32x4*)p = v;
    return;
  }
  if (valid > 0) p[0] = v[0];
  if (valid > 1) p[1] = v[1];
  if (valid > 2) p[2] = v[2];
  if (valid > 3) p[3] = v[3];
}

// ---------------------------------------------------------------- forward
struct SvmDotArgs {
  const float* X;
  const float* W;
  float* zpart;  // [splits][N][8]
  long ldx, ldw;
  int N, F, P, chunk;  // chunk: pieces per split, a multiple of 64
  bool vec_x, vec_w;
};

// grid (ceil(N / 8), splits), one wave
__global__ __launch_bounds__(64) void svm_dot_kernel(SvmDotArgs a) {
  const int lane = threadIdx.x;
  const long row0 = (long)blockIdx.x * SVM_ROWS;
  const int pieces = (a.F + 3) >> 2;
  const int pc0 = blockIdx.y * a.chunk, pc1 = min(pieces, pc0 + a.chunk);
  float acc[SVM_ROWS][SVM_P];
#pragma unroll
  for (int r = 0; r < SVM_ROWS; ++r)
#pragma unroll
    for (int p = 0; p < SVM_P; ++p) acc[r][p] = 0.f;
  for (int pc = pc0 + lane; pc < pc1; pc += 64) {
    const int f = pc * 4, valid = a.F - f;
    f32x4 w[SVM_P];
#pragma unroll
    for (int p = 0; p < SVM_P; ++p) w[p] = ld_piece(a.W + p * a.ldw + f, p < a.P ? valid : 0, a.vec_w);
#pragma unroll
    for (int r = 0; r < SVM_ROWS; ++r) {
      const f32x4 x = ld_piece(a.X + (row0 + r) * a.ldx + f, row0 + r < a.N ? valid : 0, a.vec_x);
#pragma unroll
      for (int p = 0; p < SVM_P; ++p)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[r][p] = fmaf(x[e], w[p][e], acc[r][p]);
    }
  }
#pragma unroll
  for (int r = 0; r < SVM_ROWS; ++r) {
#pragma unroll
    for (int p = 0; p < SVM_P; ++p) acc[r][p] = wave_sum(acc[r][p]);
    if (lane == r && row0 + r < a.N) {
      float* z = a.zpart + ((long)blockIdx.y * a.N + row0 + r) * SVM_P;
      *(f32x4*)z = f32x4{acc[r][0], acc[r][1], acc[r][2], acc[r][3]};
      *(f32x4*)(z + 4) = f32x4{acc[r][4], acc[r][5], acc[r][6], acc[r][7]};
    }
  }
}

struct SvmEpiArgs {
  const float* zpart;
  const float* bias;
  const long long* labels;
  const long long* classes;
  const float* Cp;
  const float* Cn;
  float* Z;
  float* R;
  float* Dw;  // hinge: written; scale: read
  float* losspart;  // [workgroups][8]
  long ldz, ldr, ldd;
  int N, P, splits, hinge;
};

// grid ceil(N / 256), 256 threads: thread = row
__global__ __launch_bounds__(256) void svm_epilogue_kernel(SvmEpiArgs a) {
  __shared__ float red[4][SVM_P];
  const long row = (long)blockIdx.x * SVM_EPI_ROWS + threadIdx.x;
  float l[SVM_P];
#pragma unroll
  for (int p = 0; p < SVM_P; ++p) l[p] = 0.f;
  if (row < a.N) {
    const float* zp = a.zpart + row * SVM_P;
    f32x4 lo = *(const f32x4*)zp, hi = *(const f32x4*)(zp + 4);
    for (int s = 1; s < a.splits; ++s) {
      zp += (long)a.N * SVM_P;
      lo += *(const f32x4*)zp;
      hi += *(const f32x4*)(zp + 4);
    }
    const float zs[SVM_P] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    const long long y = a.hinge ? a.labels[row] : 0;
#pragma unroll
    for (int p = 0; p < SVM_P; ++p) {
      if (p < a.P) {
        const float z = zs[p] + a.bias[p];
        if (a.Z) a.Z[row * a.ldz + p] = z;
        if (a.hinge) {
          const bool pos = y == a.classes[p];
          const float s = pos ? 1.f : -1.f;
          const float m = 1.f - s * z;
          const float ca = m > 0.f ? (pos ? a.Cp[p] : a.Cn[p]) : 0.f;
          a.R[row * a.ldr + p] = ca * s * m;
          a.Dw[row * a.ldd + p] = ca;
          l[p] = ca * m * m;
        } else {
          a.R[row * a.ldr + p] = a.Dw[row * a.ldd + p] * z;
        }
      }
    }
  }
  if (a.hinge) {
    block_sum<SVM_P>(l, red);
#pragma unroll
    for (int p = 0; p < SVM_P; ++p)
      if (threadIdx.x == p) a.losspart[(long)blockIdx.x * SVM_P + p] = l[p];
  }
}

// one wave: lane p adds column p's partial sums in workgroup order
__global__ __launch_bounds__(64) void svm_loss_kernel(const float* part, int nblk, int P, float* loss) {
  const int p = threadIdx.x;
  if (p >= P) return;
  float s = 0.f;
  for (int b = 0; b < nblk; ++b) s += part[(long)b * SVM_P + p];
  loss[p] = s;
}

// chunk (pieces per split, a multiple of 64) of svm_dot_kernel; returns the number of splits
static int svm_splits(int N, int F, int* chunk) {
  const int pieces = ceil_div(F, 4), rowblocks = ceil_div(N, SVM_ROWS);
  const int want = std::max(1, std::min(ceil_div(SVM_WAVES, rowblocks), ceil_div(pieces, 64)));
  *chunk = ceil_div(ceil_div(pieces, want), 64) * 64;
  return ceil_div(pieces, *chunk);
}

static long svm_forward_ws_floats(int N, int F) {
  int chunk;
  const long splits = svm_splits(N, F, &chunk);
  return splits * N * SVM_P + (long)ceil_div(N, SVM_EPI_ROWS) * SVM_P;
}

// ---------------------------------------------------------------- xtr
struct SvmXtrArgs {
  const float* X;
  const float* R;
  float* part;    // [groups][8][F4]
  float* gbpart;  // [groups][8]
  long ldx, ldr;
  int N, F, P, F4, gs;  // F4: F rounded up to 4; gs: slabs per group
  bool vec_x;
};

// grid (ceil(F4 / 256), groups), one wave: lane = piece
__global__ __launch_bounds__(64) void svm_xtr_kernel(SvmXtrArgs a) {
  const int lane = threadIdx.x;
  const int f = (blockIdx.x * 64 + lane) * 4, valid = a.F - f;
  float tot[SVM_P][4], totb[SVM_P];
#pragma unroll
  for (int p = 0; p < SVM_P; ++p) {
    totb[p] = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) tot[p][e] = 0.f;
  }
  for (int s = 0; s < a.gs; ++s) {
    const long r0 = ((long)blockIdx.y * a.gs + s) * FER_SVM_SLAB;
    if (r0 >= a.N) break;
    const int nr = (int)std::min<long>(FER_SVM_SLAB, a.N - r0);
    float acc[SVM_P][4], accb[SVM_P];
#pragma unroll
    for (int p = 0; p < SVM_P; ++p) {
      accb[p] = 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[p][e] = 0.f;
    }
#pragma unroll 4
    for (int i = 0; i < nr; ++i) {
      const f32x4 x = ld_piece(a.X + (r0 + i) * a.ldx + f, valid, a.vec_x);
      const float* r = a.R + (r0 + i) * a.ldr;
#pragma unroll
      for (int p = 0; p < SVM_P; ++p) {
        const float rp = p < a.P ? r[p] : 0.f;
        accb[p] += rp;
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[p][e] = fmaf(rp, x[e], acc[p][e]);
      }
    }
#pragma unroll
    for (int p = 0; p < SVM_P; ++p) {
      totb[p] += accb[p];
#pragma unroll
      for (int e = 0; e < 4; ++e) tot[p][e] += acc[p][e];
    }
  }
  if (f < a.F4) {
#pragma unroll
    for (int p = 0; p < SVM_P; ++p)
      *(f32x4*)(a.part + ((long)blockIdx.y * SVM_P + p) * a.F4 + f) = f32x4{tot[p][0], tot[p][1], tot[p][2], tot[p][3]};
  }
  if (blockIdx.x == 0) {
#pragma unroll
    for (int p = 0; p < SVM_P; ++p)
      if (lane == p) a.gbpart[(long)blockIdx.y * SVM_P + p] = totb[p];
  }
}

// a thread per (column, piece) of G, then P threads for gb: the groups' sums in group order
__global__ __launch_bounds__(256) void svm_xtr_reduce_kernel(const float* part, const float* gbpart, int groups, int P,
                                                             int F, int F4, float* G, long ldg, bool vec_g, float* gb) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  const int np = F4 >> 2;
  if (t < (long)P * np) {
    if (!G) return;
    const int p = (int)(t / np), f = (int)(t % np) * 4;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    for (int g = 0; g < groups; ++g) s += *(const f32x4*)(part + ((long)g * SVM_P + p) * F4 + f);
    st_piece(G + p * ldg + f, s, F - f, vec_g);
  } else if (t < (long)P * np + P) {
    if (!gb) return;
    const int p = (int)(t - (long)P * np);
    float s = 0.f;
    for (int g = 0; g < groups; ++g) s += gbpart[(long)g * SVM_P + p];
    gb[p] = s;
  }
}

// slabs per group and the number of groups for N rows
static int svm_groups(int N, int* gs) {
  const int slabs = ceil_div(N, FER_SVM_SLAB);
  *gs = ceil_div(slabs, FER_SVM_MAX_GROUPS);
  return ceil_div(slabs, *gs);
}

static long svm_xtr_ws_floats(int N, int F) {
  int gs;
  const long groups = svm_groups(N, &gs);
  return groups * SVM_P * (ceil_div(F, 4) * 4L) + groups * SVM_P;
}

static long svm_ws_bytes(int N, int F) { return 4 * std::max(svm_forward_ws_floats(N, F), svm_xtr_ws_floats(N, F)); }

}  // namespace fer

using namespace fer;

// ---------------------------------------------------------------- entry points
extern "C" int fer_svm_slab(void) { return FER_SVM_SLAB; }
extern "C" int fer_svm_max_groups(void) { return FER_SVM_MAX_GROUPS; }
extern "C" int64_t fer_svm_ws(int N, int F) { return N > 0 && F > 0 ? svm_ws_bytes(N, F) : 0; }

// what both passes ask of X, the shape and the workspace; `what` is the entry's name
static int svm_common(const char* what, const float* X, int64_t ldx, int N, int F, int P, const float* ws,
                      int64_t ws_bytes) {
  char msg[160];
  const char* bad = nullptr;
  if (F < 1) bad = "F must be >= 1";
  else if (P < 1 || P > 8) bad = "P must be 1..8 columns per launch";
  else if (!X || ldx < F) bad = "X is required, with a row stride >= F";
  else if (N > 0 && (!ws || !al16(ws) || ws_bytes < svm_ws_bytes(N, F)))
    bad = "the workspace must be 16-byte aligned and hold fer_svm_ws(N, F) bytes";
  if (!bad) return 0;
  snprintf(msg, sizeof(msg), "%s: %s", what, bad);
  return set_error(msg);
}

extern "C" int fer_svm_forward(const float* X, int64_t ldx, const float* W, int64_t ldw, const float* bias, int N,
                               int F, int P, int epilogue, const int64_t* labels, const int64_t* classes,
                               const float* Cp, const float* Cn, float* Z, int64_t ldz, float* R, int64_t ldr,
                               float* Dw, int64_t ldd, float* loss, float* ws, int64_t ws_bytes, fer_stream_t stream) {
  if (svm_common("svm_forward", X, ldx, N, F, P, ws, ws_bytes)) return -1;
  if (epilogue != 0 && epilogue != 1) return set_error("svm_forward: epilogue must be 0 (hinge) or 1 (scale)");
  if (!W || ldw < F || !bias) return set_error("svm_forward: W (row stride >= F) and bias are required");
  if (!R || ldr < P || !Dw || ldd < P) return set_error("svm_forward: R and Dw are required, with row strides >= P");
  if (Z && ldz < P) return set_error("svm_forward: Z's row stride must be >= P");
  if (epilogue == 0 && (!labels || !classes || !Cp || !Cn || !loss))
    return set_error("svm_forward: the hinge epilogue needs labels, classes, Cp, Cn and loss");
  if (N <= 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  SvmDotArgs d{};
  d.X = X, d.W = W, d.zpart = ws, d.ldx = ldx, d.ldw = ldw, d.N = N, d.F = F, d.P = P;
  const int splits = svm_splits(N, F, &d.chunk);
  d.vec_x = al16(X) && ldx % 4 == 0, d.vec_w = al16(W) && ldw % 4 == 0;
  hipLaunchKernelGGL(svm_dot_kernel, dim3(ceil_div(N, SVM_ROWS), splits), dim3(64), 0, st, d);
  SvmEpiArgs e{};
  e.zpart = ws, e.bias = bias, e.labels = (const long long*)labels, e.classes = (const long long*)classes;
  e.Cp = Cp, e.Cn = Cn, e.Z = Z, e.R = R, e.Dw = Dw, e.ldz = ldz, e.ldr = ldr, e.ldd = ldd;
  e.N = N, e.P = P, e.splits = splits, e.hinge = epilogue == 0;
  e.losspart = ws + (long)splits * N * SVM_P;
  const int nblk = ceil_div(N, SVM_EPI_ROWS);
  hipLaunchKernelGGL(svm_epilogue_kernel, dim3(nblk), dim3(256), 0, st, e);
  if (e.hinge) hipLaunchKernelGGL(svm_loss_kernel, dim3(1), dim3(64), 0, st, e.losspart, nblk, P, loss);
  return hip_check("svm_forward");
}

extern "C" int fer_svm_xtr(const float* X, int64_t ldx, const float* R, int64_t ldr, int N, int F, int P, float* G,
                           int64_t ldg, float* gb, float* ws, int64_t ws_bytes, fer_stream_t stream) {
  if (svm_common("svm_xtr", X, ldx, N, F, P, ws, ws_bytes)) return -1;
  if (!R || ldr < P) return set_error("svm_xtr: R is required, with a row stride >= P");
  if (!G && !gb) return set_error("svm_xtr: no output requested");
  if (G && ldg < F) return set_error("svm_xtr: G's row stride must be >= F");
  if (N <= 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  SvmXtrArgs a{};
  a.X = X, a.R = R, a.ldx = ldx, a.ldr = ldr, a.N = N, a.F = F, a.P = P, a.F4 = ceil_div(F, 4) * 4;
  const int groups = svm_groups(N, &a.gs);
  a.part = ws, a.gbpart = ws + (long)groups * SVM_P * a.F4;
  a.vec_x = al16(X) && ldx % 4 == 0;
  hipLaunchKernelGGL(svm_xtr_kernel, dim3(ceil_div(a.F4, 256), groups), dim3(64), 0, st, a);
  const long threads = (long)P * (a.F4 / 4) + P;
  hipLaunchKernelGGL(svm_xtr_reduce_kernel, dim3(blocks_for(threads)), dim3(256), 0, st, a.part, a.gbpart, groups, P, F,
                     a.F4, G, ldg, G && al16(G) && ldg % 4 == 0, gb);
  return hip_check("svm_xtr");
}
