// Latents pushed along direction vectors (reference `sefa/verify_directions.py:57-58`,
// `data/augment_latents.py:56`: w + step * direction, the direction broadcast over the L layers).
//
//   out[r][l][:] = x[src(r)][l][:] + steps[c % S] * dirs[c / S][l or 0][:]
//
// grid mode (choice == NULL): r = (k*S + s)*n + i, src = i, c = k*S + s: every (direction, step) variant of
// a batch from one launch. choice mode: src(r) = r, c = choice[r]; a value outside [0, K*S) copies the row
// bit for bit and indexes neither dirs nor steps. Nothing is drawn here (no step counter in this code object).
//
// Memory-bound: each element is read once and written once, dirs and steps stay in cache. A thread moves one
// piece of V consecutive floats of a row (V = 4: one 16-byte load and store, when D % 4 == 0 and every
// pointer and stride is 16-byte aligned; V = 1 otherwise), consecutive threads consecutive pieces, in a
// grid-stride loop over the rows*L*D/V pieces. The product and the sum are rounded separately (no FMA), as
// torch's two CPU operators do.
#include "common.h"
#include "fervit_internal.h"

namespace fer {

struct ShiftArgs {
  long ldx, ldo;     // sample strides of x and out, floats
  unsigned pieces;   // rows * L * D / V
  unsigned row_pc;   // pieces per row, L * D / V
  unsigned d_pc;     // pieces per layer, D / V
  unsigned n;        // grid mode: samples of x
  int KS, S, per_layer;
};

// Two roundings. The Makefile compiles this file with -ffp-contract=off: the intrinsics are ordinary * and +
// in the HIP headers, and under hipcc's default contraction mode the pair becomes one v_fma (a pragma here
// does not reach the headers' definitions).
FER_DEV float shift1(float x, float step, float d) { return __fadd_rn(x, __fmul_rn(step, d)); }

// x and out may be the same buffer in choice mode (a piece is read and written by the same thread): no
// __restrict__ on either. The pointers are kernel arguments of their own (global-typed loads and stores; inside
// the struct they would be generic pointers).
template <int V>
__global__ __launch_bounds__(256) void latent_shift_kernel(const float* x, const float* __restrict__ dirs,
                                                           const float* __restrict__ steps,
                                                           const int* __restrict__ choice, float* out, ShiftArgs a) {
  const unsigned stride = gridDim.x * 256u;
  // pieces <= 2^31 - 1 and stride <= 2^19: p + stride does not wrap
  for (unsigned p = blockIdx.x * 256u + threadIdx.x; p < a.pieces; p += stride) {
    const unsigned r = p / a.row_pc, q = p - r * a.row_pc;  // row, piece of the row
    unsigned src = r;
    int c;
    if (choice) {
      c = choice[r];
    } else {
      c = (int)(r / a.n);
      src = r - (unsigned)c * a.n;
    }
    const float* xp = x + (long)src * a.ldx + (long)q * V;
    float* op = out + (long)r * a.ldo + (long)q * V;
    if (c < 0 || c >= a.KS) {  // unchanged: the bits move as they are
      if (V == 4) *(f32x4*)op = *(const f32x4*)xp;
      else *op = *xp;
      continue;
    }
    const int k = c / a.S;
    const float step = steps[c - k * a.S];
    const unsigned dq = a.per_layer ? q : q % a.d_pc;
    const float* dp = dirs + ((long)k * (a.per_layer ? a.row_pc : a.d_pc) + dq) * V;
    if (V == 4) {
      const f32x4 xv = *(const f32x4*)xp, dv = *(const f32x4*)dp;
      *(f32x4*)op = f32x4{shift1(xv[0], step, dv[0]), shift1(xv[1], step, dv[1]), shift1(xv[2], step, dv[2]),
                          shift1(xv[3], step, dv[3])};
    } else {
      *op = shift1(*xp, step, *dp);
    }
  }
}

}  // namespace fer

using namespace fer;

// Blocks of a memory-bound grid-stride launch: what fills every CU's wave slots once (8 blocks of 4 waves
// per CU on 256 CUs); more blocks only queue behind them.
static int shift_grid(long pieces) { return (int)std::max<long>(1, std::min<long>((pieces + 255) / 256, 2048)); }

extern "C" int fer_latent_shift(const float* x, int64_t ldx, const float* dirs, int dir_layers, const float* steps,
                                const int32_t* choice, float* out, int64_t ldo, int64_t n, int K, int S, int L,
                                int D, fer_stream_t stream) {
  if (K < 1) return set_error("latent_shift: K must be >= 1");
  if (S < 1) return set_error("latent_shift: S must be >= 1");
  if (L < 1 || D < 1) return set_error("latent_shift: L and D must be >= 1");
  if (dir_layers != 1 && dir_layers != L) return set_error("latent_shift: dir_layers must be 1 or L");
  if ((long)K * S > 0x7FFFFFFFL) return set_error("latent_shift: K * S does not fit 31 bits");
  const long LD = (long)L * D;
  if (LD > 0x7FFFFFFFL) return set_error("latent_shift: too many elements in a sample");
  if (n <= 0) return 0;
  if (!x || !dirs || !steps || !out) return set_error("latent_shift: x, dirs, steps and out are required");
  if (ldx < LD || ldo < LD) return set_error("latent_shift: a sample stride is below L * D");
  if (n > 0x7FFFFFFFL / LD || (!choice && n * LD > 0x7FFFFFFFL / ((long)K * S)))
    return set_error("latent_shift: too many elements (more than 2^31 - 1 outputs per call)");
  const long rows = choice ? n : n * K * S;
  const bool vec = D % 4 == 0 && ldx % 4 == 0 && ldo % 4 == 0 && al16(x) && al16(out) && al16(dirs);
  const int V = vec ? 4 : 1;
  ShiftArgs a{};
  a.ldx = ldx, a.ldo = ldo;
  a.pieces = (unsigned)(rows * LD / V), a.row_pc = (unsigned)(LD / V), a.d_pc = (unsigned)(D / V);
  a.n = (unsigned)n, a.KS = K * S, a.S = S, a.per_layer = dir_layers == L && L > 1;
  const dim3 grid(shift_grid(a.pieces));
  if (vec) hipLaunchKernelGGL(latent_shift_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, x, dirs, steps,
                          choice, out, a);
  else hipLaunchKernelGGL(latent_shift_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, x, dirs, steps,
                          choice, out, a);
  return hip_check("latent_shift");
}
