// Internal host/device declarations shared by the kernel translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <stdint.h>

#include "../../include/fervit.h"

namespace fer {

typedef fer_epilogue EpiArgs;
typedef fer_gemm_desc GemmDesc;

struct GemmArgs {
  const void* A;
  const void* B;
  long lda, ldb;
  int M, N, K;
  int tiles_m, tiles_n;
  int splits, k_chunk, partial;
  float* ws;
  float* cs_part;  // fused column sums: per-tile partials [tiles_m][N] (or null)
  int* tq;               // persistent 8-phase kernel: work-queue counters (common.h wq_*), null = fixed stride
  unsigned tq_base[8];   // their values at launch
};

int set_error(const char* msg);
// step_seed.h hands each including code object's setter of its device step-counter pointer to the
// registry that fer_set_step_counter walks (capi.cpp); called from static constructors, no HIP call
void register_step_ptr_setter(hipError_t (*set)(const uint64_t*));
int hip_check(const char* what);
// persistent GEMM / attention kernels: walk a fixed blockIdx stride instead of the work queue
// (fer_set_persistent_mode(1))
bool fixed_stride_mode();
// compute units of the current device (256 when the query fails), asked once per process
int num_cus();
int gemm_launch(const GemmDesc& d, const EpiArgs& e, hipStream_t st);
inline int ceil_div(long a, long b);
// out_k[c % seg] (+)= scale * sum_b part[b*ld + c]  (deterministic, reduce.hip)
void part_reduce(const float* part, int nb, long ld, int ncols, int seg, float* o0, float* o1, float* o2,
                 int accumulate, const float* scale, hipStream_t st);
// Workspace for column partials that part_reduce will sum: inside fer_reduce_defer's window (same
// stream, a shape the batched reduction takes) a slice of the deferral arena, else ws itself (reduce.hip)
float* reduction_ws(float* ws, size_t bytes, int ncols, hipStream_t st);

inline int ceil_div(long a, long b) { return (int)((a + b - 1) / b); }

// Dropout element indices are 32-bit (common.h fer_hash): a dropout site covers < 2^32 elements.
inline int check_drop_range(uint32_t thresh, long elements, const char* what) {
  if (thresh && elements > 0xFFFFFFFFL) return set_error(what);
  return 0;
}

// Host checks of the operators that move rows in 16-byte pieces (convbn.hip, attnpool.hip).
inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
// a [rows][C] operand read or written in 16-byte pieces
inline bool piece_ok(const void* p, int64_t ld, int C, int V) { return p && al16(p) && ld >= C && ld % V == 0; }
inline int blocks_for(long n) { return (int)((n + 255) / 256); }
// blocks of 256 threads for a grid-stride loop over n items (vit_edge.hip, wplus.hip, optim.hip)
inline int grid_for(long n) { return (int)std::max<long>(1, std::min<long>((n + 255) / 256, 8192)); }
// one thread per work item, 256 per block: the block count must fit the grid's 31 bits
inline bool too_many(long n) { return n > 0x7FFFFFFFL * 256; }
// elements of a 16-byte piece
inline int piece_len(int dtype) { return dtype == FER_BF16 ? 8 : 4; }

// The ABI's dtype code. Every entry point that takes one starts with
//   if (check_dtype(dtype, "<entry>: unknown dtype")) return -1;
// (before its empty-shape returns), and launches a kernel template on the element type through
//   with_dtype(dtype, [&](auto tag) { using T = typename decltype(tag)::type; ... k<T> ... (const T*)x ... });
// so each launch and its argument list is written once. Branches that select a bf16-only or fp32-only
// kernel (not an element type) stay ordinary ifs.
inline int check_dtype(int dtype, const char* msg) {
  return dtype == FER_BF16 || dtype == FER_F32 ? 0 : set_error(msg);
}
template <typename T> struct DtypeTag { typedef T type; };
template <typename F>
inline void with_dtype(int dtype, F&& f) {  // dtype has passed check_dtype
  if (dtype == FER_BF16) f(DtypeTag<__bf16>{});
  else f(DtypeTag<float>{});
}

// A run-time integer that selects a template instantiation (attention's NB and dh variants, the
// GEMM epilogue kinds):
//   dispatch_int<1, 2, 3>(v, [&](auto I) { constexpr int NB = decltype(I)::value; ... k<NB> ... });
// calls f with the listed value equal to v; false when none is (f did not run). A left fold, so that f's
// instantiations, and with them the kernels of the code object, come out in list order (a right fold
// emits them reversed; the ViT-B step measured 0.09 ms slower with the attention and GEMM kernels laid
// out in that order, DESIGN.md section 4 "Host dispatch").
template <int V> struct IntTag { static constexpr int value = V; };
template <int... Vs, typename F>
inline bool dispatch_int(int v, F&& f) {
  return (... || (v == Vs && (f(IntTag<Vs>{}), true)));
}

}  // namespace fer
