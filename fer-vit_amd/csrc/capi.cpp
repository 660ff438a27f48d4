// C ABI glue: error state, the process-wide settings (persistent mode, step counter), streams and the
// GEMM entry point. Every other entry point stands beside its kernels.
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fervit_internal.h"

namespace fer {

static thread_local char g_err[512] = "";

int set_error(const char* msg) {
  snprintf(g_err, sizeof(g_err), "%s", msg);
  return -1;
}

int hip_check(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
    return -2;
  }
  return 0;
}

static int g_fixed_stride = [] {  // fer_set_persistent_mode; FERVIT_FIXED_STRIDE=1 at start-up (fervit.h)
  const char* v = getenv("FERVIT_FIXED_STRIDE");
  return v && v[0] == '1' ? 1 : 0;
}();

bool fixed_stride_mode() { return g_fixed_stride == 1; }

int num_cus() {
  static const int n = [] {
    int dev = 0, c = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
      c = 256;
    return c > 0 ? c : 256;
  }();
  return n;
}

// Step-counter setters, one per code object that includes step_seed.h, registered by static
// constructors at load: a function-local, constant-initialised array (no heap, valid whichever
// translation unit's constructors run first). n counts every registration, kept or not.
constexpr int kStepSetters = 32;
struct StepSetters {
  hipError_t (*set[kStepSetters])(const uint64_t*);
  int n;
};
static StepSetters& step_setters() {
  static StepSetters s = {};
  return s;
}
void register_step_ptr_setter(hipError_t (*set)(const uint64_t*)) {
  StepSetters& s = step_setters();
  if (s.n < kStepSetters) s.set[s.n] = set;
  ++s.n;
}

}  // namespace fer

extern "C" int fer_set_persistent_mode(int mode) {
  if (mode < 0 || mode > 1) return fer::set_error("set_persistent_mode: mode must be 0 (work queue) or 1 (fixed stride)");
  fer::g_fixed_stride = mode;
  return 0;
}

extern "C" const char* fer_last_error(void) { return fer::g_err; }
extern "C" const char* fer_version(void) { return "fervit-mi355x 0.1 (gfx950)"; }

extern "C" int fer_gemm(const fer_gemm_desc* d, const fer_epilogue* e, fer_stream_t stream) {
  if (!d || !e) return fer::set_error("gemm: null descriptor");
  if (fer::check_dtype(d->dtype, "gemm: unknown dtype")) return -1;
  return fer::gemm_launch(*d, *e, (hipStream_t)stream);
}

extern "C" int fer_set_step_counter(const uint64_t* counter) {
  // every code object that has dropout kernels keeps its own copy of the pointer (step_seed.h)
  const fer::StepSetters& s = fer::step_setters();
  if (s.n > fer::kStepSetters) return fer::set_error("set_step_counter: more code objects than the registry holds");
  for (int i = 0; i < s.n; ++i)
    if (s.set[i](counter) != hipSuccess) return fer::set_error("set_step_counter: hipMemcpyToSymbol failed");
  return 0;
}

extern "C" int fer_stream_create_cu_mask(const uint32_t* mask, int nwords, int priority, fer_stream_t* out) {
  if (!out || nwords < 0 || (nwords > 0 && !mask)) return fer::set_error("stream_create_cu_mask: bad arguments");
  // hipExtStreamCreateWithCUMask has neither a priority nor a flags argument: refuse a priority it
  // would silently drop (the masked stream is created blocking, at the default priority)
  if (nwords > 0 && priority != 0) return fer::set_error("stream_create_cu_mask: priority must be 0 with a CU mask");
  hipStream_t s = nullptr;
  hipError_t e = nwords == 0 ? hipStreamCreateWithPriority(&s, hipStreamNonBlocking, priority)
                             : hipExtStreamCreateWithCUMask(&s, (uint32_t)nwords, mask);
  if (e != hipSuccess) {
    char msg[160];
    snprintf(msg, sizeof(msg), "stream_create_cu_mask: %s", hipGetErrorString(e));
    return fer::set_error(msg);
  }
  *out = (fer_stream_t)s;
  return 0;
}

extern "C" int fer_stream_destroy(fer_stream_t s) {
  if (s && hipStreamDestroy((hipStream_t)s) != hipSuccess) return fer::set_error("stream_destroy failed");
  return 0;
}
