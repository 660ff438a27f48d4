// C ABI glue: error state and the GEMM entry point.
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

// ---------------------------------------------------------------- evaluation metrics (kernels: metrics.hip)
extern "C" int fer_cls_stats(const float* logits, int64_t ld, const int64_t* labels, int B, int C, int64_t* preds,
                             float* conf, float* probs, int64_t ld_probs, int64_t* confusion, int64_t* counters,
                             fer_stream_t stream) {
  if (C < 1) return fer::set_error("cls_stats: C must be >= 1");
  if (!logits || !labels) return fer::set_error("cls_stats: logits and labels are required");
  if (ld < C) return fer::set_error("cls_stats: the logits' row stride must be >= C");
  if (probs && ld_probs < C) return fer::set_error("cls_stats: the probabilities' row stride must be >= C");
  if (B <= 0) return 0;
  if (fer::too_many((long)B * 64)) return fer::set_error("cls_stats: B is too large for one launch");
  fer::cls_stats_launch(logits, ld, labels, B, C, preds, conf, probs, ld_probs, confusion, counters, (hipStream_t)stream);
  return fer::hip_check("cls_stats");
}

extern "C" int fer_cls_report(const int64_t* confusion, int C, double* out, fer_stream_t stream) {
  if (C < 1) return fer::set_error("cls_report: C must be >= 1");
  if (!confusion || !out) return fer::set_error("cls_report: confusion and out are required");
  fer::cls_report_launch(confusion, C, out, (hipStream_t)stream);
  return fer::hip_check("cls_report");
}

extern "C" int fer_token_cosine(int dtype, const void* tokens, int64_t ld, int B, int N, int D, float eps,
                                float* cls_sim, int64_t ld_cls, float* tok_sim, int64_t ld_tok, fer_stream_t stream) {
  if (fer::check_dtype(dtype, "token_cosine: unknown dtype")) return -1;
  if (N < 2) return fer::set_error("token_cosine: N must be >= 2 (row 0 and at least one more token)");
  const int V = fer::piece_len(dtype);
  if (D < 1 || D % (dtype == FER_BF16 ? 32 : 4))
    return fer::set_error("token_cosine: D must be a positive multiple of 32 (bf16: one MFMA step) or 4 (fp32)");
  if (!fer::piece_ok(tokens, ld, D, V))
    return fer::set_error("token_cosine: tokens need 16-byte aligned rows (stride >= D, a multiple of 8 bf16 / 4 fp32)");
  if (!cls_sim && !tok_sim) return fer::set_error("token_cosine: no output requested");
  if ((cls_sim && ld_cls < N - 1) || (tok_sim && ld_tok < N - 1))
    return fer::set_error("token_cosine: an output's row stride must be >= N - 1");
  if (!(eps >= 0.f)) return fer::set_error("token_cosine: eps must be >= 0");
  if (B <= 0) return 0;
  if (B > 65535 || N > 65535) return fer::set_error("token_cosine: B or N is above the launch grid's limit");
  fer::token_cosine_launch(dtype, tokens, ld, B, N, D, eps, cls_sim, ld_cls, tok_sim, ld_tok, (hipStream_t)stream);
  return fer::hip_check("token_cosine");
}

// ---------------------------------------------------------------- linear-SVM passes (kernels: svm.hip)
extern "C" int fer_svm_slab(void) { return FER_SVM_SLAB; }
extern "C" int fer_svm_max_groups(void) { return FER_SVM_MAX_GROUPS; }
extern "C" int64_t fer_svm_ws(int N, int F) { return N > 0 && F > 0 ? fer::svm_ws_bytes(N, F) : 0; }

// what both passes ask of X, the shape and the workspace; `what` is the entry's name
static int svm_common(const char* what, const float* X, int64_t ldx, int N, int F, int P, const float* ws,
                      int64_t ws_bytes) {
  char msg[160];
  const char* bad = nullptr;
  if (F < 1) bad = "F must be >= 1";
  else if (P < 1 || P > 8) bad = "P must be 1..8 columns per launch";
  else if (!X || ldx < F) bad = "X is required, with a row stride >= F";
  else if (N > 0 && (!ws || !fer::al16(ws) || ws_bytes < fer::svm_ws_bytes(N, F)))
    bad = "the workspace must be 16-byte aligned and hold fer_svm_ws(N, F) bytes";
  if (!bad) return 0;
  snprintf(msg, sizeof(msg), "%s: %s", what, bad);
  return fer::set_error(msg);
}

extern "C" int fer_svm_forward(const float* X, int64_t ldx, const float* W, int64_t ldw, const float* bias, int N,
                               int F, int P, int epilogue, const int64_t* labels, const int64_t* classes,
                               const float* Cp, const float* Cn, float* Z, int64_t ldz, float* R, int64_t ldr,
                               float* Dw, int64_t ldd, float* loss, float* ws, int64_t ws_bytes, fer_stream_t stream) {
  if (svm_common("svm_forward", X, ldx, N, F, P, ws, ws_bytes)) return -1;
  if (epilogue != 0 && epilogue != 1) return fer::set_error("svm_forward: epilogue must be 0 (hinge) or 1 (scale)");
  if (!W || ldw < F || !bias) return fer::set_error("svm_forward: W (row stride >= F) and bias are required");
  if (!R || ldr < P || !Dw || ldd < P) return fer::set_error("svm_forward: R and Dw are required, with row strides >= P");
  if (Z && ldz < P) return fer::set_error("svm_forward: Z's row stride must be >= P");
  if (epilogue == 0 && (!labels || !classes || !Cp || !Cn || !loss))
    return fer::set_error("svm_forward: the hinge epilogue needs labels, classes, Cp, Cn and loss");
  if (N <= 0) return 0;
  fer::svm_forward_launch(X, ldx, W, ldw, bias, N, F, P, epilogue == 0, labels, classes, Cp, Cn, Z, ldz, R, ldr, Dw, ldd,
                          loss, ws, (hipStream_t)stream);
  return fer::hip_check("svm_forward");
}

extern "C" int fer_svm_xtr(const float* X, int64_t ldx, const float* R, int64_t ldr, int N, int F, int P, float* G,
                           int64_t ldg, float* gb, float* ws, int64_t ws_bytes, fer_stream_t stream) {
  if (svm_common("svm_xtr", X, ldx, N, F, P, ws, ws_bytes)) return -1;
  if (!R || ldr < P) return fer::set_error("svm_xtr: R is required, with a row stride >= P");
  if (!G && !gb) return fer::set_error("svm_xtr: no output requested");
  if (G && ldg < F) return fer::set_error("svm_xtr: G's row stride must be >= F");
  if (N <= 0) return 0;
  fer::svm_xtr_launch(X, ldx, R, ldr, N, F, P, G, ldg, gb, ws, (hipStream_t)stream);
  return fer::hip_check("svm_xtr");
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
