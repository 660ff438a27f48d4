// Device-side step counter for graph-replayed training steps (fer_set_step_counter): a captured
// launch keeps its host seed, so every dropout kernel mixes the current step into it (step_seed).
//
// Each .hip file is its own code object and has its own copy of the pointer (null = no counter).
// This header is the only way to obtain step_seed, and including it is all a file has to do:
// the registrar below hands this code object's setter to the registry in capi.cpp when the
// library is loaded (no HIP call is made then), and fer_set_step_counter walks the registry.
// Include it only from files whose kernels call step_seed.
#pragma once
#include "common.h"
#include "fervit_internal.h"

// The setter below names the variable on the host, so the compiler gives it a global symbol in this
// code object and keeps it whatever the kernels do: that is what hipMemcpyToSymbol looks up. (Not
// __attribute__((used)): a static device variable marked so stays a local symbol, which the runtime
// cannot find, and kernels then address it directly instead of through the GOT.)
static __device__ const uint64_t* fer_step_ptr = nullptr;
FER_DEV uint64_t step_seed(uint64_t seed) {
  const uint64_t* p = fer_step_ptr;
  if (!p) return seed;
  // global-typed load (a generic pointer compiles to a flat load: vmcnt AND lgkmcnt waits)
  const uint64_t c = *(const __attribute__((address_space(1))) uint64_t*)(const void*)p;
  uint64_t z = seed ^ (c * 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// A non-dropout draw under the same counter (mixup.hip): the seed mixed with the step, then stream `s` of it by
// the same finaliser (s takes the counter's place), so related seeds and neighbouring streams share nothing.
// Kept apart from the dropout call sites, whose table and per-kernel cases are tests/test_gpu_step_seed_kernels.py;
// a kernel that draws through this helper brings its own counter test (tests/test_gpu_mixup_kernels.py).
FER_DEV uint64_t step_stream_seed(uint64_t seed, uint64_t s) {
  uint64_t z = step_seed(seed) ^ (s * 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

namespace fer {
// host side, per code object
static hipError_t set_step_ptr_here(const uint64_t* p) {
  return hipMemcpyToSymbol(HIP_SYMBOL(fer_step_ptr), &p, sizeof(p));
}
static const struct StepPtrRegistrar {
  StepPtrRegistrar() { register_step_ptr_setter(&set_step_ptr_here); }
} g_step_ptr_registrar;
}  // namespace fer
