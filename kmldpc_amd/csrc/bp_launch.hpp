// bp_launch.hpp — the host-side launch layer the BP kernel families share
// (bp.hip, bp_regular.hip, bp_regular_f32.hip, bp_irregular.hip, bp_coop.hip).
// Host code only: nothing here is compiled into a kernel.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace kml {

constexpr size_t kLdsLimit = 160 * 1024;  // LDS of one gfx950 CU = the most one workgroup can take

// CUs of the current device (asked on every call, never cached).
inline int device_cus() {
  int dev = 0, ncu = 0;
  hipGetDevice(&dev);
  hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev);
  return ncu;
}

// The two steps every BP launch starts with, cooperative ones included.
inline hipError_t set_dynamic_lds(const void *kern, size_t lds) {
  return hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}
inline hipError_t reset_queue(const BpLaunch &a, hipStream_t s) {
  return hipMemsetAsync(a.queue, 0, sizeof(unsigned int), s);
}

constexpr long long kNoGridCap = -1;

// Persistent-grid launch: min(CUs * wgs_per_cu, grid_cap, a.B) workgroups of
// `block` threads that pull codewords from a.queue until it runs past a.B.
// count_static_lds: the kernel's static LDS (the PROF instances' tallies)
// counts against kLdsLimit too, hipErrorNotSupported when it does not fit.
// args are the kernel's own arguments, checked against its signature here.
template <class Kern, class... Args>
hipError_t launch_persistent(Kern kern, int block, size_t lds, int wgs_per_cu, long long grid_cap,
                             bool count_static_lds, const BpLaunch &a, hipStream_t s, const Args &...args) {
  hipError_t e;
  if (count_static_lds) {
    hipFuncAttributes fa;
    e = hipFuncGetAttributes(&fa, (const void *)kern);
    if (e != hipSuccess) return e;
    if (lds + fa.sharedSizeBytes > kLdsLimit) return hipErrorNotSupported;
  }
  e = set_dynamic_lds((const void *)kern, lds);
  if (e != hipSuccess) return e;
  long long grid = (long long)device_cus() * wgs_per_cu;
  if (grid_cap != kNoGridCap) {
    if (grid > grid_cap) grid = grid_cap;
    if (grid < 1) return hipErrorInvalidValue;
  }
  if (grid > a.B) grid = a.B;
  e = reset_queue(a, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(block), lds, s, args...);
  return hipGetLastError();
}

// The FAST launch over the batch, then the EXACT launch over the codewords it
// deferred (usually none: its workgroups read a zero count and leave).  Both
// are callables taking the BpLaunch to run.
template <class Fast, class Exact>
hipError_t launch_fast_then_exact(const BpLaunch &a, hipStream_t s, Fast fast_launch, Exact exact_launch) {
  if (!a.defer_idx || !a.defer_cnt) return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(a.defer_cnt, 0, sizeof(unsigned), s);
  if (e != hipSuccess) return e;
  e = fast_launch(a);
  if (e != hipSuccess) return e;
  BpLaunch b = a;
  b.cw_idx = a.defer_idx;
  b.B_dev = a.defer_cnt;
  return exact_launch(b);
}

// Can a run the PROF instances of a family?  extra_ok: the family's own limit.
inline hipError_t prof_launch_check(const BpLaunch &a, bool extra_ok = true) {
  if (a.syn || !a.ref_bits || a.iter_count < 1) return hipErrorInvalidValue;
  if (a.iter_count > kBpProfMaxIter || !extra_ok) return hipErrorNotSupported;
  return hipSuccess;
}

}  // namespace kml
