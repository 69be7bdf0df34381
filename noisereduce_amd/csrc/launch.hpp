// The one way to launch a kernel with dynamic LDS.  Holds no kernels: every unit that launches includes it.
#pragma once
#include <hip/hip_runtime.h>

namespace sg {
namespace host {

// Raises the kernel's dynamic-LDS limit once per (device, kernel, size): the runtime call costs microseconds of host
// time, and a short call enqueues ten launches (create.hip)
hipError_t set_lds(const void* kern, size_t bytes);

// One kernel launch with `lds` bytes of dynamic LDS.  `raise`: the size may exceed the 64 KiB a kernel gets without asking
// (set_lds first); a caller that knows its size is below passes false and saves the mutex and the map lookup.
template <typename... KA, typename... A>
static hipError_t launch_lds_if(bool raise, void (*kern)(KA...), dim3 grid, dim3 block, size_t lds, hipStream_t st, const A&... a) {
  if (raise) {
    hipError_t e = set_lds(reinterpret_cast<const void*>(kern), lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(kern, grid, block, lds, st, a...);
  return hipGetLastError();
}
template <typename... KA, typename... A>
static hipError_t launch_lds(void (*kern)(KA...), dim3 grid, dim3 block, size_t lds, hipStream_t st, const A&... a) {
  return launch_lds_if(true, kern, grid, block, lds, st, a...);
}

}  // namespace host
}  // namespace sg
