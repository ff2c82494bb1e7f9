// ionode_host.hpp -- host-only helpers shared by the two ABI units (ionode_capi.hip, ionode_grad_capi.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace ionode {

// Compute units of the CALLER's current device (a process may drive several devices, or partitions of one); 256 -- an unpartitioned
// MI355X -- where there is no device: plans are also computed on hosts without a GPU.
inline int compute_units() {
  int dev = 0, n = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1) {
    (void)hipGetLastError();
    return 256;
  }
  return n;
}

}  // namespace ionode
