// TEST INFRASTRUCTURE: the device build of the kernel entry points (harness_entries.hpp), for the GPU half of
// tests/test_kernels_emulated.py and for tests/test_gpu_encoder_kernels.py.  Compiled by hipcc for gfx950 and linked against
// the product's own kernel objects (build_device.py), so the machine code under test is the code libvp_hip.so ships.
// Every pointer a kernel reads or writes is device memory (staged by the Python backend); each entry point waits for the
// device and returns the first error: the launch's own, else what the synchronisation reports.
#include <hip/hip_runtime.h>

#include "act_io.hpp"

static hipError_t harness_done(hipError_t e) {
  const hipError_t s = hipDeviceSynchronize();
  return e != hipSuccess ? e : s;
}

static const float* harness_ones() {
  static float* d = nullptr;
  if (!d) {
    float h[4096];
    for (float& v : h) v = 1.0f;
    float* p = nullptr;
    if (hipMalloc(&p, sizeof(h)) != hipSuccess) return nullptr;
    if (hipMemcpy(p, h, sizeof(h), hipMemcpyHostToDevice) != hipSuccess) {
      (void)hipFree(p);
      return nullptr;
    }
    d = p;
  }
  return d;
}

static unsigned* harness_minmax_seed() {
  static unsigned* d = nullptr;
  if (!d && hipMalloc(&d, 2 * sizeof(unsigned)) != hipSuccess) return d = nullptr;
  const unsigned h[2] = {0xFFFFFFFFu, 0u};
  if (hipMemcpy(d, h, sizeof(h), hipMemcpyHostToDevice) != hipSuccess) return nullptr;
  return d;
}

#include "harness_entries.hpp"
