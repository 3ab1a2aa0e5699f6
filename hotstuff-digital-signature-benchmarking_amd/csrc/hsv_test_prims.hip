// Test kernels of libhsv_test.so (never linked into libhsv.so): the one-lane
// field, scalar and lattice primitives on raw operands, one item per lane, so
// that tests/test_prims_gpu.py can compare what the device computes -- the
// inline-asm branches of hsv_fe26x10.hpp, the hardware reciprocal and the wave
// votes of hsv_lattice.hpp -- with big integers and with the host build of the
// same text (csrc/hsv_test_prims.hpp).
#include <hip/hip_runtime.h>

#include "hsv_internal.h"
#include "hsv_test_prims.hpp"

namespace hsv {

// Lanes past n take the last item and store nothing: no lane returns early,
// because lattice_reduce votes across the wave and fe_select ballots.
__global__ void __launch_bounds__(64) hsv_test_field_ops_kernel(const uint32_t *__restrict__ in, uint32_t n,
                                                                uint32_t *__restrict__ out) {
  const uint32_t id = blockIdx.x * 64u + threadIdx.x;
  const uint32_t item = id < n ? id : n - 1u;
  uint32_t rec[kPrimFieldIn], res[kPrimFieldOut];
  HSV_UNROLL
  for (int i = 0; i < kPrimFieldIn; ++i) rec[i] = in[(uint64_t)item * kPrimFieldIn + i];
  HSV_UNROLL
  for (int i = 0; i < kPrimFieldOut; ++i) res[i] = 0;
  prim_field_op(rec, item, res);
  if (id < n) {
    HSV_UNROLL
    for (int i = 0; i < kPrimFieldOut; ++i) out[(uint64_t)id * kPrimFieldOut + i] = res[i];
  }
}

__global__ void __launch_bounds__(64) hsv_test_scalar_ops_kernel(const uint32_t *__restrict__ in, uint32_t n,
                                                                 uint32_t *__restrict__ out) {
  const uint32_t id = blockIdx.x * 64u + threadIdx.x;
  const uint32_t item = id < n ? id : n - 1u;
  uint32_t rec[kPrimScalarIn], res[kPrimScalarOut];
  HSV_UNROLL
  for (int i = 0; i < kPrimScalarIn; ++i) rec[i] = in[(uint64_t)item * kPrimScalarIn + i];
  HSV_UNROLL
  for (int i = 0; i < kPrimScalarOut; ++i) res[i] = 0;
  prim_scalar_op(rec, res);
  if (id < n) {
    HSV_UNROLL
    for (int i = 0; i < kPrimScalarOut; ++i) out[(uint64_t)id * kPrimScalarOut + i] = res[i];
  }
}

}  // namespace hsv

namespace {

// n host records of win words through `kernel` on the current device's null
// stream, wout words back per record; 0 or a hipError_t
int run_ops(void (*kernel)(const uint32_t *, uint32_t, uint32_t *), const uint32_t *in, uint32_t n, uint32_t *out,
            size_t win, size_t wout) {
  if (n == 0) return 0;
  struct Pause {  // a device-wide wait and frees below
    Pause() { hsvi_resident_pause(1); }
    ~Pause() { hsvi_resident_pause(0); }
  } pause;
  uint32_t *d_in = nullptr, *d_out = nullptr;
  hipError_t e = hipMalloc(&d_in, (size_t)n * win * 4);
  if (e == hipSuccess) e = hipMalloc(&d_out, (size_t)n * wout * 4);
  if (e == hipSuccess) e = hipMemcpy(d_in, in, (size_t)n * win * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(d_out, 0, (size_t)n * wout * 4);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(kernel, dim3((n + 63u) / 64u), dim3(64), 0, 0, d_in, n, d_out);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, d_out, (size_t)n * wout * 4, hipMemcpyDeviceToHost);
  if (d_in) (void)hipFree(d_in);
  if (d_out) (void)hipFree(d_out);
  return (int)e;
}

}  // namespace

extern "C" int hsvi_test_field_ops(const uint32_t *in, uint32_t n, uint32_t *out) {
  return run_ops(hsv::hsv_test_field_ops_kernel, in, n, out, hsv::kPrimFieldIn, hsv::kPrimFieldOut);
}

extern "C" int hsvi_test_scalar_ops(const uint32_t *in, uint32_t n, uint32_t *out) {
  return run_ops(hsv::hsv_test_scalar_ops_kernel, in, n, out, hsv::kPrimScalarIn, hsv::kPrimScalarOut);
}
