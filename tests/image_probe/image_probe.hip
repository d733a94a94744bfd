// image_probe.hip -- TEST INFRASTRUCTURE (tests/test_gpu_closest_image.py compiles it into its tmp_path).
//
// The minimum-image device functions of csrc/polar_common.hpp, called as they are: one thread per pair writes what
// min_image_del, min_image_rint and min_image_rint_w<false / true> return for it.  No image arithmetic of its own.
//
//   out  [n][12]: del of min_image_del | min_image_rint | min_image_rint_w<false> | min_image_rint_w<true>   (x, y, z each)
//   flag [n][2] : what min_image_rint_w<false>, min_image_rint_w<true> returned
#include <hip/hip_runtime.h>

#include "polar_common.hpp"

using polar::Box;

static __global__ __launch_bounds__(256) void k_image_probe(Box box, long long n, const double *__restrict__ pairs,
                                                            double *__restrict__ out, int *__restrict__ flag) {
  const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const double *xi = pairs + 6 * p, *xj = xi + 3;
  double *o = out + 12 * p;
  polar::min_image_del(box, xi[0], xi[1], xi[2], xj[0], xj[1], xj[2], o[0], o[1], o[2]);
  polar::min_image_rint(box, xi[0], xi[1], xi[2], xj[0], xj[1], xj[2], o[3], o[4], o[5]);
  flag[2 * p] = polar::min_image_rint_w<false>(box, xi[0], xi[1], xi[2], xj[0], xj[1], xj[2], o[6], o[7], o[8]) ? 1 : 0;
  flag[2 * p + 1] = polar::min_image_rint_w<true>(box, xi[0], xi[1], xi[2], xj[0], xj[1], xj[2], o[9], o[10], o[11]) ? 1 : 0;
}

// prd[3], tilt[3] = (xy, xz, yz), periodic[3], triclinic: filled as polar_set_box fills the handle's Box (polar_api.hip).
// pairs [n][6] = (xi, xj), out [n][12], flag [n][2] are host arrays.  Returns 0 or the HIP error code.
extern "C" int image_probe_run(const double *prd, const double *tilt, const int *periodic, int triclinic, long long n,
                               const double *pairs, double *out, int *flag) {
  Box b;
  for (int k = 0; k < 3; k++) {
    b.prd[k] = prd[k]; b.half[k] = 0.5 * prd[k]; b.inv[k] = 1.0 / prd[k]; b.periodic[k] = periodic[k] ? 1 : 0;
  }
  b.triclinic = triclinic ? 1 : 0;
  b.xy = triclinic ? tilt[0] : 0.0; b.xz = triclinic ? tilt[1] : 0.0; b.yz = triclinic ? tilt[2] : 0.0;
  if (n <= 0) return 0;
  double *d_pairs = nullptr, *d_out = nullptr;
  int *d_flag = nullptr;
  hipError_t e = hipSuccess;
#define PROBE_TRY(call) if (e == hipSuccess) e = (call)
  PROBE_TRY(hipMalloc(&d_pairs, sizeof(double) * 6 * (size_t)n));
  PROBE_TRY(hipMalloc(&d_out, sizeof(double) * 12 * (size_t)n));
  PROBE_TRY(hipMalloc(&d_flag, sizeof(int) * 2 * (size_t)n));
  PROBE_TRY(hipMemcpy(d_pairs, pairs, sizeof(double) * 6 * (size_t)n, hipMemcpyHostToDevice));
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_image_probe, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, b, n, d_pairs, d_out, d_flag);
    e = hipGetLastError();
  }
  PROBE_TRY(hipDeviceSynchronize());
  PROBE_TRY(hipMemcpy(out, d_out, sizeof(double) * 12 * (size_t)n, hipMemcpyDeviceToHost));
  PROBE_TRY(hipMemcpy(flag, d_flag, sizeof(int) * 2 * (size_t)n, hipMemcpyDeviceToHost));
#undef PROBE_TRY
  if (d_pairs) (void)hipFree(d_pairs);
  if (d_out) (void)hipFree(d_out);
  if (d_flag) (void)hipFree(d_flag);
  return (int)e;
}
