// math_probe.hip -- TEST INFRASTRUCTURE (tests/test_gpu_math_probe.py compiles it into its tmp_path).
//
// The device arithmetic of the kernels, called as it is: one thread per input writes what the project's own device
// functions return for it.  No arithmetic of its own (the one exception: the pair probe also returns the rsq it hands on,
// dx*dx + dy*dy + dz*dz as polar_force_pair() forms it, so that the test can decide the cutoffs with the same number).
// ExpCoef comes from make_expcoef() on the host and travels as a kernel argument, as in the product kernels; PairMath is
// the product's own struct (polar_rows.hpp).
//
//   math_probe_rsqrt : out [n][3]  = __builtin_amdgcn_rsq (the seed) | rsqrt_pos | rsqrt_pos3
//   math_probe_exp   : out [n][3]  = exp_neg | exp_neg_fast<10> | exp_neg_fast<12>
//   math_probe_tensor: out [n][12] = (s3, s5) of tensor_scalars_lp<0>, <1> | tensor_scalars<0>, <1> | tensor_scalars_k<0>, <1>
//   math_probe_ewald : out [n][3]  = ewald_b1 | b1, b2 of ewald_b12
//   math_probe_pair  : in  [n][17] = d (3) | mu_i (3) | q_i | alpha_i | mu_j (3) | q_j | alpha_j | molok | cut_coulsq | ddcutsq | f_shift
//                      out [n][12] = cd (3) | dd (3) | uef | udd | p (3) | rsq, the first eight started from sentinel[0..7]
//                      and p from sentinel[8]
#include <hip/hip_runtime.h>

#include "polar_common.hpp"
#include "polar_rows.hpp"
#include "polar_solver.hpp"

using polar::ExpCoef;

#define PROBE_THREAD(n)                                                    \
  const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;   \
  if (p >= (n)) return

static __global__ __launch_bounds__(256) void k_probe_rsqrt(long long n, const double *__restrict__ x, double *__restrict__ out) {
  PROBE_THREAD(n);
  out[3 * p] = __builtin_amdgcn_rsq(x[p]);
  out[3 * p + 1] = polar::rsqrt_pos(x[p]);
  out[3 * p + 2] = polar::rsqrt_pos3(x[p]);
}

static __global__ __launch_bounds__(256) void k_probe_exp(ExpCoef K, long long n, const double *__restrict__ x, double *__restrict__ out) {
  PROBE_THREAD(n);
  out[3 * p] = polar::exp_neg(x[p], K);
  out[3 * p + 1] = polar::exp_neg_fast<10>(x[p], K);
  out[3 * p + 2] = polar::exp_neg_fast<12>(x[p], K);
}

static __global__ __launch_bounds__(256) void k_probe_tensor(ExpCoef K, long long n, const double *__restrict__ r2, double pd,
                                                             double *__restrict__ out) {
  PROBE_THREAD(n);
  double *o = out + 12 * p;
  polar::tensor_scalars_lp<0>(r2[p], pd, K, o[0], o[1]);
  polar::tensor_scalars_lp<1>(r2[p], pd, K, o[2], o[3]);
  polar::tensor_scalars<0>(r2[p], pd, o[4], o[5]);
  polar::tensor_scalars<1>(r2[p], pd, o[6], o[7]);
  polar::tensor_scalars_k<0>(r2[p], pd, K, o[8], o[9]);
  polar::tensor_scalars_k<1>(r2[p], pd, K, o[10], o[11]);
}

static __global__ __launch_bounds__(256) void k_probe_ewald(long long n, const double *__restrict__ rsq, double g,
                                                            const int *__restrict__ kept, double *__restrict__ out) {
  PROBE_THREAD(n);
  out[3 * p] = polar::ewald_b1(rsq[p], g, kept[p] != 0);
  polar::ewald_b12(rsq[p], g, kept[p] != 0, out[3 * p + 1], out[3 * p + 2]);
}

struct Sentinel { double v[9]; };

template <bool ALLPAIRS, int DAMP, bool EW>
static __global__ __launch_bounds__(256) void k_probe_pair(ExpCoef K, long long n, const double *__restrict__ in, double pd, double e2s,
                                                           double g_ewald, Sentinel s, double *__restrict__ out) {
  PROBE_THREAD(n);
  const double *a = in + 17 * p;
  double *o = out + 12 * p;
  const polar::PairRow ri = polar::make_pair_row(a[3], a[4], a[5], a[6], a[7], e2s);
  const polar::PairCut cut{a[14], a[15], a[16], pd};
  const polar::PairMath pm{K, g_ewald};
  double cdx = s.v[0], cdy = s.v[1], cdz = s.v[2], ddx = s.v[3], ddy = s.v[4], ddz = s.v[5], uef = s.v[6], udd = s.v[7];
  double px = s.v[8], py = s.v[8], pz = s.v[8];
  polar::polar_force_pair<ALLPAIRS, DAMP, true, EW, true>(pm, a[0], a[1], a[2], ri, a[8], a[9], a[10], a[11], a[12], a[13] != 0.0, cut,
                                                          cdx, cdy, cdz, ddx, ddy, ddz, uef, udd, px, py, pz);
  o[0] = cdx; o[1] = cdy; o[2] = cdz; o[3] = ddx; o[4] = ddy; o[5] = ddz; o[6] = uef; o[7] = udd;
  o[8] = px; o[9] = py; o[10] = pz;
  o[11] = a[0] * a[0] + a[1] * a[1] + a[2] * a[2];
}

namespace {
// copy in, launch once, copy out; returns 0 or the HIP error code
template <class Launch>
int run_probe(long long n, const double *in, int nin, const int *iin, double *out, int nout, Launch launch) {
  if (n <= 0) return 0;
  double *d_in = nullptr, *d_out = nullptr;
  int *d_iin = nullptr;
  hipError_t e = hipSuccess;
#define PROBE_TRY(call) if (e == hipSuccess) e = (call)
  PROBE_TRY(hipMalloc(&d_in, sizeof(double) * nin * (size_t)n));
  PROBE_TRY(hipMalloc(&d_out, sizeof(double) * nout * (size_t)n));
  PROBE_TRY(hipMemcpy(d_in, in, sizeof(double) * nin * (size_t)n, hipMemcpyHostToDevice));
  if (iin) {
    PROBE_TRY(hipMalloc(&d_iin, sizeof(int) * (size_t)n));
    PROBE_TRY(hipMemcpy(d_iin, iin, sizeof(int) * (size_t)n, hipMemcpyHostToDevice));
  }
  if (e == hipSuccess) {
    launch(dim3((unsigned)((n + 255) / 256)), dim3(256), d_in, d_iin, d_out);
    e = hipGetLastError();
  }
  PROBE_TRY(hipDeviceSynchronize());
  PROBE_TRY(hipMemcpy(out, d_out, sizeof(double) * nout * (size_t)n, hipMemcpyDeviceToHost));
#undef PROBE_TRY
  if (d_in) (void)hipFree(d_in);
  if (d_out) (void)hipFree(d_out);
  if (d_iin) (void)hipFree(d_iin);
  return (int)e;
}
}  // namespace

extern "C" int math_probe_rsqrt(long long n, const double *x, double *out) {
  return run_probe(n, x, 1, nullptr, out, 3, [&](dim3 g, dim3 b, const double *in, const int *, double *o) {
    hipLaunchKernelGGL(k_probe_rsqrt, g, b, 0, 0, n, in, o);
  });
}

extern "C" int math_probe_exp(long long n, const double *x, double *out) {
  const ExpCoef K = polar::make_expcoef();
  return run_probe(n, x, 1, nullptr, out, 3, [&](dim3 g, dim3 b, const double *in, const int *, double *o) {
    hipLaunchKernelGGL(k_probe_exp, g, b, 0, 0, K, n, in, o);
  });
}

extern "C" int math_probe_tensor(long long n, const double *r2, double pd, double *out) {
  const ExpCoef K = polar::make_expcoef();
  return run_probe(n, r2, 1, nullptr, out, 12, [&](dim3 g, dim3 b, const double *in, const int *, double *o) {
    hipLaunchKernelGGL(k_probe_tensor, g, b, 0, 0, K, n, in, pd, o);
  });
}

extern "C" int math_probe_ewald(long long n, const double *rsq, double g_ewald, const int *kept, double *out) {
  return run_probe(n, rsq, 1, kept, out, 3, [&](dim3 g, dim3 b, const double *in, const int *k, double *o) {
    hipLaunchKernelGGL(k_probe_ewald, g, b, 0, 0, n, in, g_ewald, k, o);
  });
}

extern "C" int math_probe_pair(int allpairs, int damp, int ew, long long n, const double *in, double pd, double e2s, double g_ewald,
                               const double *sentinel, double *out) {
  const ExpCoef K = polar::make_expcoef();
  Sentinel s;
  for (int k = 0; k < 9; k++) s.v[k] = sentinel[k];
  return run_probe(n, in, 17, nullptr, out, 12, [&](dim3 g, dim3 b, const double *i, const int *, double *o) {
#define PROBE_PAIR(A, D, E) hipLaunchKernelGGL((k_probe_pair<A, D, E>), g, b, 0, 0, K, n, i, pd, e2s, g_ewald, s, o)
    if (allpairs) {
      if (damp == 0) { if (ew) PROBE_PAIR(true, 0, true); else PROBE_PAIR(true, 0, false); }
      else           { if (ew) PROBE_PAIR(true, 1, true); else PROBE_PAIR(true, 1, false); }
    } else {
      if (damp == 0) { if (ew) PROBE_PAIR(false, 0, true); else PROBE_PAIR(false, 0, false); }
      else           { if (ew) PROBE_PAIR(false, 1, true); else PROBE_PAIR(false, 1, false); }
    }
#undef PROBE_PAIR
  });
}
