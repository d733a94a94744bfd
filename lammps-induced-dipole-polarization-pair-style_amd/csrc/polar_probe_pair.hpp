// polar_probe_pair.hpp -- what ONE atom j adds to the Lennard-Jones energy of a test site p and to the LJ force on it: the
// pair arithmetic of k_probe_lj (polar_probe_at.hpp, polar_probe_at() of include/polar_mi355x.h).
//
// Plain C++ with no HIP header behind it, as polar_point_pair.hpp: the device kernel includes it, and so does a host test
// that compares it pair by pair with a 40-digit reference (tests/test_probe_pair_host.py).
//
// With d = x_p - x_j(image), r = |d| and the entry of the packed LJ table (pack_lj_table, polar_input.hpp) of the type pair
// (t_p, t_j) -- cutsq, cut_ljsq, lj1, lj2, lj3, lj4, offset, pad -- the pair of PS.cpp:283-286 / 310-314 (single: PS.cpp:1071 / 1090, pair_host.hpp:332 / 345) with
// factor_lj = 1 (a probe has no bonds):
//      r^2 < cut_ljsq (strict) and r^2 > 0:
//      e_lj += r^-6 (lj3 r^-6 - lj4) - offset
//      f_lj += (lj1 r^-6 - lj2) r^-6 r^-2 d              (FORCE; the force on the probe, -grad_p of the term)
// r2inv = 1.0 / rsq is the IEEE division; r6inv = r2inv r2inv r2inv.
#pragma once

#if defined(__HIPCC__)
#define POLAR_PROBE_FN __host__ __device__ __forceinline__
#else
#define POLAR_PROBE_FN inline
#endif

namespace polar {

#define POLAR_LJ_ENTRY 8   // doubles per type pair of the packed table

// The running sums of one test site (per lane in the kernel).
struct ProbeSums {
  double e, fx, fy, fz;
};

// One atom of type tj, added into the caller's running sums.  `row`: the probe type's row of the packed table, i.e.
// ljpack + POLAR_LJ_ENTRY * t_p * (ntypes + 1).  FORCE = false leaves fx, fy, fz untouched.
// Every sum and product below is rounded as written and every fused multiply-add is spelled out (compiler contraction off
// inside the function): e of a FORCE = false call then has the bits of the FORCE = true one, whatever the compiler would have
// fused in either instance.
template <bool FORCE>
POLAR_PROBE_FN void polar_probe_pair(double dx, double dy, double dz, int tj, const double *row, ProbeSums &s) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double rsq = __builtin_fma(dx, dx, __builtin_fma(dy, dy, dz * dz));
  const double *e = row + POLAR_LJ_ENTRY * tj;
  if (rsq > 0.0 && rsq < e[1]) {
    const double r2inv = 1.0 / rsq;
    const double r6inv = r2inv * r2inv * r2inv;
    s.e += __builtin_fma(r6inv, __builtin_fma(e[4], r6inv, -e[5]), -e[6]);
    if (FORCE) {
      const double fpair = (r6inv * __builtin_fma(e[2], r6inv, -e[3])) * r2inv;
      s.fx = __builtin_fma(fpair, dx, s.fx); s.fy = __builtin_fma(fpair, dy, s.fy); s.fz = __builtin_fma(fpair, dz, s.fz);
    }
  }
}

// What the probe's charge and polarizability make of the field block of the same point (polar_field_at /
// polar_ewald_field_at): e_total = e_static + e_induced, one add per component; e_coul = (q e2s) (phi_static + phi_induced);
// e_pol = -1/2 alpha |e_total|^2.  Contraction off: the grouping is the one written.
POLAR_PROBE_FN void polar_probe_combine(const double es[3], const double ei[3], double ps, double pi, double q, double alpha,
                                        double e2s, double et[3], double &e_coul, double &e_pol) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  et[0] = es[0] + ei[0]; et[1] = es[1] + ei[1]; et[2] = es[2] + ei[2];
  e_coul = (q * e2s) * (ps + pi);
  e_pol = (-0.5 * alpha) * __builtin_fma(et[0], et[0], __builtin_fma(et[1], et[1], et[2] * et[2]));
}

}  // namespace polar
