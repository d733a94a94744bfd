// polar_point_pair.hpp -- what ONE atom j adds to the field and the potential of the polarized box at a point p: the pair
// arithmetic of k_field_at (polar_field_at.hpp, polar_field_at() of include/polar_mi355x.h).
//
// Plain C++ with no HIP header behind it, as polar_force_pair.hpp: the device kernel includes it, and so does a host test
// that compares it pair by pair with a 40-digit reference (tests/test_point_pair_host.py).  The square root and the
// exponential come from a policy `M` (device: PairMath of polar_rows.hpp, whose bounds are in the ledger of DESIGN
// section 4; host: libm).
//
// With d = x_p - x_j(image), r = |d|, rc = cut_coul:
//
//  static part, the sum of k_static_field (PS.cpp:324-361) taken at a point: r^2 <= rc^2 (note <=, PS.cpp:342) and the
//  molecule rule `mol_p != mol_j || mol_p == 0`.  Without the factor e2s = sqrt(qqrd2e), which the caller applies to the sums:
//      e_static   += q_j (1/r^2 - 1/rc^2) d / r
//      phi_static += q_j (1/r + r/rc^2 - 2/rc)          (-grad phi_static = e_static; zero at r = rc)
//
//  induced part, the field of the dipole mu_j through the style's tensor T = s3 I - s5 d d^T (PS.cpp:1284-1306, s3 = damp1 / r^3,
//  s5 = 3 damp2 / r^5; with damping `none` 1 / r^3 and 3 / r^5): every pair (ALLPAIRS) or r^2 < dd_cutoff^2 (strict, as the
//  sweep), no molecule rule (PS.cpp:512-602 has none):
//      e_induced   += -(s3 mu_j - s5 (mu_j.d) d)
//      phi_induced += s3 (mu_j.d)                        (-grad phi_induced = e_induced, damped or not)
//  A record with alpha_j == 0 may hold a stale dipole (see polar_force_pair.hpp): it takes no part.
//
// An atom at r^2 == 0 adds nothing.
#pragma once

#if defined(__HIPCC__)
#define POLAR_PAIR_FN __host__ __device__ __forceinline__
#else
#define POLAR_PAIR_FN inline
#endif
#define POLAR_POINT_FMA(a, b, c) __builtin_fma(a, b, c)   // one rounding: v_fma_f64 on the device, fma() of libm on a host without the instruction

namespace polar {

// The settings a point pair needs.
struct PointCut {
  double cut_coulsq;     // static part: rsq <= cut_coulsq
  double ddcutsq;        // induced part: rsq < ddcutsq, or every pair (ALLPAIRS)
  double rc2inv;         // 1 / cut_coulsq
  double two_rcinv;      // 2 / cut_coul
  double pd;             // polar_damp
};

// The running sums of one point (per lane in the kernel).  esx..esz and ps lack the factor e2s.
struct PointSums {
  double esx, esy, esz, ps;   // e_static / e2s, phi_static / e2s
  double eix, eiy, eiz, pi;   // e_induced, phi_induced
};

// One atom, added into the caller's running sums -- each part inside its own (lane-divergent) condition.
// PHI = false leaves ps and pi untouched (a field-only call does not pay for the potentials).
// molok: the point carries no molecule id, or another one than atom j.  (mjx, mjy, mjz), qj, aj: the atom's dipole, charge, alpha.
// Every sum and product below is rounded as written and every fused multiply-add is spelled out (compiler contraction off inside the
// function): the field of a PHI = false call then has the bits of the PHI = true one, whatever the compiler would have fused in
// either instance.
template <bool ALLPAIRS, int DAMP, bool PHI, class M>
POLAR_PAIR_FN void polar_point_pair(const M &m, double dx, double dy, double dz, double qj, double mjx, double mjy, double mjz,
                                    double aj, bool molok, const PointCut &c, PointSums &s) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double rsq = POLAR_POINT_FMA(dx, dx, POLAR_POINT_FMA(dy, dy, dz * dz));
  if (rsq > 0.0) {
    const double rinv = m.rsqrt(rsq);
    const double r2inv = rinv * rinv;
    if (rsq <= c.cut_coulsq && molok) {
      const double t = ((r2inv - c.rc2inv) * rinv) * qj;
      s.esx = POLAR_POINT_FMA(t, dx, s.esx); s.esy = POLAR_POINT_FMA(t, dy, s.esy); s.esz = POLAR_POINT_FMA(t, dz, s.esz);
      if (PHI) s.ps = POLAR_POINT_FMA(qj, POLAR_POINT_FMA(rsq * rinv, c.rc2inv, rinv) - c.two_rcinv, s.ps);
    }
    if (aj != 0.0 && (ALLPAIRS || rsq < c.ddcutsq)) {
      const double r3inv = r2inv * rinv;
      const double r5inv = r3inv * r2inv;
      double s3, s5;
      if (DAMP == 0) {   // exponential damping
        const double a = c.pd * (rsq * rinv);
        const double t = m.exp_neg(-a);
        const double a2 = a * a;
        const double p2 = POLAR_POINT_FMA(0.5, a2, 1.0 + a);
        const double p3 = POLAR_POINT_FMA(1.0 / 6.0, a2 * a, p2);
        s3 = POLAR_POINT_FMA(-t, p2, 1.0) * r3inv;
        s5 = 3.0 * (POLAR_POINT_FMA(-t, p3, 1.0) * r5inv);
      } else {
        s3 = r3inv;
        s5 = 3.0 * r5inv;
      }
      const double md = POLAR_POINT_FMA(mjx, dx, POLAR_POINT_FMA(mjy, dy, mjz * dz));
      const double cc = s5 * md;
      s.eix = POLAR_POINT_FMA(cc, dx, POLAR_POINT_FMA(-s3, mjx, s.eix));
      s.eiy = POLAR_POINT_FMA(cc, dy, POLAR_POINT_FMA(-s3, mjy, s.eiy));
      s.eiz = POLAR_POINT_FMA(cc, dz, POLAR_POINT_FMA(-s3, mjz, s.eiz));
      if (PHI) s.pi = POLAR_POINT_FMA(s3, md, s.pi);
    }
  }
}

}  // namespace polar
