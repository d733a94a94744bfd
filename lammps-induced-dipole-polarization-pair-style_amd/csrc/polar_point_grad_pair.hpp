// polar_point_grad_pair.hpp -- what ONE atom j adds to the field of the polarized box at a point p AND to the gradient of that
// field: the pair arithmetic of k_field_grad_at (polar_field_grad_at.hpp, polar_field_grad_at() of include/polar_mi355x.h;
// DESIGN section 6h).
//
// Plain C++ with no HIP header behind it, as polar_point_pair.hpp: the device kernel includes it, and so does a host test
// that compares it pair by pair with a 40-digit reference (tests/test_point_grad_host.py).  The square root and the
// exponential come from a policy `M` (device: PairMath of polar_rows.hpp; host: libm).
//
// With d = x_p - x_j(image), r = |d|, rc = cut_coul, and G_ab = d e_a / d x_b (symmetric in both parts, since -grad phi = e
// holds for both: six components, in the order xx, yy, zz, xy, xz, yz).  The selection rules are polar_point_pair's:
//
//  static part (r^2 <= rc^2 and the molecule rule), without the factor e2s, which the caller applies to the sums:
//      e_static    += q_j (1/r^2 - 1/rc^2) d / r
//      g_static_ab += q_j [ (r^-3 - rc^-2 r^-1) delta_ab + (rc^-2 r^-3 - 3 r^-5) d_a d_b ]
//  Its trace per pair is -2 q_j / (rc^2 r): the shifted-force field is not harmonic.
//
//  induced part (alpha_j != 0; every pair (ALLPAIRS) or r^2 < dd_cutoff^2), through the style's tensor scalars s3, s5
//  (PS.cpp:1284-1306) and the next one, s7 = -(1/r) d s5 / d r:
//      e_induced    += -(s3 mu_j - s5 (mu_j.d) d)
//      g_induced_ab += s5 (mu_a d_b + d_a mu_b + (mu.d) delta_ab) - s7 (mu.d) d_a d_b
//  damping `none`: s7 = 15 r^-7 and the induced gradient is traceless.  Exponential damping, a = polar_damp r, t = e^-a:
//      s7 = 15 r^-7 (1 - t p4),   p4 = p3 + a^4 / 30,   p3 = 1 + a + a^2/2 + a^3/6
//  (d s5 / d r = -15 r^-6 (1 - t p3) + 3 r^-5 polar_damp t (p3 - p2), and p3 - p2 = a^3 / 6).
//
// An atom at r^2 == 0 adds nothing.  The six field sums take the expressions of polar_point_pair<ALLPAIRS, DAMP, false>, in its
// order and with its roundings: they have its bits (the host test compares them).
#pragma once

#include "polar_point_pair.hpp"

namespace polar {

// The running sums of one point (per lane in the kernel): PointSums' six field components (ps and pi stay untouched) and the
// twelve of the gradient, xx, yy, zz, xy, xz, yz.  gs lacks the factor e2s, as esx..esz.
struct PointGradSums {
  PointSums f;
  double gs[6];
  double gi[6];
};

// One atom, added into the caller's running sums -- each part inside its own (lane-divergent) condition.  Arguments as
// polar_point_pair.
// Every sum and product below is rounded as written and every fused multiply-add is spelled out (compiler contraction off).
template <bool ALLPAIRS, int DAMP, class M>
POLAR_PAIR_FN void polar_point_grad_pair(const M &m, double dx, double dy, double dz, double qj, double mjx, double mjy, double mjz,
                                         double aj, bool molok, const PointCut &c, PointGradSums &g) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  PointSums &s = g.f;
  const double rsq = POLAR_POINT_FMA(dx, dx, POLAR_POINT_FMA(dy, dy, dz * dz));
  if (rsq > 0.0) {
    const double rinv = m.rsqrt(rsq);
    const double r2inv = rinv * rinv;
    if (rsq <= c.cut_coulsq && molok) {
      const double t = ((r2inv - c.rc2inv) * rinv) * qj;
      s.esx = POLAR_POINT_FMA(t, dx, s.esx); s.esy = POLAR_POINT_FMA(t, dy, s.esy); s.esz = POLAR_POINT_FMA(t, dz, s.esz);
      // q (rc^-2 r^-3 - 3 r^-5) = q r^-3 (rc^-2 - 3 r^-2): inside the cutoff 3 / r^2 > 1 / rc^2, nothing cancels
      const double b = (qj * (r2inv * rinv)) * POLAR_POINT_FMA(-3.0, r2inv, c.rc2inv);
      const double bx = b * dx, by = b * dy, bz = b * dz;
      g.gs[0] = POLAR_POINT_FMA(bx, dx, g.gs[0] + t); g.gs[1] = POLAR_POINT_FMA(by, dy, g.gs[1] + t); g.gs[2] = POLAR_POINT_FMA(bz, dz, g.gs[2] + t);
      g.gs[3] = POLAR_POINT_FMA(bx, dy, g.gs[3]); g.gs[4] = POLAR_POINT_FMA(bx, dz, g.gs[4]); g.gs[5] = POLAR_POINT_FMA(by, dz, g.gs[5]);
    }
    if (aj != 0.0 && (ALLPAIRS || rsq < c.ddcutsq)) {
      const double r3inv = r2inv * rinv;
      const double r5inv = r3inv * r2inv;
      double s3, s5, s7;
      if (DAMP == 0) {   // exponential damping
        const double a = c.pd * (rsq * rinv);
        const double t = m.exp_neg(-a);
        const double a2 = a * a;
        const double p2 = POLAR_POINT_FMA(0.5, a2, 1.0 + a);
        const double p3 = POLAR_POINT_FMA(1.0 / 6.0, a2 * a, p2);
        const double p4 = POLAR_POINT_FMA(1.0 / 30.0, a2 * a2, p3);
        s3 = POLAR_POINT_FMA(-t, p2, 1.0) * r3inv;
        s5 = 3.0 * (POLAR_POINT_FMA(-t, p3, 1.0) * r5inv);
        s7 = 15.0 * (POLAR_POINT_FMA(-t, p4, 1.0) * (r5inv * r2inv));
      } else {
        s3 = r3inv;
        s5 = 3.0 * r5inv;
        s7 = 15.0 * (r5inv * r2inv);
      }
      const double md = POLAR_POINT_FMA(mjx, dx, POLAR_POINT_FMA(mjy, dy, mjz * dz));
      const double cc = s5 * md;
      s.eix = POLAR_POINT_FMA(cc, dx, POLAR_POINT_FMA(-s3, mjx, s.eix));
      s.eiy = POLAR_POINT_FMA(cc, dy, POLAR_POINT_FMA(-s3, mjy, s.eiy));
      s.eiz = POLAR_POINT_FMA(cc, dz, POLAR_POINT_FMA(-s3, mjz, s.eiz));
      const double ux = s5 * mjx, uy = s5 * mjy, uz = s5 * mjz;       // s5 mu
      const double c7 = s7 * md;
      const double wx = c7 * dx, wy = c7 * dy, wz = c7 * dz;          // s7 (mu.d) d
      g.gi[0] = POLAR_POINT_FMA(-wx, dx, POLAR_POINT_FMA(ux + ux, dx, g.gi[0] + cc));
      g.gi[1] = POLAR_POINT_FMA(-wy, dy, POLAR_POINT_FMA(uy + uy, dy, g.gi[1] + cc));
      g.gi[2] = POLAR_POINT_FMA(-wz, dz, POLAR_POINT_FMA(uz + uz, dz, g.gi[2] + cc));
      g.gi[3] = POLAR_POINT_FMA(-wx, dy, POLAR_POINT_FMA(ux, dy, POLAR_POINT_FMA(uy, dx, g.gi[3])));
      g.gi[4] = POLAR_POINT_FMA(-wx, dz, POLAR_POINT_FMA(ux, dz, POLAR_POINT_FMA(uz, dx, g.gi[4])));
      g.gi[5] = POLAR_POINT_FMA(-wy, dz, POLAR_POINT_FMA(uy, dz, POLAR_POINT_FMA(uz, dy, g.gi[5])));
    }
  }
}

// What a probe's charge and polarizability make of the gradient block of the same point (polar_probe_force_at): with
// e = e_static + e_induced and G = g_static + g_induced, one add per component,
//     f_coul = (q e2s) e        f_pol_b = alpha fma(e_x, G_xb, fma(e_y, G_yb, e_z G_zb))      (= -grad(-1/2 alpha |e|^2), G symmetric)
// Contraction off: the grouping is the one written.
POLAR_PAIR_FN void polar_probe_force_combine(const double es[3], const double ei[3], const double gs[6], const double gi[6], double q,
                                             double alpha, double e2s, double f_coul[3], double f_pol[3]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double ex = es[0] + ei[0], ey = es[1] + ei[1], ez = es[2] + ei[2];
  const double gxx = gs[0] + gi[0], gyy = gs[1] + gi[1], gzz = gs[2] + gi[2], gxy = gs[3] + gi[3], gxz = gs[4] + gi[4], gyz = gs[5] + gi[5];
  const double qe = q * e2s;
  f_coul[0] = qe * ex; f_coul[1] = qe * ey; f_coul[2] = qe * ez;
  f_pol[0] = alpha * POLAR_POINT_FMA(ex, gxx, POLAR_POINT_FMA(ey, gxy, ez * gxz));
  f_pol[1] = alpha * POLAR_POINT_FMA(ex, gxy, POLAR_POINT_FMA(ey, gyy, ez * gyz));
  f_pol[2] = alpha * POLAR_POINT_FMA(ex, gxz, POLAR_POINT_FMA(ey, gyz, ez * gzz));
}

}  // namespace polar
