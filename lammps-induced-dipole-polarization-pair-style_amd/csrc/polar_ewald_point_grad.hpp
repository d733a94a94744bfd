// polar_ewald_point_grad.hpp -- what ONE atom j adds to the Ewald field of the polarized box at a point p AND to the gradient of
// that field, and what a run of k-vector rows adds to them: the arithmetic of k_ew_grad_real and k_ew_grad_recip
// (polar_ewald_field_grad_at.hpp, polar_ewald_field_grad_at() of include/polar_mi355x.h; formulas: DESIGN section 6i).
//
// Plain C++ with no HIP header behind it, as polar_ewald_point.hpp: the device kernels include it, and so does a host test that
// compares it pair by pair with a 40-digit reference and row by row with NumPy (tests/test_ewald_point_grad_host.py).  Square
// root, exponentials, erfc, erf and sincospi come from a policy `M` (device: EwPointMath of polar_ewald_field_at.hpp; host: libm).
//
// With d = x_p - x_j(image), r = |d|, g = g_ewald, rc = cut_coul, G(r) = 2g/sqrt(pi) e^(-g^2 r^2), ph = erfc(gr)/r for a kept
// atom and -erf(gr)/r for an excluded one, B1 = (ph + G) / r^2, and G_ab = d e_a / d x_b (xx, yy, zz, xy, xz, yz):
//
//  static part, real space, r^2 <= rc^2, the kept / excluded rule of polar_point_pair_ew, without the factor e2s:
//      e_static    += q_j B1 d
//      g_static_ab += q_j [ B1 delta_ab - B2 d_a d_b ],     B2 = (3 B1 + 2 g^2 G(r)) / r^2
//  (ph' = -r B1 and B1' / r = -B2 hold for the erfc and the erf form alike).  The trace of one pair is -2 g^2 q_j G(r), 4 pi times
//  the screening Gaussian: the real-space part is not harmonic, the reciprocal part carries the other half.
//      excluded atom at r^2 == 0 (the limit of the erf form): nothing in the field, nothing off the diagonal,
//      g_static_aa += -(2/3) g^2 (2g/sqrt(pi)) q_j    for a = x, y, z
//  An excluded atom at g^2 r^2 < 2^-26 counts as on the point in the gradient: the closed forms cancel there.
//
//  induced part: the induced branch of polar_point_grad_pair, called (s7 included; `polar_ewald` leaves the dipole tensor cut at
//  the minimum image or at dd_cutoff); not for the point's skip_atom (`induced` false); an atom at r^2 == 0 adds nothing there.
//
//  reciprocal part of one point, over the half space of k_ew_field, without e2s:
//      e_static    += sum_k c_k k Im(e^{ik.p} conj S(k)),      g_static_ab += sum_k c_k k_a k_b Re(e^{ik.p} conj S(k))
//  (the neutralising-background term is a constant of the potential and adds nothing).
//
// The field sums take the expressions of polar_point_pair_ew<ALLPAIRS, DAMP, false> and of ew_point_rows<false>, in their order
// and with their roundings: they have their bits (the host test compares them).
#pragma once

#include "polar_ewald_point.hpp"
#include "polar_point_grad_pair.hpp"

namespace polar {

// the atom on the point: B1 of the erf form -> -(2/3) g^2 2g/sqrt(pi) as r -> 0, and d_a d_b B2 -> 0
POLAR_PAIR_FN void ew_grad_on_point(const EwPointParm &e, double qj, PointGradSums &g) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double t0 = ((-2.0 / 3.0) * e.g2) * e.tgs;
  g.gs[0] = POLAR_POINT_FMA(t0, qj, g.gs[0]); g.gs[1] = POLAR_POINT_FMA(t0, qj, g.gs[1]); g.gs[2] = POLAR_POINT_FMA(t0, qj, g.gs[2]);
}

// One atom, added into the caller's running sums.  kept, induced: as polar_point_pair_ew.  k_ew_grad_real walks a point's records
// twice and splits this call as k_ew_point_real splits polar_point_pair_ew: the induced walk calls polar_point_grad_pair's
// induced branch itself, the static walk calls this with induced = false; the host test calls it whole.
// Every product and sum is rounded as written, every fused multiply-add is spelled out (contraction off inside the function).
template <bool ALLPAIRS, int DAMP, class M>
POLAR_PAIR_FN void polar_point_grad_pair_ew(const M &m, double dx, double dy, double dz, double qj, double mjx, double mjy, double mjz,
                                            double aj, bool kept, bool induced, const PointCut &c, const EwPointParm &e,
                                            PointGradSums &g) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  PointSums &s = g.f;
  const double rsq = POLAR_POINT_FMA(dx, dx, POLAR_POINT_FMA(dy, dy, dz * dz));
  if (rsq <= c.cut_coulsq) {
    if (rsq > 0.0) {
      const double rinv = m.rsqrt(rsq);
      const double r = rsq * rinv, r2inv = rinv * rinv;
      // G(r), erfc(gr) and B1: the lines of polar_point_pair_ew (the double-double g^2, the first-order correction of erfc's argument)
      const double t = e.g2 * rsq;
      const double tlo = POLAR_POINT_FMA(e.g2, rsq, -t) + e.g2lo * rsq;
      const double e0 = m.exp(-t) * (1.0 - tlo);
      const double gs = e.tgs * e0;
      const double gr = e.g * r;
      double b1, ph;
      if (kept) {
        const double rlo = POLAR_POINT_FMA(-r, r, rsq) * (0.5 * rinv);
        const double grlo = POLAR_POINT_FMA(e.g, r, -gr) + e.g * rlo;
        ph = POLAR_POINT_FMA(-(1.1283791670955126 * e0), grlo, m.erfc(gr)) * rinv;
        b1 = (ph + gs) * r2inv;
      } else {
        ph = -(m.erf(gr) * rinv);
        b1 = (ph + gs) * r2inv;
      }
      const double tq = b1 * qj;
      s.esx = POLAR_POINT_FMA(tq, dx, s.esx); s.esy = POLAR_POINT_FMA(tq, dy, s.esy); s.esz = POLAR_POINT_FMA(tq, dz, s.esz);
      if (kept || t >= 0x1p-26) {
        // -q B2 = -q (3 B1 + 2 g^2 G) / r^2
        const double nb = -((POLAR_POINT_FMA(3.0, b1, 2.0 * (e.g2 * gs)) * r2inv) * qj);
        const double bx = nb * dx, by = nb * dy, bz = nb * dz;
        g.gs[0] = POLAR_POINT_FMA(bx, dx, g.gs[0] + tq); g.gs[1] = POLAR_POINT_FMA(by, dy, g.gs[1] + tq); g.gs[2] = POLAR_POINT_FMA(bz, dz, g.gs[2] + tq);
        g.gs[3] = POLAR_POINT_FMA(bx, dy, g.gs[3]); g.gs[4] = POLAR_POINT_FMA(bx, dz, g.gs[4]); g.gs[5] = POLAR_POINT_FMA(by, dz, g.gs[5]);
      } else {
        // An excluded atom all but on the point (a guest put back onto its own site, up to rounding).  -erf(gr)/r + G cancels to
        // (gr)^2 of its terms and 3 B1 + 2 g^2 G to (gr)^4, and the quotients by r^2 magnify what is left without bound: at
        // t = g^2 r^2 = 2^-26 (r = 3.8e-4 A at g = 0.3243) the closed forms are wrong by up to 8 eps / (2/3 t) = 9e-8 of the value.
        // Below that the atom counts as on the point: B1 = -(2/3) g^2 2g/sqrt(pi) (1 - 3/5 t ...), r^2 B2 = 6/5 t of it, which
        // leaves 1.8 t = 2.7e-8 of the value out.  (A longer series would reach eps, but its constants do not fit the pair
        // loop of k_ew_grad_real: with four of them the list-mode instances spill scalar registers.)
        // The field sums above keep polar_point_pair_ew's expression and bits.
        ew_grad_on_point(e, qj, g);
      }
    } else {
      ew_grad_on_point(e, qj, g);
    }
  }
  if (induced) polar_point_grad_pair<ALLPAIRS, DAMP>(m, dx, dy, dz, qj, mjx, mjy, mjz, aj, false, c, g);   // (molok = false: its static branch is off)
}

// One point's reciprocal sums acc = {ex, ey, ez, gxx, gyy, gzz, gxy, gxz, gyz} over the rows r0 .. r1-1 of the k-vector table:
// arguments, the sincospi per row and the l-recurrence as ew_point_rows (polar_ewald_point.hpp).
template <class M, class I4, class D4, class D2>
POLAR_PAIR_FN void ew_point_grad_rows(const M &m, double sx, double sy, double sz, const I4 *rows, const D4 *kv, const D2 *S, int r0, int r1,
                                      double acc[9]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double bzs, bzc;
  m.sincospi(2.0 * sz, &bzs, &bzc);
  double ex = acc[0], ey = acc[1], ez = acc[2];
  double gxx = acc[3], gyy = acc[4], gzz = acc[5], gxy = acc[6], gxz = acc[7], gyz = acc[8];
  for (int r = r0; r < r1; r++) {
    const I4 rw = rows[r];
    const int k1 = rows[r + 1].w;
    const double arg = POLAR_POINT_FMA((double)rw.x, sx, POLAR_POINT_FMA((double)rw.y, sy, (double)rw.z * sz));
    double ps, pc;
    m.sincospi(2.0 * arg, &ps, &pc);
    for (int k = rw.w; k < k1; k++) {
      const D4 kc = kv[k];
      const D2 sk = S[k];
      const double im = POLAR_POINT_FMA(ps, sk.x, -(pc * sk.y));
      const double v = kc.w * im;
      ex = POLAR_POINT_FMA(v, kc.x, ex); ey = POLAR_POINT_FMA(v, kc.y, ey); ez = POLAR_POINT_FMA(v, kc.z, ez);
      const double v2 = kc.w * POLAR_POINT_FMA(pc, sk.x, ps * sk.y);
      const double wx = v2 * kc.x, wy = v2 * kc.y, wz = v2 * kc.z;
      gxx = POLAR_POINT_FMA(wx, kc.x, gxx); gyy = POLAR_POINT_FMA(wy, kc.y, gyy); gzz = POLAR_POINT_FMA(wz, kc.z, gzz);
      gxy = POLAR_POINT_FMA(wx, kc.y, gxy); gxz = POLAR_POINT_FMA(wx, kc.z, gxz); gyz = POLAR_POINT_FMA(wy, kc.z, gyz);
      const double nc = POLAR_POINT_FMA(pc, bzc, -(ps * bzs)), ns = POLAR_POINT_FMA(pc, bzs, ps * bzc);
      pc = nc; ps = ns;
    }
  }
  acc[0] = ex; acc[1] = ey; acc[2] = ez;
  acc[3] = gxx; acc[4] = gyy; acc[5] = gzz; acc[6] = gxy; acc[7] = gxz; acc[8] = gyz;
}

}  // namespace polar
