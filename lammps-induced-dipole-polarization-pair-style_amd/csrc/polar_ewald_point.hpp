// polar_ewald_point.hpp -- what ONE atom j adds to the Ewald field and potential of the polarized box at a point p, and
// what a run of k-vector rows adds to them: the arithmetic of k_ew_point_real and k_ew_point_recip (polar_ewald_field_at.hpp,
// polar_ewald_field_at() of include/polar_mi355x.h; formulas: DESIGN section 6e).
//
// Plain C++ with no HIP header behind it, as polar_point_pair.hpp: the device kernels include it, and so does a host test that
// compares it pair by pair with a 40-digit reference and row by row with NumPy (tests/test_ewald_point_host.py).  Square
// root, exponentials, erfc, erf and sincospi come from a policy `M` (device: EwPointMath of polar_ewald_field_at.hpp; host: libm).
//
// With d = x_p - x_j(image), r = |d|, g = g_ewald, rc = cut_coul, G(r) = 2g/sqrt(pi) e^(-g^2 r^2):
//
//  static part, real space (the sums of k_ew_static_field taken at a point), r^2 <= rc^2, without the factor e2s:
//      kept atom      e_static += q_j B1(r) d,             B1 = (erfc(gr)/r + G) / r^2;     phi_static += q_j erfc(gr) / r
//      excluded atom  e_static += q_j (B1 - 1/r^3) d  = -q_j (erf(gr)/r - G) / r^2 d;       phi_static -= q_j erf(gr) / r
//      excluded atom at r^2 == 0 (the limit of the erf form): nothing in the field,         phi_static -= q_j 2g/sqrt(pi)
//  An atom is excluded when the caller says so (the point's molecule, the point's skip_atom) or when it sits on the point
//  (r^2 == 0): exclusion takes the nearest image's 1/r part off and leaves the periodic images in, which is the step's rule.
//
//  induced part: the induced branch of polar_point_pair, called (`polar_ewald` leaves the dipole tensor cut at the minimum
//  image or at dd_cutoff); not for the point's skip_atom (`induced` false), and an atom at r^2 == 0 adds nothing there.
//
//  reciprocal part of one point, over the half space of k_ew_field, without e2s:
//      e_static   += sum_k c_k k Im(e^{ik.p} conj S(k)),      phi_static += sum_k c_k Re(e^{ik.p} conj S(k))
#pragma once

#include "polar_point_pair.hpp"

namespace polar {

// g_ewald and what every pair needs of it: g^2 as a double-double (the exponent of the Gaussian carries its rounding errors
// along, as ewald_gauss of polar_common.hpp does) and 2g/sqrt(pi).
struct EwPointParm {
  double g, g2, g2lo, tgs;
};
inline EwPointParm make_ew_point_parm(double g) {
  const double a = g * g;
  return EwPointParm{g, a, __builtin_fma(g, g, -a), 1.1283791670955126 * g};
}

// One atom, added into the caller's running sums.  kept: the static sums take the atom as a kept one (the point carries no
// molecule id, or another one than atom j, and atom j is not the point's skip_atom); induced: atom j is not the skip_atom.
// k_ew_point_real walks a point's records twice (registers: polar_ewald_field_at.hpp) and splits this call accordingly: the
// static walk calls it with induced = false (and no dipole), the induced walk calls polar_point_pair's induced branch itself
// for the atoms that are not the skip_atom -- the same two branches, the same arithmetic per sum; the host test calls it whole.
// PHI = false leaves ps and pi untouched.  Every product and sum is rounded as written, every fused multiply-add is spelled
// out (contraction off inside the function): a PHI = false call gives the field bits of the PHI = true one.
template <bool ALLPAIRS, int DAMP, bool PHI, class M>
POLAR_PAIR_FN void polar_point_pair_ew(const M &m, double dx, double dy, double dz, double qj, double mjx, double mjy, double mjz,
                                       double aj, bool kept, bool induced, const PointCut &c, const EwPointParm &e, PointSums &s) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double rsq = POLAR_POINT_FMA(dx, dx, POLAR_POINT_FMA(dy, dy, dz * dz));
  if (rsq <= c.cut_coulsq) {
    if (rsq > 0.0) {
      const double rinv = m.rsqrt(rsq);
      const double r = rsq * rinv, r2inv = rinv * rinv;
      // G(r): the exponent g^2 r^2 with the low parts of its two products, folded into the exponential to first order
      const double t = e.g2 * rsq;
      const double tlo = POLAR_POINT_FMA(e.g2, rsq, -t) + e.g2lo * rsq;
      const double e0 = m.exp(-t) * (1.0 - tlo);
      const double gs = e.tgs * e0;
      const double gr = e.g * r;
      double b1, ph;
      if (kept) {
        // erfc(gr): a relative error eps of its argument moves it by 2 g^2 r^2 eps (17 eps at g = 0.3243, r = 9), and the
        // potential is this term alone.  The argument carries the residual of the square root and the rounding of g r
        // along, and erfc takes them to first order: erfc'(x) = -2/sqrt(pi) e^(-x^2), the Gaussian that is there already.
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
      if (PHI) s.ps = POLAR_POINT_FMA(qj, ph, s.ps);
    } else if (PHI) {
      s.ps = POLAR_POINT_FMA(-qj, e.tgs, s.ps);
    }
  }
  if (induced) polar_point_pair<ALLPAIRS, DAMP, PHI>(m, dx, dy, dz, qj, mjx, mjy, mjz, aj, false, c, s);   // (molok = false: its static branch is off)
}

// Rows of the k-vector table per chunk of k_ew_point_recip's grid: about 1024 k-vectors each, from the table's two counts
// alone -- never from the points -- so that a point's partial sums, and the order they are folded in, are the same in every call.
inline int ew_point_rows_per_chunk(int nrow, int nk) {
  if (nrow <= 0 || nk <= 0) return 1;
  const long long r = ((long long)nrow * 1024 + nk - 1) / nk;
  return (int)(r < 1 ? 1 : (r > nrow ? nrow : r));
}
inline int ew_point_chunks(int nrow, int nk) {
  if (nrow <= 0 || nk <= 0) return 0;
  const int rpc = ew_point_rows_per_chunk(nrow, nk);
  return (nrow + rpc - 1) / rpc;
}

// One point's reciprocal sums acc = {ex, ey, ez, phi} over the rows r0 .. r1-1 of the k-vector table (rows[r] = {h, k, first l,
// index of the row's first k-vector}, rows[nrow].w = nk; kv[k] = {kx, ky, kz, c_k}; S[k] = the structure factor).
// (sx, sy, sz): the point's fractional coordinates s = H^-1 p, the point already wrapped into the box (the phase arguments
// stay small).  One sincospi per row, then the row's l's by the recurrence p <- p e^{2 pi i s_z}, as k_ew_field.
// PHI = false leaves acc[3] untouched and gives the same field bits.
template <bool PHI, class M, class I4, class D4, class D2>
POLAR_PAIR_FN void ew_point_rows(const M &m, double sx, double sy, double sz, const I4 *rows, const D4 *kv, const D2 *S, int r0, int r1,
                                 double acc[4]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double bzs, bzc;
  m.sincospi(2.0 * sz, &bzs, &bzc);
  double ex = acc[0], ey = acc[1], ez = acc[2], ph = acc[3];
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
      if (PHI) ph = POLAR_POINT_FMA(kc.w, POLAR_POINT_FMA(pc, sk.x, ps * sk.y), ph);
      const double nc = POLAR_POINT_FMA(pc, bzc, -(ps * bzs)), ns = POLAR_POINT_FMA(pc, bzs, ps * bzc);
      pc = nc; ps = ns;
    }
  }
  acc[0] = ex; acc[1] = ey; acc[2] = ez;
  if (PHI) acc[3] = ph;
}

}  // namespace polar
