// polar_force_pair.hpp -- the polarization force and energy of ONE ordered pair (i, j): what the row kernels
// k_polar_force / k_ew_polar_force (polar_rows.hpp) sum over a row, PS.cpp:406-641, in closed form.
//
// Plain C++ with no HIP header behind it: the device kernels include it, and so does a host test that sums it over
// all ordered pairs of a small system and compares with the oracle (tests/test_force_pair_host.py).  The square root
// and the exponentials come from a policy `M` (device: the Newton / polynomial forms with their constants in scalar
// registers, polar_rows.hpp; host: libm).
//
// The algebra (d = x_i - x_j, r = |d|, e2s = sqrt(qqrd2e), f_shift = -1 / cut_coul^2):
//
//  charge-dipole (PS.cpp:454-510).  The shifted-force tensor of the reference, M_pp = (-2 p^2 + q^2 + s^2) r^-2 +
//  f_shift (q^2 + s^2), M_pq = -p q (3 r^-2 + f_shift), is  M v = (1 + f_shift r^2) v - (3 r^-2 + f_shift)(v.d) d,
//  and the two directions (dipole on i / charge on j, and the reverse) differ only in v.  With
//      w = e2s (q_j mu_i - q_i mu_j)
//  both are  p = r^-3 [(1 + f_shift r^2) w - (3 r^-2 + f_shift)(w.d) d]  and  u_ef = -(r^-2 + f_shift) r^-1 (w.d).
//  Under `polar_ewald` the same w gives  p = B1 w - B2 (w.d) d  (gradient of the real-space Ewald field).
//  The reference applies each direction only when that side's alpha and the other side's charge are non-zero: a zero
//  charge zeroes its half of w by itself; a zero alpha is honoured by the caller, who passes mu = 0 (row side:
//  PairRow, partner side: a select on q_i) -- so a record with alpha = 0 and a stale mu still contributes nothing.
//
//  dipole-dipole, exponential damping (PS.cpp:512-602).  With a = polar_damp * r, t = e^-a,
//  g2 = 1 - t (1 + a + a^2/2), g3 = g2 - t a^3/6, the reference's pre4 and pre5 are differences whose leading terms
//  cancel analytically:
//      -t (pd/r + pd^2) + t pd (1 + a + a^2/2) / r = pd^3 r t / 2
//      -t (pd/r + pd^2 + r pd^3/2) + t pd (1 + a + a^2/2 + a^3/6) / r = pd^4 r^2 t / 6
//  which leaves three coefficients that depend on r alone,
//      c_pp = r^-5 (3 g2 - a^3 t / 2),   c_dd = r^-7 (a^4 t / 2 - 15 g3),   s5 = 3 r^-5 g3,
//      p_dd = [c_pp (mu_i.mu_j) + c_dd (mu_i.d)(mu_j.d)] d + s5 (mu_j.d) mu_i + s5 (mu_i.d) mu_j,
//      u_dd = r^-3 g2 (mu_i.mu_j) - s5 (mu_i.d)(mu_j.d).
//  Without damping g2 = g3 = 1 and t = 0.
#pragma once

#if defined(__HIPCC__)
#define POLAR_PAIR_FN __host__ __device__ __forceinline__
#else
#define POLAR_PAIR_FN inline
#endif

namespace polar {

// Row-side factors: the same for every pair of a row (wave-uniform in the kernels), computed once per row.
struct PairRow {
  double mx, my, mz;     // mu_i, zeroed when alpha_i == 0
  double wx, wy, wz;     // e2s * mu_i (same zeroing)
  double eq;             // e2s * q_i
  bool pol;              // alpha_i != 0
};
POLAR_PAIR_FN PairRow make_pair_row(double mx, double my, double mz, double q, double alpha, double e2s) {
  PairRow r;
  r.pol = alpha != 0.0;
  r.mx = r.pol ? mx : 0.0; r.my = r.pol ? my : 0.0; r.mz = r.pol ? mz : 0.0;
  r.wx = e2s * r.mx; r.wy = e2s * r.my; r.wz = e2s * r.mz;
  r.eq = e2s * q;
  return r;
}

// The settings a pair needs.
struct PairCut {
  double cut_coulsq;     // charge-dipole part: rsq < cut_coulsq (strict, PS.cpp:454); rsq <= cut_coulsq under polar_ewald
  double ddcutsq;        // dipole-dipole part: rsq < ddcutsq, or every pair (ALLPAIRS)
  double f_shift;        // -1 / cut_coulsq
  double pd;             // polar_damp
};

// One pair, added into the caller's running sums -- each part inside its own (lane-divergent) condition, so that a lane that
// skips a part executes nothing for it, not even a zero:
//   cd  += the charge-dipole part of the force on i from j (the negative of the force on j from i);
//   dd  += its dipole-dipole part.  The force is cd + dd; kept apart, `debug yes` (which reports the dipole-dipole part
//          of atom 0's force) costs the loop nothing;
//   uef, udd += the pair's energies when EFLAG (the caller halves them: every pair is seen from both of its rows);
//   p    = the pair's whole force when WANT_P (the pairwise virial tally), else untouched.
// molok: i and j are in different molecules, or i is in none.  (mjx, mjy, mjz), qj, aj: the partner's dipole, charge, alpha.
template <bool ALLPAIRS, int DAMP, bool EFLAG, bool EW, bool WANT_P, class M>
POLAR_PAIR_FN void polar_force_pair(const M &m, double dx, double dy, double dz, const PairRow &ri, double mjx, double mjy,
                                    double mjz, double qj, double aj, bool molok, const PairCut &c, double &cdx, double &cdy,
                                    double &cdz, double &ddx, double &ddy, double &ddz, double &uef, double &udd, double &px,
                                    double &py, double &pz) {
  const double rsq = dx * dx + dy * dy + dz * dz;
  const double rinv = m.rsqrt(rsq);
  const double r2inv = rinv * rinv;
  const double r3inv = r2inv * rinv;
  const bool polj = aj != 0.0;
  if (WANT_P) { px = 0.0; py = 0.0; pz = 0.0; }
  if (EW ? (rsq <= c.cut_coulsq) : (rsq < c.cut_coulsq && molok)) {
    const double eqi = polj ? ri.eq : 0.0;   // the half of w that needs alpha_j != 0
    const double wx = qj * ri.wx - eqi * mjx, wy = qj * ri.wy - eqi * mjy, wz = qj * ri.wz - eqi * mjz;
    const double wd = wx * dx + wy * dy + wz * dz;
    double ca, cb;
    if (EW) {
      m.ewald_b12(rsq, molok, ca, cb);
    } else {
      ca = (1.0 + c.f_shift * rsq) * r3inv;
      cb = (3.0 * r2inv + c.f_shift) * r3inv;
      if (EFLAG) uef -= ((r2inv + c.f_shift) * rinv) * wd;   // (polar_ewald: u_ef is -sum mu.E, left to k_ew_force)
    }
    const double t = cb * wd;
    const double cx = ca * wx - t * dx, cy = ca * wy - t * dy, cz = ca * wz - t * dz;
    cdx += cx; cdy += cy; cdz += cz;
    if (WANT_P) { px = cx; py = cy; pz = cz; }
  }
  if (ri.pol && polj && (ALLPAIRS || rsq < c.ddcutsq)) {
    const double r5inv = r3inv * r2inv;
    const double pdotp = ri.mx * mjx + ri.my * mjy + ri.mz * mjz;
    const double pidotr = ri.mx * dx + ri.my * dy + ri.mz * dz;
    const double pjdotr = mjx * dx + mjy * dy + mjz * dz;
    const double pipj = pidotr * pjdotr;
    double cpp, cdd, s5, u3;
    if (DAMP == 0) {
      const double a = c.pd * (rsq * rinv);
      const double t = m.exp_neg(-a);
      const double a2 = a * a, a3 = a2 * a;
      const double p2 = 1.0 + a + 0.5 * a2;
      const double ta3 = t * a3;
      const double g2 = 1.0 - t * p2;
      const double g3 = g2 - (1.0 / 6.0) * ta3;
      s5 = 3.0 * r5inv * g3;
      cpp = r5inv * (3.0 * g2 - 0.5 * ta3);
      cdd = (r5inv * r2inv) * (0.5 * (ta3 * a) - 15.0 * g3);
      u3 = r3inv * g2;
    } else {
      s5 = 3.0 * r5inv;
      cpp = s5;
      cdd = -5.0 * (s5 * r2inv);
      u3 = r3inv;
    }
    const double pre_r = cpp * pdotp + cdd * pipj;
    const double pre2 = s5 * pjdotr, pre3 = s5 * pidotr;
    const double qx = pre_r * dx + pre2 * ri.mx + pre3 * mjx;
    const double qy = pre_r * dy + pre2 * ri.my + pre3 * mjy;
    const double qz = pre_r * dz + pre2 * ri.mz + pre3 * mjz;
    ddx += qx; ddy += qy; ddz += qz;
    if (WANT_P) { px += qx; py += qy; pz += qz; }
    if (EFLAG) udd += u3 * pdotp - s5 * pipj;
  }
}

}  // namespace polar
