// lab/force_pair_literal.hpp -- LAB BUILD ONLY (-DPOLAR_LAB, libpolar_mi355x_lab.so): code that was built, measured and did not become the
// product path.  Included by polar_rows.hpp inside `#ifdef POLAR_LAB`; the product library never sees it.
//
// The pair arithmetic of the polarization force kernel as it stood before the closed forms of polar_force_pair.hpp: the
// reference's terms one by one (six entries of the shifted-force tensor and two mat-vecs behind lane-divergent guards;
// pre4 / pre5 as differences of cancelling terms; the generic rsqrt() and the degree-13 exp_neg()).  POLAR_FORCE_LITERAL=1
// selects it in the lab library: the A/B partner of the closed form in time and in value
// (tests/test_gpu_force_closed_form.py).  It sets its outputs -- (px, py, pz) the charge-dipole part, (ddx, ddy, ddz) the dipole-dipole
// part, each exactly as the old body computed it, zero where a part does not apply --; the row kernel adds them up.
#pragma once

namespace polar {

template <bool ALLPAIRS, int DAMP, bool EFLAG, bool EW>
__device__ __forceinline__ void polar_force_pair_literal(const ExpCoef &K, double g_ewald, double dx, double dy, double dz,
                                                         const AtomRec &ri, const AtomRec &rj, bool molok, double cut_coulsq,
                                                         double ddcutsq, double pd, double e2s, double &px, double &py,
                                                         double &pz, double &ddx, double &ddy, double &ddz, double &uef,
                                                         double &udd) {
  const double f_shift = -1.0 / cut_coulsq;
  const double xsq = dx * dx, ysq = dy * dy, zsq = dz * dz;
  const double rsq = xsq + ysq + zsq;
  const double rinv = rsqrt(rsq);
  const double r2inv = rinv * rinv;
  const double r = rsq * rinv;
  const double r3inv = r2inv * rinv;
  px = 0; py = 0; pz = 0; ddx = 0; ddy = 0; ddz = 0; uef = 0; udd = 0;
  if (EW) {
    if (rsq <= cut_coulsq) {  // F_i = e2s [q_j (B1 mu_i - B2 (mu_i.d) d) - q_i (B1 mu_j - B2 (mu_j.d) d)]
      double b1, b2;
      ewald_b12(rsq, g_ewald, molok, b1, b2);
      if (ri.a != 0.0 && rj.q != 0.0) {
        const double c = rj.q * e2s, pr = (ri.mx * dx + ri.my * dy + ri.mz * dz) * b2;
        px += c * (b1 * ri.mx - pr * dx); py += c * (b1 * ri.my - pr * dy); pz += c * (b1 * ri.mz - pr * dz);
      }
      if (rj.a != 0.0 && ri.q != 0.0) {
        const double c = ri.q * e2s, pr = (rj.mx * dx + rj.my * dy + rj.mz * dz) * b2;
        px -= c * (b1 * rj.mx - pr * dx); py -= c * (b1 * rj.my - pr * dy); pz -= c * (b1 * rj.mz - pr * dz);
      }
    }
  } else if (rsq < cut_coulsq && molok) {  // note <, PS.cpp:454
    // shifted-force charge-dipole tensor G_pq = delta_pq (r^-2 + f_shift) r^2 ... written as the
    // reference does: M_pp = (-2 p^2 + q^2 + s^2) r2inv + f_shift (q^2 + s^2), M_pq = -pq (3 r2inv + f_shift)
    const double mxx = (-2.0 * xsq + ysq + zsq) * r2inv + f_shift * (ysq + zsq);
    const double myy = (-2.0 * ysq + xsq + zsq) * r2inv + f_shift * (xsq + zsq);
    const double mzz = (-2.0 * zsq + xsq + ysq) * r2inv + f_shift * (xsq + ysq);
    const double k = -(3.0 * r2inv + f_shift);
    const double mxy = k * dx * dy, mxz = k * dx * dz, myz = k * dy * dz;
    const double ef_temp = (r2inv + f_shift) * rinv * e2s;
    if (ri.a != 0.0 && rj.q != 0.0) {  // dipole on i, charge on j
      const double cf = rj.q * e2s * r3inv;
      px += cf * (ri.mx * mxx + ri.my * mxy + ri.mz * mxz);
      py += cf * (ri.mx * mxy + ri.my * myy + ri.mz * myz);
      pz += cf * (ri.mx * mxz + ri.my * myz + ri.mz * mzz);
      if (EFLAG) uef -= ef_temp * rj.q * (ri.mx * dx + ri.my * dy + ri.mz * dz);
    }
    if (rj.a != 0.0 && ri.q != 0.0) {  // dipole on j, charge on i
      const double cf = ri.q * e2s * r3inv;
      px -= cf * (rj.mx * mxx + rj.my * mxy + rj.mz * mxz);
      py -= cf * (rj.mx * mxy + rj.my * myy + rj.mz * myz);
      pz -= cf * (rj.mx * mxz + rj.my * myz + rj.mz * mzz);
      if (EFLAG) uef += ef_temp * ri.q * (rj.mx * dx + rj.my * dy + rj.mz * dz);
    }
  }
  if (ri.a != 0.0 && rj.a != 0.0 && (ALLPAIRS || rsq < ddcutsq)) {  // dipole-dipole, PS.cpp:512-602
    const double r5inv = r3inv * r2inv, r7inv = r5inv * r2inv;
    const double pdotp = ri.mx * rj.mx + ri.my * rj.my + ri.mz * rj.mz;
    const double pidotr = ri.mx * dx + ri.my * dy + ri.mz * dz;
    const double pjdotr = rj.mx * dx + rj.my * dy + rj.mz * dz;
    double pre_r, pre2, pre3;
    if (DAMP == 0) {
      const double t1 = exp_neg(-pd * r, K);
      const double t2 = 1.0 + pd * r + 0.5 * pd * pd * r * r;
      const double t3 = t2 + (1.0 / 6.0) * pd * pd * pd * r * r * r;
      const double g2 = 1.0 - t1 * t2, g3 = 1.0 - t1 * t3;
      const double pre1 = 3.0 * r5inv * pdotp * g2 - 15.0 * r7inv * pidotr * pjdotr * g3;
      pre2 = 3.0 * r5inv * pjdotr * g3;
      pre3 = 3.0 * r5inv * pidotr * g3;
      const double pre4 = -pdotp * r3inv * (-t1 * (pd * rinv + pd * pd) + t1 * pd * t2 * rinv);
      const double pre5 = 3.0 * pidotr * pjdotr * r5inv *
                          (-t1 * (pd * rinv + pd * pd + 0.5 * r * pd * pd * pd) + t1 * pd * t3 * rinv);
      pre_r = pre1 + pre4 + pre5;
      if (EFLAG) udd += r3inv * pdotp * g2 - 3.0 * r5inv * pidotr * pjdotr * g3;
    } else {
      pre_r = 3.0 * r5inv * pdotp - 15.0 * r7inv * pidotr * pjdotr;
      pre2 = 3.0 * r5inv * pjdotr;
      pre3 = 3.0 * r5inv * pidotr;
      if (EFLAG) udd += r3inv * pdotp - 3.0 * r5inv * pidotr * pjdotr;
    }
    ddx = pre_r * dx + pre2 * ri.mx + pre3 * rj.mx; ddy = pre_r * dy + pre2 * ri.my + pre3 * rj.my;
    ddz = pre_r * dz + pre2 * ri.mz + pre3 * rj.mz;
  }
}

}  // namespace polar
