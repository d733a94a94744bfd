// Host build of csrc/polar_force_pair.hpp for tests/test_force_pair_host.py: the closed-form pair function summed over all
// ordered pairs of a small system, with libm behind the math policy.  No HIP, no GPU.
#include <cmath>

#include "polar_force_pair.hpp"

namespace {
struct HostMath {
  double g_ewald;
  double rsqrt(double x) const { return 1.0 / std::sqrt(x); }
  double exp_neg(double x) const { return std::exp(x); }
  // (not called here -- only the non-Ewald instances are built -- but polar_force_pair() names it in a plain `if (EW)`)
  void ewald_b12(double rsq, bool kept, double &b1, double &b2) const {
    const double g = g_ewald, r = std::sqrt(rsq), r2inv = 1.0 / rsq;
    const double e = 1.1283791670955126 * g * std::exp(-g * g * rsq);
    b1 = kept ? (std::erfc(g * r) / r + e) * r2inv : -(std::erf(g * r) / r - e) * r2inv;
    b2 = (3.0 * b1 + 2.0 * g * g * e) * r2inv;
  }
};

template <int DAMP>
void sum_pairs(int n, const double *del, const double *mu, const double *q, const double *alpha, const int *mol,
               double cut_coul, double pd, double e2s, double *f, double *fp, double *dd, double *u) {
  const HostMath m{0.0};
  const polar::PairCut cut{cut_coul * cut_coul, 0.0, -1.0 / (cut_coul * cut_coul), pd};
  double uef = 0.0, udd = 0.0;
  for (int i = 0; i < n; i++) {
    const polar::PairRow ri = polar::make_pair_row(mu[3 * i], mu[3 * i + 1], mu[3 * i + 2], q[i], alpha[i], e2s);
    double c[3] = {0, 0, 0}, d[3] = {0, 0, 0}, ps[3] = {0, 0, 0};
    for (int j = 0; j < n; j++) {
      if (j == i) continue;
      const double *dl = del + 3 * ((long)i * n + j);
      const bool molok = mol[i] != mol[j] || mol[i] == 0;
      double px, py, pz;
      polar::polar_force_pair<true, DAMP, true, false, true>(m, dl[0], dl[1], dl[2], ri, mu[3 * j], mu[3 * j + 1], mu[3 * j + 2], q[j],
                                                             alpha[j], molok, cut, c[0], c[1], c[2], d[0], d[1], d[2], uef, udd, px, py,
                                                             pz);
      ps[0] += px; ps[1] += py; ps[2] += pz;
    }
    for (int k = 0; k < 3; k++) { f[3 * i + k] = c[k] + d[k]; dd[3 * i + k] = d[k]; fp[3 * i + k] = ps[k]; }
  }
  u[0] = 0.5 * uef; u[1] = 0.5 * udd;   // every pair was seen from both sides
}
}  // namespace

// del[i][j][3] = x_i - closest image of x_j.  f: force on every atom, fp: the same from the per-pair totals (the virial
// tally's input), dd: its dipole-dipole part, u = {u_ef, u_dd}.  damp: 0 exponential, 1 none.
extern "C" void force_pair_sum(int n, const double *del, const double *mu, const double *q, const double *alpha, const int *mol,
                               int damp, double cut_coul, double pd, double e2s, double *f, double *fp, double *dd, double *u) {
  if (damp == 0) sum_pairs<0>(n, del, mu, q, alpha, mol, cut_coul, pd, e2s, f, fp, dd, u);
  else sum_pairs<1>(n, del, mu, q, alpha, mol, cut_coul, pd, e2s, f, fp, dd, u);
}
