// Host build of csrc/polar_force_pair.hpp with libm behind the math policy.  No HIP, no GPU.
//   force_pair_sum   (tests/test_force_pair_host.py): the closed-form pair function summed over all ordered pairs of a small system;
//   force_pair_probe (tests/test_pair_ref_host.py): the same function one pair at a time, every instance the device probe
//                    tests/math_probe/math_probe.hip runs, with the same input and output layout.
#include <cmath>

#include "polar_force_pair.hpp"

namespace {
struct HostMath {
  double g_ewald;
  double rsqrt(double x) const { return 1.0 / std::sqrt(x); }
  double exp_neg(double x) const { return std::exp(x); }
  // (the form of polar::ewald_b12, csrc/polar_common.hpp, which needs the HIP headers)
  void ewald_b12(double rsq, bool kept, double &b1, double &b2) const {
    const double g = g_ewald, r = std::sqrt(rsq), r2inv = 1.0 / rsq;
    const double a = g * g, alo = std::fma(g, g, -a);
    const double t = a * rsq, tlo = std::fma(a, rsq, -t) + alo * rsq;
    const double e = 1.1283791670955126 * g * (std::exp(-t) * (1.0 - tlo));
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

// in [n][17] = d (3) | mu_i (3) | q_i | alpha_i | mu_j (3) | q_j | alpha_j | molok | cut_coulsq | ddcutsq | f_shift
// out [n][12] = cd (3) | dd (3) | uef | udd | p (3) | rsq; the first eight start from sentinel[0..7], p from sentinel[8]
template <bool ALLPAIRS, int DAMP, bool EW>
void probe_pairs(long long n, const double *in, double pd, double e2s, double g_ewald, const double *s, double *out) {
  const HostMath m{g_ewald};
  for (long long p = 0; p < n; p++) {
    const double *a = in + 17 * p;
    double *o = out + 12 * p;
    const polar::PairRow ri = polar::make_pair_row(a[3], a[4], a[5], a[6], a[7], e2s);
    const polar::PairCut cut{a[14], a[15], a[16], pd};
    for (int k = 0; k < 8; k++) o[k] = s[k];
    o[8] = o[9] = o[10] = s[8];
    polar::polar_force_pair<ALLPAIRS, DAMP, true, EW, true>(m, a[0], a[1], a[2], ri, a[8], a[9], a[10], a[11], a[12], a[13] != 0.0, cut,
                                                            o[0], o[1], o[2], o[3], o[4], o[5], o[6], o[7], o[8], o[9], o[10]);
    o[11] = a[0] * a[0] + a[1] * a[1] + a[2] * a[2];
  }
}
}  // namespace

extern "C" int force_pair_probe(int allpairs, int damp, int ew, long long n, const double *in, double pd, double e2s, double g_ewald,
                                const double *sentinel, double *out) {
#define PROBE_PAIR(A, D, E) probe_pairs<A, D, E>(n, in, pd, e2s, g_ewald, sentinel, out)
  if (allpairs) {
    if (damp == 0) { if (ew) PROBE_PAIR(true, 0, true); else PROBE_PAIR(true, 0, false); }
    else           { if (ew) PROBE_PAIR(true, 1, true); else PROBE_PAIR(true, 1, false); }
  } else {
    if (damp == 0) { if (ew) PROBE_PAIR(false, 0, true); else PROBE_PAIR(false, 0, false); }
    else           { if (ew) PROBE_PAIR(false, 1, true); else PROBE_PAIR(false, 1, false); }
  }
#undef PROBE_PAIR
  return 0;
}

// del[i][j][3] = x_i - closest image of x_j.  f: force on every atom, fp: the same from the per-pair totals (the virial
// tally's input), dd: its dipole-dipole part, u = {u_ef, u_dd}.  damp: 0 exponential, 1 none.
extern "C" void force_pair_sum(int n, const double *del, const double *mu, const double *q, const double *alpha, const int *mol,
                               int damp, double cut_coul, double pd, double e2s, double *f, double *fp, double *dd, double *u) {
  if (damp == 0) sum_pairs<0>(n, del, mu, q, alpha, mol, cut_coul, pd, e2s, f, fp, dd, u);
  else sum_pairs<1>(n, del, mu, q, alpha, mol, cut_coul, pd, e2s, f, fp, dd, u);
}
