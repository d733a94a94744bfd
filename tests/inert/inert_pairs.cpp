// Host program: an inert site (q == 0 and alpha == 0, an LJ-only site) adds EXACTLY nothing to the polarization sums.
// The list build leaves such sites out of the full list and the force kernels skip their rows (SITE_INERT,
// csrc/polar_common.hpp); that is right only while every term they would have added is a signed zero.  This program pins it on
// csrc/polar_force_pair.hpp itself, bit for bit, for every instance the header can be built as on the host:
//   ALLPAIRS x DAMP x EFLAG x EW x WANT_P = 32 instances, libm behind the math policy (the one of tests/force_pair).
// Per instance and input (random finite displacement, row, partner, cutoffs; accumulators start at random non-zero values):
//   1. a partner with q_j = 0, alpha_j = 0 and an arbitrary finite stale mu_j leaves all eight accumulators bit-equal, and
//      the pair's whole force p (WANT_P) is +-0;
//   2. so does a row made by make_pair_row(mu, 0, 0, e2s) -- stale mu again -- against ANY partner;
//   3. the static-field term of a partner with q_j = 0, factor * q_j * d, is +-0 in the shifted-force and in the Ewald form
//      (the expressions of static_field_body, csrc/polar_rows.hpp) and leaves a non-zero field sum bit-equal.
// Prints the number of checks and returns 0, or prints the first failures and returns 1.  No HIP, no GPU.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

#include "polar_force_pair.hpp"

namespace {
struct HostMath {
  double g_ewald;
  double rsqrt(double x) const { return 1.0 / std::sqrt(x); }
  double exp_neg(double x) const { return std::exp(x); }
  void ewald_b12(double rsq, bool kept, double &b1, double &b2) const {
    const double g = g_ewald, r = std::sqrt(rsq), r2inv = 1.0 / rsq;
    const double e = 1.1283791670955126 * g * std::exp(-g * g * rsq);
    b1 = kept ? (std::erfc(g * r) / r + e) * r2inv : -(std::erf(g * r) / r - e) * r2inv;
    b2 = (3.0 * b1 + 2.0 * g * g * e) * r2inv;
  }
};

struct Rng {
  std::mt19937_64 g;
  explicit Rng(uint64_t seed) : g(seed) {}
  double uni(double a, double b) { return a + (b - a) * std::generate_canonical<double, 53>(g); }
  bool coin(double p) { return uni(0.0, 1.0) < p; }
  double nonzero(double scale) { const double v = uni(0.05, 1.0) * scale; return coin(0.5) ? v : -v; }
  // a stale dipole component: ordinary, tiny, huge -- any finite value
  double stale() {
    const double u = uni(0.0, 1.0);
    const double v = u < 0.7 ? uni(-5.0, 5.0) : (u < 0.8 ? 0.0 : (u < 0.9 ? uni(-1.0, 1.0) * 1e-300 : uni(-1.0, 1.0) * 1e300));
    return v;
  }
};

long long checks = 0, failures = 0;

void fail(const char *what, int inst, long long k) {
  if (failures < 10) std::fprintf(stderr, "FAIL %s: instance %d input %lld\n", what, inst, k);
  failures++;
}

bool is_zero(double v) { return v == 0.0; }   // +0 or -0

template <bool ALLPAIRS, int DAMP, bool EFLAG, bool EW, bool WANT_P>
void run_instance(int inst, long long n, uint64_t seed) {
  Rng r(seed);
  const double e2s = std::sqrt(332.06371);
  for (long long k = 0; k < n; k++) {
    const HostMath m{r.uni(0.15, 0.45)};
    // displacement: any direction, 0.4 ... 13 A (inside and outside both cutoffs)
    const double len = r.uni(0.4, 13.0);
    double d[3] = {r.uni(-1.0, 1.0), r.uni(-1.0, 1.0), r.uni(-1.0, 1.0)};
    const double nd = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) + 1e-3;
    for (double &c : d) c *= len / nd;
    const double cc = r.uni(6.0, 12.0), dc = r.uni(4.0, cc);
    const polar::PairCut cut{cc * cc, dc * dc, -1.0 / (cc * cc), r.uni(1.0, 3.0)};
    const bool molok = r.coin(0.7);
    double acc0[8], p0[3];
    for (double &a : acc0) a = r.nonzero(10.0);
    for (double &a : p0) a = r.nonzero(10.0);

    // 1. an inert partner in the row of any atom (charged or not, polarizable or not)
    {
      const double qi = r.coin(0.2) ? 0.0 : r.nonzero(1.0), ai = r.coin(0.2) ? 0.0 : r.uni(0.1, 2.0);
      const polar::PairRow ri = polar::make_pair_row(r.stale(), r.stale(), r.stale(), qi, ai, e2s);
      double a[8], p[3];
      std::memcpy(a, acc0, sizeof(a)); std::memcpy(p, p0, sizeof(p));
      polar::polar_force_pair<ALLPAIRS, DAMP, EFLAG, EW, WANT_P>(m, d[0], d[1], d[2], ri, r.stale(), r.stale(), r.stale(), 0.0, 0.0, molok, cut,
                                                                 a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], p[0], p[1], p[2]);
      checks++;
      if (std::memcmp(a, acc0, sizeof(a)) != 0) fail("inert partner changed an accumulator", inst, k);
      if (WANT_P ? !(is_zero(p[0]) && is_zero(p[1]) && is_zero(p[2])) : std::memcmp(p, p0, sizeof(p)) != 0) fail("inert partner: pair force", inst, k);
    }
    // 2. an inert row atom against any partner
    {
      const polar::PairRow ri = polar::make_pair_row(r.stale(), r.stale(), r.stale(), 0.0, 0.0, e2s);
      const double qj = r.coin(0.2) ? 0.0 : r.nonzero(1.0), aj = r.coin(0.2) ? 0.0 : r.uni(0.1, 2.0);
      double a[8], p[3];
      std::memcpy(a, acc0, sizeof(a)); std::memcpy(p, p0, sizeof(p));
      polar::polar_force_pair<ALLPAIRS, DAMP, EFLAG, EW, WANT_P>(m, d[0], d[1], d[2], ri, r.uni(-5.0, 5.0), r.uni(-5.0, 5.0), r.uni(-5.0, 5.0), qj, aj, molok,
                                                                 cut, a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], p[0], p[1], p[2]);
      checks++;
      if (std::memcmp(a, acc0, sizeof(a)) != 0) fail("inert row changed an accumulator", inst, k);
      if (WANT_P ? !(is_zero(p[0]) && is_zero(p[1]) && is_zero(p[2])) : std::memcmp(p, p0, sizeof(p)) != 0) fail("inert row: pair force", inst, k);
    }
    // 3. the static field of a partner without charge (q_j = +0 or -0): ef_temp * d with ef_temp = factor(r) * q_j
    {
      const double rsq = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
      const double qj = r.coin(0.5) ? 0.0 : -0.0;
      double fac;
      if (EW) { double b2; m.ewald_b12(rsq, molok, fac, b2); }
      else { const double rinv = m.rsqrt(rsq); fac = (rinv * rinv + cut.f_shift) * rinv; }
      const double ef_temp = fac * qj;
      double e[3] = {acc0[0], acc0[1], acc0[2]};
      e[0] += ef_temp * d[0]; e[1] += ef_temp * d[1]; e[2] += ef_temp * d[2];
      checks++;
      if (!(is_zero(ef_temp * d[0]) && is_zero(ef_temp * d[1]) && is_zero(ef_temp * d[2]))) fail("static-field term is not a zero", inst, k);
      if (std::memcmp(e, acc0, sizeof(e)) != 0) fail("static-field term changed the sum", inst, k);
    }
  }
}

template <bool A, int D, bool E, bool W>
void run_ew_p(int &inst, long long n) {
  run_instance<A, D, E, W, false>(inst, n, 1000 + inst); inst++;
  run_instance<A, D, E, W, true>(inst, n, 1000 + inst); inst++;
}
template <bool A, int D>
void run_e(int &inst, long long n) {
  run_ew_p<A, D, false, false>(inst, n); run_ew_p<A, D, false, true>(inst, n);
  run_ew_p<A, D, true, false>(inst, n); run_ew_p<A, D, true, true>(inst, n);
}
}  // namespace

int main(int argc, char **argv) {
  const long long n = argc > 1 ? std::atoll(argv[1]) : 20000;
  int inst = 0;
  run_e<false, 0>(inst, n); run_e<false, 1>(inst, n); run_e<true, 0>(inst, n); run_e<true, 1>(inst, n);
  std::printf("instances %d inputs %lld checks %lld failures %lld\n", inst, n, checks, failures);
  return failures ? 1 : 0;
}
