// csrc/polar_point_pair.hpp on the host: libm behind the math policy, one call per pair.
//
// As a shared library (tests/test_point_pair_host.py): point_pair_eval() evaluates n pairs with one of the eight instances
// (ALLPAIRS x DAMP x PHI) and returns the eight sums of each pair, the static ones times e2s as k_field_at stores them.
// With -DPOINT_PAIR_MAIN a stand-alone program (the sanitizer build): random pairs through every instance, and the exact
// properties the kernel relies on -- an atom at r = 0, an atom outside both cutoffs and a chargeless atom with alpha = 0 and a
// stale dipole add nothing (the sums keep their bits), and the field of a PHI = false call has the bits of the PHI = true one.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "polar_point_pair.hpp"

namespace {

struct LibmMath {
  double rsqrt(double x) const { return 1.0 / std::sqrt(x); }
  double exp_neg(double x) const { return std::exp(x); }
};

template <bool AP, int DAMP, bool PHI>
void eval(int n, const double *d, const double *q, const double *mu, const double *alpha, const int *molok, const polar::PointCut &c,
          double e2s, double *out) {
  const LibmMath m;
  for (int k = 0; k < n; k++) {
    polar::PointSums s = {0, 0, 0, 0, 0, 0, 0, 0};
    polar::polar_point_pair<AP, DAMP, PHI>(m, d[3 * k], d[3 * k + 1], d[3 * k + 2], q[k], mu[3 * k], mu[3 * k + 1], mu[3 * k + 2], alpha[k],
                                           molok[k] != 0, c, s);
    double *o = out + 8 * (size_t)k;
    o[0] = e2s * s.esx; o[1] = e2s * s.esy; o[2] = e2s * s.esz; o[3] = e2s * s.ps;
    o[4] = s.eix; o[5] = s.eiy; o[6] = s.eiz; o[7] = s.pi;
  }
}

polar::PointCut make_cut(double cut_coul, double dd_cutoff, double pd) {
  return polar::PointCut{cut_coul * cut_coul, dd_cutoff * dd_cutoff, 1.0 / (cut_coul * cut_coul), 2.0 / cut_coul, pd};
}

}  // namespace

extern "C" void point_pair_eval(int n, const double *d, const double *q, const double *mu, const double *alpha, const int *molok,
                                int allpairs, int damp, int phi, double cut_coul, double dd_cutoff, double pd, double e2s, double *out) {
  const polar::PointCut c = make_cut(cut_coul, dd_cutoff, pd);
#define GO(AP, D, P) eval<AP, D, P>(n, d, q, mu, alpha, molok, c, e2s, out)
#define GOP(AP, D) do { if (phi) GO(AP, D, true); else GO(AP, D, false); } while (0)
  if (allpairs) { if (damp == 0) GOP(true, 0); else GOP(true, 1); }
  else          { if (damp == 0) GOP(false, 0); else GOP(false, 1); }
#undef GOP
#undef GO
}

#ifdef POINT_PAIR_MAIN
namespace {

struct Rng {
  uint64_t s;
  double uni() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)(s >> 11) * (1.0 / 9007199254740992.0); }
  double sym(double a) { return a * (2.0 * uni() - 1.0); }
};

bool same_bits(const double *a, const double *b, int n) { return memcmp(a, b, (size_t)n * sizeof(double)) == 0; }

template <bool AP, int DAMP>
void instance(int n, Rng &g, long long &checks, long long &failures, double &sum) {
  const polar::PointCut c = make_cut(9.0, 7.5, 2.1304);
  const LibmMath m;
  for (int k = 0; k < n; k++) {
    const double r = 0.05 + 11.95 * g.uni();
    double u[3] = {g.sym(1.0), g.sym(1.0), g.sym(1.0)};
    const double un = std::sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]) + 1e-300;
    const double d[3] = {r * u[0] / un, r * u[1] / un, r * u[2] / un};
    const double q = g.sym(1.0), mu[3] = {g.sym(0.5), g.sym(0.5), g.sym(0.5)}, a = g.uni() < 0.25 ? 0.0 : 0.2 + g.uni();
    const bool molok = g.uni() < 0.8;
    polar::PointSums s0;
    double *v = &s0.esx;
    for (int j = 0; j < 8; j++) v[j] = g.sym(3.0);   // running sums that are not zero
    // the pair itself, with and without the potentials: the same field bits, ps and pi untouched without
    polar::PointSums s1 = s0, s2 = s0;
    polar::polar_point_pair<AP, DAMP, true>(m, d[0], d[1], d[2], q, mu[0], mu[1], mu[2], a, molok, c, s1);
    polar::polar_point_pair<AP, DAMP, false>(m, d[0], d[1], d[2], q, mu[0], mu[1], mu[2], a, molok, c, s2);
    checks++;
    if (!(same_bits(&s1.esx, &s2.esx, 3) && same_bits(&s1.eix, &s2.eix, 3) && same_bits(&s2.ps, &s0.ps, 1) && same_bits(&s2.pi, &s0.pi, 1))) failures++;
    for (int j = 0; j < 8; j++) sum += (&s1.esx)[j];
    // an atom on the point
    polar::PointSums s3 = s0;
    polar::polar_point_pair<AP, DAMP, true>(m, 0.0, 0.0, 0.0, q, mu[0], mu[1], mu[2], a, molok, c, s3);
    checks++;
    if (!same_bits(&s3.esx, &s0.esx, 8)) failures++;
    // no charge, alpha = 0, a stale dipole
    polar::PointSums s4 = s0;
    polar::polar_point_pair<AP, DAMP, true>(m, d[0], d[1], d[2], 0.0, 5.0 * mu[0], 5.0 * mu[1], 5.0 * mu[2], 0.0, molok, c, s4);
    checks++;
    for (int j = 0; j < 8; j++) if (!((&s4.esx)[j] == (&s0.esx)[j])) { failures++; break; }   // (signed zeros added: values compare equal)
    // beyond both cutoffs (list form), or excluded from the static sums and without polarizability
    polar::PointSums s5 = s0;
    if (!AP) polar::polar_point_pair<AP, DAMP, true>(m, 9.5 * u[0] / un, 9.5 * u[1] / un, 9.5 * u[2] / un, q, mu[0], mu[1], mu[2], a, true, c, s5);
    else polar::polar_point_pair<AP, DAMP, true>(m, d[0], d[1], d[2], q, mu[0], mu[1], mu[2], 0.0, false, c, s5);
    checks++;
    if (!same_bits(&s5.esx, &s0.esx, 8)) failures++;
  }
}

}  // namespace

int main(int argc, char **argv) {
  const int n = argc > 1 ? atoi(argv[1]) : 2000;
  Rng g{0x9E3779B97F4A7C15ull};
  long long checks = 0, failures = 0;
  double sum = 0.0;
  instance<true, 0>(n, g, checks, failures, sum);
  instance<true, 1>(n, g, checks, failures, sum);
  instance<false, 0>(n, g, checks, failures, sum);
  instance<false, 1>(n, g, checks, failures, sum);
  // the library entry on a few pairs as well (the same code path the Python test calls)
  double d[6] = {1.0, 2.0, -0.5, 0.0, 0.0, 0.0}, q[2] = {0.3, -0.2}, mu[6] = {0.1, 0.0, -0.2, 0.3, 0.3, 0.3}, al[2] = {1.0, 0.0}, out[16];
  int mk[2] = {1, 1};
  for (int inst = 0; inst < 8; inst++) {
    point_pair_eval(2, d, q, mu, al, mk, inst & 1, (inst >> 1) & 1, (inst >> 2) & 1, 9.0, 7.5, 2.1304, 18.22, out);
    for (int j = 0; j < 16; j++) sum += out[j];
  }
  printf("instances 4 inputs %d checks %lld failures %lld sum %.17g\n", n, checks, failures, sum);
  return failures == 0 && std::isfinite(sum) ? 0 : 1;
}
#endif
