// csrc/polar_point_grad_pair.hpp on the host: libm behind the math policy, one call per pair.
//
// As a shared library (tests/test_point_grad_host.py): point_grad_eval() evaluates n pairs with one of the four instances
// (ALLPAIRS x DAMP) and returns the 18 sums of each pair -- e_static, e_induced, g_static, g_induced, the static ones times e2s as
// k_field_grad_at stores them -- and, behind them, the six field sums of polar_point_pair<..., false> on the same pair.
// With -DPOINT_GRAD_MAIN a stand-alone program (the sanitizer build): random pairs through every instance, and the exact
// properties the kernel relies on -- the field sums have the bits of polar_point_pair, and an atom at r = 0 or one that takes no
// part leaves every sum's bits.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "polar_point_grad_pair.hpp"

namespace {

struct LibmMath {
  double rsqrt(double x) const { return 1.0 / std::sqrt(x); }
  double exp_neg(double x) const { return std::exp(x); }
};

const polar::PointGradSums kZero = {{0, 0, 0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0}};

template <bool AP, int DAMP>
void eval(int n, const double *d, const double *q, const double *mu, const double *alpha, const int *molok, const polar::PointCut &c,
          double e2s, double *out) {
  const LibmMath m;
  for (int k = 0; k < n; k++) {
    polar::PointGradSums g = kZero;
    polar::PointSums s = {0, 0, 0, 0, 0, 0, 0, 0};
    polar::polar_point_grad_pair<AP, DAMP>(m, d[3 * k], d[3 * k + 1], d[3 * k + 2], q[k], mu[3 * k], mu[3 * k + 1], mu[3 * k + 2], alpha[k],
                                           molok[k] != 0, c, g);
    polar::polar_point_pair<AP, DAMP, false>(m, d[3 * k], d[3 * k + 1], d[3 * k + 2], q[k], mu[3 * k], mu[3 * k + 1], mu[3 * k + 2], alpha[k],
                                             molok[k] != 0, c, s);
    double *o = out + 24 * (size_t)k;
    o[0] = e2s * g.f.esx; o[1] = e2s * g.f.esy; o[2] = e2s * g.f.esz;
    o[3] = g.f.eix; o[4] = g.f.eiy; o[5] = g.f.eiz;
    for (int j = 0; j < 6; j++) { o[6 + j] = e2s * g.gs[j]; o[12 + j] = g.gi[j]; }
    o[18] = e2s * s.esx; o[19] = e2s * s.esy; o[20] = e2s * s.esz;
    o[21] = s.eix; o[22] = s.eiy; o[23] = s.eiz;
  }
}

polar::PointCut make_cut(double cut_coul, double dd_cutoff, double pd) {
  return polar::PointCut{cut_coul * cut_coul, dd_cutoff * dd_cutoff, 1.0 / (cut_coul * cut_coul), 2.0 / cut_coul, pd};
}

}  // namespace

extern "C" void point_grad_eval(int n, const double *d, const double *q, const double *mu, const double *alpha, const int *molok,
                                int allpairs, int damp, double cut_coul, double dd_cutoff, double pd, double e2s, double *out) {
  const polar::PointCut c = make_cut(cut_coul, dd_cutoff, pd);
  if (allpairs) { if (damp == 0) eval<true, 0>(n, d, q, mu, alpha, molok, c, e2s, out); else eval<true, 1>(n, d, q, mu, alpha, molok, c, e2s, out); }
  else          { if (damp == 0) eval<false, 0>(n, d, q, mu, alpha, molok, c, e2s, out); else eval<false, 1>(n, d, q, mu, alpha, molok, c, e2s, out); }
}

#ifdef POINT_GRAD_MAIN
namespace {

struct Rng {
  uint64_t s;
  double uni() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)(s >> 11) * (1.0 / 9007199254740992.0); }
  double sym(double a) { return a * (2.0 * uni() - 1.0); }
};

bool same_bits(const double *a, const double *b, int n) { return memcmp(a, b, (size_t)n * sizeof(double)) == 0; }
bool same_sums(const polar::PointGradSums &a, const polar::PointGradSums &b) { return memcmp(&a, &b, sizeof a) == 0; }   // (20 doubles, no padding)
bool same_field(const polar::PointSums &a, const polar::PointSums &b) { return memcmp(&a, &b, sizeof a) == 0; }

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
    polar::PointGradSums s0;
    s0.f = polar::PointSums{g.sym(3.0), g.sym(3.0), g.sym(3.0), g.sym(3.0), g.sym(3.0), g.sym(3.0), g.sym(3.0), g.sym(3.0)};   // running sums that are not zero
    for (int j = 0; j < 6; j++) { s0.gs[j] = g.sym(3.0); s0.gi[j] = g.sym(3.0); }
    // the pair itself: the field sums have the bits of polar_point_pair, ps and pi stay
    polar::PointGradSums s1 = s0;
    polar::PointSums f = s0.f;
    polar::polar_point_grad_pair<AP, DAMP>(m, d[0], d[1], d[2], q, mu[0], mu[1], mu[2], a, molok, c, s1);
    polar::polar_point_pair<AP, DAMP, false>(m, d[0], d[1], d[2], q, mu[0], mu[1], mu[2], a, molok, c, f);
    checks++;
    if (!same_field(s1.f, f)) failures++;
    for (int j = 0; j < 6; j++) sum += s1.gs[j] + s1.gi[j];
    // no charge, alpha = 0, a stale dipole: the values stay (signed zeros may have been added)
    polar::PointGradSums s2 = s0;
    polar::polar_point_grad_pair<AP, DAMP>(m, d[0], d[1], d[2], 0.0, 5.0 * mu[0], 5.0 * mu[1], 5.0 * mu[2], 0.0, molok, c, s2);
    checks++;
    {
      bool ok = s2.f.esx == s0.f.esx && s2.f.esy == s0.f.esy && s2.f.esz == s0.f.esz && same_bits(&s2.f.eix, &s0.f.eix, 1) &&
                same_bits(&s2.f.eiy, &s0.f.eiy, 1) && same_bits(&s2.f.eiz, &s0.f.eiz, 1) && same_bits(s2.gi, s0.gi, 6);
      for (int j = 0; j < 6; j++) ok = ok && s2.gs[j] == s0.gs[j];
      if (!ok) failures++;
    }
    // an atom on the point
    polar::PointGradSums s4 = s0;
    polar::polar_point_grad_pair<AP, DAMP>(m, 0.0, 0.0, 0.0, q, mu[0], mu[1], mu[2], a, molok, c, s4);
    checks++;
    if (!same_sums(s4, s0)) failures++;
    // beyond both cutoffs (list form), or excluded from the static sums and without polarizability
    polar::PointGradSums s5 = s0;
    if (!AP) polar::polar_point_grad_pair<AP, DAMP>(m, 9.5 * u[0] / un, 9.5 * u[1] / un, 9.5 * u[2] / un, q, mu[0], mu[1], mu[2], a, true, c, s5);
    else polar::polar_point_grad_pair<AP, DAMP>(m, d[0], d[1], d[2], q, mu[0], mu[1], mu[2], 0.0, false, c, s5);
    checks++;
    if (!same_sums(s5, s0)) failures++;
  }
}

}  // namespace

int main(int argc, char **argv) {
  static_assert(sizeof(polar::PointGradSums) == 20 * sizeof(double), "the sums are 20 consecutive doubles");
  const int n = argc > 1 ? atoi(argv[1]) : 2000;
  Rng g{0x9E3779B97F4A7C15ull};
  long long checks = 0, failures = 0;
  double sum = 0.0;
  instance<true, 0>(n, g, checks, failures, sum);
  instance<true, 1>(n, g, checks, failures, sum);
  instance<false, 0>(n, g, checks, failures, sum);
  instance<false, 1>(n, g, checks, failures, sum);
  // the library entry and the force combination on a few pairs as well
  double d[6] = {1.0, 2.0, -0.5, 0.0, 0.0, 0.0}, q[2] = {0.3, -0.2}, mu[6] = {0.1, 0.0, -0.2, 0.3, 0.3, 0.3}, al[2] = {1.0, 0.0}, out[48];
  int mk[2] = {1, 1};
  for (int inst = 0; inst < 4; inst++) {
    point_grad_eval(2, d, q, mu, al, mk, inst & 1, (inst >> 1) & 1, 9.0, 7.5, 2.1304, 18.22, out);
    for (int j = 0; j < 48; j++) sum += out[j];
    double fc[3], fp[3];
    polar::polar_probe_force_combine(out, out + 3, out + 6, out + 12, 0.4, 0.9, 18.22, fc, fp);
    for (int j = 0; j < 3; j++) sum += fc[j] + fp[j];
  }
  printf("instances 4 inputs %d checks %lld failures %lld sum %.17g\n", n, checks, failures, sum);
  return failures == 0 && std::isfinite(sum) ? 0 : 1;
}
#endif
