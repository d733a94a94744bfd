// csrc/polar_probe_pair.hpp on the host, one call per pair.
//
// As a shared library (tests/test_probe_pair_host.py): probe_pair_eval() evaluates n pairs, each with its own table entry, with
// one of the two instances (FORCE) and returns {e, fx, fy, fz} of each pair; probe_combine_eval() the combine step.
// With -DPROBE_PAIR_MAIN a stand-alone program (the sanitizer build): random pairs through both instances, and the exact
// properties the kernel relies on -- an atom at r = 0 and an atom on or beyond the cutoff add nothing (the sums keep their bits),
// e of a FORCE = false call has the bits of the FORCE = true one and leaves the force sums alone.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "polar_probe_pair.hpp"

// table: n entries of POLAR_LJ_ENTRY doubles (cutsq, cut_ljsq, lj1, lj2, lj3, lj4, offset, pad); pair k uses entry k
extern "C" void probe_pair_eval(int n, const double *d, const double *table, int force, double *out) {
  for (int k = 0; k < n; k++) {
    polar::ProbeSums s = {0, 0, 0, 0};
    if (force) polar::polar_probe_pair<true>(d[3 * k], d[3 * k + 1], d[3 * k + 2], k, table, s);
    else polar::polar_probe_pair<false>(d[3 * k], d[3 * k + 1], d[3 * k + 2], k, table, s);
    double *o = out + 4 * (size_t)k;
    o[0] = s.e; o[1] = s.fx; o[2] = s.fy; o[3] = s.fz;
  }
}

extern "C" void probe_combine_eval(int n, const double *es, const double *ei, const double *ps, const double *pi, const double *q,
                                   const double *alpha, double e2s, double *et, double *e_coul, double *e_pol) {
  for (int k = 0; k < n; k++) polar::polar_probe_combine(es + 3 * k, ei + 3 * k, ps[k], pi[k], q[k], alpha[k], e2s, et + 3 * k, e_coul[k], e_pol[k]);
}

#ifdef PROBE_PAIR_MAIN
namespace {

struct Rng {
  uint64_t s;
  double uni() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)(s >> 11) * (1.0 / 9007199254740992.0); }
  double sym(double a) { return a * (2.0 * uni() - 1.0); }
};

bool same_bits(const double *a, const double *b, int n) { return memcmp(a, b, (size_t)n * sizeof(double)) == 0; }

}  // namespace

int main(int argc, char **argv) {
  const int n = argc > 1 ? atoi(argv[1]) : 2000;
  Rng g{0x9E3779B97F4A7C15ull};
  long long checks = 0, failures = 0;
  double sum = 0.0;
  for (int k = 0; k < n; k++) {
    // a table of three types' entries for the probe's row; the atom takes one of them
    double row[3 * POLAR_LJ_ENTRY];
    for (int t = 0; t < 3; t++) {
      const double eps = 0.02 + 0.3 * g.uni(), sig = 2.5 + 1.5 * g.uni(), cut = 4.0 + 8.0 * g.uni(), s6 = std::pow(sig, 6.0);
      double *e = row + POLAR_LJ_ENTRY * t;
      e[0] = 144.0; e[1] = cut * cut; e[2] = 48.0 * eps * s6 * s6; e[3] = 24.0 * eps * s6; e[4] = 4.0 * eps * s6 * s6; e[5] = 4.0 * eps * s6;
      e[6] = g.uni() < 0.5 ? 0.0 : 4.0 * eps * (s6 * s6 / std::pow(cut, 12.0) - s6 / std::pow(cut, 6.0)); e[7] = 0.0;
    }
    const int tj = (int)(3.0 * g.uni()) % 3;
    const double cut = std::sqrt(row[POLAR_LJ_ENTRY * tj + 1]);
    const double r = 0.8 + (cut * 0.999 - 0.8) * g.uni();
    double u[3] = {g.sym(1.0), g.sym(1.0), g.sym(1.0)};
    const double un = std::sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]) + 1e-300;
    const double d[3] = {r * u[0] / un, r * u[1] / un, r * u[2] / un};
    polar::ProbeSums s0 = {g.sym(3.0), g.sym(3.0), g.sym(3.0), g.sym(3.0)};   // running sums that are not zero
    // the pair itself, with and without the force: the same energy bits, the force sums untouched without
    polar::ProbeSums s1 = s0, s2 = s0;
    polar::polar_probe_pair<true>(d[0], d[1], d[2], tj, row, s1);
    polar::polar_probe_pair<false>(d[0], d[1], d[2], tj, row, s2);
    checks++;
    if (!(same_bits(&s1.e, &s2.e, 1) && same_bits(&s2.fx, &s0.fx, 3) && !same_bits(&s1.e, &s0.e, 1))) failures++;
    sum += s1.e + s1.fx + s1.fy + s1.fz;
    // an atom on the point
    polar::ProbeSums s3 = s0;
    polar::polar_probe_pair<true>(0.0, 0.0, 0.0, tj, row, s3);
    checks++;
    if (!same_bits(&s3.e, &s0.e, 4)) failures++;
    // an atom exactly on the cutoff shell (rsq == cut_ljsq: the comparison is strict) and one beyond it
    polar::ProbeSums s4 = s0;
    double shell[POLAR_LJ_ENTRY];
    memcpy(shell, row + POLAR_LJ_ENTRY * tj, sizeof(shell));
    shell[1] = __builtin_fma(d[0], d[0], __builtin_fma(d[1], d[1], d[2] * d[2]));
    polar::polar_probe_pair<true>(d[0], d[1], d[2], 0, shell, s4);
    polar::polar_probe_pair<true>(1.01 * cut * u[0] / un, 1.01 * cut * u[1] / un, 1.01 * cut * u[2] / un, tj, row, s4);
    checks++;
    if (!same_bits(&s4.e, &s0.e, 4)) failures++;
  }
  // the library entries on a few pairs as well (the same code path the Python test calls)
  double d[6] = {1.0, 2.0, -0.5, 0.0, 0.0, 0.0}, tab[16] = {144, 100, 48, 24, 4, 4, 0.001, 0, 144, 100, 48, 24, 4, 4, 0, 0}, out[8];
  for (int f = 0; f < 2; f++) {
    probe_pair_eval(2, d, tab, f, out);
    for (int j = 0; j < 8; j++) sum += out[j];
  }
  double es[3] = {0.1, -0.2, 0.3}, ei[3] = {0.01, 0.02, -0.03}, ps = 0.4, pi = -0.1, q = 0.5, al = 0.8, et[3], ec, ep;
  probe_combine_eval(1, es, ei, &ps, &pi, &q, &al, 18.22, et, &ec, &ep);
  sum += et[0] + et[1] + et[2] + ec + ep;
  printf("instances 2 inputs %d checks %lld failures %lld sum %.17g\n", n, checks, failures, sum);
  return failures == 0 && std::isfinite(sum) ? 0 : 1;
}
#endif
