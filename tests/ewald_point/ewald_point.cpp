// csrc/polar_ewald_point.hpp on the host: libm behind the math policy.
//
// As a shared library (tests/test_ewald_point_host.py): ew_point_pair_eval() evaluates n pairs with one of the eight instances
// of polar_point_pair_ew (ALLPAIRS x DAMP x PHI) and returns the eight sums of each pair, the static ones times e2s as
// k_ew_point_real stores them; ew_point_rows_eval() runs ew_point_rows for a set of points over a range of rows of a k-vector
// table; ew_point_chunking() returns the row chunking of a table.
// With -DEWALD_POINT_MAIN a stand-alone program (the sanitizer build): random pairs through every instance and a small
// k-vector table through ew_point_rows, with the exact properties the kernels rely on -- the field of a PHI = false call has the
// bits of the PHI = true one, an atom beyond cut_coul without polarizability adds nothing, an excluded atom on the point adds
// -q 2g/sqrt(pi) to the potential and nothing else, and the rows of a table summed chunk by chunk are the rows summed at once
// when the chunks continue each other's sums.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "polar_ewald_point.hpp"

namespace {

struct LibmMath {
  double rsqrt(double x) const { return 1.0 / std::sqrt(x); }
  double exp_neg(double x) const { return std::exp(x); }
  double exp(double x) const { return std::exp(x); }
  double erfc(double x) const { return std::erfc(x); }
  double erf(double x) const { return std::erf(x); }
  void sincospi(double x, double *s, double *c) const {
    const double y = x - 2.0 * std::rint(0.5 * x);   // exact: |y| <= 1
    const double pi = 3.14159265358979323846;
    *s = std::sin(pi * y); *c = std::cos(pi * y);
  }
};

struct I4 { int x, y, z, w; };
struct D4 { double x, y, z, w; };
struct D2 { double x, y; };

template <bool AP, int DAMP, bool PHI>
void eval(int n, const double *d, const double *q, const double *mu, const double *alpha, const int *kept, const int *induced,
          const polar::PointCut &c, const polar::EwPointParm &e, double e2s, double *out) {
  const LibmMath m;
  for (int k = 0; k < n; k++) {
    polar::PointSums s = {0, 0, 0, 0, 0, 0, 0, 0};
    polar::polar_point_pair_ew<AP, DAMP, PHI>(m, d[3 * k], d[3 * k + 1], d[3 * k + 2], q[k], mu[3 * k], mu[3 * k + 1], mu[3 * k + 2], alpha[k],
                                              kept[k] != 0, induced[k] != 0, c, e, s);
    double *o = out + 8 * (size_t)k;
    o[0] = e2s * s.esx; o[1] = e2s * s.esy; o[2] = e2s * s.esz; o[3] = e2s * s.ps;
    o[4] = s.eix; o[5] = s.eiy; o[6] = s.eiz; o[7] = s.pi;
  }
}

polar::PointCut make_cut(double cut_coul, double dd_cutoff, double pd) {
  return polar::PointCut{cut_coul * cut_coul, dd_cutoff * dd_cutoff, 1.0 / (cut_coul * cut_coul), 2.0 / cut_coul, pd};
}

}  // namespace

extern "C" void ew_point_pair_eval(int n, const double *d, const double *q, const double *mu, const double *alpha, const int *kept,
                                   const int *induced, int allpairs, int damp, int phi, double cut_coul, double dd_cutoff, double pd,
                                   double e2s, double g, double *out) {
  const polar::PointCut c = make_cut(cut_coul, dd_cutoff, pd);
  const polar::EwPointParm e = polar::make_ew_point_parm(g);
#define GO(AP, D, P) eval<AP, D, P>(n, d, q, mu, alpha, kept, induced, c, e, e2s, out)
#define GOP(AP, D) do { if (phi) GO(AP, D, true); else GO(AP, D, false); } while (0)
  if (allpairs) { if (damp == 0) GOP(true, 0); else GOP(true, 1); }
  else          { if (damp == 0) GOP(false, 0); else GOP(false, 1); }
#undef GOP
#undef GO
}

// out[4 * p .. 4 * p + 3] = {ex, ey, ez, phi} of point p (fractional coordinates s[3 * p ..]) over the rows r0 .. r1-1, added to
// what out holds on entry
extern "C" void ew_point_rows_eval(int phi, int npts, const double *s, const int *rows, const double *kv, const double *S, int r0, int r1,
                                   double *out) {
  const LibmMath m;
  const I4 *rw = reinterpret_cast<const I4 *>(rows);
  const D4 *k4 = reinterpret_cast<const D4 *>(kv);
  const D2 *s2 = reinterpret_cast<const D2 *>(S);
  for (int p = 0; p < npts; p++) {
    if (phi) polar::ew_point_rows<true>(m, s[3 * p], s[3 * p + 1], s[3 * p + 2], rw, k4, s2, r0, r1, out + 4 * (size_t)p);
    else polar::ew_point_rows<false>(m, s[3 * p], s[3 * p + 1], s[3 * p + 2], rw, k4, s2, r0, r1, out + 4 * (size_t)p);
  }
}

extern "C" void ew_point_chunking(int nrow, int nk, int *rows_per_chunk, int *nchunk) {
  *rows_per_chunk = polar::ew_point_rows_per_chunk(nrow, nk);
  *nchunk = polar::ew_point_chunks(nrow, nk);
}

#ifdef EWALD_POINT_MAIN
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
  const polar::EwPointParm e = polar::make_ew_point_parm(0.3243);
  const LibmMath m;
  for (int k = 0; k < n; k++) {
    const double r = 0.05 + 11.95 * g.uni();
    double u[3] = {g.sym(1.0), g.sym(1.0), g.sym(1.0)};
    const double un = std::sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]) + 1e-300;
    const double d[3] = {r * u[0] / un, r * u[1] / un, r * u[2] / un};
    const double q = g.sym(1.0), mu[3] = {g.sym(0.5), g.sym(0.5), g.sym(0.5)}, a = g.uni() < 0.25 ? 0.0 : 0.2 + g.uni();
    const bool kept = g.uni() < 0.8, induced = g.uni() < 0.9;
    polar::PointSums s0;
    double *v = &s0.esx;
    for (int j = 0; j < 8; j++) v[j] = g.sym(3.0);   // running sums that are not zero
    // the pair itself, with and without the potentials: the same field bits, ps and pi untouched without
    polar::PointSums s1 = s0, s2 = s0;
    polar::polar_point_pair_ew<AP, DAMP, true>(m, d[0], d[1], d[2], q, mu[0], mu[1], mu[2], a, kept, induced, c, e, s1);
    polar::polar_point_pair_ew<AP, DAMP, false>(m, d[0], d[1], d[2], q, mu[0], mu[1], mu[2], a, kept, induced, c, e, s2);
    checks++;
    if (!(same_bits(&s1.esx, &s2.esx, 3) && same_bits(&s1.eix, &s2.eix, 3) && same_bits(&s2.ps, &s0.ps, 1) && same_bits(&s2.pi, &s0.pi, 1))) failures++;
    for (int j = 0; j < 8; j++) sum += (&s1.esx)[j];
    // an atom on the point, kept or not: -q 2g/sqrt(pi) into the potential, nothing else
    polar::PointSums s3 = s0, s3e = s0;
    polar::polar_point_pair_ew<AP, DAMP, true>(m, 0.0, 0.0, 0.0, q, mu[0], mu[1], mu[2], a, kept, induced, c, e, s3);
    s3e.ps = __builtin_fma(-q, e.tgs, s0.ps);
    checks++;
    if (!same_bits(&s3.esx, &s3e.esx, 8)) failures++;
    // beyond cut_coul: an atom without polarizability (a stale dipole), or the skip_atom: nothing
    polar::PointSums s4 = s0;
    polar::polar_point_pair_ew<AP, DAMP, true>(m, 9.5 * u[0] / un, 9.5 * u[1] / un, 9.5 * u[2] / un, q, 5.0 * mu[0], 5.0 * mu[1], 5.0 * mu[2],
                                               (k & 1) ? 0.0 : a, kept, (k & 1) != 0, c, e, s4);
    checks++;
    if (!same_bits(&s4.esx, &s0.esx, 8)) failures++;
    // the skip_atom inside cut_coul: the static sums move (erf form), the induced ones do not
    polar::PointSums s5 = s0;
    polar::polar_point_pair_ew<AP, DAMP, true>(m, d[0], d[1], d[2], q, mu[0], mu[1], mu[2], a, false, false, c, e, s5);
    checks++;
    if (!(same_bits(&s5.eix, &s0.eix, 4))) failures++;
  }
}

// a small cubic table: rows over (h, k) with l = -2 .. 2 (without the origin), random S
void rows_check(Rng &g, long long &checks, long long &failures, double &sum) {
  std::vector<I4> rows;
  std::vector<D4> kv;
  std::vector<D2> S;
  for (int h = 0; h <= 2; h++)
    for (int k = (h == 0 ? 0 : -2); k <= 2; k++) {
      const int l0 = (h == 0 && k == 0) ? 1 : -2;
      rows.push_back(I4{h, k, l0, (int)kv.size()});
      for (int l = l0; l <= 2; l++) {
        kv.push_back(D4{0.3 * h, 0.3 * k, 0.3 * l, 1.0 / (1.0 + h * h + k * k + l * l)});
        S.push_back(D2{g.sym(2.0), g.sym(2.0)});
      }
    }
  const int nrow = (int)rows.size(), nk = (int)kv.size();
  rows.push_back(I4{0, 0, 0, nk});
  const LibmMath m;
  for (int p = 0; p < 50; p++) {
    const double s[3] = {g.uni(), g.uni(), g.uni()};
    double all[4] = {0, 0, 0, 0}, parts[4] = {0, 0, 0, 0}, nophi[4] = {0, 0, 0, 7.0};
    polar::ew_point_rows<true>(m, s[0], s[1], s[2], rows.data(), kv.data(), S.data(), 0, nrow, all);
    for (int r0 = 0; r0 < nrow; r0 += 5) polar::ew_point_rows<true>(m, s[0], s[1], s[2], rows.data(), kv.data(), S.data(), r0, std::min(nrow, r0 + 5), parts);
    polar::ew_point_rows<false>(m, s[0], s[1], s[2], rows.data(), kv.data(), S.data(), 0, nrow, nophi);
    checks += 2;
    if (!same_bits(all, parts, 4)) failures++;
    if (!(same_bits(all, nophi, 3) && nophi[3] == 7.0)) failures++;
    // the direct sum with libm phases
    double ref[4] = {0, 0, 0, 0}, scale = 0.0;
    for (int k = 0, r = 0; k < nk; k++) {
      while (rows[r + 1].w <= k) r++;
      const int l = rows[r].z + (k - rows[r].w);
      const double ph = 2.0 * 3.14159265358979323846 * (rows[r].x * s[0] + rows[r].y * s[1] + l * s[2]);
      const double im = std::sin(ph) * S[k].x - std::cos(ph) * S[k].y, re = std::cos(ph) * S[k].x + std::sin(ph) * S[k].y;
      ref[0] += kv[k].w * im * kv[k].x; ref[1] += kv[k].w * im * kv[k].y; ref[2] += kv[k].w * im * kv[k].z; ref[3] += kv[k].w * re;
      scale += kv[k].w * std::sqrt(S[k].x * S[k].x + S[k].y * S[k].y);
    }
    checks++;
    for (int j = 0; j < 4; j++) if (!(std::fabs(all[j] - ref[j]) <= 1e-12 * scale)) { failures++; break; }
    for (int j = 0; j < 4; j++) sum += all[j];
  }
  int rpc = 0, nchunk = 0;
  ew_point_chunking(nrow, nk, &rpc, &nchunk);
  checks++;
  if (!(rpc >= 1 && nchunk >= 1 && (long long)rpc * nchunk >= nrow && (long long)rpc * (nchunk - 1) < nrow)) failures++;
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
  const long long pair_checks = checks;
  rows_check(g, checks, failures, sum);
  // the library entry on a few pairs as well (the same code path the Python test calls)
  double d[6] = {1.0, 2.0, -0.5, 0.0, 0.0, 0.0}, q[2] = {0.3, -0.2}, mu[6] = {0.1, 0.0, -0.2, 0.3, 0.3, 0.3}, al[2] = {1.0, 0.0}, out[16];
  int kp[2] = {1, 0}, in[2] = {1, 1};
  for (int inst = 0; inst < 8; inst++) {
    ew_point_pair_eval(2, d, q, mu, al, kp, in, inst & 1, (inst >> 1) & 1, (inst >> 2) & 1, 9.0, 7.5, 2.1304, 18.22, 0.3243, out);
    for (int j = 0; j < 16; j++) sum += out[j];
  }
  printf("instances 4 inputs %d pair checks %lld row checks %lld failures %lld sum %.17g\n", n, pair_checks, checks - pair_checks, failures, sum);
  return failures == 0 && std::isfinite(sum) ? 0 : 1;
}
#endif
