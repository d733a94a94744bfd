// csrc/polar_ewald_point_grad.hpp on the host: libm behind the math policy.
//
// As a shared library (tests/test_ewald_point_grad_host.py): ew_point_grad_pair_eval() evaluates n pairs with one of the four
// instances of polar_point_grad_pair_ew (ALLPAIRS x DAMP) and returns 24 doubles per pair: the block as k_ew_grad_real stores it
// (e_static and g_static times e2s; e_static[3], e_induced[3], g_static[6], g_induced[6]) and the six field sums of
// polar_point_pair_ew<ALLPAIRS, DAMP, false> on the same pair.  ew_point_grad_rows_eval() runs ew_point_grad_rows for a set of
// points over a range of rows of a k-vector table, ew_point_rows_field_eval() runs ew_point_rows<false> over the same range.
// With -DEWALD_POINT_GRAD_MAIN a stand-alone program (the sanitizer build): random pairs through every instance and a small
// k-vector table through ew_point_grad_rows, with the exact properties the kernels rely on -- the field sums have the bits of
// polar_point_pair_ew / ew_point_rows, an atom beyond cut_coul without polarizability adds nothing, an atom on the point adds
// -(2/3) g^2 2g/sqrt(pi) q to the diagonal and nothing else, the skip_atom leaves the induced sums alone, and the rows of a
// table summed chunk by chunk are the rows summed at once when the chunks continue each other's sums.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "polar_ewald_point_grad.hpp"

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

const polar::PointGradSums kZero = {{0, 0, 0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0}};

template <bool AP, int DAMP>
void eval(int n, const double *d, const double *q, const double *mu, const double *alpha, const int *kept, const int *induced,
          const polar::PointCut &c, const polar::EwPointParm &e, double e2s, double *out) {
  const LibmMath m;
  for (int k = 0; k < n; k++) {
    polar::PointGradSums g = kZero;
    polar::PointSums s = {0, 0, 0, 0, 0, 0, 0, 0};
    polar::polar_point_grad_pair_ew<AP, DAMP>(m, d[3 * k], d[3 * k + 1], d[3 * k + 2], q[k], mu[3 * k], mu[3 * k + 1], mu[3 * k + 2], alpha[k],
                                              kept[k] != 0, induced[k] != 0, c, e, g);
    polar::polar_point_pair_ew<AP, DAMP, false>(m, d[3 * k], d[3 * k + 1], d[3 * k + 2], q[k], mu[3 * k], mu[3 * k + 1], mu[3 * k + 2], alpha[k],
                                                kept[k] != 0, induced[k] != 0, c, e, s);
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

extern "C" void ew_point_grad_pair_eval(int n, const double *d, const double *q, const double *mu, const double *alpha, const int *kept,
                                        const int *induced, int allpairs, int damp, double cut_coul, double dd_cutoff, double pd,
                                        double e2s, double g, double *out) {
  const polar::PointCut c = make_cut(cut_coul, dd_cutoff, pd);
  const polar::EwPointParm e = polar::make_ew_point_parm(g);
#define GO(AP, D) eval<AP, D>(n, d, q, mu, alpha, kept, induced, c, e, e2s, out)
  if (allpairs) { if (damp == 0) GO(true, 0); else GO(true, 1); }
  else          { if (damp == 0) GO(false, 0); else GO(false, 1); }
#undef GO
}

// out[9 * p .. 9 * p + 8] = {ex, ey, ez, gxx, gyy, gzz, gxy, gxz, gyz} of point p (fractional coordinates s[3 * p ..]) over the
// rows r0 .. r1-1, added to what out holds on entry
extern "C" void ew_point_grad_rows_eval(int npts, const double *s, const int *rows, const double *kv, const double *S, int r0, int r1,
                                        double *out) {
  const LibmMath m;
  for (int p = 0; p < npts; p++)
    polar::ew_point_grad_rows(m, s[3 * p], s[3 * p + 1], s[3 * p + 2], reinterpret_cast<const I4 *>(rows), reinterpret_cast<const D4 *>(kv),
                              reinterpret_cast<const D2 *>(S), r0, r1, out + 9 * (size_t)p);
}

// out[4 * p .. 4 * p + 2] = the field sums of ew_point_rows<false> over the same rows, added to what out holds on entry
extern "C" void ew_point_rows_field_eval(int npts, const double *s, const int *rows, const double *kv, const double *S, int r0, int r1,
                                         double *out) {
  const LibmMath m;
  for (int p = 0; p < npts; p++)
    polar::ew_point_rows<false>(m, s[3 * p], s[3 * p + 1], s[3 * p + 2], reinterpret_cast<const I4 *>(rows), reinterpret_cast<const D4 *>(kv),
                                reinterpret_cast<const D2 *>(S), r0, r1, out + 4 * (size_t)p);
}

#ifdef EWALD_POINT_GRAD_MAIN
namespace {

struct Rng {
  uint64_t s;
  double uni() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)(s >> 11) * (1.0 / 9007199254740992.0); }
  double sym(double a) { return a * (2.0 * uni() - 1.0); }
};

bool same_bits(const double *a, const double *b, int n) { return memcmp(a, b, (size_t)n * sizeof(double)) == 0; }

polar::PointGradSums random_sums(Rng &g) {
  polar::PointGradSums s = kZero;
  double *v = &s.f.esx;
  for (int j = 0; j < 8; j++) v[j] = g.sym(3.0);
  for (int j = 0; j < 6; j++) { s.gs[j] = g.sym(3.0); s.gi[j] = g.sym(3.0); }
  return s;
}

template <bool AP, int DAMP>
void instance(int n, Rng &g, long long &checks, long long &failures, double &sum) {
  const polar::PointCut c = make_cut(9.0, 7.5, 2.1304);
  const polar::EwPointParm e = polar::make_ew_point_parm(0.3243);
  const LibmMath m;
  for (int k = 0; k < n; k++) {
    const double r = 0.3 + 11.7 * g.uni();
    double u[3] = {g.sym(1.0), g.sym(1.0), g.sym(1.0)};
    const double un = std::sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]) + 1e-300;
    const double d[3] = {r * u[0] / un, r * u[1] / un, r * u[2] / un};
    const double q = g.sym(1.0), mu[3] = {g.sym(0.5), g.sym(0.5), g.sym(0.5)}, a = g.uni() < 0.25 ? 0.0 : 0.2 + g.uni();
    const bool kept = g.uni() < 0.8, induced = g.uni() < 0.9;
    const polar::PointGradSums s0 = random_sums(g);   // running sums that are not zero
    // the pair itself: its six field sums have the bits of polar_point_pair_ew<..., false>, ps and pi stay untouched
    polar::PointGradSums s1 = s0;
    polar::PointSums f1 = s0.f;
    polar::polar_point_grad_pair_ew<AP, DAMP>(m, d[0], d[1], d[2], q, mu[0], mu[1], mu[2], a, kept, induced, c, e, s1);
    polar::polar_point_pair_ew<AP, DAMP, false>(m, d[0], d[1], d[2], q, mu[0], mu[1], mu[2], a, kept, induced, c, e, f1);
    checks++;
    if (!same_bits(&s1.f.esx, &f1.esx, 8)) failures++;
    for (int j = 0; j < 6; j++) sum += s1.gs[j] + s1.gi[j];
    // an atom on the point, kept or not: -(2/3) g^2 2g/sqrt(pi) q onto xx, yy, zz, nothing else
    polar::PointGradSums s3 = s0, s3e = s0;
    polar::polar_point_grad_pair_ew<AP, DAMP>(m, 0.0, 0.0, 0.0, q, mu[0], mu[1], mu[2], a, kept, induced, c, e, s3);
    const double t0 = ((-2.0 / 3.0) * e.g2) * e.tgs;
    for (int j = 0; j < 3; j++) s3e.gs[j] = __builtin_fma(t0, q, s0.gs[j]);
    checks++;
    if (!(same_bits(&s3.f.esx, &s3e.f.esx, 8) && same_bits(s3.gs, s3e.gs, 6) && same_bits(s3.gi, s3e.gi, 6))) failures++;
    // beyond cut_coul: an atom without polarizability (a stale dipole), or the skip_atom: nothing
    polar::PointGradSums s4 = s0;
    polar::polar_point_grad_pair_ew<AP, DAMP>(m, 9.5 * u[0] / un, 9.5 * u[1] / un, 9.5 * u[2] / un, q, 5.0 * mu[0], 5.0 * mu[1], 5.0 * mu[2],
                                              (k & 1) ? 0.0 : a, kept, (k & 1) != 0, c, e, s4);
    checks++;
    if (!(same_bits(&s4.f.esx, &s0.f.esx, 8) && same_bits(s4.gs, s0.gs, 6) && same_bits(s4.gi, s0.gi, 6))) failures++;
    // the skip_atom inside cut_coul: the static sums move (erf form), the induced ones do not
    polar::PointGradSums s5 = s0;
    polar::polar_point_grad_pair_ew<AP, DAMP>(m, d[0], d[1], d[2], q, mu[0], mu[1], mu[2], a, false, false, c, e, s5);
    checks++;
    if (!(same_bits(&s5.f.eix, &s0.f.eix, 3) && same_bits(s5.gi, s0.gi, 6))) failures++;
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
  const int comp[6][2] = {{0, 0}, {1, 1}, {2, 2}, {0, 1}, {0, 2}, {1, 2}};
  for (int p = 0; p < 50; p++) {
    const double s[3] = {g.uni(), g.uni(), g.uni()};
    double all[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, parts[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, field[4] = {0, 0, 0, 7.0};
    polar::ew_point_grad_rows(m, s[0], s[1], s[2], rows.data(), kv.data(), S.data(), 0, nrow, all);
    for (int r0 = 0; r0 < nrow; r0 += 5) polar::ew_point_grad_rows(m, s[0], s[1], s[2], rows.data(), kv.data(), S.data(), r0, std::min(nrow, r0 + 5), parts);
    polar::ew_point_rows<false>(m, s[0], s[1], s[2], rows.data(), kv.data(), S.data(), 0, nrow, field);
    checks += 2;
    if (!same_bits(all, parts, 9)) failures++;
    if (!(same_bits(all, field, 3) && field[3] == 7.0)) failures++;
    // the direct sum with libm phases
    double ref[6] = {0, 0, 0, 0, 0, 0}, scale = 0.0;
    for (int k = 0, r = 0; k < nk; k++) {
      while (rows[r + 1].w <= k) r++;
      const int l = rows[r].z + (k - rows[r].w);
      const double ph = 2.0 * 3.14159265358979323846 * (rows[r].x * s[0] + rows[r].y * s[1] + l * s[2]);
      const double re = std::cos(ph) * S[k].x + std::sin(ph) * S[k].y;
      const double kk[3] = {kv[k].x, kv[k].y, kv[k].z};
      for (int j = 0; j < 6; j++) ref[j] += kv[k].w * re * kk[comp[j][0]] * kk[comp[j][1]];
      scale += kv[k].w * (kk[0] * kk[0] + kk[1] * kk[1] + kk[2] * kk[2]) * std::sqrt(S[k].x * S[k].x + S[k].y * S[k].y);
    }
    checks++;
    for (int j = 0; j < 6; j++) if (!(std::fabs(all[3 + j] - ref[j]) <= 1e-12 * scale)) { failures++; break; }
    for (int j = 0; j < 9; j++) sum += all[j];
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
  const long long pair_checks = checks;
  rows_check(g, checks, failures, sum);
  // the library entries on a few pairs and rows as well (the same code paths the Python test calls)
  double d[6] = {1.0, 2.0, -0.5, 0.0, 0.0, 0.0}, q[2] = {0.3, -0.2}, mu[6] = {0.1, 0.0, -0.2, 0.3, 0.3, 0.3}, al[2] = {1.0, 0.0}, out[48];
  int kp[2] = {1, 0}, in[2] = {1, 1};
  for (int inst = 0; inst < 4; inst++) {
    ew_point_grad_pair_eval(2, d, q, mu, al, kp, in, inst & 1, (inst >> 1) & 1, 9.0, 7.5, 2.1304, 18.22, 0.3243, out);
    for (int j = 0; j < 48; j++) sum += out[j];
  }
  const int rows[8] = {0, 0, 1, 0, 0, 0, 0, 2};
  const double kv[8] = {0.0, 0.0, 0.3, 0.5, 0.0, 0.0, 0.6, 0.25}, S[4] = {1.0, -0.5, 0.25, 2.0}, s3[3] = {0.1, 0.2, 0.3};
  double o9[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, o4[4] = {0, 0, 0, 0};
  ew_point_grad_rows_eval(1, s3, rows, kv, S, 0, 1, o9);
  ew_point_rows_field_eval(1, s3, rows, kv, S, 0, 1, o4);
  checks++;
  if (!same_bits(o9, o4, 3)) failures++;
  for (int j = 0; j < 9; j++) sum += o9[j];
  printf("instances 4 inputs %d pair checks %lld row checks %lld failures %lld sum %.17g\n", n, pair_checks, checks - pair_checks, failures, sum);
  return failures == 0 && std::isfinite(sum) ? 0 : 1;
}
#endif
