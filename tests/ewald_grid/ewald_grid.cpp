// csrc/polar_ewald_grid.hpp on the host, with the layout arithmetic of csrc/polar_plan.hpp and the input decisions of
// csrc/polar_input.hpp behind it: libm behind the math policy.
//
// As a shared library (tests/test_ewald_grid_host.py): ew_grid_recip_eval() runs a whole call the way the launchers of
// polar_step.hip do -- layout from the rows table, phase tables, stage 1, then pass by pass and run of lines by run of lines
// stages 2 and 3 -- and returns {ex, ey, ez, phi} per point, without e2s; ew_grid_points_eval() the points of a range of flat
// indices; ew_grid_plan_eval() / ew_grid_runs_eval() the layout; ew_grid_check() what check_grid decides.
// With -DEWALD_GRID_MAIN a stand-alone program (the sanitizer build): a small tilted table through the three stages on a few
// grids against the direct sum with libm phases, passes and line runs of every size against one pass bit for bit, the
// field bits with and without the potential, the tiling of passes into runs, and the refusals of check_grid.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "polar_input.hpp"
#include "polar_ewald_grid.hpp"

namespace {

struct LibmMath {
  void sincospi(double x, double *s, double *c) const {
    const double y = x - 2.0 * std::rint(0.5 * x);   // exact: |y| <= 1
    const double pi = 3.14159265358979323846;
    *s = std::sin(pi * y); *c = std::cos(pi * y);
  }
};

struct D4 { double x, y, z, w; };
struct D2 { double x, y; };
using I4 = polar::PlanI4;

polar::EwGrid make_grid(const int n[3], const double off[3], const double lo[3], const double box[6], const double cell[6]) {
  polar::EwGrid g;
  for (int a = 0; a < 3; a++) { g.n[a] = n[a]; g.off[a] = off[a]; g.lo[a] = lo[a]; }
  g.ax = box[0]; g.bx = box[1]; g.by = box[2]; g.cx = box[3]; g.cy = box[4]; g.cz = box[5];
  polar::ew_grid_slo(cell, lo, g.slo);
  return g;
}

// a call, as ewald_field_grid_begin / ewald_field_grid_pass lay it out: `chunk` points per pass, `lpr` lines per run (0: the
// plan's own).  Returns the largest V of a run, in bytes.
template <bool PHI>
size_t recip(const polar::EwGrid &g, int nrow, const I4 *rows, const D4 *kv, const D2 *S, long long chunk, long long lpr, double *out) {
  const LibmMath m;
  const polar::EwGridPlan plan = polar::ew_grid_plan(rows, nrow);
  const polar::EwGridSizes sz = polar::ew_grid_sizes(plan, nrow, g.n);
  if (lpr <= 0) lpr = polar::ew_grid_lines_per_run(sz.v_line_bytes);
  const int nx = g.n[0], ny = g.n[1], nz = g.n[2], hmax = plan.hmax;
  std::vector<D2> tab(sz.tab), T(sz.t);
  for (size_t e = 0; e < sz.tab; e++) polar::ew_grid_tab_entry(m, g, plan.kmax, plan.lmax, sz.off_y, sz.off_z, e, tab[e].x, tab[e].y);
  for (int r = 0; r < nrow; r++)
    for (int gz = 0; gz < nz; gz++) polar::ew_grid_stage_l(rows, kv, S, tab.data() + sz.off_z, nz, plan.lmax, r, gz, T.data() + ((size_t)r * nz + gz) * 4);
  const long long npts = (long long)nx * ny * nz;
  size_t vmax = 0;
  std::vector<D2> V;
  for (long long p0 = 0; p0 < npts; p0 += chunk) {
    const long long mm = std::min(chunk, npts - p0);
    for (const polar::EwGridRun &r : polar::ew_grid_runs(p0, mm, nx, lpr)) {
      const size_t nl = (size_t)(r.lb - r.la);
      V.assign(nl * (size_t)(hmax + 1) * 4, D2{0.0, 0.0});
      vmax = std::max(vmax, V.size() * sizeof(D2));
      for (int h = 0; h <= hmax; h++)
        for (long long line = r.la; line < r.lb; line++)
          polar::ew_grid_stage_k(rows, T.data(), tab.data() + sz.off_y, plan.first[h], plan.first[h + 1], nz, ny, plan.kmax, (int)(line / ny),
                                 (int)(line % ny), V.data() + ((size_t)h * nl + (size_t)(line - r.la)) * 4);
      for (long long q = r.q0; q < r.q1; q++) {
        const long long line = q / nx;
        polar::ew_grid_stage_h<PHI>(V.data() + (size_t)(line - r.la) * 4, nl * 4, tab.data(), nx, hmax, (int)(q - line * nx), out + 4 * (size_t)q);
      }
    }
  }
  return vmax;
}

}  // namespace

extern "C" long long ew_grid_recip_eval(int phi, const int *n, const double *off, const double *lo, const double *box, const double *cell,
                                        int nrow, const int *rows, const double *kv, const double *S, long long chunk, long long lpr,
                                        double *out) {
  const polar::EwGrid g = make_grid(n, off, lo, box, cell);
  const I4 *rw = reinterpret_cast<const I4 *>(rows);
  const D4 *k4 = reinterpret_cast<const D4 *>(kv);
  const D2 *s2 = reinterpret_cast<const D2 *>(S);
  return (long long)(phi ? recip<true>(g, nrow, rw, k4, s2, chunk, lpr, out) : recip<false>(g, nrow, rw, k4, s2, chunk, lpr, out));
}

extern "C" void ew_grid_points_eval(const int *n, const double *off, const double *lo, const double *box, const double *cell, long long p0,
                                    long long m, double *x) {
  const polar::EwGrid g = make_grid(n, off, lo, box, cell);
  for (long long t = 0; t < m; t++) polar::ew_grid_point(g, p0 + t, x[3 * t], x[3 * t + 1], x[3 * t + 2]);
}

// bounds = {hmax, kmax, lmax, ok}; first[hmax + 2] (the caller's array holds nfirst entries; what does not fit is left out);
// sizes = {off_y, off_z, tab, t, v_line_bytes, lines_per_run}
extern "C" void ew_grid_plan_eval(int nrow, const int *rows, const int *n, int *bounds, int *first, int nfirst, long long *sizes) {
  const polar::EwGridPlan p = polar::ew_grid_plan(reinterpret_cast<const I4 *>(rows), nrow);
  bounds[0] = p.hmax; bounds[1] = p.kmax; bounds[2] = p.lmax; bounds[3] = p.ok ? 1 : 0;
  for (size_t k = 0; k < p.first.size() && (int)k < nfirst; k++) first[k] = p.first[k];
  const polar::EwGridSizes s = polar::ew_grid_sizes(p, nrow, n);
  sizes[0] = (long long)s.off_y; sizes[1] = (long long)s.off_z; sizes[2] = (long long)s.tab; sizes[3] = (long long)s.t;
  sizes[4] = (long long)s.v_line_bytes; sizes[5] = polar::ew_grid_lines_per_run(s.v_line_bytes);
}

// runs[4 r ..] = {la, lb, q0, q1}; returns the number of runs (at most max are written)
extern "C" int ew_grid_runs_eval(long long p0, long long m, long long nx, long long lpr, int max, long long *runs) {
  const std::vector<polar::EwGridRun> r = polar::ew_grid_runs(p0, m, nx, lpr);
  for (size_t k = 0; k < r.size() && (int)k < max; k++) { runs[4 * k] = r[k].la; runs[4 * k + 1] = r[k].lb; runs[4 * k + 2] = r[k].q0; runs[4 * k + 3] = r[k].q1; }
  return (int)r.size();
}

// POLAR_OK or POLAR_ERR_INPUT; off and npts are filled when the grid is accepted.  offset may be null
extern "C" int ew_grid_check(const int *n, const double *offset, double *off, long long *npts) {
  try {
    *npts = polar::check_grid(n, offset, off);
    return POLAR_OK;
  } catch (const polar::InputError &) {
    return POLAR_ERR_INPUT;
  }
}

#ifdef EWALD_GRID_MAIN
namespace {

struct Rng {
  uint64_t s;
  double uni() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)(s >> 11) * (1.0 / 9007199254740992.0); }
  double sym(double a) { return a * (2.0 * uni() - 1.0); }
};

bool same_bits(const double *a, const double *b, size_t n) { return memcmp(a, b, n * sizeof(double)) == 0; }

}  // namespace

int main() {
  Rng g{0x9E3779B97F4A7C15ull};
  long long checks = 0, failures = 0;
  double sum = 0.0;
  // a tilted box with its origin off zero; the half space |h| <= 2, |k| <= 3, |l| <= 2 with a dent, so that the rows differ in length
  const double box[6] = {11.0, 1.3, 9.0, -0.8, 0.6, 10.0}, lo[3] = {-3.0, 2.5, 40.0};
  const double lx = box[0], xy = box[1], ly = box[2], xz = box[3], yz = box[4], lz = box[5];
  const double cell[6] = {1.0 / lx, -xy / (lx * ly), (xy * yz - ly * xz) / (lx * ly * lz), 1.0 / ly, -yz / (ly * lz), 1.0 / lz};
  const double twopi = 2.0 * 3.14159265358979323846;
  std::vector<I4> rows;
  std::vector<D4> kv;
  std::vector<D2> S;
  for (int h = 0; h <= 2; h++)
    for (int k = (h == 0 ? 0 : -3); k <= 3; k++) {
      const int lmax = 2 - (std::abs(k) == 3 ? 1 : 0), l0 = (h == 0 && k == 0) ? 1 : -lmax;
      rows.push_back(I4{h, k, l0, (int)kv.size()});
      for (int l = l0; l <= lmax; l++) {
        const double kx = twopi * (h * cell[0]), ky = twopi * (h * cell[1] + k * cell[3]), kz = twopi * (h * cell[2] + k * cell[4] + l * cell[5]);
        kv.push_back(D4{kx, ky, kz, 1.0 / (1.0 + h * h + k * k + l * l)});
        S.push_back(D2{g.sym(2.0), g.sym(2.0)});
      }
    }
  const int nrow = (int)rows.size(), nk = (int)kv.size();
  rows.push_back(I4{0, 0, 0, nk});
  double scale_e = 0.0, scale_p = 0.0;
  for (int k = 0; k < nk; k++) {
    const double a = kv[k].w * std::sqrt(S[k].x * S[k].x + S[k].y * S[k].y);
    scale_p += a; scale_e += a * std::sqrt(kv[k].x * kv[k].x + kv[k].y * kv[k].y + kv[k].z * kv[k].z);
  }
  const int grids[4][3] = {{8, 6, 4}, {5, 7, 3}, {67, 3, 2}, {1, 1, 1}};
  const double offs[4][3] = {{0.5, 0.5, 0.5}, {0.0, 0.25, 0.9}, {0.5, 0.5, 0.5}, {0.5, 0.5, 0.5}};
  for (int c = 0; c < 4; c++) {
    const int *n = grids[c];
    const long long npts = (long long)n[0] * n[1] * n[2];
    std::vector<double> all(4 * npts, 0.0), x(3 * npts);
    ew_grid_recip_eval(1, n, offs[c], lo, box, cell, nrow, &rows[0].x, &kv[0].x, &S[0].x, npts, 0, all.data());
    ew_grid_points_eval(n, offs[c], lo, box, cell, 0, npts, x.data());
    // the direct sum at the points, libm phases of k.p
    for (long long p = 0; p < npts; p++) {
      double ref[4] = {0, 0, 0, 0};
      for (int k = 0; k < nk; k++) {
        const double ph = kv[k].x * x[3 * p] + kv[k].y * x[3 * p + 1] + kv[k].z * x[3 * p + 2];
        const double im = std::sin(ph) * S[k].x - std::cos(ph) * S[k].y, re = std::cos(ph) * S[k].x + std::sin(ph) * S[k].y;
        ref[0] += kv[k].w * im * kv[k].x; ref[1] += kv[k].w * im * kv[k].y; ref[2] += kv[k].w * im * kv[k].z; ref[3] += kv[k].w * re;
      }
      checks++;
      for (int j = 0; j < 4; j++)
        if (!(std::fabs(all[4 * p + j] - ref[j]) <= 1e-12 * (j < 3 ? scale_e : scale_p))) { failures++; break; }
      for (int j = 0; j < 4; j++) sum += all[4 * p + j];
    }
    // passes and runs of lines of other sizes: the same bits; without the potential: the same field bits, phi untouched
    const long long chunks[3] = {1, 37, 5}, lprs[3] = {1, 2, 3};
    for (int v = 0; v < 3; v++) {
      std::vector<double> part(4 * npts, 0.0);
      ew_grid_recip_eval(1, n, offs[c], lo, box, cell, nrow, &rows[0].x, &kv[0].x, &S[0].x, chunks[v], lprs[v], part.data());
      checks++;
      if (!same_bits(all.data(), part.data(), all.size())) failures++;
    }
    std::vector<double> nophi(4 * npts, 7.0);
    for (long long p = 0; p < npts; p++) nophi[4 * p] = nophi[4 * p + 1] = nophi[4 * p + 2] = 0.0;
    ew_grid_recip_eval(0, n, offs[c], lo, box, cell, nrow, &rows[0].x, &kv[0].x, &S[0].x, 37, 2, nophi.data());
    checks++;
    for (long long p = 0; p < npts; p++)
      if (!(same_bits(&all[4 * p], &nophi[4 * p], 3) && nophi[4 * p + 3] == 7.0)) { failures++; break; }
  }
  // the layout: bounds, first rows, tiling
  int bounds[4], first[8];
  long long sizes[6];
  const int n3[3] = {8, 6, 4};
  ew_grid_plan_eval(nrow, &rows[0].x, n3, bounds, first, 8, sizes);
  checks++;
  if (!(bounds[0] == 2 && bounds[1] == 3 && bounds[2] == 2 && bounds[3] == 1 && first[0] == 0 && first[1] == 4 && first[2] == 11 && first[3] == nrow &&
        sizes[0] == 3 * 8 && sizes[1] == 3 * 8 + 7 * 6 && sizes[2] == 3 * 8 + 7 * 6 + 5 * 4 && sizes[3] == (long long)nrow * 4 * 4 && sizes[4] == 3 * 64))
    failures++;
  for (long long p0 = 0; p0 < 100; p0 += 13)
    for (long long m = 1; m < 60; m += 7)
      for (long long lpr = 1; lpr <= 4; lpr++) {
        long long runs[4 * 64];
        const int nr = ew_grid_runs_eval(p0, m, 8, lpr, 64, runs);
        long long q = p0;
        bool ok = nr >= 1 && nr <= 64;
        for (int r = 0; ok && r < nr; r++) {
          ok = runs[4 * r + 2] == q && runs[4 * r + 3] > q && runs[4 * r + 1] - runs[4 * r] <= lpr && runs[4 * r] * 8 <= runs[4 * r + 2] && runs[4 * r + 3] <= runs[4 * r + 1] * 8;
          q = runs[4 * r + 3];
        }
        checks++;
        if (!(ok && q == p0 + m)) failures++;
      }
  // check_grid
  double off[3];
  long long npts = 0;
  const int bad_n[3][3] = {{0, 4, 4}, {4, -1, 4}, {2048, 2048, 512}}, good_n[3] = {2047, 1024, 1024};
  const double nan = std::nan(""), bad_off[3][3] = {{1.0, 0.5, 0.5}, {0.5, -1e-9, 0.5}, {0.5, 0.5, nan}};
  for (int k = 0; k < 3; k++) { checks++; if (ew_grid_check(bad_n[k], nullptr, off, &npts) != POLAR_ERR_INPUT) failures++; }
  for (int k = 0; k < 3; k++) { checks++; if (ew_grid_check(n3, bad_off[k], off, &npts) != POLAR_ERR_INPUT) failures++; }
  checks++;
  if (!(ew_grid_check(good_n, nullptr, off, &npts) == POLAR_OK && npts == 2047ll * 1024 * 1024 && off[0] == 0.5 && off[1] == 0.5 && off[2] == 0.5)) failures++;
  printf("grids 4 k-vectors %d rows %d checks %lld failures %lld sum %.17g\n", nk, nrow, checks, failures, sum);
  return failures == 0 && std::isfinite(sum) ? 0 : 1;
}
#endif
