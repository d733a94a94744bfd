// csrc/polar_ewald_grid_grad.hpp on the host, with the layout arithmetic of csrc/polar_plan.hpp behind it: libm behind the math
// policy, as tests/ewald_grid/ewald_grid.cpp.
//
// As a shared library (tests/test_ewald_grid_grad_host.py): ew_gg_recip_eval() runs a whole call the way the launchers of
// polar_step.hip do -- layout from the rows table with nine sets, phase tables, stage 1, then pass by pass and run of lines by run
// of lines stages 2 and 3 -- and returns {ex, ey, ez, gxx, gyy, gzz, gxy, gxz, gyz} per point, without e2s; ew_gg_sizes_eval() the
// layout sizes.
// With -DEWALD_GRID_GRAD_MAIN a stand-alone program (the sanitizer build): a small tilted table through the three stages on a few
// grids against the direct sum with libm phases, passes and line runs of every size against one pass bit for bit, the gradient
// bits with and without the field, and the field bits against the four-set stages of csrc/polar_ewald_grid.hpp.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "polar_input.hpp"
#include "polar_ewald_grid_grad.hpp"

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
constexpr int NS = polar::EW_GG_SETS;

polar::EwGrid make_grid(const int n[3], const double off[3], const double lo[3], const double box[6], const double cell[6]) {
  polar::EwGrid g;
  for (int a = 0; a < 3; a++) { g.n[a] = n[a]; g.off[a] = off[a]; g.lo[a] = lo[a]; }
  g.ax = box[0]; g.bx = box[1]; g.by = box[2]; g.cx = box[3]; g.cy = box[4]; g.cz = box[5];
  polar::ew_grid_slo(cell, lo, g.slo);
  return g;
}

// a call, as ewald_field_grad_grid_begin / ewald_field_grad_grid_pass lay it out: `chunk` points per pass, `lpr` lines per run
// (0: the plan's own).  Returns the largest V of a run, in bytes.
template <bool FIELD>
size_t recip(const polar::EwGrid &g, int nrow, const I4 *rows, const D4 *kv, const D2 *S, long long chunk, long long lpr, double *out) {
  const LibmMath m;
  const polar::EwGridPlan plan = polar::ew_grid_plan(rows, nrow);
  const polar::EwGridSizes sz = polar::ew_grid_sizes(plan, nrow, g.n, NS);
  if (lpr <= 0) lpr = polar::ew_grid_lines_per_run(sz.v_line_bytes);
  const int nx = g.n[0], ny = g.n[1], nz = g.n[2], hmax = plan.hmax;
  std::vector<D2> tab(sz.tab), T(sz.t);
  for (size_t e = 0; e < sz.tab; e++) polar::ew_grid_tab_entry(m, g, plan.kmax, plan.lmax, sz.off_y, sz.off_z, e, tab[e].x, tab[e].y);
  for (int r = 0; r < nrow; r++)
    for (int gz = 0; gz < nz; gz++) polar::ew_gg_stage_l(rows, kv, S, tab.data() + sz.off_z, nz, plan.lmax, r, gz, T.data() + ((size_t)r * nz + gz) * NS);
  const long long npts = (long long)nx * ny * nz;
  size_t vmax = 0;
  std::vector<D2> V;
  for (long long p0 = 0; p0 < npts; p0 += chunk) {
    const long long mm = std::min(chunk, npts - p0);
    for (const polar::EwGridRun &r : polar::ew_grid_runs(p0, mm, nx, lpr)) {
      const size_t nl = (size_t)(r.lb - r.la);
      V.assign(nl * (size_t)(hmax + 1) * NS, D2{0.0, 0.0});
      vmax = std::max(vmax, V.size() * sizeof(D2));
      for (int h = 0; h <= hmax; h++)
        for (long long line = r.la; line < r.lb; line++)
          polar::ew_gg_stage_k(rows, T.data(), tab.data() + sz.off_y, plan.first[h], plan.first[h + 1], nz, ny, plan.kmax, (int)(line / ny),
                               (int)(line % ny), V.data() + ((size_t)h * nl + (size_t)(line - r.la)) * NS);
      for (long long q = r.q0; q < r.q1; q++) {
        const long long line = q / nx;
        polar::ew_gg_stage_h<FIELD>(V.data() + (size_t)(line - r.la) * NS, nl * NS, tab.data(), nx, hmax, (int)(q - line * nx), out + NS * (size_t)q);
      }
    }
  }
  return vmax;
}

}  // namespace

extern "C" long long ew_gg_recip_eval(int field, const int *n, const double *off, const double *lo, const double *box, const double *cell,
                                      int nrow, const int *rows, const double *kv, const double *S, long long chunk, long long lpr,
                                      double *out) {
  const polar::EwGrid g = make_grid(n, off, lo, box, cell);
  const I4 *rw = reinterpret_cast<const I4 *>(rows);
  const D4 *k4 = reinterpret_cast<const D4 *>(kv);
  const D2 *s2 = reinterpret_cast<const D2 *>(S);
  return (long long)(field ? recip<true>(g, nrow, rw, k4, s2, chunk, lpr, out) : recip<false>(g, nrow, rw, k4, s2, chunk, lpr, out));
}

// sizes = {sets, t, v_line_bytes, lines_per_run, hmax}
extern "C" void ew_gg_sizes_eval(int nrow, const int *rows, const int *n, long long *sizes) {
  const polar::EwGridPlan p = polar::ew_grid_plan(reinterpret_cast<const I4 *>(rows), nrow);
  const polar::EwGridSizes s = polar::ew_grid_sizes(p, nrow, n, NS);
  sizes[0] = NS; sizes[1] = (long long)s.t; sizes[2] = (long long)s.v_line_bytes; sizes[3] = polar::ew_grid_lines_per_run(s.v_line_bytes);
  sizes[4] = p.hmax;
}

#ifdef EWALD_GRID_GRAD_MAIN
namespace {

struct Rng {
  uint64_t s;
  double uni() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)(s >> 11) * (1.0 / 9007199254740992.0); }
  double sym(double a) { return a * (2.0 * uni() - 1.0); }
};

bool same_bits(const double *a, const double *b, size_t n) { return memcmp(a, b, n * sizeof(double)) == 0; }

// the field of the four-set stages of polar_ewald_grid.hpp, one pass, one run of all lines: {ex, ey, ez} per point
void field4(const polar::EwGrid &g, int nrow, const I4 *rows, const D4 *kv, const D2 *S, double *out3) {
  const LibmMath m;
  const polar::EwGridPlan plan = polar::ew_grid_plan(rows, nrow);
  const polar::EwGridSizes sz = polar::ew_grid_sizes(plan, nrow, g.n);
  const int nx = g.n[0], ny = g.n[1], nz = g.n[2], hmax = plan.hmax;
  std::vector<D2> tab(sz.tab), T(sz.t);
  for (size_t e = 0; e < sz.tab; e++) polar::ew_grid_tab_entry(m, g, plan.kmax, plan.lmax, sz.off_y, sz.off_z, e, tab[e].x, tab[e].y);
  for (int r = 0; r < nrow; r++)
    for (int gz = 0; gz < nz; gz++) polar::ew_grid_stage_l(rows, kv, S, tab.data() + sz.off_z, nz, plan.lmax, r, gz, T.data() + ((size_t)r * nz + gz) * 4);
  const size_t nl = (size_t)ny * nz;
  std::vector<D2> V(nl * (size_t)(hmax + 1) * 4);
  for (int h = 0; h <= hmax; h++)
    for (size_t line = 0; line < nl; line++)
      polar::ew_grid_stage_k(rows, T.data(), tab.data() + sz.off_y, plan.first[h], plan.first[h + 1], nz, ny, plan.kmax, (int)(line / ny), (int)(line % ny),
                             V.data() + ((size_t)h * nl + line) * 4);
  for (size_t q = 0; q < nl * nx; q++) {
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    polar::ew_grid_stage_h<false>(V.data() + (q / nx) * 4, nl * 4, tab.data(), nx, hmax, (int)(q % nx), a);
    out3[3 * q] = a[0]; out3[3 * q + 1] = a[1]; out3[3 * q + 2] = a[2];
  }
}

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
  double scale_e = 0.0, scale_g = 0.0;
  for (int k = 0; k < nk; k++) {
    const double a = kv[k].w * std::sqrt(S[k].x * S[k].x + S[k].y * S[k].y), k2 = kv[k].x * kv[k].x + kv[k].y * kv[k].y + kv[k].z * kv[k].z;
    scale_e += a * std::sqrt(k2); scale_g += a * k2;
  }
  const int grids[5][3] = {{8, 6, 4}, {5, 7, 3}, {67, 3, 2}, {1, 1, 1}, {3, 1, 130}};
  const double offs[5][3] = {{0.5, 0.5, 0.5}, {0.0, 0.25, 0.9}, {0.5, 0.5, 0.5}, {0.5, 0.5, 0.5}, {0.0, 0.25, 0.9}};
  for (int c = 0; c < 5; c++) {
    const int *n = grids[c];
    const long long npts = (long long)n[0] * n[1] * n[2];
    const polar::EwGrid grid = make_grid(n, offs[c], lo, box, cell);
    std::vector<double> all(NS * npts, 0.0), x(3 * npts), f4(3 * npts);
    ew_gg_recip_eval(1, n, offs[c], lo, box, cell, nrow, &rows[0].x, &kv[0].x, &S[0].x, npts, 0, all.data());
    for (long long p = 0; p < npts; p++) polar::ew_grid_point(grid, p, x[3 * p], x[3 * p + 1], x[3 * p + 2]);
    // the direct sum at the points, libm phases of k.p
    for (long long p = 0; p < npts; p++) {
      double ref[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
      for (int k = 0; k < nk; k++) {
        const double ph = kv[k].x * x[3 * p] + kv[k].y * x[3 * p + 1] + kv[k].z * x[3 * p + 2];
        const double im = std::sin(ph) * S[k].x - std::cos(ph) * S[k].y, re = std::cos(ph) * S[k].x + std::sin(ph) * S[k].y;
        const double kk[3] = {kv[k].x, kv[k].y, kv[k].z};
        const int ia[6] = {0, 1, 2, 0, 0, 1}, ib[6] = {0, 1, 2, 1, 2, 2};
        for (int j = 0; j < 3; j++) ref[j] += kv[k].w * im * kk[j];
        for (int j = 0; j < 6; j++) ref[3 + j] += kv[k].w * re * kk[ia[j]] * kk[ib[j]];
      }
      checks++;
      for (int j = 0; j < 9; j++)
        if (!(std::fabs(all[NS * p + j] - ref[j]) <= 1e-12 * (j < 3 ? scale_e : scale_g))) { failures++; break; }
      for (int j = 0; j < 9; j++) sum += all[NS * p + j];
    }
    // the field sets: the bits of the four-set stages
    field4(grid, nrow, rows.data(), kv.data(), S.data(), f4.data());
    checks++;
    for (long long p = 0; p < npts; p++)
      if (!same_bits(&all[NS * p], &f4[3 * p], 3)) { failures++; break; }
    // passes and runs of lines of other sizes: the same bits; without the field: the same gradient bits, the field untouched
    const long long chunks[3] = {1, 37, 5}, lprs[3] = {1, 2, 3};
    for (int v = 0; v < 3; v++) {
      std::vector<double> part(NS * npts, 0.0);
      ew_gg_recip_eval(1, n, offs[c], lo, box, cell, nrow, &rows[0].x, &kv[0].x, &S[0].x, chunks[v], lprs[v], part.data());
      checks++;
      if (!same_bits(all.data(), part.data(), all.size())) failures++;
    }
    std::vector<double> nof(NS * npts, 0.0);
    for (long long p = 0; p < npts; p++) nof[NS * p] = nof[NS * p + 1] = nof[NS * p + 2] = 7.0;
    ew_gg_recip_eval(0, n, offs[c], lo, box, cell, nrow, &rows[0].x, &kv[0].x, &S[0].x, 37, 2, nof.data());
    checks++;
    for (long long p = 0; p < npts; p++)
      if (!(same_bits(&all[NS * p + 3], &nof[NS * p + 3], 6) && nof[NS * p] == 7.0 && nof[NS * p + 1] == 7.0 && nof[NS * p + 2] == 7.0)) { failures++; break; }
  }
  // the layout: nine sets in T and V
  long long sizes[5];
  const int n3[3] = {8, 6, 4};
  ew_gg_sizes_eval(nrow, &rows[0].x, n3, sizes);
  checks++;
  if (!(sizes[0] == 9 && sizes[1] == (long long)nrow * 4 * 9 && sizes[2] == 3 * 9 * 16 && sizes[3] == (64ll << 20) / (3 * 9 * 16) && sizes[4] == 2)) failures++;
  printf("grids 5 k-vectors %d rows %d checks %lld failures %lld sum %.17g\n", nk, nrow, checks, failures, sum);
  return failures == 0 && std::isfinite(sum) ? 0 : 1;
}
#endif
