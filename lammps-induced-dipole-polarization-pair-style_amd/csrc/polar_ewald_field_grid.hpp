// polar_ewald_field_grid.hpp -- the Ewald field and potential of the polarized box on a regular grid of the cell
// (polar_ewald_field_grid() of include/polar_mi355x.h; arithmetic and formulas: polar_ewald_grid.hpp).  Part
// of the hand-written HIP kernels (gfx950 / CDNA4, wave64) of the lj/cut/coul/long/polarization pair style.
//
// The real-space static sums and the induced sums are k_ew_point_real's (polar_ewald_field_at.hpp), on points that
// k_ew_grid_points writes on the device.  The reciprocal sums over the step's k-vector table run as three 1-D transforms:
// k_ew_grid_tab: the three phase tables, one thread per entry, one sincospi each.  Once per call.
// k_ew_grid_l: stage 1, T[row][g_z][4].  One wave per (row, 64 g_z): kv, S and rows are wave-uniform loads, the z table is read
//   coalesced.  Once per call.
// k_ew_grid_k: stage 2, V[h][line][4] for a run of whole lines.  One wave per (h, g_z, 64 g_y): T is wave-uniform, the y table
//   coalesced; lanes outside the run's lines write nothing.
// k_ew_grid_h: stage 3 and the fold.  One wave per (line, 64 g_x), one thread per point: the line's V column is wave-uniform
//   (four 16-byte values per h, read through the scalar cache), the x table coalesced; eight FMAs per (point, h), six without
//   the potential.  Folds onto the real-space results in k_ew_point_fold's form -- fma(e2s, a, es), the potential with the
//   neutralising-background term -- so the per-point partials never exist.
// No atomics, no LDS; every output element is one fixed-order loop, so a point's bits depend on the grid, the records and the
// k-vector table, not on its pass or on the run of lines it was computed in.
#pragma once

#include "polar_common.hpp"
#include "polar_ewald_field_at.hpp"   // EwRecipMath, FieldAtOut
#include "polar_ewald_grid.hpp"

namespace polar {

// the points p0 .. p0 + np - 1 of the flat order -> xp[3 t]
static __global__ __launch_bounds__(256) void k_ew_grid_points(int np, long long p0, EwGrid g, double *__restrict__ xp) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= np) return;
  double px, py, pz;
  ew_grid_point(g, p0 + t, px, py, pz);
  xp[3 * (size_t)t] = px; xp[3 * (size_t)t + 1] = py; xp[3 * (size_t)t + 2] = pz;
}

static __global__ __launch_bounds__(256) void k_ew_grid_tab(size_t ntab, EwGrid g, int kmax, int lmax, size_t off_y, size_t off_z,
                                                            double2 *__restrict__ tab) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= ntab) return;
  const EwRecipMath m;
  double c, s;
  ew_grid_tab_entry(m, g, kmax, lmax, off_y, off_z, e, c, s);
  tab[e] = make_double2(c, s);
}

// grid = nrow x nzb blocks of 64 threads
static __global__ __launch_bounds__(64) void k_ew_grid_l(int nrow, int nz, int nzb, int lmax, const int4 *__restrict__ rows,
                                                         const double4 *__restrict__ kv, const double2 *__restrict__ S,
                                                         const double2 *__restrict__ pz, double2 *__restrict__ T) {
  const int row = blockIdx.x / nzb, gz = (blockIdx.x - row * nzb) * 64 + threadIdx.x;
  if (row >= nrow || gz >= nz) return;
  double2 t[4];
  ew_grid_stage_l(rows, kv, S, pz, nz, lmax, row, gz, t);
  double2 *o = T + ((size_t)row * (size_t)nz + (size_t)gz) * 4;
  o[0] = t[0]; o[1] = t[1]; o[2] = t[2]; o[3] = t[3];
}

// V of the lines la .. lb-1 (nl = lb - la): grid = (hmax + 1) x ngz x nyb blocks of 64 threads, gz0 = la / ny
static __global__ __launch_bounds__(64) void k_ew_grid_k(long long la, long long lb, int gz0, int ngz, int nyb, int nz, int ny, int kmax,
                                                         const int *__restrict__ first, const int4 *__restrict__ rows,
                                                         const double2 *__restrict__ T, const double2 *__restrict__ py,
                                                         double2 *__restrict__ V) {
  const int per_h = ngz * nyb;
  const int h = blockIdx.x / per_h, rest = blockIdx.x - h * per_h;
  const int gz = gz0 + rest / nyb, gy = (rest % nyb) * 64 + threadIdx.x;
  if (gy >= ny || gz >= nz) return;
  const long long line = (long long)gz * ny + gy;
  if (line < la || line >= lb) return;
  double2 v[4];
  ew_grid_stage_k(rows, T, py, first[h], first[h + 1], nz, ny, kmax, gz, gy, v);
  double2 *o = V + ((size_t)h * (size_t)(lb - la) + (size_t)(line - la)) * 4;
  o[0] = v[0]; o[1] = v[1]; o[2] = v[2]; o[3] = v[3];
}

// The points [q0, q1) of the lines la .. la + nl - 1 (a pass that starts at point p0 and holds npts): grid = nl x nxb blocks of
// 64 threads.  qterm = -pi / (g^2 V), q_tot: as k_ew_point_fold.
template <bool PHI>
static __global__ __launch_bounds__(64) void k_ew_grid_h(long long q0, long long q1, long long la, int nl, int nx, int nxb, int hmax,
                                                         const double2 *__restrict__ V, const double2 *__restrict__ px, long long p0,
                                                         int npts, double e2s, double qterm, const double *__restrict__ q_tot,
                                                         FieldAtOut out) {
  const int ll = blockIdx.x / nxb, gx = (blockIdx.x - ll * nxb) * 64 + threadIdx.x;
  if (ll >= nl || gx >= nx) return;
  const long long flat = (la + ll) * nx + gx;
  if (flat < q0 || flat >= q1) return;
  double a[4] = {0.0, 0.0, 0.0, 0.0};
  ew_grid_stage_h<PHI>(V + (size_t)ll * 4, (size_t)nl * 4, px, nx, hmax, gx, a);
  const size_t p = (size_t)(flat - p0);
  double *es = out.es() + 3 * p;
  es[0] = fma(e2s, a[0], es[0]); es[1] = fma(e2s, a[1], es[1]); es[2] = fma(e2s, a[2], es[2]);
  if (PHI) out.ps(npts)[p] = fma(e2s, fma(qterm, q_tot[0], a[3]), out.ps(npts)[p]);
}

}  // namespace polar
