// polar_ewald_field_grad_grid.hpp -- the Ewald field of the polarized box and its gradient G_ab = d e_a / d x_b on a regular grid
// of the cell (polar_ewald_field_grad_grid() of include/polar_mi355x.h; arithmetic and formulas: polar_ewald_grid_grad.hpp,
// DESIGN section 6j).  Part of the hand-written HIP kernels (gfx950 / CDNA4, wave64) of the lj/cut/coul/long/polarization pair
// style.
//
// The points are k_ew_grid_points' and the phase tables k_ew_grid_tab's (polar_ewald_field_grid.hpp); the real-space static sums
// and the induced sums are k_ew_grad_real's (polar_ewald_field_grad_at.hpp) on those points.  The reciprocal sums over the step's
// k-vector table run as three 1-D transforms with nine coefficient sets -- three for the field, six for the gradient:
// k_ew_gg_l: stage 1, T[row][g_z][9].  One wave per (row, 64 g_z): kv, S and rows are wave-uniform loads, the z table is read
//   coalesced.  Once per call.
// k_ew_gg_k: stage 2, V[h][line][9] for a run of whole lines.  One wave per (h, g_z, 64 g_y): T is wave-uniform, the y table
//   coalesced; lanes outside the run's lines write nothing.
// k_ew_gg_h: stage 3 and the fold.  One wave per (line, 64 g_x), one thread per point: the line's V column is wave-uniform
//   (nine 16-byte values per h, read through the scalar cache), the x table coalesced; eighteen FMAs per (point, h), twelve
//   without the field.  Folds onto the real-space results in k_ew_grad_fold's form -- fma(e2s, a, es), fma(e2s, a, gs) -- so
//   the per-point partials never exist.
// No atomics, no LDS; every output element is one fixed-order loop, so a point's bits depend on the grid, the records and the
// k-vector table, not on its pass, on the run of lines it was computed in or on whether the field was asked for.
#pragma once

#include "polar_common.hpp"
#include "polar_ewald_grid_grad.hpp"
#include "polar_field_grad_at.hpp"   // FieldGradOut

namespace polar {

// grid = nrow x nzb blocks of 64 threads
static __global__ __launch_bounds__(64) void k_ew_gg_l(int nrow, int nz, int nzb, int lmax, const int4 *__restrict__ rows,
                                                       const double4 *__restrict__ kv, const double2 *__restrict__ S,
                                                       const double2 *__restrict__ pz, double2 *__restrict__ T) {
  const int row = blockIdx.x / nzb, gz = (blockIdx.x - row * nzb) * 64 + threadIdx.x;
  if (row >= nrow || gz >= nz) return;
  double2 t[EW_GG_SETS];
  ew_gg_stage_l(rows, kv, S, pz, nz, lmax, row, gz, t);
  double2 *o = T + ((size_t)row * (size_t)nz + (size_t)gz) * EW_GG_SETS;
#pragma unroll
  for (int c = 0; c < EW_GG_SETS; c++) o[c] = t[c];
}

// V of the lines la .. lb-1 (nl = lb - la): grid = (hmax + 1) x ngz x nyb blocks of 64 threads, gz0 = la / ny
static __global__ __launch_bounds__(64) void k_ew_gg_k(long long la, long long lb, int gz0, int ngz, int nyb, int nz, int ny, int kmax,
                                                       const int *__restrict__ first, const int4 *__restrict__ rows,
                                                       const double2 *__restrict__ T, const double2 *__restrict__ py,
                                                       double2 *__restrict__ V) {
  const int per_h = ngz * nyb;
  const int h = blockIdx.x / per_h, rest = blockIdx.x - h * per_h;
  const int gz = gz0 + rest / nyb, gy = (rest % nyb) * 64 + threadIdx.x;
  if (gy >= ny || gz >= nz) return;
  const long long line = (long long)gz * ny + gy;
  if (line < la || line >= lb) return;
  double2 v[EW_GG_SETS];
  ew_gg_stage_k(rows, T, py, first[h], first[h + 1], nz, ny, kmax, gz, gy, v);
  double2 *o = V + ((size_t)h * (size_t)(lb - la) + (size_t)(line - la)) * EW_GG_SETS;
#pragma unroll
  for (int c = 0; c < EW_GG_SETS; c++) o[c] = v[c];
}

// The points [q0, q1) of the lines la .. la + nl - 1 (a pass that starts at point p0 and holds npts): grid = nl x nxb blocks of
// 64 threads.  FIELD = false leaves e_static at its real-space sums (the caller does not take it home).
template <bool FIELD>
static __global__ __launch_bounds__(64) void k_ew_gg_h(long long q0, long long q1, long long la, int nl, int nx, int nxb, int hmax,
                                                       const double2 *__restrict__ V, const double2 *__restrict__ px, long long p0,
                                                       int npts, double e2s, FieldGradOut out) {
  const int ll = blockIdx.x / nxb, gx = (blockIdx.x - ll * nxb) * 64 + threadIdx.x;
  if (ll >= nl || gx >= nx) return;
  const long long flat = (la + ll) * nx + gx;
  if (flat < q0 || flat >= q1) return;
  double a[EW_GG_SETS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  ew_gg_stage_h<FIELD>(V + (size_t)ll * EW_GG_SETS, (size_t)nl * EW_GG_SETS, px, nx, hmax, gx, a);
  const size_t p = (size_t)(flat - p0);
  if (FIELD) {
    double *es = out.es() + 3 * p;
    es[0] = fma(e2s, a[0], es[0]); es[1] = fma(e2s, a[1], es[1]); es[2] = fma(e2s, a[2], es[2]);
  }
  double *gs = out.gs(npts) + 6 * p;
#pragma unroll
  for (int k = 0; k < 6; k++) gs[k] = fma(e2s, a[3 + k], gs[k]);
}

}  // namespace polar
