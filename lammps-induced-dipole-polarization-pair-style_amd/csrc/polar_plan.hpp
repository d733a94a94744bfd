// polar_plan.hpp -- host-side step planning: the arithmetic that decides how a step is laid out (list grid, list pitches,
// sweep stream, the Ewald k-vector table and its LDS tiling, block size of the dense Gauss-Seidel) and what follows a sweep of
// the solve (stop rule, mixing, all-reduce, the host's looks at the loop state).
//
// Pure functions, plain C++17: no HIP header, no handle, nothing read from the environment.  polar_step.hip, polar_api.hip and
// polar_dist.hip call them between their launches; tests/test_plan_host.py drives the same functions on the host through
// tests/plan/plan_host.cpp.  Functions that take the box are templates over anything with prd, xy, xz, yz, periodic and
// triclinic (polar::Box, polar_common.hpp).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <vector>

namespace polar {

constexpr double PLAN_PI = 3.14159265358979323846;

// layout of double4 / int4 (polar_step.hip asserts the sizes and copies vectors of them to the device as bytes)
struct PlanD4 { double x, y, z, w; };
struct PlanI4 { int x, y, z, w; };

// at least one workgroup: every kernel bounds-checks its index, and a zero-sized grid is a launch error
inline int nblk(long long n, int per) { return n <= 0 ? 1 : (int)((n + per - 1) / per); }

// ---- cell geometry ------------------------------------------------------------------------------------------------------
// widths of the simulation cell between opposite faces: the box lengths, or V / |face area| when the box is tilted
template <class B>
inline void box_widths(const B &b, double w[3]) {
  w[0] = b.prd[0]; w[1] = b.prd[1]; w[2] = b.prd[2];
  if (!b.triclinic) return;
  const double vol = b.prd[0] * b.prd[1] * b.prd[2];
  const double bxc[3] = {b.prd[1] * b.prd[2], -b.xy * b.prd[2], b.xy * b.yz - b.prd[1] * b.xz};  // b x c
  w[0] = vol / std::sqrt(bxc[0] * bxc[0] + bxc[1] * bxc[1] + bxc[2] * bxc[2]);
  w[1] = vol / (b.prd[0] * std::sqrt(b.prd[2] * b.prd[2] + b.yz * b.yz));                      // |a x c|
}
// cut_coul beyond half the smallest distance between lattice planes: a second image of a partner can lie within cut_coul
inline bool ewald_short_box(const double width[3], double cut_coul) {
  return cut_coul > 0.5 * std::min(width[0], std::min(width[1], width[2]));
}

// ---- list grid ----------------------------------------------------------------------------------------------------------
// cells of the list grid per dimension: cell height >= cutoff / 2 (+-2 stencil).  false: a periodic dimension is narrower
// than two cutoffs (a row would meet two images of a partner) and nc is not set
inline bool list_grid(const double width[3], const int periodic[3], double cutall, int nc[3]) {
  for (int k = 0; k < 3; k++)
    if (periodic[k] && width[k] < 2.0 * cutall * (1.0 - 1e-12)) return false;
  for (int k = 0; k < 3; k++) nc[k] = std::max(1, (int)std::floor(width[k] / (0.5 * cutall)));
  return true;
}

// ---- cell order: inert sites behind the grid ------------------------------------------------------------------------------
// With the split on, the counting sort of build_cells runs over two copies of the list grid laid back to back: bin c holds
// the sites of cell c that carry a charge or a polarizability, bin ncell + c its inert ones (q == 0 and alpha == 0:
// site_is_inert, polar_common.hpp).  cell_first[0 .. ncell] then spans the active sites alone -- what every candidate walk
// reads -- and the inert sites follow them in cell order.  Off: one copy, every site in its cell's bin.
// (k_cell_count calls cell_bin on the device; everything else here is host arithmetic.)
#if defined(__HIPCC__)
#define POLAR_PLAN_FN __host__ __device__ inline
#else
#define POLAR_PLAN_FN inline
#endif
POLAR_PLAN_FN long long cell_bin(long long c, long long ncell, bool inert, bool split) { return (split && inert) ? ncell + c : c; }
// what build_cells sizes by the bins: the count / scan / fill / sort range, the entries of the count table (zeroed), of the
// fill counters (zeroed; front counters first, the back counters of "polarizable first" from fill_back on) and of the
// scan's output (nbins + 1 written)
struct CellBins { long long nbins, cnt, fill, fill_back, first; };
inline CellBins cell_bins(long long ncell, bool split) {
  const long long nb = split ? 2 * ncell : ncell;
  return CellBins{nb, nb + 1, 2 * (nb + 1), nb + 1, nb + 2};
}
// cell indices and bin indices are 32-bit on the device
inline bool cell_bins_fit(long long ncell, bool split) { return cell_bins(ncell, split).nbins < (1ll << 31) - 1; }

// ---- pitches of the row lists (multiples of 64) ---------------------------------------------------------------------------
// first build: `factor` x the mean sphere population
inline long long pitch_first(double mean, double factor) { return (((long long)(factor * mean) + 64) / 64 + 1) * 64; }
// after an overflow: 1.25 x the longest row the build met (the value of the overflow flag)
inline long long pitch_grown(int flag) { return ((long long)(1.25 * flag) / 64 + 1) * 64; }
// POLAR_INIT_PITCH (tests: force the overflow path)
inline int pitch_forced(int value) { return ((std::max(64, value) + 63) / 64) * 64; }

// volume of the OCCUPIED part of the box (a shard handle holds one slab plus its halo, not the whole box): the share of
// non-empty cells of a coarse host grid with edge ~cutoff, times the box volume.  x = n positions
inline double occupied_volume(int n, const double *x, const double lo[3], const double prd[3], double cutall) {
  double vol = prd[0] * prd[1] * prd[2];
  int nc[3];
  long long tot = 1;
  for (int k = 0; k < 3; k++) { nc[k] = std::max(1, std::min(64, (int)(prd[k] / cutall))); tot *= nc[k]; }
  std::vector<char> occ((size_t)tot, 0);
  for (int a = 0; a < n; a++) {
    long long c = 0, mul = 1;
    for (int k = 0; k < 3; k++) {
      double fr = (x[3 * (size_t)a + k] - lo[k]) / prd[k];
      fr -= std::floor(fr);
      c += mul * std::min(nc[k] - 1, (int)(fr * nc[k]));
      mul *= nc[k];
    }
    occ[(size_t)c] = 1;
  }
  long long filled = 0;
  for (char v : occ) filled += v;
  if (filled > 0) vol *= (double)filled / (double)tot;
  return vol;
}

// ---- what the sweep streams per pair ----------------------------------------------------------------------------------
// 0 cached (s3, s5); 1 cached r^2; 2 nothing (r^2 rebuilt from the gathered positions); 3 the index alone, as a byte
// offset (lane-per-pair sweep); 4 no per-atom dd rows (cluster and tile sweeps).  cache_r2 < 0: 1 or 2 by size.
// Measured (tools/exp_nocache.sh): while index + r^2 of all pairs (12 B/pair) stay resident in the 256 MB Infinity Cache
// between sweeps the cached r^2 wins (36k atoms, 160 MB: 99 vs 107 us/sweep); beyond that the stream comes from HBM every
// sweep and rebuilding r^2 from the gathered positions wins (135k atoms, 595 MB: 320 vs 350 us/sweep).
inline int stream_mode(int cache_r2, int sweep_kernel, long long dd_pairs, int own_rows, long long dd_pitch) {
  int mode = cache_r2;
  if (sweep_kernel == 1) mode = 0;
  if (sweep_kernel == 2) mode = 3;
  if (sweep_kernel >= 3) mode = 4;
  if (mode < 0) {
    const double est_pairs = dd_pairs > 0 ? (double)dd_pairs : 0.35 * (double)own_rows * (double)dd_pitch;
    mode = (12.0 * est_pairs < 200.0e6) ? 1 : 2;
  }
  return mode;
}

// ---- `polar_ewald`: the k-vector table --------------------------------------------------------------------------------
// The half-space k-vectors with |k| <= k_cut = 2 g sqrt(-ln accuracy), in (h, k, l) order.  kv = {kx, ky, kz, c_k},
// hkl = {h, k, l, 0}.  rows = {h, k, first l, index of the row's first k}: a row holds the k-vectors of one (h, k), and its
// l values are consecutive (k^2 is convex in l), which is what lets k_ew_field and k_ew_force walk a row by the recurrence
// p <- p e^{2 pi i s_z}.  rows[nrow] = {0, 0, 0, nk} ends the table.  nm = the largest index bound of the three axes (the
// power tables of k_ew_sfac hold nm + 1 entries).  cell = the six entries of H^-1 (s = H^-1 r), upper triangle by rows.
struct EwaldPlan {
  std::vector<PlanD4> kv;
  std::vector<PlanI4> hkl, rows;
  int nk = 0, nrow = 0, nm = 0;
  double cell[6] = {0, 0, 0, 0, 0, 0};
};
template <class B>
inline EwaldPlan ewald_kvectors(const B &b, double g, double acc) {
  EwaldPlan p;
  const double lx = b.prd[0], ly = b.prd[1], lz = b.prd[2], xy = b.xy, xz = b.xz, yz = b.yz;
  // H = [a b c] = [[lx, xy, xz], [0, ly, yz], [0, 0, lz]];  s = H^-1 r;  k = 2 pi H^-T n
  const double i00 = 1.0 / lx, i01 = -xy / (lx * ly), i02 = (xy * yz - ly * xz) / (lx * ly * lz), i11 = 1.0 / ly,
               i12 = -yz / (ly * lz), i22 = 1.0 / lz;
  const double vol = lx * ly * lz, twopi = 2.0 * PLAN_PI;
  const double kcut = 2.0 * g * std::sqrt(-std::log(acc)), kcut2 = kcut * kcut;
  // |n_a| <= k_cut |lattice vector a| / 2 pi
  const int hm = (int)std::floor(kcut * lx / twopi), km = (int)std::floor(kcut * std::sqrt(xy * xy + ly * ly) / twopi),
            lm = (int)std::floor(kcut * std::sqrt(xz * xz + yz * yz + lz * lz) / twopi);
  for (int ih = 0; ih <= hm; ih++)
    for (int ik = (ih == 0 ? 0 : -km); ik <= km; ik++) {
      int row = -1;
      for (int il = (ih == 0 && ik == 0 ? 1 : -lm); il <= lm; il++) {
        const double kx = twopi * (ih * i00), ky = twopi * (ih * i01 + ik * i11), kz = twopi * (ih * i02 + ik * i12 + il * i22);
        const double k2 = kx * kx + ky * ky + kz * kz;
        if (k2 > kcut2 || k2 == 0.0) continue;
        if (row < 0) { row = (int)p.rows.size(); p.rows.push_back(PlanI4{ih, ik, il, (int)p.kv.size()}); }
        p.kv.push_back(PlanD4{kx, ky, kz, 8.0 * PLAN_PI / vol * std::exp(-k2 / (4.0 * g * g)) / k2});
        p.hkl.push_back(PlanI4{ih, ik, il, 0});
      }
    }
  p.nk = (int)p.kv.size();
  p.nrow = (int)p.rows.size();
  p.rows.push_back(PlanI4{0, 0, 0, p.nk});
  p.nm = std::max(hm, std::max(km, lm));
  p.cell[0] = i00; p.cell[1] = i01; p.cell[2] = i02; p.cell[3] = i11; p.cell[4] = i12; p.cell[5] = i22;
  return p;
}

// LDS of k_ew_sfac: per staged atom, three power tables of nm + 1 entries (16 bytes each) and three weights; up to 32 atoms in 48 KB
inline size_t ewald_lds_per_atom(int nm) { return 3 * (size_t)(nm + 1) * 16 + 3 * sizeof(double); }
inline int ewald_tile(int nm) { return (int)std::max<size_t>(1, std::min<size_t>(32, (48 * 1024) / ewald_lds_per_atom(nm))); }
// grid of k_ew_sfac: kb workgroups of 256 k-vectors times nchunk chunks of `chunk` atoms (whole tiles while there are atoms
// enough; about 4096 workgroups at most)
struct SfacChunks { int kb, nchunk, chunk; };
inline SfacChunks ewald_sfac_chunks(int n, int nk, int tile) {
  SfacChunks c;
  c.kb = nblk(nk, 256);
  c.nchunk = std::max(1, std::min(nblk(std::max(n, 1), tile), nblk(4096, c.kb)));
  c.chunk = std::max(1, nblk(std::max(n, 1), c.nchunk));
  c.nchunk = nblk(std::max(n, 1), c.chunk);
  return c;
}

// ---- polar_ewald_field_grid: the layout of a call, from the k-vector table alone (polar_ewald_grid.hpp) ------------------------
// Index bounds of the rows table (rows[r] = {h, k, first l, first index}, rows[nrow].w = nk): hmax, kmax = max |k|,
// lmax = max |l| over the rows' runs of l; first[h] = the first row of h, first[hmax + 1] = nrow (the table is in (h, k) order:
// the rows of an h are one run -- `ok` says that this table's are, and that h starts at 0 and skips no value).
struct EwGridPlan {
  int hmax = 0, kmax = 0, lmax = 0;
  std::vector<int> first;
  bool ok = true;
};
inline EwGridPlan ew_grid_plan(const PlanI4 *rows, int nrow) {
  EwGridPlan p;
  for (int r = 0; r < nrow; r++) {
    const int l0 = rows[r].z, l1 = l0 + (rows[r + 1].w - rows[r].w) - 1;
    p.hmax = std::max(p.hmax, rows[r].x);
    p.kmax = std::max(p.kmax, std::abs(rows[r].y));
    p.lmax = std::max(p.lmax, std::max(std::abs(l0), std::abs(l1)));
    if (rows[r].x < 0 || l1 < l0 || (r > 0 && rows[r].x < rows[r - 1].x)) p.ok = false;
  }
  p.first.assign((size_t)p.hmax + 2, nrow);
  for (int r = nrow - 1; r >= 0; r--)
    if (rows[r].x >= 0 && rows[r].x <= p.hmax) p.first[(size_t)rows[r].x] = r;
  for (int h = p.hmax - 1; h >= 0; h--)   // (an h without rows -- no table of ewald_kvectors has one -- starts where the next one does)
    if (p.first[(size_t)h] > p.first[(size_t)h + 1]) p.first[(size_t)h] = p.first[(size_t)h + 1];
  if (nrow > 0 && p.first[0] != 0) p.ok = false;
  return p;
}
// Table and scratch sizes of a call on an (nx, ny, nz) grid, in entries of 16 bytes (one complex number): the three phase
// tables in one array (x at 0, y at off_y, z at off_z, `tab` in all), T[nrow][nz][4], and the bytes of V per line,
// (hmax + 1) x 4 sets.  nset: the coefficient sets per element of T and V -- 4 for polar_ewald_field_grid, 9 (EW_GG_SETS of
// polar_ewald_grid_grad.hpp) for polar_ewald_field_grad_grid: T[nrow][nz][nset], (hmax + 1) x nset x 16 bytes of V per line.
struct EwGridSizes { size_t off_y, off_z, tab, t, v_line_bytes; };
inline EwGridSizes ew_grid_sizes(const EwGridPlan &p, int nrow, const int n[3], int nset = 4) {
  EwGridSizes s;
  s.off_y = (size_t)(p.hmax + 1) * (size_t)n[0];
  s.off_z = s.off_y + (size_t)(2 * p.kmax + 1) * (size_t)n[1];
  s.tab = s.off_z + (size_t)(2 * p.lmax + 1) * (size_t)n[2];
  s.t = (size_t)nrow * (size_t)n[2] * (size_t)nset;
  s.v_line_bytes = (size_t)(p.hmax + 1) * (size_t)nset * 16;
  return s;
}
// whole lines of the grid whose V fits the 64 MB that the per-point path spends on its chunk partials (at least one)
inline long long ew_grid_lines_per_run(size_t v_line_bytes) { return std::max<long long>(1, (long long)(((size_t)64 << 20) / std::max<size_t>(v_line_bytes, 1))); }
// A pass holds the points [p0, p0 + m) of the flat order and may start and end inside a line of nx points.  Its line
// sub-ranges: run r computes V of the lines [la, lb) and stage 3 takes the pass's points [q0, q1) of them.
struct EwGridRun { long long la, lb, q0, q1; };
inline std::vector<EwGridRun> ew_grid_runs(long long p0, long long m, long long nx, long long lines_per_run) {
  std::vector<EwGridRun> runs;
  if (m <= 0 || nx <= 0) return runs;
  const long long first = p0 / nx, last = (p0 + m - 1) / nx, lpr = std::max<long long>(1, lines_per_run);
  for (long long la = first; la <= last; la += lpr) {
    const long long lb = std::min(la + lpr, last + 1);
    runs.push_back(EwGridRun{la, lb, std::max(p0, la * nx), std::min(p0 + m, lb * nx)});
  }
  return runs;
}

// ---- exact-order Gauss-Seidel on the HBM-resident tensor (polar_exact.hpp) --------------------------------------------------
// n <= 64: one block, the matrix-free form; 32 GB of tensor (48 n^2 bytes) = 25,819 atoms
inline bool dense_gs_fits(int n) { return n > 64 && 48.0 * (double)n * (double)n <= 3.2e10; }
// atoms per block of the sweep (at least two blocks: dense_gs_fits needs n > 64)
inline int dense_gs_block(int n) { return n >= 1024 ? 256 : n >= 384 ? 128 : 64; }

// ---- the end of a sweep -------------------------------------------------------------------------------------------------
// What follows sweep `sw` of at most max_sweeps = iterations_max + 1, the same for solve(), the stepwise calls and both
// schedules of the multi-GPU driver (ranks that disagreed here would leave the loop at different sweeps, and one of them would
// wait in an exchange for ever).  `accel`: Anderson mixing is on (what accel_begin returned); reduce_every: the driver's
// all-reduce cadence, 0 on one handle.
// Fixed-iteration Gauss-Seidel (`lazy`) takes no decision between sweeps: its end-of-sweep logic (k_solver_step) runs after
// the last two sweeps only -- for all sweeps but the last at once, then for the last one, whose sum |dmu|^2 is the one
// reported -- and it mixes after every sweep but the last.  Everything else decides after every sweep: in k_solver_step, or,
// where it mixes, inside the mixing launch (k_solver_accel).  In precision mode the driver's stop rule reads the all-reduced
// change every reduce_every-th sweep and on every sweep that can end the solve by running out of iterations ("not converged
// yet" in between); with mixing the change rides the all-reduce of the dot products instead.
struct SweepEnd {
  bool mix;            // Anderson mixing follows this sweep ...
  bool decide_in_mix;  // ... and carries the end-of-sweep decision (k_solver_step is not launched)
  int count;           // sweeps the k_solver_step launched now accounts for; 0: none is launched
  bool reduce;         // this sweep's change is all-reduced for the stop rule
  bool jacobi;         // k_solver_step flips the dipole buffers
};
inline SweepEnd sweep_end(int sw, int max_sweeps, bool fixed_iteration, bool gs, bool accel, int reduce_every) {
  const bool lazy = fixed_iteration && gs;
  SweepEnd e;
  e.mix = accel && (!lazy || sw < max_sweeps - 1);
  e.decide_in_mix = accel && !lazy;
  if (lazy) e.count = sw == max_sweeps - 2 ? max_sweeps - 1 : sw == max_sweeps - 1 ? 1 : 0;
  else e.count = accel ? 0 : 1;
  e.reduce = reduce_every > 0 && !fixed_iteration && !accel && ((sw % reduce_every) == reduce_every - 1 || sw >= max_sweeps - 1);
  e.jacobi = !gs;
  return e;
}
// When the host looks at the device-resident loop state (a stream synchronisation: the queue drains, ~12 us before the next
// sweep starts).  Without history: after every `every`-th sweep.  With the sweep count of the handle's LAST converged solve
// (`last_sweeps`; 0: none yet) -- counts change by a sweep or two from step to step, in MD as in the resident bench -- the
// first look comes where that solve ended (one look instead of eight at 31 sweeps, no launches past the end), then after every
// sweep for a few, then the old cadence.  Sweeps launched past the end of a finished solve are no-ops on the device either
// way.  `step` = sweeps per possible change of the state (multi-GPU: the all-reduce cadence; the state can only flip after an
// all-reduced sweep).
inline bool look_at_state(int last_sweeps, int sw, int every, int step = 1) {
  const int done_sweeps = sw + 1;
  const int pred = last_sweeps;
  if (pred <= 0) return (sw % every) == every - 1;
  if (done_sweeps < pred) return (done_sweeps % 16) == 0;   // (a coarse look on the way: a solve that ends much earlier than the last one wastes at most 16 no-op sweeps)
  const int past = done_sweeps - pred;
  if (past <= 4 * step) return (past % step) == 0;
  return (past % every) == 0;
}

}  // namespace polar
