// polar_ewald_field_grad_at.hpp -- the Ewald field of the polarized box at arbitrary points together with its gradient
// G_ab = d e_a / d x_b, for handles with `polar_ewald` (polar_ewald_field_grad_at() and polar_ewald_probe_force_at() of
// include/polar_mi355x.h; formulas: polar_ewald_point_grad.hpp).  Part of the hand-written HIP kernels
// (gfx950 / CDNA4, wave64) of the lj/cut/coul/long/polarization pair style.
//
// k_ew_grad_real: the real-space static sums and the induced sums, 9 + 9.  The mapping, the wrap, the LDS run list of list mode
//   and the walk are k_ew_point_real's (polar_ewald_field_at.hpp): ONE WAVE PER POINT, four points per 256-thread workgroup, two
//   walks per point.  The induced walk comes first and its nine sums are reduced and stored before the static walk begins, so
//   that the static loop -- erfc, erf, the Gaussian and nine accumulators -- does not carry them.  Lanes stride the records,
//   eighteen wave_sums, lane 0 stores, no atomics.
// k_ew_grad_recip: the reciprocal sums, nine per point.  One thread per point, blockIdx.y a chunk of (h, k) rows
//   (ew_point_rows_per_chunk), per-chunk partials part[chunk][9][npts].
// k_ew_grad_fold: adds the partials in chunk order onto the real-space results and applies e2s -- the three field sums exactly
//   as k_ew_point_fold<false>.
// A point's bits depend on the point, the records and the k-vector table -- not on its pass, its neighbours or their order.
// The field sums are formed by the expressions of k_ew_point_real / k_ew_point_recip / k_ew_point_fold in their order: they
// have the bits of polar_ewald_field_at.
#pragma once

#include "polar_common.hpp"
#include "polar_ewald_field_at.hpp"     // EwPointMath, EwRecipMath, ew_point_walk
#include "polar_ewald_point_grad.hpp"
#include "polar_field_grad_at.hpp"      // FieldGradOut

namespace polar {

template <bool ALLPAIRS, int DAMP>
static __global__ __launch_bounds__(POLAR_BLOCK) void k_ew_grad_real(int npts, const double *__restrict__ xp, const int *__restrict__ skip_atom,
                                                              const int *__restrict__ pmol, const int *__restrict__ inv, int nlocal,
                                                              const Scal *scal, const AtomRec *__restrict__ recA,
                                                              const AtomRec *__restrict__ recB, const int *__restrict__ mol_s, Box box,
                                                              CellGrid g, const long long *__restrict__ cell_first,
                                                              PointCut cut_in, EwPointParm ew_in, double e2s_in, ExpCoef K, FieldGradOut out) {
  const int lane = threadIdx.x & 63;
  const int p = blockIdx.x * POLAR_ROWS_PER_BLOCK + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (p >= npts) return;   // (wave-uniform)
  const AtomRec *__restrict__ rec = __builtin_amdgcn_readfirstlane(scal->cur) ? recB : recA;   // the dipoles the last compute left
  const int *__restrict__ mol = mol_s;
  if (!ALLPAIRS) { asm volatile("" : "+v"(mol)); asm volatile("" : "+v"(rec)); }   // (list mode: the table pointers to the vector file too, see in_vgpr)
  double px = in_vgpr(xp[3 * (size_t)p]), py = in_vgpr(xp[3 * (size_t)p + 1]), pz = in_vgpr(xp[3 * (size_t)p + 2]);
  const PointCut cut{in_vgpr(cut_in.cut_coulsq), in_vgpr(cut_in.ddcutsq), in_vgpr(cut_in.rc2inv), in_vgpr(cut_in.two_rcinv), in_vgpr(cut_in.pd)};
  const EwPointParm ew{in_vgpr(ew_in.g), in_vgpr(ew_in.g2), in_vgpr(ew_in.g2lo), in_vgpr(ew_in.tgs)};
  const double e2s = in_vgpr(e2s_in);
  int sk = skip_atom ? __builtin_amdgcn_readfirstlane(skip_atom[p]) : -1;
  if (sk >= 0 && inv) sk = __builtin_amdgcn_readfirstlane(inv[sk]);   // the caller's index -> record order
  const int pm = pmol ? __builtin_amdgcn_readfirstlane(pmol[p]) : 0;
  double *obase = out.base;
  if (!ALLPAIRS) asm volatile("" : "+v"(obase));   // (what only the stores need does not sit in scalar registers through the loops)
  ExpCoef Kp = K;
  if (!ALLPAIRS && DAMP == 0) { Kp.log2e = in_vgpr(K.log2e); Kp.ln2hi = in_vgpr(K.ln2hi); Kp.ln2lo = in_vgpr(K.ln2lo); }   // (as k_field_at)
  const EwPointMath pmath{Kp};
  point_wrap(box, g.lo, px, py, pz);
  // The box of the pair loops and the stencil's runs in LDS: k_ew_point_real's lines, repeated.  Moved into a function that both
  // kernels call, they give k_ew_point_real other instructions (11,016 instead of 11,048 over its eight instances, the same
  // registers), and that kernel's text is not this file's to change: a change to those lines is made in both places.
  Box pbox = box;
  __shared__ int s_runs[POLAR_ROWS_PER_BLOCK][2 * 64];
  int *runs = s_runs[threadIdx.x >> 6];
  int nruns = 0;
  if (!ALLPAIRS) {
    const int c = __builtin_amdgcn_readfirstlane(cell_of(g, box, px, py, pz));
#pragma unroll
    for (int k = 0; k < 3; k++) {
      pbox.periodic[k] = 1;
      pbox.prd[k] = in_vgpr(box.prd[k]); pbox.inv[k] = in_vgpr(box.inv[k]);
    }
    pbox.xy = in_vgpr(box.xy); pbox.xz = in_vgpr(box.xz); pbox.yz = in_vgpr(box.yz);
    const int nc0 = g.nc[0], nc1 = g.nc[1], nc2 = g.nc[2];
    const ProbeAxis a0 = stencil_axis(c % nc0, nc0), a1 = stencil_axis((c / nc0) % nc1, nc1), a2 = stencil_axis(c / (nc0 * nc1), nc2);
    nruns = 2 * a1.count * a2.count;                           // <= 50
    if (lane < nruns) {
      const int o1 = (lane >> 1) % a1.count, o2 = (lane >> 1) / a1.count;
      int z = a2.first + o2, y = a1.first + o1;
      z -= z >= nc2 ? nc2 : 0;
      y -= y >= nc1 ? nc1 : 0;
      const long long base = ((long long)z * nc1 + y) * nc0;
      const ProbeAxis run = seam_part(a0, nc0, lane & 1);
      runs[2 * lane] = run.count > 0 ? (int)cell_first[base + run.first] : 0;
      runs[2 * lane + 1] = run.count > 0 ? (int)cell_first[base + run.first + run.count] : 0;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  const FieldGradOut o{obase};
  // Two walks, the induced sums first, as k_ew_point_real; the nine induced sums leave the registers before the static walk.
  {
    PointGradSums s = {{0, 0, 0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0}};
    ew_point_walk<ALLPAIRS>(lane, nlocal, rec, pbox, px, py, pz, runs, nruns, [&](int j, const AtomRec &rj, double dx, double dy, double dz) {
      if (j != sk) polar_point_grad_pair<ALLPAIRS, DAMP>(pmath, dx, dy, dz, rj.q, rj.mx, rj.my, rj.mz, rj.a, false, cut, s);   // (the induced branch)
    });
    s.f.eix = wave_sum(s.f.eix); s.f.eiy = wave_sum(s.f.eiy); s.f.eiz = wave_sum(s.f.eiz);
#pragma unroll
    for (int k = 0; k < 6; k++) s.gi[k] = wave_sum(s.gi[k]);
    if (lane == 0) {
      double *ei = o.ei(npts) + 3 * (size_t)p, *gi = o.gi(npts) + 6 * (size_t)p;
      ei[0] = s.f.eix; ei[1] = s.f.eiy; ei[2] = s.f.eiz;
#pragma unroll
      for (int k = 0; k < 6; k++) gi[k] = s.gi[k];
    }
  }
  {
    PointGradSums s = {{0, 0, 0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0}};
    ew_point_walk<ALLPAIRS>(lane, nlocal, rec, pbox, px, py, pz, runs, nruns, [&](int j, const AtomRec &rj, double dx, double dy, double dz) {
      const bool kept = (pm == 0 || pm != mol[j]) && j != sk;
      polar_point_grad_pair_ew<ALLPAIRS, DAMP>(pmath, dx, dy, dz, rj.q, 0.0, 0.0, 0.0, 0.0, kept, false, cut, ew, s);
    });
    s.f.esx = wave_sum(s.f.esx); s.f.esy = wave_sum(s.f.esy); s.f.esz = wave_sum(s.f.esz);
#pragma unroll
    for (int k = 0; k < 6; k++) s.gs[k] = wave_sum(s.gs[k]);
    if (lane == 0) {
      double *es = o.es() + 3 * (size_t)p, *gs = o.gs(npts) + 6 * (size_t)p;
      es[0] = e2s * s.f.esx; es[1] = e2s * s.f.esy; es[2] = e2s * s.f.esz;
#pragma unroll
      for (int k = 0; k < 6; k++) gs[k] = e2s * s.gs[k];
    }
  }
}

// the reciprocal sums of the points p0 .. p0 + np - 1 of a pass over the rows of chunk blockIdx.y -> part[chunk][9][np]
static __global__ __launch_bounds__(256) void k_ew_grad_recip(int np, int p0, const double *__restrict__ xp, Box box, double lo0, double lo1,
                                                              double lo2, EwCell cell, int nrow, int rows_per_chunk,
                                                              const int4 *__restrict__ rows, const double4 *__restrict__ kv,
                                                              const double2 *__restrict__ S, double *__restrict__ part) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= np) return;
  const size_t p = (size_t)p0 + t;
  double px = xp[3 * p], py = xp[3 * p + 1], pz = xp[3 * p + 2];
  const double lo[3] = {lo0, lo1, lo2};
  point_wrap(box, lo, px, py, pz);
  double sx, sy, sz;
  ew_frac(cell, px, py, pz, sx, sy, sz);
  const int r0 = blockIdx.y * rows_per_chunk, r1 = min(nrow, r0 + rows_per_chunk);
  double acc[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  const EwRecipMath m;
  ew_point_grad_rows(m, sx, sy, sz, rows, kv, S, r0, r1, acc);
  double *o = part + (size_t)blockIdx.y * 9 * np + t;
#pragma unroll
  for (int k = 0; k < 9; k++) o[k * (size_t)np] = acc[k];
}

// chunk partials, in chunk order, onto the real-space results of the points p0 .. p0 + np - 1 of a pass of npts points
static __global__ __launch_bounds__(256) void k_ew_grad_fold(int np, int p0, int npts, int nchunk, const double *__restrict__ part, double e2s,
                                                             FieldGradOut out) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= np) return;
  double a[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int c = 0; c < nchunk; c++) {
    const double *b = part + (size_t)c * 9 * np + t;
#pragma unroll
    for (int k = 0; k < 9; k++) a[k] += b[k * (size_t)np];
  }
  const size_t p = (size_t)p0 + t;
  double *es = out.es() + 3 * p, *gs = out.gs(npts) + 6 * p;
  es[0] = fma(e2s, a[0], es[0]); es[1] = fma(e2s, a[1], es[1]); es[2] = fma(e2s, a[2], es[2]);
#pragma unroll
  for (int k = 0; k < 6; k++) gs[k] = fma(e2s, a[3 + k], gs[k]);
}

}  // namespace polar
