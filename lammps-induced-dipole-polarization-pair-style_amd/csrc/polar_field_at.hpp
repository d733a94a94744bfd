// polar_field_at.hpp -- the field and the potential of the polarized box at arbitrary points (polar_field_at() of
// include/polar_mi355x.h; formulas: polar_point_pair.hpp).  Part of the hand-written HIP kernels (gfx950 /
// CDNA4, wave64) of the lj/cut/coul/long/polarization pair style; see polar_kernels.hpp for the mapping and the index spaces.
//
// k_field_at: ONE WAVE PER POINT, four points per 256-thread workgroup, consecutive points in one workgroup (a grid is
// handed over with x running fastest: neighbouring points re-read the same records out of L1 / L2).  The lanes stride the
// candidate atoms, the eight sums are reduced with wave_sum, lane 0 stores: no atomics, and a point's result depends on
// nothing but the point and the records -- not on the pass it ran in, nor on what else the call holds.
//   ALLPAIRS (exact mode): every record 0 .. nlocal-1, image by min_image_del (closest_image), as k_static_field<true>.
//   Before either, whole lattice vectors come off the point along the periodic directions, once and in closed form (floor of
//   the fractional coordinates, as k_pack wraps an atom; the host has refused points further than 2^30 box lengths out):
//   closest_image's add / subtract loops then see an in-box point, as they do for an atom, however far out the caller's was.
//   list mode: the point's cell is cell_of's, and the records of the +-2 stencil of the list grid are walked through d_cell_first: list_grid
//   (polar_plan.hpp) makes a cell at least cutall / 2 high, so +-2 cells cover the cutoff sphere of any point of the centre
//   cell.  Image by min_image_rint.  Along x the stencil's cells are consecutive cells, i.e. ONE run of consecutive records
//   (two where it crosses the periodic seam): empty cells cost nothing, short cells share a trip.  An axis with fewer than
//   five cells (a periodic one has at least four) is walked once, cells 0 .. nc-1: the 5-cell stencil would meet a cell twice.
//   Every axis must be periodic (the host refuses other boxes).
#pragma once

#include "polar_common.hpp"
#include "polar_point_pair.hpp"
#include "polar_rows.hpp"    // PairMath
#include "polar_lists.hpp"   // CellGrid, cell_of

namespace polar {

// The results of a pass of npts points, one block of 8 * npts doubles: e_static [npts][3], e_induced [npts][3], phi_static
// [npts], phi_induced [npts] (the last two written by the PHI instances only).
struct FieldAtOut {
  double *base;
  __host__ __device__ double *es() const { return base; }
  __host__ __device__ double *ei(size_t npts) const { return base + 3 * npts; }
  __host__ __device__ double *ps(size_t npts) const { return base + 6 * npts; }
  __host__ __device__ double *pi(size_t npts) const { return base + 7 * npts; }
};

// A wave-uniform value parked in a VECTOR register.  The list-mode instances hold the box, the exponential's constants, the
// stencil's loop state and the table pointers in scalar registers -- more than the 102 a wave has: the point, the cutoffs,
// e2s and the list mode's box, read once per pair or once per point, go to the vector file, which has room (no scalar register is spilled).
__device__ __forceinline__ double in_vgpr(double v) {
  asm volatile("" : "+v"(v));
  return v;
}

template <bool ALLPAIRS, int DAMP, bool PHI>
static __global__ __launch_bounds__(POLAR_BLOCK) void k_field_at(int npts, const double *__restrict__ xp, const int *__restrict__ skip_atom,
                                                          const int *__restrict__ pmol, const int *__restrict__ inv, int nlocal,
                                                          const Scal *scal, const AtomRec *__restrict__ recA,
                                                          const AtomRec *__restrict__ recB, const int *__restrict__ mol_s, Box box,
                                                          CellGrid g, const long long *__restrict__ cell_first,
                                                          PointCut cut_in, double e2s_in, ExpCoef K, FieldAtOut out) {
  const int lane = threadIdx.x & 63;
  const int p = blockIdx.x * POLAR_ROWS_PER_BLOCK + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (p >= npts) return;   // (wave-uniform)
  const AtomRec *__restrict__ rec = __builtin_amdgcn_readfirstlane(scal->cur) ? recB : recA;   // the dipoles the last compute left, as k_unpack
  double px = in_vgpr(xp[3 * (size_t)p]), py = in_vgpr(xp[3 * (size_t)p + 1]), pz = in_vgpr(xp[3 * (size_t)p + 2]);
  const PointCut cut{in_vgpr(cut_in.cut_coulsq), in_vgpr(cut_in.ddcutsq), in_vgpr(cut_in.rc2inv), in_vgpr(cut_in.two_rcinv), in_vgpr(cut_in.pd)};
  const double e2s = in_vgpr(e2s_in);
  int sk = skip_atom ? __builtin_amdgcn_readfirstlane(skip_atom[p]) : -1;
  if (sk >= 0 && inv) sk = __builtin_amdgcn_readfirstlane(inv[sk]);   // the caller's index -> record order
  const int pm = pmol ? __builtin_amdgcn_readfirstlane(pmol[p]) : 0;
  ExpCoef Kp = K;
  if (!ALLPAIRS && DAMP == 0) { Kp.log2e = in_vgpr(K.log2e); Kp.ln2hi = in_vgpr(K.ln2hi); Kp.ln2lo = in_vgpr(K.ln2lo); }   // (the last scalar registers over budget)
  const PairMath pmath{Kp, 0.0};
  PointSums s = {0, 0, 0, 0, 0, 0, 0, 0};
  {   // into the box: n lattice vectors c, b, a off, each product and difference in one rounding
    double fr[3];
    frac_coords(box, g.lo, px, py, pz, fr);
    const double n2 = box.periodic[2] ? floor(fr[2]) : 0.0, n1 = box.periodic[1] ? floor(fr[1]) : 0.0, n0 = box.periodic[0] ? floor(fr[0]) : 0.0;
    pz = fma(-n2, box.prd[2], pz);
    py = fma(-n1, box.prd[1], fma(-n2, box.yz, py));
    px = fma(-n0, box.prd[0], fma(-n1, box.xy, fma(-n2, box.xz, px)));
  }
  if (ALLPAIRS) {
    for (int j = lane; j < nlocal; j += 64) {
      const AtomRec rj = rec[j];
      double dx, dy, dz;
      min_image_del(box, px, py, pz, rj.x, rj.y, rj.z, dx, dy, dz);
      const bool molok = pm == 0 || pm != mol_s[j];
      if (j != sk) polar_point_pair<true, DAMP, PHI>(pmath, dx, dy, dz, rj.q, rj.mx, rj.my, rj.mz, rj.a, molok, cut, s);
    }
  } else {
    const int c = __builtin_amdgcn_readfirstlane(cell_of(g, box, px, py, pz));
    // the box of the pair loop: every direction is periodic here, which min_image_rint then knows at compile time; the damped
    // instances, whose exponential takes 32 scalar registers for its constants, keep it in vector registers (in_vgpr)
    Box pbox = box;
#pragma unroll
    for (int k = 0; k < 3; k++) {
      pbox.periodic[k] = 1;
      if (DAMP == 0) { pbox.prd[k] = in_vgpr(box.prd[k]); pbox.inv[k] = in_vgpr(box.inv[k]); }
    }
    if (DAMP == 0) { pbox.xy = in_vgpr(box.xy); pbox.xz = in_vgpr(box.xz); pbox.yz = in_vgpr(box.yz); }
    const int nc0 = g.nc[0], nc1 = g.nc[1], nc2 = g.nc[2];
    const int c0 = c % nc0, c1 = (c / nc0) % nc1, c2 = c / (nc0 * nc1);
    // per axis: the cells start, start + 1, ... (count of them), wrapped; fewer than five cells: all of them, once
    const int n0 = nc0 < 5 ? nc0 : 5, n1 = nc1 < 5 ? nc1 : 5, n2 = nc2 < 5 ? nc2 : 5;
    int x0 = nc0 < 5 ? 0 : c0 - 2, y0 = nc1 < 5 ? 0 : c1 - 2, z0 = nc2 < 5 ? 0 : c2 - 2;
    x0 += x0 < 0 ? nc0 : 0; y0 += y0 < 0 ? nc1 : 0; z0 += z0 < 0 ? nc2 : 0;   // first cell per axis, in [0, nc)
    const int lenA = n0 < nc0 - x0 ? n0 : nc0 - x0;          // cells up to the seam; the other n0 - lenA start at cell 0
    for (int o2 = 0; o2 < n2; o2++) {
      int z = z0 + o2;
      z -= z >= nc2 ? nc2 : 0;
      for (int o1 = 0; o1 < n1; o1++) {
        int y = y0 + o1;
        y -= y >= nc1 ? nc1 : 0;
        const long long base = ((long long)z * nc1 + y) * nc0;
        for (int part = 0; part < 2; part++) {
          const int first = part ? 0 : x0, len = part ? n0 - lenA : lenA;
          if (len <= 0) continue;   // (wave-uniform)
          const int beg = (int)cell_first[base + first], end = (int)cell_first[base + first + len];
          for (int j = beg + lane; j < end; j += 64) {
            const AtomRec rj = rec[j];
            double dx, dy, dz;
            min_image_rint(pbox, px, py, pz, rj.x, rj.y, rj.z, dx, dy, dz);
            const bool molok = pm == 0 || pm != mol_s[j];
            if (j != sk) polar_point_pair<false, DAMP, PHI>(pmath, dx, dy, dz, rj.q, rj.mx, rj.my, rj.mz, rj.a, molok, cut, s);
          }
        }
      }
    }
  }
  s.esx = wave_sum(s.esx); s.esy = wave_sum(s.esy); s.esz = wave_sum(s.esz);
  s.eix = wave_sum(s.eix); s.eiy = wave_sum(s.eiy); s.eiz = wave_sum(s.eiz);
  if (PHI) { s.ps = wave_sum(s.ps); s.pi = wave_sum(s.pi); }
  if (lane == 0) {
    double *es = out.es() + 3 * (size_t)p, *ei = out.ei(npts) + 3 * (size_t)p;
    es[0] = e2s * s.esx; es[1] = e2s * s.esy; es[2] = e2s * s.esz;
    ei[0] = s.eix; ei[1] = s.eiy; ei[2] = s.eiz;
    if (PHI) { out.ps(npts)[p] = e2s * s.ps; out.pi(npts)[p] = s.pi; }
  }
}

}  // namespace polar
