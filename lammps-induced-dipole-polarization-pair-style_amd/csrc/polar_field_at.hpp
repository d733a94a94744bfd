// polar_field_at.hpp -- the field and the potential of the polarized box at arbitrary points (polar_field_at() of
// include/polar_mi355x.h; formulas: polar_point_pair.hpp).  Part of the hand-written HIP kernels (gfx950 /
// CDNA4, wave64) of the lj/cut/coul/long/polarization pair style; see polar_kernels.hpp for the mapping and the index spaces.
//
// k_field_at: ONE WAVE PER POINT, four points per 256-thread workgroup, consecutive points in one workgroup (a grid is
// handed over with x running fastest: neighbouring points re-read the same records out of L1 / L2).  The lanes stride the
// candidate atoms, the eight sums are reduced with wave_sum, lane 0 stores: no atomics, and a point's result depends on
// nothing but the point and the records -- not on the pass it ran in, nor on what else the call holds.
// The wrap of the point into the box and the two walks -- every record in exact mode (ALLPAIRS), the +-2 stencil of the point's
// cell in list mode -- are polar_point_walk.hpp's, described there.
#pragma once

#include "polar_common.hpp"
#include "polar_point_pair.hpp"
#include "polar_rows.hpp"    // PairMath
#include "polar_point_walk.hpp"   // in_vgpr, point_wrap, point_walk_all, point_walk_cells

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
  point_wrap(box, g.lo, px, py, pz);
  const auto pair = [&](int j, const AtomRec &rj, double dx, double dy, double dz) {
    const bool molok = pm == 0 || pm != mol_s[j];
    if (j != sk) polar_point_pair<ALLPAIRS, DAMP, PHI>(pmath, dx, dy, dz, rj.q, rj.mx, rj.my, rj.mz, rj.a, molok, cut, s);
  };
  if (ALLPAIRS) {
    point_walk_all(lane, nlocal, rec, box, px, py, pz, pair);
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
    point_walk_cells(lane, rec, pbox, g, cell_first, stencil_axis(c % nc0, nc0), stencil_axis((c / nc0) % nc1, nc1),
                     stencil_axis(c / (nc0 * nc1), nc2), px, py, pz, pair);
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
