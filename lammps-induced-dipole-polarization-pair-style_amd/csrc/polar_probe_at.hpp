// polar_probe_at.hpp -- the Lennard-Jones energy of test sites against every atom of the box, and what a site's charge and
// polarizability make of the field block of the same point (polar_probe_at() of include/polar_mi355x.h; formulas:
// polar_probe_pair.hpp).  Part of the hand-written HIP kernels (gfx950 / CDNA4, wave64) of the
// lj/cut/coul/long/polarization pair style; see polar_kernels.hpp for the mapping and the index spaces.
//
// k_probe_lj has the mapping of k_field_at (polar_field_at.hpp), so the same caches serve a grid: ONE WAVE PER POINT, four
// consecutive points per 256-thread workgroup, the lanes stride the candidate records, the one sum (four with FORCE) is reduced
// with wave_sum, lane 0 stores: no atomics, no LDS, and a point's bits depend on the point, the records and the table alone.
// The wrap and the walks are polar_point_walk.hpp's: every record in exact mode (ALLPAIRS); in list mode the TRIMMED stencil of
// the wrapped point (probe_axis, polar_probe_plan.hpp): per axis the cells a sphere of the probe type's reach touches -- cut_lj
// is often a fraction of cutall, and the +-2 stencil of k_field_at would walk 125 cells for the partners of one or two.  Every
// run is walked in the front copy of the grid first; then, where the cell order is split (polar_handle::cell_split), the same
// runs in the inert copy at ncell + c: the LJ sum covers ALL atoms, the inert ones included.
// The probe's row of the packed table and its reach are wave-uniform (scalar registers); the partner's entry is a
// lane-divergent read of a table of a few hundred bytes.  A record's type comes from a table in record order (k_probe_types,
// made once per call window).
// When the field half of the call ran as well, lane 0 reads the pass's field block and writes e_total, e_coul, e_pol
// (polar_probe_combine); k_probe_combine does the same, one thread per point, when the LJ half is skipped.
#pragma once

#include "polar_common.hpp"
#include "polar_field_at.hpp"    // FieldAtOut
#include "polar_point_walk.hpp"  // point_wrap, point_walk_all, point_walk_cells
#include "polar_probe_pair.hpp"
#include "polar_probe_plan.hpp"

namespace polar {

// The results of a pass of npts points, one block of 9 * npts doubles: e_lj [npts], f_lj [npts][3], e_total [npts][3],
// e_coul [npts], e_pol [npts].
struct ProbeOut {
  double *base;
  __host__ __device__ double *elj() const { return base; }
  __host__ __device__ double *flj(size_t npts) const { return base + npts; }
  __host__ __device__ double *et(size_t npts) const { return base + 4 * npts; }
  __host__ __device__ double *ec(size_t npts) const { return base + 7 * npts; }
  __host__ __device__ double *ep(size_t npts) const { return base + 8 * npts; }
};
// What the combine step reads: the field block of the pass (polar_field_at.hpp) and the sites' charges and polarizabilities
// (either may be null = 0).  field.base == null: no field half in this call, nothing to combine.
struct ProbeField {
  FieldAtOut field;
  const double *q, *alpha;
  double e2s;
};

__device__ __forceinline__ void probe_combine_store(int p, int npts, const ProbeField &f, const ProbeOut &out) {
  const double *es = f.field.es() + 3 * (size_t)p, *ei = f.field.ei(npts) + 3 * (size_t)p;
  double et[3], ec, ep;
  polar_probe_combine(es, ei, f.field.ps(npts)[p], f.field.pi(npts)[p], f.q ? f.q[p] : 0.0, f.alpha ? f.alpha[p] : 0.0, f.e2s, et, ec, ep);
  double *o = out.et(npts) + 3 * (size_t)p;
  o[0] = et[0]; o[1] = et[1]; o[2] = et[2];
  out.ec(npts)[p] = ec; out.ep(npts)[p] = ep;
}

// the combine step alone (a call without e_lj and f_lj)
static __global__ void k_probe_combine(int npts, ProbeField f, ProbeOut out) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p < npts) probe_combine_store(p, npts, f, out);
}

// type of every record: type_s[s] = type[perm[s]] (perm null: the records are in atom order)
static __global__ void k_probe_types(int n, const int *__restrict__ perm, const int *__restrict__ type, int *__restrict__ type_s) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s < n) type_s[s] = type[perm ? perm[s] : s];
}

// The list mode's grid as the kernel needs it: the cells, the second copy (0: none), dfrac per unit of reach and axis.
struct ProbeGrid {
  CellGrid g;
  long long ncell_inert;   // cell_split: ncell, the offset of the inert copy in cell_first; else 0
  double dscale[3];        // (1 + 1e-9) / perpendicular width
};

template <bool ALLPAIRS, bool FORCE>
static __global__ __launch_bounds__(POLAR_BLOCK) void k_probe_lj(int npts, const double *__restrict__ xp, const int *__restrict__ ptype,
                                                          const int *__restrict__ skip_atom, const int *__restrict__ pmol,
                                                          const int *__restrict__ inv, int nlocal, const Scal *scal,
                                                          const AtomRec *__restrict__ recA, const AtomRec *__restrict__ recB,
                                                          const int *__restrict__ type_s, const int *__restrict__ mol_s, Box box,
                                                          ProbeGrid pg, const long long *__restrict__ cell_first,
                                                          const double *__restrict__ ljpack, int ntypes, const double *__restrict__ reach,
                                                          ProbeField fld, ProbeOut out) {
  const int lane = threadIdx.x & 63;
  const int p = blockIdx.x * POLAR_ROWS_PER_BLOCK + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (p >= npts) return;   // (wave-uniform)
  const AtomRec *__restrict__ rec = __builtin_amdgcn_readfirstlane(scal->cur) ? recB : recA;   // (the positions are the same in both)
  double px = xp[3 * (size_t)p], py = xp[3 * (size_t)p + 1], pz = xp[3 * (size_t)p + 2];
  int sk = skip_atom ? __builtin_amdgcn_readfirstlane(skip_atom[p]) : -1;
  if (sk >= 0 && inv) sk = __builtin_amdgcn_readfirstlane(inv[sk]);   // the caller's index -> record order
  const int pm = pmol ? __builtin_amdgcn_readfirstlane(pmol[p]) : 0;
  const int tp = __builtin_amdgcn_readfirstlane(ptype[p]);
  const double *__restrict__ row = ljpack + (size_t)POLAR_LJ_ENTRY * tp * (ntypes + 1);
  const CellGrid &g = pg.g;
  ProbeSums s = {0, 0, 0, 0};
  point_wrap(box, g.lo, px, py, pz);
  // (the LJ pair needs the record's position alone, which the walk has read: the record itself is not looked at, and the walk's
  // loads of its other fields are dead code -- the resource remarks are those of a loop that reads x, y and z through a pointer)
  const auto pair = [&](int j, const AtomRec &, double dx, double dy, double dz) {
    const bool molok = pm == 0 || pm != mol_s[j];
    if (j != sk && molok) polar_probe_pair<FORCE>(dx, dy, dz, type_s[j], row, s);
  };
  if (ALLPAIRS) {
    point_walk_all(lane, nlocal, rec, box, px, py, pz, pair);
  } else {
    Box pbox = box;   // every direction is periodic here, which min_image_rint then knows at compile time
#pragma unroll
    for (int k = 0; k < 3; k++) pbox.periodic[k] = 1;
    const double rho = wave_uniform(reach[tp]);
    double fr[3];
    frac_coords(box, g.lo, px, py, pz, fr);
    const ProbeAxis a0 = probe_axis(wave_uniform(fr[0]), rho * pg.dscale[0], g.nc[0]);
    const ProbeAxis a1 = probe_axis(wave_uniform(fr[1]), rho * pg.dscale[1], g.nc[1]);
    const ProbeAxis a2 = probe_axis(wave_uniform(fr[2]), rho * pg.dscale[2], g.nc[2]);
    const int ncopy = pg.ncell_inert > 0 ? 2 : 1;
    for (int copy = 0; copy < ncopy; copy++)   // the front copy of the grid, then the inert one
      point_walk_cells(lane, rec, pbox, g, cell_first + (copy ? pg.ncell_inert : 0), a0, a1, a2, px, py, pz, pair);
  }
  s.e = wave_sum(s.e);
  if (FORCE) { s.fx = wave_sum(s.fx); s.fy = wave_sum(s.fy); s.fz = wave_sum(s.fz); }
  if (lane == 0) {
    out.elj()[p] = s.e;
    if (FORCE) { double *f = out.flj(npts) + 3 * (size_t)p; f[0] = s.fx; f[1] = s.fy; f[2] = s.fz; }
    if (fld.field.base) probe_combine_store(p, npts, fld, out);
  }
}

}  // namespace polar
