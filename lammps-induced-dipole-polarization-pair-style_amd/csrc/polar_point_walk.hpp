// polar_point_walk.hpp -- how a wave finds the candidate records of one caller-supplied point: what the point kernels
// k_field_at (polar_field_at.hpp), k_field_grad_at (polar_field_grad_at.hpp), k_probe_lj (polar_probe_at.hpp),
// k_ew_point_real / k_ew_point_recip (polar_ewald_field_at.hpp) and k_ew_grad_real / k_ew_grad_recip (polar_ewald_field_grad_at.hpp)
// share (k_field_grad_at: all but the list-mode loops).  Part of the hand-written HIP kernels (gfx950 / CDNA4,
// wave64) of the lj/cut/coul/long/polarization pair style; see polar_kernels.hpp for the mapping and the index spaces.
//
// The mapping of all of them is ONE WAVE PER POINT, four consecutive points per 256-thread workgroup (a grid is handed over
// with x running fastest: neighbouring points re-read the same records out of L1 / L2); the lanes stride the candidate records,
// the kernel's own pair lambda f(j, record, dx, dy, dz) adds to per-lane sums, which the kernel reduces with wave_sum.
//   point_wrap: before either walk, whole lattice vectors come off the point along the periodic directions, once and in closed
//   form (floor of the fractional coordinates, as k_pack wraps an atom; the host has refused points further than 2^30 box
//   lengths out): closest_image's add / subtract loops then see an in-box point, as they do for an atom.
//   point_walk_all (exact mode): every record 0 .. nlocal-1, image by min_image_del (closest_image), as k_static_field<true>.
//   point_walk_cells (list mode): the records of a stencil of the list grid around the point's cell, through d_cell_first,
//   image by min_image_rint (the caller's box has every direction periodic: the host refuses other boxes).  Per axis the
//   stencil is a range {first, count} of cells, wrapped: stencil_axis's +-2 cells (list_grid of polar_plan.hpp makes a cell at
//   least cutall / 2 high, so they cover the cutoff sphere of any point of the centre cell), or probe_axis's trimmed range
//   (both polar_probe_plan.hpp).  Along x the range's cells are consecutive cells, i.e. ONE run of consecutive records -- two
//   where it crosses the periodic seam (seam_part): empty cells cost nothing, short cells share a trip.
// A kernel's wave-uniform state may exceed the scalar registers a wave has; what each kernel parks in vector registers
// (in_vgpr) is the kernel's own business and stays in its file.
#pragma once

#include "polar_common.hpp"
#include "polar_lists.hpp"        // CellGrid, cell_of
#include "polar_probe_plan.hpp"   // ProbeAxis, stencil_axis, seam_part

namespace polar {

// A wave-uniform value parked in a VECTOR register.  The list-mode instances hold the box, the exponential's constants, the
// stencil's loop state and the table pointers in scalar registers -- more than the 102 a wave has: the point, the cutoffs,
// e2s and the list mode's box, read once per pair or once per point, go to the vector file, which has room (no scalar register is spilled).
__device__ __forceinline__ double in_vgpr(double v) {
  asm volatile("" : "+v"(v));
  return v;
}

// into the box: n lattice vectors c, b, a off, each product and difference in one rounding
__device__ __forceinline__ void point_wrap(const Box &box, const double lo[3], double &px, double &py, double &pz) {
  double fr[3];
  frac_coords(box, lo, px, py, pz, fr);
  const double n2 = box.periodic[2] ? floor(fr[2]) : 0.0, n1 = box.periodic[1] ? floor(fr[1]) : 0.0, n0 = box.periodic[0] ? floor(fr[0]) : 0.0;
  pz = fma(-n2, box.prd[2], pz);
  py = fma(-n1, box.prd[1], fma(-n2, box.yz, py));
  px = fma(-n0, box.prd[0], fma(-n1, box.xy, fma(-n2, box.xz, px)));
}

template <class F>
__device__ __forceinline__ void point_walk_all(int lane, int nlocal, const AtomRec *__restrict__ rec, const Box &box, double px, double py,
                                               double pz, F f) {
  for (int j = lane; j < nlocal; j += 64) {
    const AtomRec rj = rec[j];
    double dx, dy, dz;
    min_image_del(box, px, py, pz, rj.x, rj.y, rj.z, dx, dy, dz);
    f(j, rj, dx, dy, dz);
  }
}

// (cell_first: of the copy of the grid to walk; a0, a1, a2: the ranges along x, y, z.  k_field_grad_at has these loops written
// out, see there: a change to them is made in both places)
template <class F>
__device__ __forceinline__ void point_walk_cells(int lane, const AtomRec *__restrict__ rec, const Box &pbox, const CellGrid &g,
                                                 const long long *__restrict__ cell_first, ProbeAxis a0, ProbeAxis a1, ProbeAxis a2,
                                                 double px, double py, double pz, F f) {
  const int nc0 = g.nc[0], nc1 = g.nc[1], nc2 = g.nc[2];
  for (int o2 = 0; o2 < a2.count; o2++) {
    int z = a2.first + o2;
    z -= z >= nc2 ? nc2 : 0;
    for (int o1 = 0; o1 < a1.count; o1++) {
      int y = a1.first + o1;
      y -= y >= nc1 ? nc1 : 0;
      const long long base = ((long long)z * nc1 + y) * nc0;
      for (int part = 0; part < 2; part++) {
        const ProbeAxis run = seam_part(a0, nc0, part);
        if (run.count <= 0) continue;   // (wave-uniform)
        const int beg = (int)cell_first[base + run.first], end = (int)cell_first[base + run.first + run.count];
        for (int j = beg + lane; j < end; j += 64) {
          const AtomRec rj = rec[j];   // (a kernel whose lambda reads no field of it, k_probe_lj: the unused loads are dead code)
          double dx, dy, dz;
          min_image_rint(pbox, px, py, pz, rj.x, rj.y, rj.z, dx, dy, dz);
          f(j, rj, dx, dy, dz);
        }
      }
    }
  }
}

}  // namespace polar
