// polar_field_grad_at.hpp -- the field of the polarized box at arbitrary points together with its gradient G_ab = d e_a / d x_b,
// and the force that field and gradient put on a charged, polarizable test site (polar_field_grad_at() and
// polar_probe_force_at() of include/polar_mi355x.h; formulas: polar_point_grad_pair.hpp).  Part of the
// hand-written HIP kernels (gfx950 / CDNA4, wave64) of the lj/cut/coul/long/polarization pair style; see polar_kernels.hpp for
// the mapping and the index spaces.
//
// k_field_grad_at has the mapping and the walk of k_field_at (polar_field_at.hpp), both polar_point_walk.hpp's: ONE WAVE PER
// POINT, the closed-form wrap of the point into the box, then every record (ALLPAIRS, exact mode) or the +-2 stencil of the
// point's cell (list mode).  The wrap and the exact-mode walk are called from there; the list-mode loops are point_walk_cells'
// written out in the kernel, because the damped instance is slower through the shared ones.
// The lanes stride the candidate records in k_field_at's order, the 18 sums (6 of the field, 12 of the gradient) are reduced with
// wave_sum, lane 0 stores: no atomics, no LDS, and a point's bits depend on the point and the records alone.  The six field sums
// are formed by k_field_at's expressions in k_field_at's order: they have its bits.
// k_probe_force_combine: one thread per point reads the pass's block and writes f_coul and f_pol of a site with charge q and
// polarizability alpha (polar_probe_force_combine).
#pragma once

#include "polar_common.hpp"
#include "polar_point_grad_pair.hpp"
#include "polar_rows.hpp"    // PairMath
#include "polar_point_walk.hpp"   // in_vgpr, point_wrap, point_walk_all

namespace polar {

// The results of a pass of npts points, one block of 18 * npts doubles: e_static [npts][3], e_induced [npts][3], g_static
// [npts][6], g_induced [npts][6] (xx, yy, zz, xy, xz, yz).  polar_probe_force_at appends f_coul [npts][3] and f_pol [npts][3].
struct FieldGradOut {
  double *base;
  __host__ __device__ double *es() const { return base; }
  __host__ __device__ double *ei(size_t npts) const { return base + 3 * npts; }
  __host__ __device__ double *gs(size_t npts) const { return base + 6 * npts; }
  __host__ __device__ double *gi(size_t npts) const { return base + 12 * npts; }
  __host__ __device__ double *fc(size_t npts) const { return base + 18 * npts; }
  __host__ __device__ double *fp(size_t npts) const { return base + 21 * npts; }
};
#define POLAR_FIELD_GRAD_DOUBLES 24   // per point of a pass buffer: the block and the two forces

template <bool ALLPAIRS, int DAMP>
static __global__ __launch_bounds__(POLAR_BLOCK) void k_field_grad_at(int npts, const double *__restrict__ xp, const int *__restrict__ skip_atom,
                                                               const int *__restrict__ pmol, const int *__restrict__ inv, int nlocal,
                                                               const Scal *scal, const AtomRec *__restrict__ recA,
                                                               const AtomRec *__restrict__ recB, const int *__restrict__ mol_s, Box box,
                                                               CellGrid g, const long long *__restrict__ cell_first,
                                                               PointCut cut_in, double e2s_in, ExpCoef K, FieldGradOut out) {
  const int lane = threadIdx.x & 63;
  const int p = blockIdx.x * POLAR_ROWS_PER_BLOCK + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (p >= npts) return;   // (wave-uniform)
  const AtomRec *__restrict__ rec = __builtin_amdgcn_readfirstlane(scal->cur) ? recB : recA;   // the dipoles the last compute left, as k_unpack
  const int *__restrict__ mol = mol_s;
  double *obase = out.base;
  // (the damped list-mode instance: the table pointers and what only the last lines need go to the vector file too, as in
  // k_ew_point_real -- with them in scalar registers two of those are spilled)
  if (!ALLPAIRS && DAMP == 0) { asm volatile("" : "+v"(mol)); asm volatile("" : "+v"(rec)); asm volatile("" : "+v"(obase)); }
  double px = in_vgpr(xp[3 * (size_t)p]), py = in_vgpr(xp[3 * (size_t)p + 1]), pz = in_vgpr(xp[3 * (size_t)p + 2]);
  const PointCut cut{in_vgpr(cut_in.cut_coulsq), in_vgpr(cut_in.ddcutsq), in_vgpr(cut_in.rc2inv), in_vgpr(cut_in.two_rcinv), in_vgpr(cut_in.pd)};
  const double e2s = in_vgpr(e2s_in);
  int sk = skip_atom ? __builtin_amdgcn_readfirstlane(skip_atom[p]) : -1;
  if (sk >= 0 && inv) sk = __builtin_amdgcn_readfirstlane(inv[sk]);   // the caller's index -> record order
  const int pm = pmol ? __builtin_amdgcn_readfirstlane(pmol[p]) : 0;
  ExpCoef Kp = K;
  if (!ALLPAIRS && DAMP == 0) { Kp.log2e = in_vgpr(K.log2e); Kp.ln2hi = in_vgpr(K.ln2hi); Kp.ln2lo = in_vgpr(K.ln2lo); }   // (as k_field_at)
  const PairMath pmath{Kp, 0.0};
  PointGradSums s = {{0, 0, 0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0}};
  point_wrap(box, g.lo, px, py, pz);
  const auto pair = [&](int j, const AtomRec &rj, double dx, double dy, double dz) {
    const bool molok = pm == 0 || pm != mol[j];
    if (j != sk) polar_point_grad_pair<ALLPAIRS, DAMP>(pmath, dx, dy, dz, rj.q, rj.mx, rj.my, rj.mz, rj.a, molok, cut, s);
  };
  if (ALLPAIRS) {
    point_walk_all(lane, nlocal, rec, box, px, py, pz, pair);
  } else {
    const int c = __builtin_amdgcn_readfirstlane(cell_of(g, box, px, py, pz));
    // the box of the pair loop: every direction is periodic here, which min_image_rint then knows at compile time; the damped
    // instance keeps it in vector registers (in_vgpr), as k_field_at's
    Box pbox = box;
#pragma unroll
    for (int k = 0; k < 3; k++) {
      pbox.periodic[k] = 1;
      if (DAMP == 0) { pbox.prd[k] = in_vgpr(box.prd[k]); pbox.inv[k] = in_vgpr(box.inv[k]); }
    }
    if (DAMP == 0) { pbox.xy = in_vgpr(box.xy); pbox.xz = in_vgpr(box.xz); pbox.yz = in_vgpr(box.yz); }
    // point_walk_cells with stencil_axis on every axis, written out: through the shared loops the damped instance comes out
    // with other code (one copy of the pair body, or two in another order) and measurably slower, see DESIGN section 6h.  Any
    // change to point_walk_cells is made here too.
    const int nc0 = g.nc[0], nc1 = g.nc[1], nc2 = g.nc[2];
    const int c0 = c % nc0, c1 = (c / nc0) % nc1, c2 = c / (nc0 * nc1);
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
            const bool molok = pm == 0 || pm != mol[j];
            if (j != sk) polar_point_grad_pair<false, DAMP>(pmath, dx, dy, dz, rj.q, rj.mx, rj.my, rj.mz, rj.a, molok, cut, s);
          }
        }
      }
    }
  }
  s.f.esx = wave_sum(s.f.esx); s.f.esy = wave_sum(s.f.esy); s.f.esz = wave_sum(s.f.esz);
  s.f.eix = wave_sum(s.f.eix); s.f.eiy = wave_sum(s.f.eiy); s.f.eiz = wave_sum(s.f.eiz);
#pragma unroll
  for (int k = 0; k < 6; k++) { s.gs[k] = wave_sum(s.gs[k]); s.gi[k] = wave_sum(s.gi[k]); }
  if (lane == 0) {
    const FieldGradOut o{obase};
    double *es = o.es() + 3 * (size_t)p, *ei = o.ei(npts) + 3 * (size_t)p;
    double *gs = o.gs(npts) + 6 * (size_t)p, *gi = o.gi(npts) + 6 * (size_t)p;
    es[0] = e2s * s.f.esx; es[1] = e2s * s.f.esy; es[2] = e2s * s.f.esz;
    ei[0] = s.f.eix; ei[1] = s.f.eiy; ei[2] = s.f.eiz;
#pragma unroll
    for (int k = 0; k < 6; k++) { gs[k] = e2s * s.gs[k]; gi[k] = s.gi[k]; }
  }
}

// The force on a site of charge q and polarizability alpha (either array may be null = 0) from the block of its point.
static __global__ void k_probe_force_combine(int npts, const double *__restrict__ q, const double *__restrict__ alpha, double e2s,
                                             FieldGradOut out) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= npts) return;
  double fc[3], fp[3];
  polar_probe_force_combine(out.es() + 3 * (size_t)p, out.ei(npts) + 3 * (size_t)p, out.gs(npts) + 6 * (size_t)p, out.gi(npts) + 6 * (size_t)p,
                            q ? q[p] : 0.0, alpha ? alpha[p] : 0.0, e2s, fc, fp);
  double *oc = out.fc(npts) + 3 * (size_t)p, *op = out.fp(npts) + 3 * (size_t)p;
  oc[0] = fc[0]; oc[1] = fc[1]; oc[2] = fc[2];
  op[0] = fp[0]; op[1] = fp[1]; op[2] = fp[2];
}

}  // namespace polar
