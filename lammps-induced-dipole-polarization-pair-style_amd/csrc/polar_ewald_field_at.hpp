// polar_ewald_field_at.hpp -- the Ewald field and potential of the polarized box at arbitrary points, for handles with
// `polar_ewald` (polar_ewald_field_at() of include/polar_mi355x.h; formulas: polar_ewald_point.hpp).  Part of
// the hand-written HIP kernels (gfx950 / CDNA4, wave64) of the lj/cut/coul/long/polarization pair style.
//
// k_ew_point_real: the real-space static sums and the induced sums.  ONE WAVE PER POINT, four points per 256-thread workgroup,
//   the closed-form wrap of the point into the box and then the walk of k_field_at (both polar_point_walk.hpp's): every record in
//   exact mode; in list mode the runs of the +-2 stencil through d_cell_first are listed once per point into LDS and walked from
//   there (ew_point_walk), so that the pair loop carries no stencil state: erfc and erf take the registers.  Lanes stride
//   the records, eight wave_sums, lane 0 stores, no atomics.  The walk runs twice per point, once for the induced sums and once
//   for the static ones.
// k_ew_point_recip: the reciprocal sums.  One thread per point, 256 per workgroup; blockIdx.y indexes a chunk of (h, k) rows of
//   the step's own k-vector table (ew_point_rows_per_chunk: a function of the table alone), so that a few hundred points still
//   fill the machine.  kv, S and rows are wave-uniform loads out of L2; per (point, k) one complex multiply and the four sums.
//   Per-chunk partials part[chunk][4][npts].
// k_ew_point_fold: adds the partials in chunk order onto the real-space results and applies e2s and the neutralising-background
//   term -pi Q / (g^2 V) of the potential.  k_ew_point_qsum: Q = sum of the records' charges, one workgroup, fixed order.
// A point's bits depend on the point, the records and the k-vector table -- not on its pass, its neighbours or their order.
#pragma once

#include "polar_common.hpp"
#include "polar_ewald.hpp"         // EwCell, ew_frac
#include "polar_ewald_point.hpp"
#include "polar_field_at.hpp"      // FieldAtOut
#include "polar_point_walk.hpp"    // in_vgpr, point_wrap, stencil_axis, seam_part, point_walk_all
#include "polar_rows.hpp"          // PairMath

namespace polar {

// the device form of polar_ewald_point.hpp's math policy: PairMath's rsqrt and exponential for the induced branch, the
// device library's erfc / erf / exp (the ones ewald_b1 of the step calls)
struct EwPointMath {
  const ExpCoef &K;
  __device__ __forceinline__ double rsqrt(double x) const { return rsqrt_pos3(x); }
  __device__ __forceinline__ double exp_neg(double x) const { return exp_neg_fast<12>(x, K); }
  __device__ __forceinline__ double exp(double x) const { return ::exp(x); }
  __device__ __forceinline__ double erfc(double x) const { return ::erfc(x); }
  __device__ __forceinline__ double erf(double x) const { return ::erf(x); }
};

struct EwRecipMath {   // (the reciprocal sums need the phases only)
  __device__ __forceinline__ void sincospi(double x, double *s, double *c) const { ::sincospi(x, s, c); }
};

// The walk of one point's candidate records, lanes striding them: every record with Domain::closest_image's image (exact mode),
// or the runs of consecutive records listed in `runs` with the list mode's rounded image.  f(j, record, dx, dy, dz) per candidate.
template <bool ALLPAIRS, class F>
__device__ __forceinline__ void ew_point_walk(int lane, int nlocal, const AtomRec *__restrict__ rec, const Box &box, double px, double py,
                                              double pz, const int *runs, int nruns, F f) {
  if (ALLPAIRS) {
    point_walk_all(lane, nlocal, rec, box, px, py, pz, f);
  } else {
    for (int r = 0; r < nruns; r++) {
      const int beg = __builtin_amdgcn_readfirstlane(runs[2 * r]), end = __builtin_amdgcn_readfirstlane(runs[2 * r + 1]);
      for (int j = beg + lane; j < end; j += 64) {
        const AtomRec rj = rec[j];
        double dx, dy, dz;
        min_image_rint(box, px, py, pz, rj.x, rj.y, rj.z, dx, dy, dz);
        f(j, rj, dx, dy, dz);
      }
    }
  }
}

template <bool ALLPAIRS, int DAMP, bool PHI>
static __global__ __launch_bounds__(POLAR_BLOCK) void k_ew_point_real(int npts, const double *__restrict__ xp, const int *__restrict__ skip_atom,
                                                               const int *__restrict__ pmol, const int *__restrict__ inv, int nlocal,
                                                               const Scal *scal, const AtomRec *__restrict__ recA,
                                                               const AtomRec *__restrict__ recB, const int *__restrict__ mol_s, Box box,
                                                               CellGrid g, const long long *__restrict__ cell_first,
                                                               PointCut cut_in, EwPointParm ew_in, double e2s_in, ExpCoef K, FieldAtOut out) {
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
  if (!ALLPAIRS) asm volatile("" : "+v"(obase));   // (what only the last lines need does not sit in scalar registers through the loops)
  ExpCoef Kp = K;
  if (!ALLPAIRS && DAMP == 0) { Kp.log2e = in_vgpr(K.log2e); Kp.ln2hi = in_vgpr(K.ln2hi); Kp.ln2lo = in_vgpr(K.ln2lo); }   // (as k_field_at)
  const EwPointMath pmath{Kp};
  PointSums s = {0, 0, 0, 0, 0, 0, 0, 0};
  point_wrap(box, g.lo, px, py, pz);
  // the box of the pair loops: list mode's is periodic in every direction (polar_ewald steps run in no other box) and sits in
  // vector registers
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
    // The runs of consecutive records of the +-2 stencil, worked out once by the first lanes and parked in LDS -- per (z, y) of
    // the stencil one run of cells along x, two where it crosses the periodic seam; an axis with fewer than five cells is
    // walked once, cells 0 .. nc-1 -- so that the pair loops, whose erfc / erf need the scalar registers, carry no stencil state.
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
  // Two walks, the induced sums first: the exponential of the damping and erfc / erf with the Gaussian each hold a set of
  // constants and a register file's worth of temporaries, and one loop with both spills scalar registers in list mode.  The
  // second walk finds the records in L1 / L2.
  ew_point_walk<ALLPAIRS>(lane, nlocal, rec, pbox, px, py, pz, runs, nruns, [&](int j, const AtomRec &rj, double dx, double dy, double dz) {
    if (j != sk) polar_point_pair<ALLPAIRS, DAMP, PHI>(pmath, dx, dy, dz, rj.q, rj.mx, rj.my, rj.mz, rj.a, false, cut, s);   // (the induced branch)
  });
  ew_point_walk<ALLPAIRS>(lane, nlocal, rec, pbox, px, py, pz, runs, nruns, [&](int j, const AtomRec &rj, double dx, double dy, double dz) {
    const bool kept = (pm == 0 || pm != mol[j]) && j != sk;
    polar_point_pair_ew<ALLPAIRS, DAMP, PHI>(pmath, dx, dy, dz, rj.q, 0.0, 0.0, 0.0, 0.0, kept, false, cut, ew, s);
  });
  s.esx = wave_sum(s.esx); s.esy = wave_sum(s.esy); s.esz = wave_sum(s.esz);
  s.eix = wave_sum(s.eix); s.eiy = wave_sum(s.eiy); s.eiz = wave_sum(s.eiz);
  if (PHI) { s.ps = wave_sum(s.ps); s.pi = wave_sum(s.pi); }
  if (lane == 0) {
    double *es = obase + 3 * (size_t)p, *ei = obase + 3 * (size_t)npts + 3 * (size_t)p;
    es[0] = e2s * s.esx; es[1] = e2s * s.esy; es[2] = e2s * s.esz;
    ei[0] = s.eix; ei[1] = s.eiy; ei[2] = s.eiz;
    if (PHI) { obase[6 * (size_t)npts + p] = e2s * s.ps; obase[7 * (size_t)npts + p] = s.pi; }   // (FieldAtOut's layout)
  }
}

// the reciprocal sums of the points p0 .. p0 + np - 1 of a pass over the rows of chunk blockIdx.y -> part[chunk][4][np]
template <bool PHI>
static __global__ __launch_bounds__(256) void k_ew_point_recip(int np, int p0, const double *__restrict__ xp, Box box, double lo0, double lo1,
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
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  const EwRecipMath m;
  ew_point_rows<PHI>(m, sx, sy, sz, rows, kv, S, r0, r1, acc);
  double *o = part + (size_t)blockIdx.y * 4 * np + t;
  o[0] = acc[0]; o[(size_t)np] = acc[1]; o[2 * (size_t)np] = acc[2];
  if (PHI) o[3 * (size_t)np] = acc[3];
}

// Q = the sum of the records' charges: one workgroup, a fixed order
static __global__ __launch_bounds__(256) void k_ew_point_qsum(int n, const AtomRec *__restrict__ rec, double *__restrict__ q_out) {
  __shared__ double lds4[4];
  double a = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) a += rec[i].q;
  const double s = ew_block_sum(a, lds4);
  if (threadIdx.x == 0) q_out[0] = s;
}

// chunk partials, in chunk order, onto the real-space results of the points p0 .. p0 + np - 1 of a pass of npts points;
// qterm = -pi / (g^2 V), the potential of the neutralising background per unit of charge
template <bool PHI>
static __global__ __launch_bounds__(256) void k_ew_point_fold(int np, int p0, int npts, int nchunk, const double *__restrict__ part, double e2s,
                                                              double qterm, const double *__restrict__ q_tot, FieldAtOut out) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= np) return;
  double a[4] = {0.0, 0.0, 0.0, 0.0};
  for (int c = 0; c < nchunk; c++) {
    const double *b = part + (size_t)c * 4 * np + t;
    a[0] += b[0]; a[1] += b[(size_t)np]; a[2] += b[2 * (size_t)np];
    if (PHI) a[3] += b[3 * (size_t)np];
  }
  const size_t p = (size_t)p0 + t;
  double *es = out.es() + 3 * p;
  es[0] = fma(e2s, a[0], es[0]); es[1] = fma(e2s, a[1], es[1]); es[2] = fma(e2s, a[2], es[2]);
  if (PHI) out.ps(npts)[p] = fma(e2s, fma(qterm, q_tot[0], a[3]), out.ps(npts)[p]);
}

}  // namespace polar
