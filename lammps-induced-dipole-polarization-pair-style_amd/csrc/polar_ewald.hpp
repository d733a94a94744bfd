// polar_ewald.hpp -- `polar_ewald <accuracy>` (extension keyword): the reciprocal-space half of an Ewald-summed static field
// and of its charge-dipole forces.  The real-space half (erfc-damped pair terms, the erf correction of the excluded
// same-molecule pairs) is the EW flag of k_static_field / k_polar_force (polar_rows.hpp).  Formulas: DESIGN section 6c.
//
// k-vectors k = 2 pi H^-T n over the half space (h > 0, or h = 0 and k > 0, or h = k = 0 and l > 0) with |k| <= k_cut,
// in lexicographic (h, k, l) order: for a fixed (h, k) the l's with |k| <= k_cut are one run ("row").
// Phases e^{i k.r} = e^{2 pi i (h s_x + k s_y + l s_z)} with s = H^-1 r: no FP64 sincos per (atom, k) --
//   structure factors: per-atom, per-axis power tables e^{2 pi i m s_a} in LDS, built by recurrences;
//   per-atom field / force: one sincospi per (atom, row), then the row's l's by the recurrence p <- p e^{2 pi i s_z}.
// No floating-point atomics: per-workgroup partials, folded in a fixed order, so `deterministic yes` stays bit-exact.
#pragma once

#include "polar_common.hpp"

namespace polar {

#define POLAR_EW_SEG 16  // power-table entries per recurrence segment (one sincospi starts each)

struct EwCell {          // H^-1 of the box (upper triangular): s = H^-1 r
  double i00, i01, i02, i11, i12, i22;
};
__device__ __forceinline__ void ew_frac(const EwCell &c, double x, double y, double z, double &sx, double &sy, double &sz) {
  sz = c.i22 * z;
  sy = c.i11 * y + c.i12 * z;
  sx = c.i00 * x + c.i01 * y + c.i02 * z;
}
__device__ __forceinline__ double2 cmul(double2 a, double2 b) {
  return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
__device__ __forceinline__ double2 cis2pi(double t) {  // e^{2 pi i t}
  double s, c;
  sincospi(2.0 * t, &s, &c);
  return make_double2(c, s);
}
__device__ __forceinline__ const AtomRec *ew_cur(const Scal *scal, const AtomRec *recA, const AtomRec *recB) {
  return (scal && __builtin_amdgcn_readfirstlane(scal->cur)) ? recB : recA;
}

// Structure factors, per-workgroup partials.  MU = false: S(k) = sum_j q_j e^{ik.r_j};  MU = true: M(k) = sum_j (k.mu_j) e^{ik.r_j}.
// grid = (k blocks of 256, atom chunks); one thread per k-vector; the atoms of the chunk are staged TILE at a time as power
// tables tab[atom][axis][m] = e^{2 pi i m s_axis}, m = 0 .. nm (contiguous in m: consecutive l's of a row hit consecutive banks).
template <bool MU>
static __global__ __launch_bounds__(256) void k_ew_sfac(int nk, const int4 *__restrict__ hkl, const double4 *__restrict__ kv, int n,
                                                       int chunk, int tile, int nm, EwCell cell, const Scal *scal,
                                                       const AtomRec *__restrict__ recA, const AtomRec *__restrict__ recB,
                                                       double2 *__restrict__ part) {
  extern __shared__ double2 ew_lds[];
  double2 *tab = ew_lds;                                         // [tile][3][nm + 1]
  double *w = reinterpret_cast<double *>(tab + (size_t)tile * 3 * (nm + 1));  // [tile][3]: q (MU = false) or mu
  const AtomRec *rec = ew_cur(scal, recA, recB);
  const int kk = blockIdx.x * 256 + threadIdx.x;
  const bool kok = kk < nk;
  const int4 n3 = kok ? hkl[kk] : make_int4(0, 0, 0, 0);
  const double4 k4 = kok ? kv[kk] : make_double4(0, 0, 0, 0);
  const int ah = n3.x, ak = n3.y < 0 ? -n3.y : n3.y, al = n3.z < 0 ? -n3.z : n3.z;
  const double sk = n3.y < 0 ? -1.0 : 1.0, sl = n3.z < 0 ? -1.0 : 1.0;
  const int nseg = nm / POLAR_EW_SEG + 1;
  const int a0 = blockIdx.y * chunk, a1 = min(n, a0 + chunk);
  double2 acc = make_double2(0.0, 0.0);
  for (int t0 = a0; t0 < a1; t0 += tile) {
    const int nt = min(tile, a1 - t0);
    __syncthreads();  // the previous tile is consumed
    for (int u = threadIdx.x; u < nt * 3 * nseg; u += 256) {
      const int t = u / (3 * nseg), r = u % (3 * nseg), ax = r / nseg, seg = r % nseg;
      const AtomRec &ra = rec[t0 + t];
      double s3[3];
      ew_frac(cell, ra.x, ra.y, ra.z, s3[0], s3[1], s3[2]);
      const double s = s3[ax];
      const int m0 = seg * POLAR_EW_SEG, m1 = min(nm, m0 + POLAR_EW_SEG - 1);
      double2 p = cis2pi((double)m0 * s);
      const double2 b = cis2pi(s);
      double2 *row = tab + ((size_t)t * 3 + ax) * (nm + 1);
      for (int m = m0; m <= m1; m++) { row[m] = p; p = cmul(p, b); }
      if (seg == 0) {
        if (MU) w[3 * t + ax] = ax == 0 ? ra.mx : (ax == 1 ? ra.my : ra.mz);
        else w[3 * t + ax] = ra.q;
      }
    }
    __syncthreads();
    if (kok) {
      for (int t = 0; t < nt; t++) {
        const double2 *tt = tab + (size_t)t * 3 * (nm + 1);
        const double2 X = tt[ah], Y = tt[(nm + 1) + ak], Z = tt[2 * (nm + 1) + al];
        const double2 p = cmul(cmul(X, make_double2(Y.x, sk * Y.y)), make_double2(Z.x, sl * Z.y));
        const double wt = MU ? (k4.x * w[3 * t] + k4.y * w[3 * t + 1] + k4.z * w[3 * t + 2]) : w[3 * t];
        acc.x += wt * p.x; acc.y += wt * p.y;
      }
    }
  }
  if (kok) part[(size_t)blockIdx.y * nk + kk] = acc;
}

// partials of the atom chunks -> one structure factor per k, summed in chunk order
static __global__ void k_ew_fold(int nk, int nchunk, const double2 *__restrict__ part, double2 *__restrict__ out) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nk) return;
  double2 a = part[k];
  for (int c = 1; c < nchunk; c++) { const double2 b = part[(size_t)c * nk + k]; a.x += b.x; a.y += b.y; }
  out[k] = a;
}

// fixed-order sum of a 256-thread workgroup (4 waves)
__device__ __forceinline__ double ew_block_sum(double v, double *lds4) {
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) lds4[wv] = v;
  __syncthreads();
  return ((lds4[0] + lds4[1]) + (lds4[2] + lds4[3]));
}

// Reciprocal static field of every atom (s space), before the solve: E_i = e2s sum_k c_k k Im(e^{ik.r_i} conj S(k)),
// c_k = (8 pi / V) e^{-k^2/4g^2} / k^2 (kv[k].w).  rows[r] = {h, k, lmin, first k index}; rows[nrow].w = nk.
static __global__ __launch_bounds__(256) void k_ew_field(int n, int nrow, const int4 *__restrict__ rows, const double4 *__restrict__ kv,
                                                        const double2 *__restrict__ S, EwCell cell, double e2s,
                                                        const AtomRec *__restrict__ rec, double *__restrict__ erec) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const AtomRec ri = rec[i];
  double sx, sy, sz;
  ew_frac(cell, ri.x, ri.y, ri.z, sx, sy, sz);
  const double2 bz = cis2pi(sz);
  double ex = 0, ey = 0, ez = 0;
  for (int r = 0; r < nrow; r++) {
    const int4 rw = rows[r];
    const int k1 = rows[r + 1].w;
    double2 p = cis2pi((double)rw.x * sx + (double)rw.y * sy + (double)rw.z * sz);
    for (int k = rw.w; k < k1; k++) {
      const double4 kc = kv[k];
      const double2 sk = S[k];
      const double v = kc.w * (p.y * sk.x - p.x * sk.y);
      ex += v * kc.x; ey += v * kc.y; ez += v * kc.z;
      p = cmul(p, bz);
    }
  }
  erec[3 * i] = e2s * ex; erec[3 * i + 1] = e2s * ey; erec[3 * i + 2] = e2s * ez;
}

// Reciprocal charge-dipole force (mu fixed), after the solve, added into f (caller's order; no other kernel writes f now):
//   F_i = e2s sum_k c_k k [ (k.mu_i) Re(e^{ik.r_i} conj S) - q_i Re(e^{ik.r_i} conj M) ]
// and the per-workgroup partials part[block][8] of
//   [0] u_ef = -sum_i mu_i . E_static,i  (the whole charge-dipole energy: real + reciprocal field)
//   [1..6] -sum_i mu_i,a E_rec,i,b  for ab = xx, yy, zz, xy, xz, yz  (the atom part of the reciprocal virial)
static __global__ __launch_bounds__(256) void k_ew_force(int n, int nrow, const int4 *__restrict__ rows, const double4 *__restrict__ kv,
                                                        const double2 *__restrict__ S, const double2 *__restrict__ M, EwCell cell,
                                                        double e2s, const Scal *scal, const AtomRec *__restrict__ recA,
                                                        const AtomRec *__restrict__ recB, const int *__restrict__ perm,
                                                        const double *__restrict__ ef_s, const double *__restrict__ erec,
                                                        double *__restrict__ f, double *__restrict__ part) {
  __shared__ double lds4[4];
  const AtomRec *rec = ew_cur(scal, recA, recB);
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  double t[7] = {0, 0, 0, 0, 0, 0, 0};
  if (i < n) {
    const AtomRec ri = rec[i];
    double sx, sy, sz;
    ew_frac(cell, ri.x, ri.y, ri.z, sx, sy, sz);
    const double2 bz = cis2pi(sz);
    double fx = 0, fy = 0, fz = 0;
    if (ri.q != 0.0 || ri.mx != 0.0 || ri.my != 0.0 || ri.mz != 0.0) {
      for (int r = 0; r < nrow; r++) {
        const int4 rw = rows[r];
        const int k1 = rows[r + 1].w;
        double2 p = cis2pi((double)rw.x * sx + (double)rw.y * sy + (double)rw.z * sz);
        for (int k = rw.w; k < k1; k++) {
          const double4 kc = kv[k];
          const double2 sk = S[k], mk = M[k];
          const double res = p.x * sk.x + p.y * sk.y, rem = p.x * mk.x + p.y * mk.y;
          const double kmu = kc.x * ri.mx + kc.y * ri.my + kc.z * ri.mz;
          const double v = kc.w * (kmu * res - ri.q * rem);
          fx += v * kc.x; fy += v * kc.y; fz += v * kc.z;
          p = cmul(p, bz);
        }
      }
      const int o = perm ? perm[i] : i;
      f[3 * o] += e2s * fx; f[3 * o + 1] += e2s * fy; f[3 * o + 2] += e2s * fz;
    }
    const double ex = erec[3 * i], ey = erec[3 * i + 1], ez = erec[3 * i + 2];
    t[0] = -(ri.mx * ef_s[3 * i] + ri.my * ef_s[3 * i + 1] + ri.mz * ef_s[3 * i + 2]);
    t[1] = -ri.mx * ex; t[2] = -ri.my * ey; t[3] = -ri.mz * ez;
    t[4] = -ri.mx * ey; t[5] = -ri.mx * ez; t[6] = -ri.my * ez;
  }
#pragma unroll
  for (int c = 0; c < 7; c++) {
    const double s = ew_block_sum(t[c], lds4);
    if (threadIdx.x == 0) part[(size_t)blockIdx.x * 8 + c] = s;
  }
}

// The k part of the reciprocal virial, per-workgroup partials part[block][8] ([1..6] as above):
//   U_k = -e2s c_k Im(M conj S),   W_ab += U_k (delta_ab - 2 k_a k_b (1/k^2 + 1/(4 g^2)))
static __global__ __launch_bounds__(256) void k_ew_kvirial(int nk, const double4 *__restrict__ kv, const double2 *__restrict__ S,
                                                          const double2 *__restrict__ M, double e2s, double inv4g2,
                                                          double *__restrict__ part) {
  __shared__ double lds4[4];
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  double t[7] = {0, 0, 0, 0, 0, 0, 0};
  if (k < nk) {
    const double4 kc = kv[k];
    const double2 sk = S[k], mk = M[k];
    const double u = -e2s * kc.w * (mk.y * sk.x - mk.x * sk.y);
    const double k2 = kc.x * kc.x + kc.y * kc.y + kc.z * kc.z;
    const double b = 2.0 * (1.0 / k2 + inv4g2);
    t[1] = u * (1.0 - b * kc.x * kc.x); t[2] = u * (1.0 - b * kc.y * kc.y); t[3] = u * (1.0 - b * kc.z * kc.z);
    t[4] = -u * b * kc.x * kc.y; t[5] = -u * b * kc.x * kc.z; t[6] = -u * b * kc.y * kc.z;
  }
#pragma unroll
  for (int c = 1; c < 7; c++) {
    const double s = ew_block_sum(t[c], lds4);
    if (threadIdx.x == 0) part[(size_t)blockIdx.x * 8 + c] = s;
  }
  if (threadIdx.x == 0) part[(size_t)blockIdx.x * 8] = 0.0;
}

// one workgroup: out[c] = sum over the nb partial rows of part[.][c], c = 0 .. 6, in a fixed order
static __global__ __launch_bounds__(256) void k_ew_finish(int nb, const double *__restrict__ part, double *__restrict__ out) {
  __shared__ double lds4[4];
  for (int c = 0; c < 7; c++) {
    double a = 0.0;
    for (int b = threadIdx.x; b < nb; b += 256) a += part[(size_t)b * 8 + c];
    const double s = ew_block_sum(a, lds4);
    if (threadIdx.x == 0) out[c] = s;
  }
}

}  // namespace polar
