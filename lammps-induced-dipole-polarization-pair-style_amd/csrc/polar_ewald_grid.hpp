// polar_ewald_grid.hpp -- the reciprocal sums of the Ewald field and potential on a regular grid of the box, as three 1-D
// transforms over the step's own k-vector table: the arithmetic of the k_ew_grid_* kernels (polar_ewald_field_grid.hpp,
// polar_ewald_field_grid() of include/polar_mi355x.h; formulas: DESIGN section 6f).
//
// Plain C++ with no HIP header behind it, as polar_ewald_point.hpp: the device kernels include it, and so does a host test that
// compares the three stages with the direct NumPy sum (tests/test_ewald_grid_host.py).  sincospi comes from a policy `M`
// (device: EwRecipMath of polar_ewald_field_at.hpp; host: libm).  Every product and sum is rounded as written, every fused
// multiply-add is spelled out (contraction off inside the functions).
//
// The grid: p(i, j, l) = lo + f_x a + f_y b + f_z c with f = ((i + o_x) / n_x, (j + o_y) / n_y, (l + o_z) / n_z), flat index
// (l n_y + j) n_x + i.  A k-vector kappa = 2 pi H^-T (h, k, l) has the phase e^{i kappa.p} = e^{2 pi i (h s_x + k s_y + l s_z)}
// with s = H^-1 p = f + H^-1 lo (the convention of ew_frac, which does not take the box origin off): one factor per axis,
//     P_a[m][g] = e^{2 pi i m s_a(g)},    s_a(g) = (g + o_a) / n_a + (H^-1 lo)_a,
// each from one sincospi of the product m s_a(g) -- no recurrence.
//
// Coefficients: FOUR sets per k-vector, W_kappa = (1, kappa_x, kappa_y, kappa_z) U_kappa with U_kappa = c_kappa conj S(kappa)
// and the Cartesian kappa of the step's table (the kv the per-point sums multiply by): the field comes out in Cartesian
// components with no 2 pi H^-T behind the sums.  Over the half space of the table, without e2s:
//     phi_recip(p) = Re sum_kappa W_0 e^{i kappa.p},      e_recip(p)_c = Im sum_kappa W_c e^{i kappa.p}
// Stage 1 (over l):  T[row][g_z][4]     = sum over the l's of a row (h, k) of the table   W_kappa P_z[l][g_z]
// Stage 2 (over k):  V[h][line][4]      = sum over the rows of h, in table order          T[row][g_z] P_y[k][g_y],  line = g_z n_y + g_y
// Stage 3 (over h):  sums of a point    = sum over h = 0 .. h_max                          V[h][line] P_x[h][g_x]
// Each stage is one fixed-order loop per output element: an element's bits depend on the grid, S(k) and the table alone.
#pragma once

#include <cstddef>

#include "polar_point_pair.hpp"   // POLAR_PAIR_FN, POLAR_POINT_FMA

namespace polar {

// A call's grid: counts, offsets, the box (a = (ax, 0, 0), b = (bx, by, 0), c = (cx, cy, cz): prd and the tilt factors) and
// slo = H^-1 lo.
struct EwGrid {
  int n[3];
  double off[3], lo[3];
  double ax, bx, by, cx, cy, cz;
  double slo[3];
};

// H^-1 lo, the products and sums of ew_frac (cell = the six entries of H^-1, upper triangle by rows), each rounded as written
inline void ew_grid_slo(const double cell[6], const double lo[3], double slo[3]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  slo[2] = cell[5] * lo[2];
  slo[1] = cell[3] * lo[1] + cell[4] * lo[2];
  slo[0] = cell[0] * lo[0] + cell[1] * lo[1] + cell[2] * lo[2];
}

// the fractional coordinate of grid index g along an axis: one sum, one division
POLAR_PAIR_FN double ew_grid_frac(int g, double off, int n) { return ((double)g + off) / (double)n; }

// The point of a flat index: (i, j, l) by two integer divisions, then z = fma(f_z, cz, lo_z), y = fma(f_y, by, fma(f_z, cy, lo_y)),
// x = fma(f_x, ax, fma(f_y, bx, fma(f_z, cx, lo_x))) -- this order, on the device and on the host.
POLAR_PAIR_FN void ew_grid_point(const EwGrid &g, long long flat, double &px, double &py, double &pz) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const long long line = flat / g.n[0];
  const int i = (int)(flat - line * g.n[0]), l = (int)(line / g.n[1]), j = (int)(line - (long long)l * g.n[1]);
  const double fx = ew_grid_frac(i, g.off[0], g.n[0]), fy = ew_grid_frac(j, g.off[1], g.n[1]), fz = ew_grid_frac(l, g.off[2], g.n[2]);
  pz = POLAR_POINT_FMA(fz, g.cz, g.lo[2]);
  py = POLAR_POINT_FMA(fy, g.by, POLAR_POINT_FMA(fz, g.cy, g.lo[1]));
  px = POLAR_POINT_FMA(fx, g.ax, POLAR_POINT_FMA(fy, g.bx, POLAR_POINT_FMA(fz, g.cx, g.lo[0])));
}

// One entry of a phase table: (c, s) = e^{2 pi i m s_a(g)}, one sincospi of the product
template <class M>
POLAR_PAIR_FN void ew_grid_phase(const M &m, int mi, int g, double off, int n, double slo, double &c, double &s) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double sa = ew_grid_frac(g, off, n) + slo;
  const double arg = (double)mi * sa;
  m.sincospi(2.0 * arg, &s, &c);
}

// The tables of a call in one array of (cos, sin): P_x[h][g_x], h = 0 .. hmax, at 0; P_y[k + kmax][g_y] at off_y;
// P_z[l + lmax][g_z] at off_z.  Entry e of the array:
template <class M>
POLAR_PAIR_FN void ew_grid_tab_entry(const M &m, const EwGrid &g, int kmax, int lmax, size_t off_y, size_t off_z, size_t e, double &c,
                                     double &s) {
  if (e < off_y) {
    const int mi = (int)(e / (size_t)g.n[0]), gi = (int)(e - (size_t)mi * g.n[0]);
    ew_grid_phase(m, mi, gi, g.off[0], g.n[0], g.slo[0], c, s);
  } else if (e < off_z) {
    const size_t r = e - off_y;
    const int mi = (int)(r / (size_t)g.n[1]), gi = (int)(r - (size_t)mi * g.n[1]);
    ew_grid_phase(m, mi - kmax, gi, g.off[1], g.n[1], g.slo[1], c, s);
  } else {
    const size_t r = e - off_z;
    const int mi = (int)(r / (size_t)g.n[2]), gi = (int)(r - (size_t)mi * g.n[2]);
    ew_grid_phase(m, mi - lmax, gi, g.off[2], g.n[2], g.slo[2], c, s);
  }
}

// Stage 1, one (row, g_z): t[4] = sum over the row's k-vectors, in table order, of W_kappa P_z[l][g_z].  rows, kv, S: the step's
// table (polar_plan.hpp) and structure factors; pz = the z table.
template <class I4, class D4, class D2>
POLAR_PAIR_FN void ew_grid_stage_l(const I4 *rows, const D4 *kv, const D2 *S, const D2 *pz, int nz, int lmax, int row, int gz, D2 t[4]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const I4 rw = rows[row];
  const int k1 = rows[row + 1].w;
  double a0r = 0.0, a0i = 0.0, a1r = 0.0, a1i = 0.0, a2r = 0.0, a2i = 0.0, a3r = 0.0, a3i = 0.0;
  for (int k = rw.w; k < k1; k++) {
    const int l = rw.z + (k - rw.w);
    const D4 kc = kv[k];
    const D2 sk = S[k];
    const D2 p = pz[(size_t)(l + lmax) * (size_t)nz + (size_t)gz];
    const double ur = kc.w * sk.x, ui = -(kc.w * sk.y);   // U = c conj S
    const double zr = POLAR_POINT_FMA(ur, p.x, -(ui * p.y)), zi = POLAR_POINT_FMA(ur, p.y, ui * p.x);
    a0r += zr; a0i += zi;
    a1r = POLAR_POINT_FMA(kc.x, zr, a1r); a1i = POLAR_POINT_FMA(kc.x, zi, a1i);
    a2r = POLAR_POINT_FMA(kc.y, zr, a2r); a2i = POLAR_POINT_FMA(kc.y, zi, a2i);
    a3r = POLAR_POINT_FMA(kc.z, zr, a3r); a3i = POLAR_POINT_FMA(kc.z, zi, a3i);
  }
  t[0].x = a0r; t[0].y = a0i; t[1].x = a1r; t[1].y = a1i; t[2].x = a2r; t[2].y = a2i; t[3].x = a3r; t[3].y = a3i;
}

// Stage 2, one (h, line): v[4] = sum over the rows r0 .. r1-1 of h, in table order, of T[row][g_z] P_y[k][g_y].
// T[(row nz + g_z) 4 + set]; py = the y table.
template <class I4, class D2>
POLAR_PAIR_FN void ew_grid_stage_k(const I4 *rows, const D2 *T, const D2 *py, int r0, int r1, int nz, int ny, int kmax, int gz, int gy,
                                   D2 v[4]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double ar[4] = {0.0, 0.0, 0.0, 0.0}, ai[4] = {0.0, 0.0, 0.0, 0.0};
  for (int r = r0; r < r1; r++) {
    const D2 p = py[(size_t)(rows[r].y + kmax) * (size_t)ny + (size_t)gy];
    const D2 *t = T + ((size_t)r * (size_t)nz + (size_t)gz) * 4;
#if defined(__clang__)
#pragma unroll
#endif
    for (int c = 0; c < 4; c++) {
      const D2 tc = t[c];
      ar[c] = POLAR_POINT_FMA(-tc.y, p.y, POLAR_POINT_FMA(tc.x, p.x, ar[c]));
      ai[c] = POLAR_POINT_FMA(tc.y, p.x, POLAR_POINT_FMA(tc.x, p.y, ai[c]));
    }
  }
  for (int c = 0; c < 4; c++) { v[c].x = ar[c]; v[c].y = ai[c]; }
}

// Stage 3, one point: acc = {ex, ey, ez, phi} += over h = 0 .. hmax of Im(V_c P_x) (c = 1, 2, 3) and Re(V_0 P_x).
// v = the point's line in V[h = 0], vstride = entries from one h to the next; px = the x table.
// PHI = false leaves acc[3] untouched and gives the same field bits.
template <bool PHI, class D2>
POLAR_PAIR_FN void ew_grid_stage_h(const D2 *v, size_t vstride, const D2 *px, int nx, int hmax, int gx, double acc[4]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double ex = acc[0], ey = acc[1], ez = acc[2], ph = acc[3];
#if defined(__clang__)
#pragma unroll 4   // (the loads of four h's in flight; the sums stay one chain in h order)
#endif
  for (int h = 0; h <= hmax; h++) {
    const D2 p = px[(size_t)h * (size_t)nx + (size_t)gx];
    const D2 *vh = v + (size_t)h * vstride;
    const D2 v1 = vh[1], v2 = vh[2], v3 = vh[3];
    ex = POLAR_POINT_FMA(v1.y, p.x, POLAR_POINT_FMA(v1.x, p.y, ex));
    ey = POLAR_POINT_FMA(v2.y, p.x, POLAR_POINT_FMA(v2.x, p.y, ey));
    ez = POLAR_POINT_FMA(v3.y, p.x, POLAR_POINT_FMA(v3.x, p.y, ez));
    if (PHI) {
      const D2 v0 = vh[0];
      ph = POLAR_POINT_FMA(-v0.y, p.y, POLAR_POINT_FMA(v0.x, p.x, ph));
    }
  }
  acc[0] = ex; acc[1] = ey; acc[2] = ez;
  if (PHI) acc[3] = ph;
}

}  // namespace polar
