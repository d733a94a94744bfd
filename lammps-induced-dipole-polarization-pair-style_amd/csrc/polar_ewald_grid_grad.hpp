// polar_ewald_grid_grad.hpp -- the reciprocal sums of the Ewald field AND of its gradient G_ab = d e_a / d x_b on a regular grid
// of the box, as three 1-D transforms over the step's own k-vector table: the arithmetic of the k_ew_gg_* kernels
// (polar_ewald_field_grad_grid.hpp, polar_ewald_field_grad_grid() of include/polar_mi355x.h; formulas: DESIGN section 6j).
//
// Plain C++ with no HIP header behind it, as polar_ewald_grid.hpp, whose grid, phase tables and grid-point function these stages
// use (EwGrid, ew_grid_slo, ew_grid_point, ew_grid_tab_entry): the device kernels include it, and so does a host test that
// compares the three stages with the direct NumPy sum (tests/test_ewald_grid_grad_host.py).  Every product and sum is rounded as
// written, every fused multiply-add is spelled out (contraction off inside the functions).
//
// Coefficients: NINE sets per k-vector, with U_kappa = c_kappa conj S(kappa) and the Cartesian kappa of the step's table,
//     sets 0..2:  W_c  = kappa_c U_kappa                      (c = x, y, z: the field sets of polar_ewald_grid.hpp)
//     sets 3..8:  W_ab = (kappa_a kappa_b) U_kappa            (ab = xx, yy, zz, xy, xz, yz; the product is rounded once)
// Over the half space of the table, without e2s:
//     e_recip(p)_c = Im sum_kappa W_c e^{i kappa.p},          g_recip(p)_ab = Re sum_kappa W_ab e^{i kappa.p}
// -- the reciprocal term sum_k c_k k_a k_b Re(e^{ik.p} conj S(k)) of polar_ewald_point_grad.hpp; the neutralising background is a
// constant of the potential and adds nothing.
// Stage 1 (over l):  T[row][g_z][9]     = sum over the l's of a row (h, k) of the table   W_kappa P_z[l][g_z]
// Stage 2 (over k):  V[h][line][9]      = sum over the rows of h, in table order          T[row][g_z] P_y[k][g_y],  line = g_z n_y + g_y
// Stage 3 (over h):  sums of a point    = sum over h = 0 .. h_max                          V[h][line] P_x[h][g_x]
// Each stage is one fixed-order loop per output element.  The three field sets keep, stage by stage, the accumulation chains of
// ew_grid_stage_l / _k / _h<false> as written there: the field's reciprocal sums have the bits of polar_ewald_field_grid.
#pragma once

#include "polar_ewald_grid.hpp"

namespace polar {

constexpr int EW_GG_SETS = 9;

// Stage 1, one (row, g_z): t[9] = sum over the row's k-vectors, in table order, of W_kappa P_z[l][g_z]
template <class I4, class D4, class D2>
POLAR_PAIR_FN void ew_gg_stage_l(const I4 *rows, const D4 *kv, const D2 *S, const D2 *pz, int nz, int lmax, int row, int gz, D2 t[9]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const I4 rw = rows[row];
  const int k1 = rows[row + 1].w;
  double ar[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, ai[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int k = rw.w; k < k1; k++) {
    const int l = rw.z + (k - rw.w);
    const D4 kc = kv[k];
    const D2 sk = S[k];
    const D2 p = pz[(size_t)(l + lmax) * (size_t)nz + (size_t)gz];
    const double ur = kc.w * sk.x, ui = -(kc.w * sk.y);   // U = c conj S
    const double zr = POLAR_POINT_FMA(ur, p.x, -(ui * p.y)), zi = POLAR_POINT_FMA(ur, p.y, ui * p.x);
    const double w[9] = {kc.x, kc.y, kc.z, kc.x * kc.x, kc.y * kc.y, kc.z * kc.z, kc.x * kc.y, kc.x * kc.z, kc.y * kc.z};
#if defined(__clang__)
#pragma unroll
#endif
    for (int c = 0; c < 9; c++) { ar[c] = POLAR_POINT_FMA(w[c], zr, ar[c]); ai[c] = POLAR_POINT_FMA(w[c], zi, ai[c]); }
  }
  for (int c = 0; c < 9; c++) { t[c].x = ar[c]; t[c].y = ai[c]; }
}

// Stage 2, one (h, line): v[9] = sum over the rows r0 .. r1-1 of h, in table order, of T[row][g_z] P_y[k][g_y].
// T[(row nz + g_z) 9 + set]; py = the y table.
template <class I4, class D2>
POLAR_PAIR_FN void ew_gg_stage_k(const I4 *rows, const D2 *T, const D2 *py, int r0, int r1, int nz, int ny, int kmax, int gz, int gy,
                                 D2 v[9]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double ar[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, ai[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int r = r0; r < r1; r++) {
    const D2 p = py[(size_t)(rows[r].y + kmax) * (size_t)ny + (size_t)gy];
    const D2 *t = T + ((size_t)r * (size_t)nz + (size_t)gz) * 9;
#if defined(__clang__)
#pragma unroll
#endif
    for (int c = 0; c < 9; c++) {
      const D2 tc = t[c];
      ar[c] = POLAR_POINT_FMA(-tc.y, p.y, POLAR_POINT_FMA(tc.x, p.x, ar[c]));
      ai[c] = POLAR_POINT_FMA(tc.y, p.x, POLAR_POINT_FMA(tc.x, p.y, ai[c]));
    }
  }
  for (int c = 0; c < 9; c++) { v[c].x = ar[c]; v[c].y = ai[c]; }
}

// Stage 3, one point: acc = {ex, ey, ez, gxx, gyy, gzz, gxy, gxz, gyz} += over h = 0 .. hmax of Im(V_c P_x) (c = 0, 1, 2) and
// Re(V_ab P_x) (sets 3..8).  v = the point's line in V[h = 0], vstride = entries from one h to the next; px = the x table.
// FIELD = false leaves acc[0..2] untouched and gives the same gradient bits.
template <bool FIELD, class D2>
POLAR_PAIR_FN void ew_gg_stage_h(const D2 *v, size_t vstride, const D2 *px, int nx, int hmax, int gx, double acc[9]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double ex = acc[0], ey = acc[1], ez = acc[2];
  double g0 = acc[3], g1 = acc[4], g2 = acc[5], g3 = acc[6], g4 = acc[7], g5 = acc[8];
#if defined(__clang__)
#pragma unroll 2   // (the loads of two h's in flight; the sums stay one chain in h order)
#endif
  for (int h = 0; h <= hmax; h++) {
    const D2 p = px[(size_t)h * (size_t)nx + (size_t)gx];
    const D2 *vh = v + (size_t)h * vstride;
    if (FIELD) {
      const D2 v1 = vh[0], v2 = vh[1], v3 = vh[2];
      ex = POLAR_POINT_FMA(v1.y, p.x, POLAR_POINT_FMA(v1.x, p.y, ex));
      ey = POLAR_POINT_FMA(v2.y, p.x, POLAR_POINT_FMA(v2.x, p.y, ey));
      ez = POLAR_POINT_FMA(v3.y, p.x, POLAR_POINT_FMA(v3.x, p.y, ez));
    }
    const D2 w0 = vh[3], w1 = vh[4], w2 = vh[5], w3 = vh[6], w4 = vh[7], w5 = vh[8];
    g0 = POLAR_POINT_FMA(-w0.y, p.y, POLAR_POINT_FMA(w0.x, p.x, g0));
    g1 = POLAR_POINT_FMA(-w1.y, p.y, POLAR_POINT_FMA(w1.x, p.x, g1));
    g2 = POLAR_POINT_FMA(-w2.y, p.y, POLAR_POINT_FMA(w2.x, p.x, g2));
    g3 = POLAR_POINT_FMA(-w3.y, p.y, POLAR_POINT_FMA(w3.x, p.x, g3));
    g4 = POLAR_POINT_FMA(-w4.y, p.y, POLAR_POINT_FMA(w4.x, p.x, g4));
    g5 = POLAR_POINT_FMA(-w5.y, p.y, POLAR_POINT_FMA(w5.x, p.x, g5));
  }
  if (FIELD) { acc[0] = ex; acc[1] = ey; acc[2] = ez; }
  acc[3] = g0; acc[4] = g1; acc[5] = g2; acc[6] = g3; acc[7] = g4; acc[8] = g5;
}

}  // namespace polar
