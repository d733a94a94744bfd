// polar_probe_plan.hpp -- what polar_probe_at (include/polar_mi355x.h) decides on the host before a
// kernel runs, and the one piece of that arithmetic its kernel shares: the input checks, the reach of every probe type in
// the LJ table, the rule that says whether the walk of k_probe_lj (polar_probe_at.hpp) meets every partner within that
// reach, and the trimmed cell stencil of a point.
//
// Pure functions, plain C++17, in the manner of polar_plan.hpp: no HIP header, no handle, nothing read from the environment
// (POLAR_PLAN_FN is __host__ __device__ under hipcc).  tests/test_probe_plan_host.py drives them through
// tests/probe_plan/probe_plan.cpp.
#pragma once

#include <algorithm>
#include <cmath>
#include <vector>

#include "pair_host.hpp"     // InputError, Unsupported
#include "polar_plan.hpp"    // POLAR_PLAN_FN

namespace polar {

// ---- input checks (beyond check_points of polar_input.hpp) ----------------------------------------------------------------
// type (1 .. ntypes per point; may be null only when no LJ output is asked for), q and alpha (either may be null = 0): finite,
// alpha >= 0.
inline void check_probe_sites(long long npoints, const int *type, int ntypes, const double *q, const double *alpha, bool want_lj) {
  if (want_lj && !type) throw InputError("polar_probe_at: e_lj / f_lj need the type of every point");
  if (type)
    for (long long p = 0; p < npoints; p++)
      if (type[p] < 1 || type[p] > ntypes) throw InputError("polar_probe_at: type outside [1, ntypes]");
  if (q)
    for (long long p = 0; p < npoints; p++)
      if (!std::isfinite(q[p])) throw InputError("polar_probe_at: non-finite charge");
  if (alpha)
    for (long long p = 0; p < npoints; p++)
      if (!std::isfinite(alpha[p]) || alpha[p] < 0.0) throw InputError("polar_probe_at: polarizability non-finite or negative");
}

// ---- per-type reach --------------------------------------------------------------------------------------------------------
// reach[t] = max_j cut_lj[t][t_j] over the types 1 .. ntypes of the packed table (pack_lj_table: entry 1 of a pair's eight
// doubles is cut_ljsq); reach[0] = 0.  Returns the largest.
inline double probe_reach(int ntypes, const double *pack, std::vector<double> &reach) {
  const int w = ntypes + 1;
  reach.assign((size_t)w, 0.0);
  double rmax = 0.0;
  for (int t = 1; t <= ntypes; t++) {
    double c2 = 0.0;
    for (int j = 1; j <= ntypes; j++) c2 = std::max(c2, pack[8 * ((size_t)t * w + j) + 1]);
    reach[t] = std::sqrt(c2);
    rmax = std::max(rmax, reach[t]);
  }
  return rmax;
}

// ---- the LJ reach rule -------------------------------------------------------------------------------------------------------
// List mode: the list grid's cells are at least cutall / 2 high (list_grid, polar_plan.hpp), cutall = max(cut_coul, dd_cutoff):
// five cells per axis cover a sphere of radius cutall, and the rounded image is the nearest one inside it.
inline bool probe_reach_ok_list(double reach_max, double cut_coul, double dd_cutoff) { return reach_max <= std::max(cut_coul, dd_cutoff); }
// Exact mode: every periodic perpendicular width >= 2 reach (1 - 1e-12).  The nearest image is then the only one within reach
// -- what the reference's neighbor list would hold -- and closest_image picks a farther image only at distances >= half the
// shortest edge.  A non-periodic direction has no rule.
inline bool probe_reach_ok_exact(const double width[3], const int periodic[3], double reach_max) {
  for (int k = 0; k < 3; k++)
    if (periodic[k] && width[k] < 2.0 * reach_max * (1.0 - 1e-12)) return false;
  return true;
}
// ... both, as the entry point asks: throws Unsupported with the rule's words
inline void check_probe_reach(bool list_mode, double reach_max, double cut_coul, double dd_cutoff, const double width[3], const int periodic[3]) {
  if (list_mode) {
    if (!probe_reach_ok_list(reach_max, cut_coul, dd_cutoff))
      throw Unsupported("polar_probe_at: an LJ cutoff beyond max(cut_coul, dd_cutoff): the list grid's stencil does not cover it (e_lj / f_lj)");
  } else if (!probe_reach_ok_exact(width, periodic, reach_max))
    throw Unsupported("polar_probe_at: a periodic box width below two LJ cutoffs: more than one image of an atom within reach (e_lj / f_lj)");
}

// ---- the trimmed stencil ---------------------------------------------------------------------------------------------------
// The cells of one axis a point walks: s = its fractional coordinate (after the closed-form wrap: in [0, 1) to rounding),
// dfrac = reach (1 + 1e-9) / width (the fractional extent of the sphere along the axis, tilted or not: width is the
// perpendicular one), nc cells.  The cells are first, first + 1, ... (count of them), wrapped into [0, nc): those from
// floor((s - dfrac) nc) to floor((s + dfrac) nc), and never further than two cells from the point's own, floor(s nc): the
// stencil k_field_at walks, which covers every reach the rule above lets through (a cell is at least cutall / 2 high) -- the
// 1e-9 of slack would otherwise add a sixth cell for a point on a cell face of a grid whose cells are exactly cutall / 2 high.
// A range of nc cells or more: all of them, once.
struct ProbeAxis { int first, count; };
POLAR_PLAN_FN ProbeAxis probe_axis(double s, double dfrac, int nc) {
  const double c = floor(s * nc);
  double lo = floor((s - dfrac) * nc), hi = floor((s + dfrac) * nc);
  lo = lo < c - 2.0 ? c - 2.0 : lo;
  hi = hi > c + 2.0 ? c + 2.0 : hi;
  if (!(hi - lo + 1.0 < (double)nc)) return ProbeAxis{0, nc};   // (also: anything not a number)
  int first = (int)lo % nc;   // (within two cells of floor(s nc), s in [0, 1] to rounding: an int)
  first += first < 0 ? nc : 0;
  return ProbeAxis{first, (int)(hi - lo) + 1};
}
// The untrimmed rule of every other point kernel (polar_point_walk.hpp): the five cells c - 2 .. c + 2 around the point's own
// cell c, the first wrapped into [0, nc); an axis with fewer than five cells (a periodic one has at least four): all of them,
// once -- the 5-cell stencil would meet a cell twice.
POLAR_PLAN_FN ProbeAxis stencil_axis(int c, int nc) {
  int first = nc < 5 ? 0 : c - 2;
  first += first < 0 ? nc : 0;
  return ProbeAxis{first, nc < 5 ? nc : 5};
}
// An axis range split at the periodic seam: part 0 = the cells from a.first up to the seam, part 1 = the rest, which start at
// cell 0 (count 0: the range does not cross).  Along x a part is one run of consecutive cells, hence of consecutive records.
POLAR_PLAN_FN ProbeAxis seam_part(ProbeAxis a, int nc, int part) {
  const int len_a = a.count < nc - a.first ? a.count : nc - a.first;
  return part ? ProbeAxis{0, a.count - len_a} : ProbeAxis{a.first, len_a};
}
// dfrac of the three axes from a reach and the perpendicular widths
POLAR_PLAN_FN void probe_dfrac_scale(const double width[3], double scale[3]) {
  for (int k = 0; k < 3; k++) scale[k] = (1.0 + 1e-9) / width[k];
}

}  // namespace polar
