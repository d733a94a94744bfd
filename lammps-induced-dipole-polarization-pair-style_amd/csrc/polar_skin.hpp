// polar_skin.hpp -- which entries of a symmetrised LJ/Coulomb row a step has to walk (polar_rows.hpp: k_sym_count, k_sym_fill,
// k_lj_walk; DESIGN.md section 4, "a3").
//
// When the symmetrised list is built every entry of a row is put into a distance class by r0, the pair's distance at that moment:
//   class 0            r0^2 < r_cmax^2 (1 + SKIN_GUARD)                    (r_cmax: the largest pair cutoff of the type table)
//   class k, 1 <= k    skin_bound(k) <= r0 < skin_bound(k + 1),            skin_bound(k) = r_cmax + (k - 1) SKIN_SHELL
//   class K - 1        skin_bound(K - 1) <= r0                             (open-ended)
// and a row holds class 0, then class 1, ... back to back.  With d_max the largest displacement of any atom since then, a pair
// is now at r >= r0 - 2 d_max: a class whose lower bound stays at or beyond r_cmax after 2 d_max came off cannot hold a pair
// inside any cutoff, and the row is walked only up to the end of the last class that can (skin_walk_classes).
//
// Plain functions, the same text for the kernels and for the host (tests/skin/skin_host.cpp): no HIP header is needed.
#pragma once

#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define POLAR_SKIN_HD __host__ __device__
#else
#define POLAR_SKIN_HD
#endif

namespace polar {

constexpr int SKIN_CLASSES = 8;        // K
constexpr double SKIN_SHELL = 0.25;    // A: width of the classes 1 .. K - 2
// Class 0 reaches a hair beyond r_cmax: the force loop forms r^2 with its own instruction sequence, and a pair the loop sees at
// r^2 < cutsq by one rounding must not have been classed outside (1e-12 relative is four orders above a rounding of r^2).
constexpr double SKIN_GUARD = 1e-12;
// ... and the drift counts a little more than measured: covers the roundings of the displacement, of its square root and of
// the squared class bounds wherever a bound minus the drift comes near r_cmax (there 2 d_max >= SKIN_SHELL)
constexpr double SKIN_SLACK = 1e-9;

// lower bound (a distance) of class k
POLAR_SKIN_HD inline double skin_bound(double r_cmax, int k) { return k <= 0 ? 0.0 : r_cmax + (k - 1) * SKIN_SHELL; }

// class of a pair that was r0sq = r0^2 apart when the list was built
POLAR_SKIN_HD inline int skin_class(double r0sq, double r_cmax) {
  if (r0sq < r_cmax * r_cmax * (1.0 + SKIN_GUARD)) return 0;
  int c = 1;
  for (int k = 2; k < SKIN_CLASSES; k++) {
    const double b = skin_bound(r_cmax, k);
    if (r0sq >= b * b) c = k;
  }
  return c;
}

// k*: how many leading classes a step walks when no atom has moved farther than sqrt(dmax_sq) since the classes were made
// (class 0 always; class k while skin_bound(k) - 2 d_max (1 + SKIN_SLACK) < r_cmax).  Anything that is not a finite
// non-negative number walks every class.
POLAR_SKIN_HD inline int skin_walk_classes(double dmax_sq, double r_cmax) {
  if (!(dmax_sq >= 0.0) || !(dmax_sq < 1e300)) return SKIN_CLASSES;
  const double reach = 2.0 * sqrt(dmax_sq) * (1.0 + SKIN_SLACK);
  int ks = 1;
  for (int k = 1; k < SKIN_CLASSES; k++)
    if (skin_bound(r_cmax, k) - reach < r_cmax) ks = k + 1;
  return ks;
}

}  // namespace polar
