// skin_host.cpp -- csrc/polar_skin.hpp on the host: the decisions the kernels make about which distance classes of a
// symmetrised LJ/Coulomb row a step walks, checked against the geometry they stand for (tests/test_skin_host.py).
//
//   skin_host r_cmax seed        random triples for every d_max, then the edge cases; prints one line per check, "ok ..." or
//                                "FAIL ...", and exits 1 after the first kind of failure
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>

#include "polar_skin.hpp"

using namespace polar;

namespace {
int failures = 0;
void report(bool ok, const char *what, double a = 0.0, double b = 0.0) {
  printf("%s %s %.17g %.17g\n", ok ? "ok" : "FAIL", what, a, b);
  if (!ok) failures++;
}

struct V3 { double x, y, z; };
// a vector of length len * u^(1/3) (uniform in the ball) -- or exactly len when `surface`
V3 in_ball(std::mt19937_64 &rng, double len, bool surface) {
  std::normal_distribution<double> g(0.0, 1.0);
  std::uniform_real_distribution<double> u(0.0, 1.0);
  V3 v{g(rng), g(rng), g(rng)};
  const double n = std::sqrt(v.x * v.x + v.y * v.y + v.z * v.z);
  const double r = n > 0.0 ? (surface ? len : len * std::cbrt(u(rng))) / n : 0.0;
  return V3{v.x * r, v.y * r, v.z * r};
}
}  // namespace

int main(int argc, char **argv) {
  const double rc = argc > 1 ? atof(argv[1]) : 12.0;
  const unsigned long long seed = argc > 2 ? strtoull(argv[2], nullptr, 10) : 1;
  std::mt19937_64 rng(seed);
  const int K = SKIN_CLASSES;
  const double last = skin_bound(rc, K - 1);

  // the bounds: class 0 from 0, class 1 from r_cmax, then steps of one shell
  report(skin_bound(rc, 0) == 0.0 && skin_bound(rc, 1) == rc, "bounds_start");
  for (int k = 2; k < K; k++) report(std::fabs(skin_bound(rc, k) - skin_bound(rc, k - 1) - SKIN_SHELL) < 1e-12, "bounds_step", k);

  const double dmaxes[6] = {0.0, 0.01, 0.3, 1.0, 1.2, 3.0};
  for (double dmax : dmaxes) {
    // how the kernels get d_max^2: the largest |dx|^2 over the atoms -- here the bound itself
    const int ks = skin_walk_classes(dmax * dmax, rc);
    if (dmax == 0.0) report(ks == 1, "dmax0_walks_class0_only", ks);
    if (2.0 * dmax > last - rc) report(ks == K, "beyond_last_shell_walks_all", dmax, ks);
    report(ks >= 1 && ks <= K, "kstar_range", dmax, ks);
    // monotone: more drift never walks less
    report(skin_walk_classes(dmax * dmax * 1.21, rc) >= ks, "kstar_monotone", dmax);
    long long missed = 0, inside = 0, walked = 0;
    double worst = 0.0;
    std::uniform_real_distribution<double> ur(0.5, rc + 2.5);
    std::uniform_real_distribution<double> near(-1.0, 1.0);
    for (int t = 0; t < 100000; t++) {
      // r0: a third anywhere, a third around the walk's edge (where a wrong k* shows), a third around r_cmax + 2 d_max
      double r0 = ur(rng);
      if (t % 3 == 1) r0 = skin_bound(rc, ks < K ? ks : K - 1) + 0.05 * near(rng);
      if (t % 3 == 2) r0 = rc + 2.0 * dmax + 0.02 * near(rng);
      const V3 d0 = in_ball(rng, r0, true);
      const bool adversarial = (t % 2) == 0;   // both atoms move straight towards each other, by the whole d_max
      V3 di, dj;
      if (adversarial) {
        const double s = dmax / r0;
        di = V3{-d0.x * s, -d0.y * s, -d0.z * s}; dj = V3{d0.x * s, d0.y * s, d0.z * s};
      } else { di = in_ball(rng, dmax, false); dj = in_ball(rng, dmax, false); }
      // the pair as the kernels see it: positions, their direct difference
      const V3 xi{3.25 + d0.x, -1.5 + d0.y, 7.125 + d0.z}, xj{3.25, -1.5, 7.125};
      const double ax = xi.x - xj.x, ay = xi.y - xj.y, az = xi.z - xj.z;
      const int c = skin_class(ax * ax + ay * ay + az * az, rc);
      const V3 yi{xi.x + di.x, xi.y + di.y, xi.z + di.z}, yj{xj.x + dj.x, xj.y + dj.y, xj.z + dj.z};
      const double bx = yi.x - yj.x, by = yi.y - yj.y, bz = yi.z - yj.z;
      const double rsq = bx * bx + by * by + bz * bz;
      // the drift as k_pack_lj measures it
      const double mi = (yi.x - xi.x) * (yi.x - xi.x) + (yi.y - xi.y) * (yi.y - xi.y) + (yi.z - xi.z) * (yi.z - xi.z);
      const double mj = (yj.x - xj.x) * (yj.x - xj.x) + (yj.y - xj.y) * (yj.y - xj.y) + (yj.z - xj.z) * (yj.z - xj.z);
      const int ksm = skin_walk_classes(std::fmax(mi, mj), rc);
      if (c < ksm) walked++;
      if (rsq < rc * rc) {
        inside++;
        if (c >= ksm) { missed++; worst = std::fmax(worst, rc - std::sqrt(rsq)); }
      }
    }
    report(missed == 0, "no_pair_inside_cutoff_is_skipped", dmax, (double)missed);
    printf("info dmax %.3g kstar %d inside %lld walked %lld worst %.3g\n", dmax, ks, inside, walked, worst);
  }

  // classes at their bounds
  report(skin_class(0.0, rc) == 0, "class_of_zero");
  report(skin_class(rc * rc * (1.0 - 1e-9), rc) == 0, "class_just_inside");
  {  // r0 = r_cmax: not inside a cutoff (the force loop tests r^2 < cutsq), class 0 or 1 are both right; walked as soon as anything moves
    const int c = skin_class(rc * rc, rc);
    report(c == 0 || c == 1, "class_at_r_cmax", c);
    report(c < skin_walk_classes(1e-8, rc), "r_cmax_walked_after_any_move", c);
  }
  report(skin_class(rc * rc * (1.0 + 1e-6), rc) == 1, "class_just_outside");
  for (int k = 2; k < K; k++) {
    const double b = skin_bound(rc, k);
    report(skin_class(b * b, rc) == k, "class_on_bound", k, skin_class(b * b, rc));
    report(skin_class(b * b * (1.0 - 1e-9), rc) == k - 1, "class_below_bound", k);
    // on the bound, moved by exactly the drift that reaches it: walked
    const double d = 0.5 * (b - rc);
    report(skin_walk_classes(d * d, rc) > k, "bound_reached_is_walked", k, skin_walk_classes(d * d, rc));
    // ... and short of it by a thousandth of a shell: not walked (the skip is not given away)
    const double e = d - 0.0005 * SKIN_SHELL;
    report(skin_walk_classes(e * e, rc) == k, "bound_not_reached_is_skipped", k, skin_walk_classes(e * e, rc));
  }
  report(skin_class(1e6, rc) == K - 1, "class_far");
  report(skin_walk_classes(std::nan(""), rc) == K && skin_walk_classes(1e308, rc) == K && skin_walk_classes(-1.0, rc) == K, "bad_drift_walks_all");
  return failures ? 1 : 0;
}
