// cell_order_host.cpp -- the bin rule and the sizes of the cell order (csrc/polar_plan.hpp: cell_bin, cell_bins,
// cell_bins_fit) on the host, and the counting sort of build_cells played through with them.
//
// Commands on stdin, one per line; answers on stdout, one line each:
//   bin   c ncell inert split            -> the bin
//   sizes ncell split                    -> nbins cnt fill fill_back first fits
//   order ncell split pol_first n        then n lines "cell q alpha"
//                                        -> line 1: perm[0 .. n-1] (s order: the caller's index of the atom at place s)
//                                           line 2: cell_first[0 .. nbins]
//                                           line 3: npol[0 .. nbins-1] (the front counters; all zero without pol_first)
// `order` follows the launches of build_cells step by step -- count, exclusive scan, fill from the front (polarizable) and
// from the back (the others), each group of a bin into ascending atom index -- in tables that have EXACTLY the sizes
// cell_bins hands out, so that a size that is one short is a heap overflow under the address sanitizer.  The site rule is
// the one of site_is_inert (csrc/polar_common.hpp, which needs the HIP headers): q == 0 and alpha == 0.
#include <algorithm>
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "polar_plan.hpp"

using namespace polar;

static bool inert_site(double q, double alpha) { return q == 0.0 && alpha == 0.0; }

int main() {
  std::string cmd;
  while (std::cin >> cmd) {
    if (cmd == "bin") {
      long long c, ncell; int inert, split;
      std::cin >> c >> ncell >> inert >> split;
      std::printf("%lld\n", cell_bin(c, ncell, inert != 0, split != 0));
    } else if (cmd == "sizes") {
      long long ncell; int split;
      std::cin >> ncell >> split;
      const CellBins cb = cell_bins(ncell, split != 0);
      std::printf("%lld %lld %lld %lld %lld %d\n", cb.nbins, cb.cnt, cb.fill, cb.fill_back, cb.first, cell_bins_fit(ncell, split != 0) ? 1 : 0);
    } else if (cmd == "order") {
      long long ncell; int split, pol_first, n;
      std::cin >> ncell >> split >> pol_first >> n;
      std::vector<long long> cell((size_t)n);
      std::vector<double> q((size_t)n), alpha((size_t)n);
      for (int i = 0; i < n; i++) std::cin >> cell[(size_t)i] >> q[(size_t)i] >> alpha[(size_t)i];
      const CellBins cb = cell_bins(ncell, split != 0);
      std::vector<int> cnt((size_t)cb.cnt, 0), fill((size_t)cb.fill, 0), id((size_t)n), perm((size_t)n, -1);
      std::vector<long long> first((size_t)cb.first, 0);
      for (int i = 0; i < n; i++) {   // k_cell_count
        const long long b = cell_bin(cell[(size_t)i], ncell, inert_site(q[(size_t)i], alpha[(size_t)i]), split != 0);
        id[(size_t)i] = (int)b;
        cnt.at((size_t)b)++;
      }
      for (long long b = 0; b < cb.nbins; b++) first[(size_t)b + 1] = first[(size_t)b] + cnt[(size_t)b];   // launch_scan: nbins + 1 written
      int *front = fill.data(), *back = pol_first ? fill.data() + cb.fill_back : nullptr;
      for (int i = n - 1; i >= 0; i--) {   // k_cell_fill, in an arrival order that is not the atom order
        const int b = id[(size_t)i];
        long long s;
        if (!back || alpha[(size_t)i] != 0.0) s = first[(size_t)b] + front[b]++;
        else s = first[(size_t)b + 1] - 1 - back[b]++;
        perm.at((size_t)s) = i;
      }
      for (long long b = 0; b < cb.nbins; b++) {   // k_cell_sort
        const long long a = first[(size_t)b], e = first[(size_t)b + 1], m = pol_first ? a + front[b] : e;
        std::sort(perm.begin() + a, perm.begin() + m);
        std::sort(perm.begin() + m, perm.begin() + e);
      }
      for (int s = 0; s < n; s++) std::printf("%d ", perm[(size_t)s]);
      std::printf("\n");
      for (long long b = 0; b <= cb.nbins; b++) std::printf("%lld ", first[(size_t)b]);
      std::printf("\n");
      for (long long b = 0; b < cb.nbins; b++) std::printf("%d ", pol_first ? front[b] : 0);
      std::printf("\n");
    } else {
      std::fprintf(stderr, "unknown command %s\n", cmd.c_str());
      return 2;
    }
  }
  return 0;
}
