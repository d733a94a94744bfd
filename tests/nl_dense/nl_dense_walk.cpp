// Host driver of the list build's dense-trip enumeration (csrc/polar_nl_dense.hpp) for tests/test_nl_dense_host.py.
// stdin: the number of run tables, then per table the number of stencil rows and "ra0 rb0 ra1 rb1" per row.
// stdout, per table: "total trips" and then the atom index of every (trip, lane) in order, -1 for an idle lane.
// The wave is emulated the way k_nl_build runs it: an exclusive scan of the row lengths, the mask of rows with atoms, and
// per trip one call of nl_dense_shift per lane, all lanes starting from the same mask and leaving with the same mask.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "polar_nl_dense.hpp"

namespace {
struct HostTab {
  std::vector<polar::NlRunEntry> e;
  unsigned m1 = 0;
  int s0(int sr) const { return e.at(sr).s0; }
  int k0(int sr) const { return e.at(sr).k0; }
  int s1(int sr) const { return e.at(sr).s1; }
  int k1(int sr) const { return e.at(sr).k1; }
  int end(int sr) const { return e.at(sr).end; }
  bool two(int sr) const { return (m1 >> sr) & 1u; }
};
}  // namespace

int main() {
  int ntab = 0;
  if (scanf("%d", &ntab) != 1) return 2;
  for (int t = 0; t < ntab; t++) {
    int nsr = 0;
    if (scanf("%d", &nsr) != 1 || nsr < 0 || nsr > 32) return 2;
    HostTab tab;
    unsigned rem = 0;
    int off = 0;
    for (int sr = 0; sr < nsr; sr++) {
      int ra0, rb0, ra1, rb1;
      if (scanf("%d %d %d %d", &ra0, &rb0, &ra1, &rb1) != 4) return 2;
      const int len = polar::nl_run_len(ra0, rb0, ra1, rb1);
      tab.e.push_back(polar::nl_run_entry(ra0, rb0, ra1, rb1, off));
      if (rb1 > ra1) tab.m1 |= 1u << sr;
      if (len > 0) rem |= 1u << sr;
      off += len;
    }
    const int total = off;
    printf("%d %d\n", total, (total + 63) / 64);
    for (int t0 = 0; t0 < total; t0 += 64) {
      unsigned after = 0;
      for (int lane = 0; lane < 64; lane++) {
        unsigned r = rem;
        const int g = t0 + lane;
        const int k = polar::nl_dense_shift(tab, r, t0, g);
        if (lane == 0) after = r;
        else if (r != after) { fprintf(stderr, "table %d trip %d: the row mask is not wave-uniform\n", t, t0 / 64); return 3; }
        printf("%d%c", g < total ? g + k : -1, lane == 63 ? '\n' : ' ');
      }
      rem = after;
    }
    if (rem != 0) { fprintf(stderr, "table %d: rows left unwalked after the last trip\n", t); return 3; }
  }
  return 0;
}
