// polar_nl_dense.hpp -- dense candidate trips of the list build (k_nl_build): "run table, stream position -> atom index".
//
// A row atom's wave visits the atoms of up to 25 stencil rows of cells, each one or two contiguous runs [ra0, rb0), [ra1, rb1)
// of atom indices (two when the row of cells wraps around the box).  Striding every run on its own in steps of 64 lanes
// rounds every run up to whole trips: on the 5x5x4 MOF-5 box a row has 24.7 runs with 1,764 candidates but takes 40.2 trips
// (2,573 lane slots).  Here the runs are laid end to end in one virtual candidate stream -- stencil rows in order, piece 0
// before piece 1, ascending index inside a piece: the visiting order of the per-run walk -- and lane l of trip t owns stream
// position g = 64 t + l: ceil(total / 64) trips, 28.1 on that box.
//
// The table: stencil row sr starts at stream position s0 = sum of the lengths before it; its piece 0 covers [s0, s1), its
// piece 1 [s1, end).  The atom at position g of piece 0 is g + k0 (k0 = ra0 - s0), of piece 1 g + k1 (k1 = ra1 - s1).
// Rows without an atom have end == s0 and are not walked at all (`rem`, the mask of rows not yet finished, holds only
// rows with atoms).
//
// Plain C++ on purpose: the device reads the table with v_readlane through an accessor, tests/test_nl_dense_host.py
// drives the same functions from arrays on the host.
#pragma once

#if defined(__HIPCC__)
#define POLAR_NLD_FN __host__ __device__ __forceinline__
#else
#define POLAR_NLD_FN inline
#endif

namespace polar {

struct NlRunEntry {
  int s0, k0, s1, k1, end;
};
// candidates of one stencil row (an empty or skipped piece has rb <= ra)
POLAR_NLD_FN int nl_run_len(int ra0, int rb0, int ra1, int rb1) {
  return (rb0 > ra0 ? rb0 - ra0 : 0) + (rb1 > ra1 ? rb1 - ra1 : 0);
}
// table entry of a stencil row whose first candidate sits at stream position `off` (the exclusive scan of nl_run_len)
POLAR_NLD_FN NlRunEntry nl_run_entry(int ra0, int rb0, int ra1, int rb1, int off) {
  NlRunEntry e;
  const int len0 = rb0 > ra0 ? rb0 - ra0 : 0, len1 = rb1 > ra1 ? rb1 - ra1 : 0;
  e.s0 = off; e.k0 = ra0 - off;
  e.s1 = off + len0; e.k1 = ra1 - e.s1;
  e.end = e.s1 + len1;
  return e;
}
// One trip: the candidates at stream positions [t0, t0 + 64), position g = t0 + lane in this lane.  Returns k with
// "atom index = g + k" for every g below the stream's total (lanes at or beyond it are idle: the caller masks them).
// `rem` = bit sr set: stencil row sr holds atoms and has not been walked to its end; wave-uniform, as is everything here
// except g and the result.  Its lowest bit is always the row that holds position t0 (rows with atoms lie back to back in
// the stream), so the walk starts there and stops at the first row that reaches into the next trip: the rows are visited
// in order and a later row's start overrides an earlier one for the lanes at or beyond it.
// Tab: s0(sr), k0(sr), s1(sr), k1(sr), end(sr), two(sr) ("row sr has a piece 1").
template <class Tab>
POLAR_NLD_FN int nl_dense_shift(const Tab &tab, unsigned &rem, int t0, int g) {
  int k = 0;
  while (rem) {
    const int sr = __builtin_ctz(rem);
    const int s0 = tab.s0(sr), k0 = tab.k0(sr);  // (read before the select: a table read is wave-wide)
    k = g >= s0 ? k0 : k;
    if (tab.two(sr)) {
      const int s1 = tab.s1(sr), k1 = tab.k1(sr);
      k = g >= s1 ? k1 : k;
    }
    if (tab.end(sr) > t0 + 64) break;  // this row goes on in the next trip
    rem &= rem - 1;
  }
  return k;
}

}  // namespace polar
