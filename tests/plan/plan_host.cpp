// Host driver of the step-planning functions (csrc/polar_plan.hpp) for tests/test_plan_host.py.
// stdin: one command per line, numbers separated by blanks; stdout: one answer per command (doubles with 17 digits).
//   widths  lx ly lz xy xz yz triclinic          -> w0 w1 w2
//   short   w0 w1 w2 cut_coul                    -> 0 | 1
//   grid    w0 w1 w2 p0 p1 p2 cutall             -> "narrow" | nc0 nc1 nc2
//   first   factor count mean...                 -> pitch...
//   grown   count flag...                        -> pitch...
//   forced  count value...                       -> pitch...
//   occ     cutall lo[3] prd[3] n x[3n]          -> volume
//   stream  cache_r2 sweep_kernel dd_pairs own_rows dd_pitch -> mode
//   kvec    lx ly lz xy xz yz g accuracy         -> "nk nrow nm", the six entries of H^-1, then nk lines "h k l kx ky kz c_k"
//                                                   and nrow + 1 lines "h k l0 first"
//   tile    nm                                   -> lds_per_atom tile
//   chunks  n nk tile                            -> kb nchunk chunk
//   gs      n                                    -> fits B
//   sweepend sw max_sweeps fixed gs accel reduce_every -> mix decide_in_mix count reduce jacobi
//   look    last_sweeps sw every step            -> 0 | 1
#include <cstdio>
#include <cstring>
#include <vector>

#include "polar_plan.hpp"

namespace {
struct HostBox {
  double prd[3], xy, xz, yz;
  int periodic[3], triclinic;
};
bool rd(double &v) { return scanf("%lf", &v) == 1; }
bool rd(int &v) { return scanf("%d", &v) == 1; }
bool rd(long long &v) { return scanf("%lld", &v) == 1; }
bool read_box(HostBox &b) {
  b.periodic[0] = b.periodic[1] = b.periodic[2] = 1;
  return rd(b.prd[0]) && rd(b.prd[1]) && rd(b.prd[2]) && rd(b.xy) && rd(b.xz) && rd(b.yz);
}
}  // namespace

int main() {
  char cmd[32];
  while (scanf("%31s", cmd) == 1) {
    if (!strcmp(cmd, "widths")) {
      HostBox b;
      double w[3];
      if (!read_box(b) || !rd(b.triclinic)) return 2;
      polar::box_widths(b, w);
      printf("%.17g %.17g %.17g\n", w[0], w[1], w[2]);
    } else if (!strcmp(cmd, "short")) {
      double w[3], cut;
      if (!rd(w[0]) || !rd(w[1]) || !rd(w[2]) || !rd(cut)) return 2;
      printf("%d\n", polar::ewald_short_box(w, cut) ? 1 : 0);
    } else if (!strcmp(cmd, "grid")) {
      double w[3], cutall;
      int per[3], nc[3];
      if (!rd(w[0]) || !rd(w[1]) || !rd(w[2]) || !rd(per[0]) || !rd(per[1]) || !rd(per[2]) || !rd(cutall)) return 2;
      if (polar::list_grid(w, per, cutall, nc)) printf("%d %d %d\n", nc[0], nc[1], nc[2]);
      else printf("narrow\n");
    } else if (!strcmp(cmd, "first")) {
      double factor, mean;
      int count;
      if (!rd(factor) || !rd(count)) return 2;
      for (int k = 0; k < count; k++) { if (!rd(mean)) return 2; printf("%lld\n", polar::pitch_first(mean, factor)); }
    } else if (!strcmp(cmd, "grown") || !strcmp(cmd, "forced")) {
      int count, v;
      if (!rd(count)) return 2;
      for (int k = 0; k < count; k++) {
        if (!rd(v)) return 2;
        if (cmd[0] == 'g') printf("%lld\n", polar::pitch_grown(v)); else printf("%d\n", polar::pitch_forced(v));
      }
    } else if (!strcmp(cmd, "occ")) {
      double cutall, lo[3], prd[3];
      int n;
      if (!rd(cutall) || !rd(lo[0]) || !rd(lo[1]) || !rd(lo[2]) || !rd(prd[0]) || !rd(prd[1]) || !rd(prd[2]) || !rd(n) || n < 0) return 2;
      std::vector<double> x(3 * (size_t)n);
      for (double &v : x) if (!rd(v)) return 2;
      printf("%.17g\n", polar::occupied_volume(n, x.data(), lo, prd, cutall));
    } else if (!strcmp(cmd, "stream")) {
      int cache_r2, sweep_kernel, own;
      long long pairs, pitch;
      if (!rd(cache_r2) || !rd(sweep_kernel) || !rd(pairs) || !rd(own) || !rd(pitch)) return 2;
      printf("%d\n", polar::stream_mode(cache_r2, sweep_kernel, pairs, own, pitch));
    } else if (!strcmp(cmd, "kvec")) {
      HostBox b;
      double g, acc;
      if (!read_box(b) || !rd(g) || !rd(acc)) return 2;
      b.triclinic = (b.xy != 0.0 || b.xz != 0.0 || b.yz != 0.0) ? 1 : 0;
      const polar::EwaldPlan p = polar::ewald_kvectors(b, g, acc);
      if (p.kv.size() != (size_t)p.nk || p.hkl.size() != (size_t)p.nk || p.rows.size() != (size_t)p.nrow + 1) return 3;
      printf("%d %d %d\n", p.nk, p.nrow, p.nm);
      printf("%.17g %.17g %.17g %.17g %.17g %.17g\n", p.cell[0], p.cell[1], p.cell[2], p.cell[3], p.cell[4], p.cell[5]);
      for (int k = 0; k < p.nk; k++)
        printf("%d %d %d %.17g %.17g %.17g %.17g\n", p.hkl[k].x, p.hkl[k].y, p.hkl[k].z, p.kv[k].x, p.kv[k].y, p.kv[k].z, p.kv[k].w);
      for (const polar::PlanI4 &r : p.rows) printf("%d %d %d %d\n", r.x, r.y, r.z, r.w);
    } else if (!strcmp(cmd, "tile")) {
      int nm;
      if (!rd(nm)) return 2;
      printf("%zu %d\n", polar::ewald_lds_per_atom(nm), polar::ewald_tile(nm));
    } else if (!strcmp(cmd, "chunks")) {
      int n, nk, tile;
      if (!rd(n) || !rd(nk) || !rd(tile)) return 2;
      const polar::SfacChunks c = polar::ewald_sfac_chunks(n, nk, tile);
      printf("%d %d %d\n", c.kb, c.nchunk, c.chunk);
    } else if (!strcmp(cmd, "gs")) {
      int n;
      if (!rd(n)) return 2;
      printf("%d %d\n", polar::dense_gs_fits(n) ? 1 : 0, polar::dense_gs_block(n));
    } else if (!strcmp(cmd, "sweepend")) {
      int sw, max_sweeps, fixed, gs, accel, reduce_every;
      if (!rd(sw) || !rd(max_sweeps) || !rd(fixed) || !rd(gs) || !rd(accel) || !rd(reduce_every)) return 2;
      const polar::SweepEnd e = polar::sweep_end(sw, max_sweeps, fixed != 0, gs != 0, accel != 0, reduce_every);
      printf("%d %d %d %d %d\n", e.mix ? 1 : 0, e.decide_in_mix ? 1 : 0, e.count, e.reduce ? 1 : 0, e.jacobi ? 1 : 0);
    } else if (!strcmp(cmd, "look")) {
      int last_sweeps, sw, every, step;
      if (!rd(last_sweeps) || !rd(sw) || !rd(every) || !rd(step)) return 2;
      printf("%d\n", polar::look_at_state(last_sweeps, sw, every, step) ? 1 : 0);
    } else {
      fprintf(stderr, "unknown command %s\n", cmd);
      return 2;
    }
  }
  return 0;
}
