// Host driver of the input functions (csrc/polar_input.hpp) for tests/test_input_host.py.
// stdin: one command per line, numbers separated by blanks (nan, inf and -inf as words); stdout: one answer per command
// (doubles with 17 digits).  SETTINGS = the 21 fields of polar_settings in the order of the struct.
//   scan     n a0 a1 lo[3] hi[3] x[3n]       -> finite lo[3] hi[3] exact   (exact: dst holds src on [a0, a1), byte for byte, and
//                                               what it held before everywhere else)
//   arith    nbits mask shift r[nt] dr[nt]   -> ok lowmask i_special[2] dr_special[2]   (nt = 2^nbits; one entry each for nbits 0)
//   packlj   ntypes, 7 tables of (ntypes+1)^2 (lj1 lj2 lj3 lj4 offset cut_ljsq cutsq)  -> r_cmax, then the packed doubles
//   packcoul nbits, 8 tables of nt (r dr f df c dc e de)                                -> the packed doubles
//   grid     lo[3] hi[3] cutmax              -> nc[3] lo[3] inv[3] ncell
//   pitch    lo[3] hi[3] cutmax2 nall        -> pitch
//   solver   zodid polar_gs polar_gs_ranked  -> "ok" | "error <text>"
//   pack     max_bytes SETTINGS              -> return value, then the bytes written as hex (max_bytes < 0: a null buffer)
//   unpack   SETTINGS nbytes hex             -> "ok" SETTINGS | "error <text>"
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "polar_input.hpp"

namespace {
bool rd(double &v) { return scanf("%lf", &v) == 1; }
bool rd(int &v) { return scanf("%d", &v) == 1; }
bool rd(long long &v) { return scanf("%lld", &v) == 1; }
bool rd3(double v[3]) { return rd(v[0]) && rd(v[1]) && rd(v[2]); }
bool rdv(std::vector<double> &v) { for (double &x : v) if (!rd(x)) return false; return true; }
bool read_settings(polar_settings &s) {
  return rd(s.cut_lj_global) && rd(s.cut_coul) && rd(s.polar_precision) && rd(s.polar_damp) && rd(s.polar_gamma) &&
         rd(s.iterations_max) && rd(s.damping_type) && rd(s.zodid) && rd(s.fixed_iteration) && rd(s.polar_gs) &&
         rd(s.polar_gs_ranked) && rd(s.use_previous) && rd(s.debug) && rd(s.dd_cutoff) && rd(s.device_neigh) &&
         rd(s.restart_polar) && rd(s.deterministic) && rd(s.polar_sor) && rd(s.rccl_halo) && rd(s.polar_accel) && rd(s.polar_ewald);
}
void print_settings(const polar_settings &s) {
  printf("%.17g %.17g %.17g %.17g %.17g %d %d %d %d %d %d %d %d %.17g %d %d %d %.17g %d %d %.17g\n", s.cut_lj_global, s.cut_coul,
         s.polar_precision, s.polar_damp, s.polar_gamma, s.iterations_max, s.damping_type, s.zodid, s.fixed_iteration, s.polar_gs,
         s.polar_gs_ranked, s.use_previous, s.debug, s.dd_cutoff, s.device_neigh, s.restart_polar, s.deterministic, s.polar_sor,
         s.rccl_halo, s.polar_accel, s.polar_ewald);
}
void print_doubles(const std::vector<double> &v) {
  for (size_t k = 0; k < v.size(); k++) printf("%.17g%c", v[k], k + 1 == v.size() ? '\n' : ' ');
}
}  // namespace

int main() {
  char cmd[32];
  while (scanf("%31s", cmd) == 1) {
    if (!strcmp(cmd, "scan")) {
      long long n, a0, a1;
      double lo[3], hi[3];
      if (!rd(n) || !rd(a0) || !rd(a1) || !rd3(lo) || !rd3(hi) || n < 0 || a0 < 0 || a1 < a0 || a1 > n) return 2;
      std::vector<double> x(3 * (size_t)n), dst(3 * (size_t)n, -7.25);
      if (!rdv(x)) return 2;
      const bool finite = polar::scan_positions(x.data(), dst.data(), (size_t)a0, (size_t)a1, lo, hi);
      bool exact = true;
      for (long long k = 0; k < 3 * n; k++) {
        const double want = (k >= 3 * a0 && k < 3 * a1) ? x[(size_t)k] : -7.25;
        exact = exact && memcmp(&dst[(size_t)k], &want, sizeof(double)) == 0;
      }
      printf("%d %.17g %.17g %.17g %.17g %.17g %.17g %d\n", finite ? 1 : 0, lo[0], lo[1], lo[2], hi[0], hi[1], hi[2], exact ? 1 : 0);
    } else if (!strcmp(cmd, "arith")) {
      int nbits, mask, shift;
      if (!rd(nbits) || !rd(mask) || !rd(shift) || nbits < 0 || nbits > 20) return 2;
      const size_t nt = nbits ? (size_t)1 << nbits : 1;
      std::vector<double> r(nt), dr(nt);
      if (!rdv(r) || !rdv(dr)) return 2;
      const polar::CoulTableArith a = polar::coul_table_arith(nbits, mask, shift, r.data(), dr.data());
      printf("%d %d %d %d %.17g %.17g\n", a.ok ? 1 : 0, a.lowmask, a.i_special[0], a.i_special[1], a.dr_special[0], a.dr_special[1]);
    } else if (!strcmp(cmd, "packlj") || !strcmp(cmd, "packcoul")) {
      const bool lj = cmd[4] == 'l';
      int arg;
      if (!rd(arg) || arg < 0 || arg > 20) return 2;
      const size_t len = lj ? (size_t)(arg + 1) * (arg + 1) : (arg ? (size_t)1 << arg : 1);
      std::vector<std::vector<double>> tabs(lj ? 7 : 8, std::vector<double>(len));
      const double *t[8] = {};
      for (size_t k = 0; k < tabs.size(); k++) { if (!rdv(tabs[k])) return 2; t[k] = tabs[k].data(); }
      std::vector<double> pack;
      if (lj) printf("%.17g\n", polar::pack_lj_table(arg, t, pack));
      else polar::pack_coul_table(arg, t, pack);
      print_doubles(pack);
    } else if (!strcmp(cmd, "grid")) {
      double lo[3], hi[3], cutmax;
      if (!rd3(lo) || !rd3(hi) || !rd(cutmax)) return 2;
      struct { int nc[3]; double lo[3], inv[3]; } g;
      const long long ncell = polar::lj_grid(lo, hi, cutmax, g);
      printf("%d %d %d %.17g %.17g %.17g %.17g %.17g %.17g %lld\n", g.nc[0], g.nc[1], g.nc[2], g.lo[0], g.lo[1], g.lo[2], g.inv[0],
             g.inv[1], g.inv[2], ncell);
    } else if (!strcmp(cmd, "pitch")) {
      double lo[3], hi[3], cutmax2;
      long long nall;
      if (!rd3(lo) || !rd3(hi) || !rd(cutmax2) || !rd(nall)) return 2;
      printf("%lld\n", polar::lj_first_pitch(lo, hi, cutmax2, nall));
    } else if (!strcmp(cmd, "solver")) {
      polar_settings s{};
      if (!rd(s.zodid) || !rd(s.polar_gs) || !rd(s.polar_gs_ranked)) return 2;
      try { polar::check_solver_choice(s); printf("ok\n"); } catch (const polar::InputError &e) { printf("error %s\n", e.what()); }
    } else if (!strcmp(cmd, "pack")) {
      int max_bytes;
      polar_settings s{};
      if (!rd(max_bytes) || !read_settings(s)) return 2;
      std::vector<unsigned char> buf(max_bytes > 0 ? (size_t)max_bytes : 1);   // (as long as it says: a write past it is the sanitizer's)
      const int rc = polar::restart_pack(s, max_bytes < 0 ? nullptr : buf.data(), max_bytes);
      printf("%d", rc);
      if (max_bytes >= 0 && rc > 0) { printf(" "); for (int k = 0; k < rc; k++) printf("%02x", buf[(size_t)k]); }
      printf("\n");
    } else if (!strcmp(cmd, "unpack")) {
      polar_settings now{};
      int nbytes;
      char hex[1024];
      if (!read_settings(now) || !rd(nbytes) || scanf("%1023s", hex) != 1 || nbytes < 0) return 2;
      std::vector<unsigned char> buf;
      if (strcmp(hex, "-") != 0)
        for (size_t k = 0; k + 1 < strlen(hex); k += 2) { unsigned v; if (sscanf(hex + k, "%2x", &v) != 1) return 2; buf.push_back((unsigned char)v); }
      if ((size_t)nbytes > buf.size()) return 2;   // (the record may say it is shorter than the buffer, never longer)
      std::vector<unsigned char> exact(buf.begin(), buf.begin() + nbytes);
      try {
        const polar_settings s = polar::restart_unpack(now, exact.empty() ? nullptr : exact.data(), nbytes);
        printf("ok ");
        print_settings(s);
      } catch (const polar::InputError &e) { printf("error %s\n", e.what()); }
    } else {
      fprintf(stderr, "unknown command %s\n", cmd);
      return 2;
    }
  }
  return 0;
}
