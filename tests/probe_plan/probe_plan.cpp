// csrc/polar_probe_plan.hpp on the host.
//
// As a shared library (tests/test_probe_plan_host.py): the trimmed stencil of a batch of points, the perpendicular widths and
// the list grid of a box, the reach table, and the refusals as status codes with their messages.
// With -DPROBE_PLAN_MAIN a stand-alone program (the sanitizer build): random axes through probe_axis, stencil_axis and
// seam_part with their invariants checked, and every refusal once.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "polar_probe_plan.hpp"

namespace {
struct HostBox { double prd[3], xy, xz, yz; int triclinic; };
std::string g_msg;
template <class F>
int status_of(F f) {
  g_msg.clear();
  try { f(); }
  catch (const polar::InputError &e) { g_msg = e.what(); return POLAR_ERR_INPUT; }
  catch (const polar::Unsupported &e) { g_msg = e.what(); return POLAR_ERR_UNSUPPORTED; }
  return POLAR_OK;
}
}  // namespace

extern "C" {
const char *plan_last_message() { return g_msg.c_str(); }

// perpendicular widths, and the list grid of cutall (returns 0 when the box is too narrow for list mode)
int plan_box(const double prd[3], const double tilt[3], int triclinic, const int periodic[3], double cutall, double width[3], int nc[3]) {
  const HostBox b{{prd[0], prd[1], prd[2]}, tilt[0], tilt[1], tilt[2], triclinic};
  polar::box_widths(b, width);
  return polar::list_grid(width, periodic, cutall, nc) ? 1 : 0;
}

// the cells of n points: s [n][3] fractional coordinates, first / count [n][3]
void plan_stencil(int n, const double *s, double reach, const double width[3], const int nc[3], int *first, int *count) {
  double scale[3];
  polar::probe_dfrac_scale(width, scale);
  for (int p = 0; p < n; p++)
    for (int k = 0; k < 3; k++) {
      const polar::ProbeAxis a = polar::probe_axis(s[3 * p + k], reach * scale[k], nc[k]);
      first[3 * p + k] = a.first; count[3 * p + k] = a.count;
    }
}

// the +-2 rule of centre cell c on an axis of nc cells, and its split at the periodic seam: axis = {first, count}, runs =
// {first, count} of part 0 and of part 1
void plan_stencil_axis(int c, int nc, int axis[2], int runs[4]) {
  const polar::ProbeAxis a = polar::stencil_axis(c, nc);
  axis[0] = a.first; axis[1] = a.count;
  for (int part = 0; part < 2; part++) {
    const polar::ProbeAxis r = polar::seam_part(a, nc, part);
    runs[2 * part] = r.first; runs[2 * part + 1] = r.count;
  }
}

// pack: (ntypes + 1)^2 entries of 8 doubles (pack_lj_table's layout); reach: ntypes + 1 doubles out
double plan_reach(int ntypes, const double *pack, double *reach) {
  std::vector<double> r;
  const double m = polar::probe_reach(ntypes, pack, r);
  for (int t = 0; t <= ntypes; t++) reach[t] = r[t];
  return m;
}

int plan_check_sites(long long n, const int *type, int ntypes, const double *q, const double *alpha, int want_lj) {
  return status_of([&]() { polar::check_probe_sites(n, type, ntypes, q, alpha, want_lj != 0); });
}

int plan_check_reach(int list_mode, double reach_max, double cut_coul, double dd_cutoff, const double width[3], const int periodic[3]) {
  return status_of([&]() { polar::check_probe_reach(list_mode != 0, reach_max, cut_coul, dd_cutoff, width, periodic); });
}
}

#ifdef PROBE_PLAN_MAIN
namespace {
struct Rng {
  uint64_t s;
  double uni() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)(s >> 11) * (1.0 / 9007199254740992.0); }
};
}  // namespace

int main(int argc, char **argv) {
  const int n = argc > 1 ? atoi(argv[1]) : 20000;
  Rng g{0x9E3779B97F4A7C15ull};
  long long checks = 0, failures = 0;
  for (int k = 0; k < n; k++) {
    const int nc = 1 + (int)(12.0 * g.uni());
    const double s = g.uni() < 0.1 ? (g.uni() < 0.5 ? 0.0 : 1.0) : -0.01 + 1.02 * g.uni(), dfrac = 0.6 * g.uni();   // (up to the whole axis and beyond)
    const polar::ProbeAxis a = polar::probe_axis(s, dfrac, nc);
    checks++;
    bool ok = a.first >= 0 && a.first < nc && a.count >= 1 && a.count <= nc;
    // the cells of s - dfrac, s and s + dfrac are among those walked
    const double reach_cells = dfrac * nc < 2.0 ? dfrac : 2.0 / nc;   // (never further than two cells from the point's own)
    for (double v : {s - reach_cells * (1.0 - 1e-12), s, s + reach_cells * (1.0 - 1e-12)}) {
      long long c = (long long)std::floor(v * nc) % nc;
      c += c < 0 ? nc : 0;
      const long long rel = ((c - a.first) % nc + nc) % nc;
      ok = ok && rel < a.count;
    }
    if (!ok) failures++;
    // ... and the +-2 rule of a cell of the same axis with its seam split: the runs lie on the axis and add up to the count
    int axis[2], runs[4];
    plan_stencil_axis((int)(nc * g.uni()), nc, axis, runs);
    checks++;
    if (!(axis[0] >= 0 && axis[1] == (nc < 5 ? nc : 5) && runs[0] == axis[0] && runs[1] >= 1 && runs[0] + runs[1] <= nc && runs[2] == 0 &&
          runs[3] >= 0 && runs[1] + runs[3] == axis[1]))
      failures++;
  }
  // the refusals, each once, and what is accepted beside them
  const int ty_ok[3] = {1, 2, 2}, ty_lo[3] = {1, 0, 2}, ty_hi[3] = {1, 3, 2};
  const double q_ok[3] = {0.1, -0.2, 0.0}, a_ok[3] = {0.0, 0.5, 1.0}, q_nan[3] = {0.1, NAN, 0.0}, a_neg[3] = {0.5, -1e-300, 0.0}, a_inf[3] = {0.5, INFINITY, 0.0};
  const int want[][2] = {{plan_check_sites(3, ty_ok, 2, q_ok, a_ok, 1), POLAR_OK}, {plan_check_sites(3, ty_lo, 2, nullptr, nullptr, 1), POLAR_ERR_INPUT},
                         {plan_check_sites(3, ty_hi, 2, nullptr, nullptr, 0), POLAR_ERR_INPUT}, {plan_check_sites(3, nullptr, 2, nullptr, nullptr, 1), POLAR_ERR_INPUT},
                         {plan_check_sites(3, nullptr, 2, q_ok, nullptr, 0), POLAR_OK}, {plan_check_sites(3, ty_ok, 2, q_nan, nullptr, 1), POLAR_ERR_INPUT},
                         {plan_check_sites(3, ty_ok, 2, nullptr, a_neg, 1), POLAR_ERR_INPUT}, {plan_check_sites(3, ty_ok, 2, nullptr, a_inf, 1), POLAR_ERR_INPUT}};
  for (const auto &w : want) { checks++; if (w[0] != w[1]) failures++; }
  const double width[3] = {20.0, 16.0, 12.0};
  const int per[3] = {1, 1, 1}, per2[3] = {1, 1, 0};
  const int want2[][2] = {{plan_check_reach(1, 9.0, 9.0, 8.0, width, per), POLAR_OK}, {plan_check_reach(1, 9.0 + 1e-9, 9.0, 8.0, width, per), POLAR_ERR_UNSUPPORTED},
                          {plan_check_reach(0, 6.0, 9.0, 0.0, width, per), POLAR_OK}, {plan_check_reach(0, 6.0 + 1e-9, 9.0, 0.0, width, per), POLAR_ERR_UNSUPPORTED},
                          {plan_check_reach(0, 7.0, 9.0, 0.0, width, per2), POLAR_OK}};
  for (const auto &w : want2) { checks++; if (w[0] != w[1]) failures++; }
  std::vector<double> pack(8 * 9, 0.0), reach(3);
  pack[8 * 4 + 1] = 25.0; pack[8 * 5 + 1] = 16.0; pack[8 * 7 + 1] = 16.0; pack[8 * 8 + 1] = 36.0;
  checks++;
  if (!(plan_reach(2, pack.data(), reach.data()) == 6.0 && reach[0] == 0.0 && reach[1] == 5.0 && reach[2] == 6.0)) failures++;
  printf("inputs %d checks %lld failures %lld\n", n, checks, failures);
  return failures == 0 ? 0 : 1;
}
#endif
