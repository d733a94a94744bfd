// polar_input.hpp -- what the entry points of polar_api.hip decide about the data a caller hands in: the scan of the
// positions, the repacking and the analysis of the pair tables, the grid of polar_build_neighbors, the solver rule of the
// settings, the restart record.
//
// Pure functions, plain C++17, in the manner of polar_plan.hpp: no HIP header, no handle, nothing read from the environment.
// The entry points keep the HIP calls and the handle's bookkeeping; tests/test_input_host.py drives the same functions on
// the host through tests/input/input_host.cpp.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <vector>

#include "pair_host.hpp"
#include "polar_plan.hpp"

namespace polar {

// ---- positions ----------------------------------------------------------------------------------------------------------
// One pass over the atoms [a0, a1) of src ([n][3]): the copy into dst, the bounding box folded into lo / hi (which keep what
// they already hold), and the answer whether every coordinate is finite (non-finite coordinates must not reach a cell build).
// Four atoms = twelve doubles at a time: twelve independent running minima / maxima (the compiler keeps them in vector
// registers; one accumulator per coordinate, fed with a stride of three, ran at a fifth of the copy's rate)
inline bool scan_positions(const double *src, double *dst, size_t a0, size_t a1, double lo3[3], double hi3[3]) {
  if (a1 > a0) memcpy(dst + 3 * a0, src + 3 * a0, 3 * (a1 - a0) * sizeof(double));
  double lo[12], hi[12], acc = 0.0;
  for (int j = 0; j < 12; j++) { lo[j] = 1e300; hi[j] = -1e300; }
  size_t a = a0;
  for (; a + 4 <= a1; a += 4) {
    const double *p = src + 3 * a;
    for (int j = 0; j < 12; j++) { const double v = p[j]; lo[j] = v < lo[j] ? v : lo[j]; hi[j] = v > hi[j] ? v : hi[j]; acc += v - v; }
  }
  for (; a < a1; a++)
    for (int k = 0; k < 3; k++) { const double v = src[3 * a + k]; lo[k] = v < lo[k] ? v : lo[k]; hi[k] = v > hi[k] ? v : hi[k]; acc += v - v; }
  for (int j = 0; j < 12; j++) { lo3[j % 3] = std::min(lo3[j % 3], lo[j]); hi3[j % 3] = std::max(hi3[j % 3], hi[j]); }
  return acc == 0.0;   // (v - v is 0 for a finite v, NaN for an infinite or NaN one)
}

// ---- polar_field_at ---------------------------------------------------------------------------------------------------------
// The points of a call: every coordinate finite, no point further than POLAR_FIELD_AT_MAX_IMAGES box lengths from the box along
// a periodic direction (fractional coordinates as Domain::x2lamda forms them; tilt = {xy, xz, yz} or null), every skip_atom
// (may be null) -1 or an atom of the handle.  The kernel takes whole lattice vectors off a point once, in closed form, before
// any image rule sees it: inside the limit what is left lies in the box to 2^-22 of a box length, so the add / subtract loops of
// closest_image (exact mode) run as they do for an atom.  Beyond it a coordinate has too few digits left to say where in the box
// the point is -- a grid made from a wrong box, garbage -- and is refused instead of mapped somewhere.
#define POLAR_FIELD_AT_MAX_IMAGES 1073741824.0   // 2^30
inline void check_points(long long npoints, const double *x, const int *skip_atom, int nlocal, const double lo[3], const double prd[3],
                         const double *tilt, const int periodic[3]) {
  double acc = 0.0;
  for (long long k = 0; k < 3 * npoints; k++) acc += x[k] - x[k];
  if (!(acc == 0.0)) throw InputError("polar_field_at: non-finite coordinate");
  const double xy = tilt ? tilt[0] : 0.0, xz = tilt ? tilt[1] : 0.0, yz = tilt ? tilt[2] : 0.0;
  for (long long p = 0; p < npoints; p++) {
    const double f2 = (x[3 * p + 2] - lo[2]) / prd[2];
    const double f1 = ((x[3 * p + 1] - lo[1]) - yz * f2) / prd[1];
    const double f0 = ((x[3 * p] - lo[0]) - xy * f1 - xz * f2) / prd[0];
    const bool far = (periodic[2] && std::fabs(f2) > POLAR_FIELD_AT_MAX_IMAGES) || (periodic[1] && std::fabs(f1) > POLAR_FIELD_AT_MAX_IMAGES) ||
                     (periodic[0] && std::fabs(f0) > POLAR_FIELD_AT_MAX_IMAGES);
    if (far || !std::isfinite(f0) || !std::isfinite(f1) || !std::isfinite(f2))
      throw InputError("polar_field_at: point further than 2^30 box lengths from the box");
  }
  if (skip_atom)
    for (long long p = 0; p < npoints; p++)
      if (skip_atom[p] < -1 || skip_atom[p] >= nlocal) throw InputError("polar_field_at: skip_atom outside [-1, nlocal)");
}
// Points per pass from POLAR_FIELD_AT_CHUNK (0 or negative: not set or nonsense -> the default 2^20); at most 2^24, so that a
// pass's buffers (100 bytes per point) stay below 2 GB
inline long long field_at_chunk(long long env) { return env <= 0 ? (1ll << 20) : std::min(env, 1ll << 24); }

// ---- polar_ewald_field_grid -------------------------------------------------------------------------------------------------
// The grid of a call: every n[a] >= 1, n[0] n[1] n[2] <= 2^31 - 1 (a flat index is an int), every offset finite and in [0, 1)
// (offset null: the cell centres, 0.5 each).  Returns the number of points and fills off.
inline long long check_grid(const int n[3], const double *offset, double off[3]) {
  if (!n) throw InputError("polar_ewald_field_grid: null pointer");
  long long npts = 1;
  for (int a = 0; a < 3; a++) {
    if (n[a] < 1) throw InputError("polar_ewald_field_grid: a grid count below 1");
    npts *= n[a];   // (at most 2^31 - 1 times a value checked to be at most 2^31 - 1: no overflow of 64 bits)
    if (npts > 2147483647LL) throw InputError("polar_ewald_field_grid: more than 2^31 - 1 grid points");
  }
  for (int a = 0; a < 3; a++) {
    off[a] = offset ? offset[a] : 0.5;
    if (!(off[a] >= 0.0 && off[a] < 1.0)) throw InputError("polar_ewald_field_grid: offset outside [0, 1)");
  }
  return npts;
}

// ---- pair tables ----------------------------------------------------------------------------------------------------------
// The LJ tables repacked so that the half-list loop reads one 64-byte line per type pair:
// t = lj1, lj2, lj3, lj4, offset, cut_ljsq, cutsq  ->  cutsq, cut_ljsq, lj1, lj2, lj3, lj4, offset, pad.
// Returns the largest pair cutoff: inside it lies class 0 of the symmetrised LJ/Coulomb rows (polar_skin.hpp)
inline double pack_lj_table(int ntypes, const double *const t[7], std::vector<double> &pack) {
  const size_t m = (size_t)(ntypes + 1) * (ntypes + 1);
  pack.assign(8 * m, 0.0);
  for (size_t k = 0; k < m; k++) {
    pack[8 * k + 0] = t[6][k]; pack[8 * k + 1] = t[5][k]; pack[8 * k + 2] = t[0][k]; pack[8 * k + 3] = t[1][k];
    pack[8 * k + 4] = t[2][k]; pack[8 * k + 5] = t[3][k]; pack[8 * k + 6] = t[4][k];
  }
  double cmax2 = 0.0;
  for (size_t k = 0; k < m; k++) cmax2 = std::max(cmax2, t[6][k]);
  return std::sqrt(cmax2);
}
// ... and the Coulomb tables, one line per bin (one zeroed line without a table):
// t = r, dr, f, df, c, dc, e, de  ->  r, dr, f, df, e, de, c, dc
inline void pack_coul_table(int nbits, const double *const t[8], std::vector<double> &pack) {
  const size_t nt = nbits ? ((size_t)1 << nbits) : 1;
  pack.assign(8 * nt, 0.0);
  static const int order[8] = {0, 1, 2, 3, 6, 7, 4, 5};
  if (nbits)
    for (size_t b = 0; b < nt; b++)
      for (int k = 0; k < 8; k++) pack[8 * b + k] = t[order[k]][b];
}

// How k_ljcoul_pers may find a pair's bin (polar_rows.hpp, ljcoul_row TAB): checked here, bin by bin, against the tables the
// caller handed over (Pair::init_tables, src/pair.cpp): r = a float whose low `shift` mantissa bits are zero and whose masked
// bits give the bin's own index; dr = the reciprocal of one bin step of that binade, an exact power of two.  Up to two bins may
// carry another dr (the last bin before the cutoff gets 1 / (cut_coulsq - r); the bin where the index wraps): they travel as
// parameters.  Anything else -> the tables stay in memory for r and dr (TAB 1).
struct CoulTableArith {
  bool ok;               // a bin's r and dr can be rebuilt from the bits of (float)rsq
  int lowmask;
  int i_special[2];
  double dr_special[2];
};
inline CoulTableArith coul_table_arith(int nbits, int mask, int shift, const double *r_tab, const double *dr_tab) {
  CoulTableArith a;
  a.lowmask = nbits ? (1 << shift) - 1 : 0;
  a.i_special[0] = a.i_special[1] = -1;
  a.dr_special[0] = a.dr_special[1] = 0.0;
  a.ok = false;
  if (nbits) {
    const size_t nt = (size_t)1 << nbits;
    bool ok = shift > 0 && shift < 23;
    int nspecial = 0;
    for (size_t b = 0; b < nt && ok; b++) {
      const double r = r_tab[b], dr = dr_tab[b];
      const float rf = (float)r;
      int bits;
      memcpy(&bits, &rf, sizeof(int));
      if ((double)rf != r || (bits & a.lowmask) != 0 || (size_t)((bits & mask) >> shift) != b) { ok = false; break; }
      const int e = (bits >> 23) & 0xFF;
      const double want = std::ldexp(1.0, 150 - shift - e);
      if (dr != want) {
        if (nspecial < 2) { a.i_special[nspecial] = (int)b; a.dr_special[nspecial] = dr; nspecial++; }
        else ok = false;
      }
    }
    a.ok = ok;
  }
  return a;
}

// ---- the grid of polar_build_neighbors -------------------------------------------------------------------------------------
// over the bounding box of locals + ghosts (recorded by polar_set_atoms), cell edge >= cutmax / 2, 1 .. 512 cells a side.
// Fills nc, lo and inv of g (LJGrid, polar_lists.hpp, or anything with the three) and returns the number of cells
template <class G>
inline long long lj_grid(const double bbox_lo[3], const double bbox_hi[3], double cutmax, G &g) {
  long long ncell = 1;
  for (int k = 0; k < 3; k++) {
    const double ext = std::max(bbox_hi[k] - bbox_lo[k], 1e-9);
    int nc = (int)std::floor(ext / (0.5 * cutmax));
    nc = std::max(1, std::min(nc, 512));
    g.nc[k] = nc; g.lo[k] = bbox_lo[k]; g.inv[k] = nc / ext;
    ncell *= nc;
  }
  return ncell;
}
// row pitch of its first build: 1.3x the mean sphere population, rounded to 64 (cutmax2 = the squared cutoff)
inline long long lj_first_pitch(const double bbox_lo[3], const double bbox_hi[3], double cutmax2, long long nall) {
  const double cutmax = std::sqrt(cutmax2);
  const double vol = std::max((bbox_hi[0] - bbox_lo[0]) * (bbox_hi[1] - bbox_lo[1]) * (bbox_hi[2] - bbox_lo[2]), 1e-9);
  const double mean = 4.18879 * cutmax * cutmax2 * nall / vol;
  return pitch_first(mean, 1.3);
}

// ---- settings ---------------------------------------------------------------------------------------------------------------
// the one solver rule outside the text parser (which refuses the same, keyword by keyword, with the same words)
inline void check_solver_choice(const polar_settings &s) {
  if (s.zodid && (s.polar_gs || s.polar_gs_ranked)) throw InputError("Zodid doesn't work with polar_gs or polar_gs_ranked");
  if (s.polar_gs && s.polar_gs_ranked) throw InputError("polar_gs and polar_gs_ranked are mutually exclusive");
}

// ---- restart record (include/polar_mi355x.h, polar_restart_pack) --------------------------------------------------------------
const int kRestartMagic = 0x524C4F50;  // 'POLR' (little endian)
const int kRestartVersion = 2;         // 2: + deterministic, rccl_halo, polar_accel (int32) and polar_sor (double) behind the version-1 payload
const int kRestartPayloadV1 = 4 * (int)sizeof(double) + 10 * (int)sizeof(int);
const int kRestartPayload = kRestartPayloadV1 + 4 * (int)sizeof(int) + (int)sizeof(double);

// bytes of the record when buf is null; POLAR_ERR_INPUT when max_bytes is too small; else the bytes written
inline int restart_pack(const polar_settings &st, void *buf, int max_bytes) {
  const int total = POLAR_RESTART_HEADER_BYTES + kRestartPayload;
  if (!buf) return total;
  if (max_bytes < total) return POLAR_ERR_INPUT;
  char *p = (char *)buf;
  const int head[3] = {kRestartMagic, kRestartVersion, kRestartPayload};
  memcpy(p, head, sizeof(head)); p += sizeof(head);
  const double d[4] = {st.polar_precision, st.polar_damp, st.polar_gamma, st.dd_cutoff};
  memcpy(p, d, sizeof(d)); p += sizeof(d);
  const int iv[10] = {st.iterations_max, st.damping_type, st.zodid, st.fixed_iteration, st.polar_gs, st.polar_gs_ranked,
                      st.use_previous, st.debug, st.device_neigh, st.restart_polar};
  memcpy(p, iv, sizeof(iv)); p += sizeof(iv);
  const int iv2[4] = {st.deterministic, st.rccl_halo, st.polar_accel, 0};
  memcpy(p, iv2, sizeof(iv2)); p += sizeof(iv2);
  memcpy(p, &st.polar_sor, sizeof(double));
  return total;
}
// the settings of a record laid over those in force (`now`)
inline polar_settings restart_unpack(const polar_settings &now, const void *buf, int nbytes) {
  if (!buf || nbytes < POLAR_RESTART_HEADER_BYTES) throw InputError("not a polarization restart record");
  const char *p = (const char *)buf;
  int head[3];
  memcpy(head, p, sizeof(head)); p += sizeof(head);
  if (head[0] != kRestartMagic) throw InputError("not a polarization restart record");
  const bool v1 = head[1] == 1 && head[2] == kRestartPayloadV1, v2 = head[1] == kRestartVersion && head[2] == kRestartPayload;
  if (!(v1 || v2) || nbytes < POLAR_RESTART_HEADER_BYTES + head[2])
    throw InputError("polarization restart record of an unknown version or length");
  double d[4]; int iv[10];
  memcpy(d, p, sizeof(d)); p += sizeof(d);
  memcpy(iv, p, sizeof(iv)); p += sizeof(iv);
  polar_settings s = now;  // the cutoffs stay as the stock record set them
  s.polar_precision = d[0]; s.polar_damp = d[1]; s.polar_gamma = d[2]; s.dd_cutoff = d[3];
  s.iterations_max = iv[0]; s.damping_type = iv[1]; s.zodid = iv[2]; s.fixed_iteration = iv[3]; s.polar_gs = iv[4];
  s.polar_gs_ranked = iv[5]; s.use_previous = iv[6]; s.debug = iv[7]; s.device_neigh = iv[8]; s.restart_polar = iv[9];
  if (v2) {  // (a version-1 record leaves these at the defaults in force)
    int iv2[4]; double sor;
    memcpy(iv2, p, sizeof(iv2)); p += sizeof(iv2);
    memcpy(&sor, p, sizeof(double));
    s.deterministic = iv2[0]; s.rccl_halo = iv2[1]; s.polar_accel = iv2[2]; s.polar_sor = sor;
    if (!(s.polar_sor > 0.0 && s.polar_sor < 2.0) || s.polar_accel < 0 || s.polar_accel > POLAR_ACCEL_MAX) throw InputError("polarization restart record holds an illegal polar_sor / polar_accel");
  }
  check_solver_choice(s);
  return s;
}

}  // namespace polar
