// polar_api.hip -- the C-ABI entry points (include/polar_mi355x.h): handle lifetime, the host mirror of the Pair text
// interface, per-step data, the compute calls and the stepwise / sharded interface.  The orchestration of a step lives in
// polar_step.hip, the colour phases in polar_color.hip, the multi-GPU driver in polar_dist.hip.
#include "polar_handle.hpp"

namespace {
// upload LJ tables + Coulomb tables from the host mirror (or raw setters) into P, repacked so that
// the half-list loop reads one 64-byte line per type pair / per Coulomb bin
void upload_types(polar_handle *h, int ntypes, const double *const t[7]) {
  need_device(h);
  std::vector<double> pack;
  // the largest pair cutoff: inside it lies class 0 of the symmetrised LJ/Coulomb rows (polar_skin.hpp); classes made for
  // another table are not used again
  const double r_cmax = pack_lj_table(ntypes, t, pack);
  h->d_lj.ensure(pack.size());
  HIPCHECK(hipMemcpy(h->d_lj.p, pack.data(), pack.size() * sizeof(double), hipMemcpyHostToDevice));
  h->P.ntypes = ntypes;
  h->P.ljpack = h->d_lj.p;
  h->ntypes = ntypes;
  h->types_set = true;
  h->r_cmax = r_cmax;
  h->skin_valid = false;
  // polar_probe_at: the table on the host, and how far a probe of every type reaches
  h->lj_host = pack;
  h->probe_reach_max = probe_reach(ntypes, h->lj_host.data(), h->probe_reach);
  h->d_pr_reach.ensure(h->probe_reach.size());
  HIPCHECK(hipMemcpy(h->d_pr_reach.p, h->probe_reach.data(), h->probe_reach.size() * sizeof(double), hipMemcpyHostToDevice));
}

void upload_coul(polar_handle *h, double g_ewald, double qqrd2e, const double *slj, const double *scoul, int nbits,
                 int mask, int shift, double tabinnersq, const double *const t[8]) {
  need_device(h);
  h->P.g_ewald = g_ewald; h->P.qqrd2e = qqrd2e;
  for (int k = 0; k < 4; k++) { h->P.special_lj[k] = slj[k]; h->P.special_coul[k] = scoul[k]; }
  h->P.ncoultablebits = nbits; h->P.ncoulmask = mask; h->P.ncoulshiftbits = shift; h->P.tabinnersq = tabinnersq;
  std::vector<double> pack;
  pack_coul_table(nbits, t, pack);
  h->d_tab.ensure(pack.size());
  HIPCHECK(hipMemcpy(h->d_tab.p, pack.data(), pack.size() * sizeof(double), hipMemcpyHostToDevice));
  h->P.ctab = h->d_tab.p;
  // whether k_ljcoul_pers may rebuild a bin's r and dr from the bits of (float)rsq, and the bins that need help
  const CoulTableArith a = coul_table_arith(nbits, mask, shift, t[0], t[1]);
  h->P.tab_lowmask = a.lowmask;
  for (int k = 0; k < 2; k++) { h->P.i_special[k] = a.i_special[k]; h->P.dr_special[k] = a.dr_special[k]; }
  h->lj_tab_arith = a.ok;
  h->coul_set = true;
}
}  // namespace

// =============================================================================================
namespace {
// polar_pair_extract "lj_walked" / "lj_entries": read back when asked for, nothing per step (the one query that is not a
// plain lookup: it waits for the streams and writes the handle's two numbers -- said so in include/polar_mi355x.h)
void lj_counters(polar_handle *h) {
  h->lj_walked = h->lj_entries = 0.0;
  if (!h->have_device || !h->neigh_set || h->inum <= 0 || !h->lj_ran) return;   // (no LJ/Coulomb launch yet on the list in force: nothing was walked)
  if (!h->lj_sym_last) { h->lj_walked = h->lj_entries = (double)h->nneigh; return; }
  HIPCHECK(hipSetDevice(h->device));
  HIPCHECK(hipStreamSynchronize(h->stream));
  if (h->lj_stream) HIPCHECK(hipStreamSynchronize(h->lj_stream));
  long long total = 0;
  HIPCHECK(hipMemcpy(&total, h->d_sym_first.p + h->lj_rows_last, sizeof(long long), hipMemcpyDeviceToHost));
  unsigned long long walked = (unsigned long long)total;
  if (h->lj_walk_last) {   // the row lengths of the last step are still on the device: summed here
    HIPCHECK(hipMemsetAsync(h->d_lj_drift.p + 1, 0, sizeof(unsigned long long), h->stream));
    k_lj_walk_sum<<<nblk(h->lj_rows_last, 1024), 256, 0, h->stream>>>(h->lj_rows_last, h->d_lj_walk.p, h->d_lj_drift.p + 1);
    HIPCHECK(hipMemcpyAsync(&walked, h->d_lj_drift.p + 1, sizeof(walked), hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
  }
  h->lj_entries = (double)total; h->lj_walked = (double)walked;
}
// polar_pair_extract "nl_entries" / "force_rows": the same way -- the entries the last list build wrote into the full list
// (0 in exact mode: there is no list) and the rows the last force launch did not skip, summed on the device when asked.
// "force_rows" is NOT observed in the launch (no per-row atomic in the hot kernel): k_nl_inert_sums applies the kernel's own
// test, site_is_inert(q, alpha), to the records and rows that launch read.  Both are 0 after polar_set_atoms or
// polar_set_row_range until the next compute call: nl_cnt, the rows and the records on the device belong to the last step.
void inert_counters(polar_handle *h) {
  h->nl_entries = h->force_rows = 0.0;
  if (!h->have_device || !h->force_ran || h->force_nrows <= 0) return;   // (no step yet)
  HIPCHECK(hipSetDevice(h->device));
  if (!h->nl_inert) h->force_rows = (double)h->force_nrows;   // nothing is skipped
  if (!h->force_listed && !h->nl_inert) return;
  h->d_inert_sums.ensure(2);
  unsigned long long sums[2] = {0ull, 0ull};
  HIPCHECK(hipMemsetAsync(h->d_inert_sums.p, 0, 2 * sizeof(unsigned long long), h->stream));
  const int n = h->force_listed ? h->nlocal : 0, m = std::max(n, h->force_nrows);
  k_nl_inert_sums<<<nblk(m, 1024), 256, 0, h->stream>>>(n, h->force_listed ? h->d_nl_cnt.p : nullptr, h->nl_pitch, h->nl_inert ? h->force_nrows : 0,
                                                      own_rows(h), h->d_rec0.p, h->d_inert_sums.p);   // (rows and records of the last step)
  HIPCHECK(hipMemcpyAsync(sums, h->d_inert_sums.p, sizeof(sums), hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(hipStreamSynchronize(h->stream));
  h->nl_entries = (double)sums[0];
  if (h->nl_inert) h->force_rows = (double)sums[1];
}
// The half list of a reneighbor step on its way to the device (PS.cpp:232-247 reads list->firstneigh): rows are packed in
// ilist order into two pinned 32 MB buffers by the helper threads -- each thread checking its entries on the way -- and a
// buffer travels (hipMemcpyAsync from pinned memory: the full PCIe rate) while the next one is packed.  270 MB at 135k atoms:
// a single-threaded flatten + check + four copies out of pageable memory took 20 ms; this takes what the link takes.
// `row(i)` = where atom i's numneigh[i] entries lie on the host (LAMMPS' pages, or a caller's flat array).
template <typename RowFn>
void upload_neighbor_rows(polar_handle *h, int inum, const int *ilist, const int *numneigh, RowFn row) {
  // The list leaves on its OWN stream and the call returns when the last row has been packed into pinned memory, not when the
  // last byte has arrived: the tail of the transfer (270 MB at 134,900 atoms: ~5 ms of PCIe) runs under whatever the caller does
  // next -- polar_set_atoms, the first kernels of polar_compute --; the LJ/Coulomb loop's stream waits for `ev_list_up` before
  // it touches the list (launch_lj).  One pinned 32-MB buffer per chunk of the list (kept for the next list; a ring beyond 2 GB).
  const int n = h->nlocal, nall = h->nlocal + h->nghost;
  if (!h->up_stream) {
    h->up_stream.create(hipStreamNonBlocking);
    h->ev_list_up.create(hipEventDisableTiming);
  }
  hipStream_t s = h->up_stream;
  HIPCHECK(hipStreamSynchronize(s));            // the previous list's transfer reads the staging buffers refilled below
  HIPCHECK(hipStreamSynchronize(h->stream));    // (and its consumers are done with the device arrays that may be re-allocated)
  if (h->lj_stream) HIPCHECK(hipStreamSynchronize(h->lj_stream));
  h->list_up_pending = false;
  std::vector<long long> &first = h->h_first;
  std::vector<int> &nn = h->h_nn;
  first.assign((size_t)std::max(n, 1), 0);
  nn.assign((size_t)std::max(n, 1), 0);
  std::vector<long long> at((size_t)inum + 1, 0);
  long long total = 0;
  for (int ii = 0; ii < inum; ii++) {
    const int i = ilist[ii];
    if (i < 0 || i >= n) throw InputError("neighbor list row index out of range");
    if (numneigh[i] < 0) throw InputError("negative neighbor count/offset");
    first[i] = total; nn[i] = numneigh[i]; at[ii] = total;
    total += numneigh[i];
  }
  at[inum] = total;
  h->inum = inum; h->nneigh = total;
  h->d_ilist.ensure(inum + 1); h->d_numneigh.ensure(n + 1); h->d_first.ensure(n + 1); h->d_neigh.ensure((size_t)total + 1);
  h->h_ilist.assign(ilist, ilist + inum);       // (the caller's ilist may change after the call)
  HIPCHECK(hipMemcpyAsync(h->d_ilist.p, h->h_ilist.data(), inum * sizeof(int), hipMemcpyHostToDevice, s));
  HIPCHECK(hipMemcpyAsync(h->d_numneigh.p, nn.data(), n * sizeof(int), hipMemcpyHostToDevice, s));
  HIPCHECK(hipMemcpyAsync(h->d_first.p, first.data(), n * sizeof(long long), hipMemcpyHostToDevice, s));
  const long long CH = 8ll << 20;   // entries per buffer (32 MB)
  constexpr size_t kRing = 64;      // at most 2 GB of pinned staging; longer lists reuse buffers as their transfers end
  HostPool &pool = HostPool::get();
  const int nt = pool.width();
  std::vector<int> bad((size_t)nt * 16, 0);
  size_t chunk = 0;
  for (int ii0 = 0; ii0 < inum;) {
    int ii1 = ii0;
    while (ii1 < inum && at[ii1 + 1] - at[ii0] <= CH) ii1++;
    if (ii1 == ii0) throw InputError("a neighbor row of more than 8M entries");
    const size_t buf = chunk % kRing;
    if (buf >= h->h_nl_stage.size()) {
      PinBuf<int> p; Event e;
      p.ensure((size_t)CH);
      e.create(hipEventDisableTiming);
      h->h_nl_stage.push_back(std::move(p)); h->ev_nl.push_back(std::move(e));
    }
    if (chunk >= kRing) HIPCHECK(hipEventSynchronize(h->ev_nl[buf]));   // the transfer that last used this buffer is over
    int *dst = h->h_nl_stage[buf].p;
    const long long t0 = at[ii0], cnt = at[ii1] - t0;
    pool.run([&](int part) {
      // thread `part` packs the rows whose first entry lies in its share of the chunk's entries
      const long long lo = t0 + cnt * part / nt, hi = t0 + cnt * (part + 1) / nt;
      int a = (int)(std::lower_bound(at.begin() + ii0, at.begin() + ii1, lo) - at.begin());
      const int b = (int)(std::lower_bound(at.begin() + ii0, at.begin() + ii1, hi) - at.begin());
      int worst = 0;
      for (; a < b; a++) {
        const int i = ilist[a], m = numneigh[i];
        const int *src = row(i);
        int *d = dst + (at[a] - t0);
        int mx = 0;
        for (int k = 0; k < m; k++) { const int v = src[k]; d[k] = v; const int j = v & 0x3FFFFFFF; mx = j > mx ? j : mx; }
        worst = mx > worst ? mx : worst;
      }
      if (worst >= nall) bad[(size_t)part * 16] = 1;
    }, nt);
    for (int t = 0; t < nt; t++) if (bad[(size_t)t * 16]) { HIPCHECK(hipStreamSynchronize(s)); throw InputError("neighbor index out of range"); }
    if (cnt > 0) HIPCHECK(hipMemcpyAsync(h->d_neigh.p + t0, dst, (size_t)cnt * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHECK(hipEventRecord(h->ev_nl[buf], s));
    ii0 = ii1; chunk++;
  }
  HIPCHECK(hipEventRecord(h->ev_list_up, s));
  h->list_up_pending = true;
  h->neigh_set = true;
  h->sym_valid = false; h->lj_ran = false;
  if (h->colors_valid) h->colors_recheck = true;  // reneighbor step: the colour phases are re-validated (k_nl_build)
  h->device_list = false;
  h->full_list = h->user_full_list;
}

/* ---- the calls that look at a finished step from caller-supplied points -------------------------------------------- */
// What every one of them refuses, in this order, under the entry's own name ...
void point_call_state(polar_handle *h, const std::string &name) {
  if (sharded(h)) throw Unsupported(name + ": not offered on a row-sharded handle");
  if (tile_mode(h)) throw Unsupported(name + ": not offered with the tile sweep (lab build)");
  if (!h->field_ready) throw std::runtime_error(name + ": no finished step to look at (call it after polar_compute / polar_step_finish and before the next polar_set_*)");
}
// ... and what those with a point list check after that (periodic_list: the list mode's walk needs a box periodic in every
// direction).  Zeroes *device_ms and, on a polar_ewald handle, the split device times.  False: no points, nothing to do.
bool point_call_begin(polar_handle *h, const std::string &name, bool periodic_list, long long npoints, const double *x,
                      const int *skip_atom, double *device_ms) {
  point_call_state(h, name);
  if (periodic_list && h->ph.st.dd_cutoff > 0.0 && !(h->box.periodic[0] && h->box.periodic[1] && h->box.periodic[2]))
    throw Unsupported(name + ": list mode (dd_cutoff > 0) needs a box periodic in every direction");
  if (npoints < 0) throw InputError(name + ": negative point count");
  if (device_ms) *device_ms = 0.0;
  if (ewald_on(h)) h->ew_fa_ms[0] = h->ew_fa_ms[1] = 0.0;
  if (npoints == 0) return false;
  if (!x) throw InputError(name + ": null pointer");
  const double tilt[3] = {h->box.xy, h->box.xz, h->box.yz};
  check_points(npoints, x, skip_atom, h->nlocal, h->boxlo, h->box.prd, h->box.triclinic ? tilt : nullptr, h->box.periodic);
  return true;
}
// The passes of a call: pass(p0, m) for the points [p0, p0 + m).  POLAR_FIELD_AT_CHUNK is read at every call: a pass holds at
// most that many points on the device.
template <class F>
void point_passes(long long npoints, F pass) {
  const char *e = getenv("POLAR_FIELD_AT_CHUNK");
  const long long chunk = field_at_chunk(e ? atoll(e) : 0);
  for (long long p0 = 0; p0 < npoints; p0 += chunk) pass(p0, (int)std::min(chunk, npoints - p0));
}
// the part of a per-point array (w values per point) that starts at point p0; null stays null
template <class T>
T *from(T *a, long long p0, int w = 1) { return a ? a + w * p0 : nullptr; }
}  // namespace


extern "C" {

const char *polar_kernel_version(void) { return POLAR_KERNEL_VERSION; }

int polar_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int polar_create(int device, polar_handle **out) {
  if (!out) return POLAR_ERR_STATE;
  polar_handle *h = new polar_handle();
  *out = h;
  h->device = device;
  if (const char *e = getenv("POLAR_COLOR_DIST")) h->color_dist = atof(e);
  h->color_keep = std::max(h->color_dist - 0.4, 0.75 * h->color_dist);
  if (const char *e = getenv("POLAR_COLOR_KEEP")) h->color_keep = atof(e);
  if (const char *e = getenv("POLAR_DETERMINISTIC")) h->deterministic = atoi(e) != 0;  // the same as the keyword `deterministic yes`
#ifdef POLAR_LAB
#include "lab/api_env_knobs.inc"
#endif
  int n = polar_device_count();
  if (n <= 0 || device < 0 || device >= n) {
    h->have_device = false;  // host mirror still usable; compute entry points will fail loudly
    h->err = "no usable HIP device";
    return POLAR_OK;
  }
  return guarded(h, [&]() {
    HIPCHECK(hipSetDevice(device));
    h->device_set = true;
    h->stream.create();
    for (auto &e : h->ev) e.create();
    {
      int prio_lo = 0, prio_hi = 0;  // numerically greatest = lowest priority
      HIPCHECK(hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
      h->lj_stream.create(hipStreamNonBlocking, prio_lo);
    }
    h->ev_fork.create(); h->ev_join.create();
    h->ev_lj0.create(); h->ev_lj1.create();
    h->ev_dl0.create(hipEventDisableTiming); h->ev_dl1.create(hipEventDisableTiming);
    h->ev_mu_ready.create(hipEventDisableTiming);
    for (auto &e : h->ev_fchunk) e.create(hipEventDisableTiming);
    for (auto &e : h->ev_ks) e.create();
    h->dl_stream.create(hipStreamNonBlocking);
    if (getenv("POLAR_NO_OVERLAP")) h->overlap_lj = false;
    if (const char *e = getenv("POLAR_LJ_PERS")) h->lj_pers = atoi(e);
    if (const char *e = getenv("POLAR_LJ_SKIN")) h->lj_skin = atoi(e) != 0;   // 0: the LJ/Coulomb rows are walked whole (the A/B partner of the distance classes)
    if (const char *e = getenv("POLAR_NL_INERT")) h->nl_inert = atoi(e) != 0;   // 0: inert sites stay in the full list and keep their force rows (the A/B partner)
    if (const char *e = getenv("POLAR_CELL_INERT")) h->cell_inert = atoi(e) != 0;   // 0: inert sites stay between the others in cell order (the split's A/B partner; no effect with POLAR_NL_INERT=0, which turns the split off too)
    if (const char *e = getenv("POLAR_LJ_PERS_THREADS")) h->lj_pers_threads = std::max(256, std::min(POLAR_LJ_PERS_THREADS, (atoi(e) / 64) * 64));
    { int ncu = 0; if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess) h->ncu = ncu; }
    h->h_scal.ensure(1);
    h->h_flags.ensure(16);
    h->h_ddtot.ensure(64 * 16);
    h->d_overflow.ensure(16); h->d_ddtot.ensure(64 * 16);
    h->d_scal.ensure(1);
    h->d_slots.ensure((size_t)POLAR_NSLOT * POLAR_SLOT_STRIDE);
    h->have_device = true;
    return POLAR_OK;
  });
}

int polar_destroy(polar_handle *h) {
  if (!h) return POLAR_OK;
  delete h;
  return POLAR_OK;
}

const char *polar_last_error(const polar_handle *h) { return h ? h->err.c_str() : "null handle"; }
const char *polar_last_warning(const polar_handle *h) { return h ? h->warn.c_str() : ""; }

int polar_pair_settings(polar_handle *h, int narg, const char *const *arg) {
  return guarded(h, [&]() { h->ph.settings(narg, arg); h->reset_plan(); return POLAR_OK; });
}
int polar_pair_coeff(polar_handle *h, int ntypes, int narg, const char *const *arg) {
  return guarded(h, [&]() { h->ph.coeff(ntypes, narg, arg); return POLAR_OK; });
}
int polar_pair_modify(polar_handle *h, int narg, const char *const *arg) {
  return guarded(h, [&]() { h->ph.modify(narg, arg); return POLAR_OK; });
}
int polar_pair_init(polar_handle *h, double g_ewald, double qqrd2e, const double special_lj[4],
                    const double special_coul[4]) {
  return guarded(h, [&]() {
    PairHost &p = h->ph;
    p.init(g_ewald, qqrd2e, special_lj, special_coul);
    h->coul_set = false;
    h->field_ready = false;   // (qqrd2e scales polar_field_at's static sums: they belong to the step that was computed with it)
    if (h->have_device) {
      HIPCHECK(hipSetDevice(h->device));
      const double *t[7] = {p.lj1.data(), p.lj2.data(), p.lj3.data(), p.lj4.data(), p.offset.data(), p.cut_ljsq.data(), p.cutsq.data()};
      upload_types(h, p.ntypes, t);
      if (p.ncoultablebits == 0) {  // pair_modify table 0: the erfc polynomial everywhere, no table to wait for
        const double *c[8];
        double dummy = 0.0;
        for (int k = 0; k < 8; k++) c[k] = &dummy;
        upload_coul(h, g_ewald, qqrd2e, special_lj, special_coul, 0, 0, 0, 0.0, c);
      }
      // otherwise the Coulomb tables of Pair::init_tables (PS.cpp:851) arrive through polar_set_coul
    }
    return POLAR_OK;
  });
}
double polar_pair_cut(const polar_handle *h, int i, int j) {
  if (!h || !h->ph.inited || i < 1 || j < 1 || i > h->ph.ntypes || j > h->ph.ntypes) return -1.0;
  return std::sqrt(h->ph.cutsq[(size_t)i * h->ph.w() + j]);
}
double polar_pair_single(const polar_handle *h, double qi, double qj, int itype, int jtype, double rsq,
                         double factor_coul, double factor_lj, double *fforce) {
  double ff = 0.0, e;
  try {
    e = h->ph.single(qi, qj, itype, jtype, rsq, factor_coul, factor_lj, ff);
  } catch (const std::exception &ex) {  // no status channel in this signature: NaN + polar_last_error
    const_cast<polar_handle *>(h)->err = ex.what();
    e = ff = std::nan("");
  }
  if (fforce) *fforce = ff;
  return e;
}
const void *polar_pair_extract(const polar_handle *h, const char *name, int *dim) {
  if (!h || !name) return nullptr;
  if (dim) *dim = 0;
  if (strcmp(name, "cut_coul") == 0) return &h->ph.st.cut_coul;
  if (strcmp(name, "nl_dense") == 0) return &h->nl_dense_used;  // 1.0: the last list build walked dense candidate trips
  // list entries the last step's LJ/Coulomb kernel walked / the entries of the rows it visited (equal unless the rows of a
  // symmetrised list were cut short by their distance classes, polar_skin.hpp)
  if (strcmp(name, "lj_walked") == 0 || strcmp(name, "lj_entries") == 0) {
    polar_handle *m = const_cast<polar_handle *>(h);
    if (guarded(m, [&]() { lj_counters(m); return POLAR_OK; }) != POLAR_OK) return nullptr;
    return name[3] == 'w' ? &h->lj_walked : &h->lj_entries;
  }
  // atoms the last cell build filed in the grid's own bins: all of them, or, with the inert sites behind the grid, the others
  if (strcmp(name, "cell_active") == 0) {
    polar_handle *m = const_cast<polar_handle *>(h);
    m->cell_active = 0.0;
    if (h->have_device && h->sorted && h->ph.st.dd_cutoff > 0.0 && h->ncell > 0 && h->d_cell_first.p) {   // (list mode, after a step)
      long long v = 0;
      if (guarded(m, [&]() {
            HIPCHECK(hipSetDevice(m->device));
            HIPCHECK(hipMemcpyAsync(&v, m->d_cell_first.p + m->ncell, sizeof(v), hipMemcpyDeviceToHost, m->stream));
            HIPCHECK(hipStreamSynchronize(m->stream));
            return POLAR_OK;
          }) != POLAR_OK) return nullptr;
      m->cell_active = (double)v;
    }
    return &h->cell_active;
  }
  // entries the last list build wrote into the full list / rows the last force launch walked (fewer than all partners and
  // all rows where the system holds inert sites: no charge, no polarizability)
  if (strcmp(name, "nl_entries") == 0 || strcmp(name, "force_rows") == 0) {
    polar_handle *m = const_cast<polar_handle *>(h);
    if (guarded(m, [&]() { inert_counters(m); return POLAR_OK; }) != POLAR_OK) return nullptr;
    return name[0] == 'n' ? &h->nl_entries : &h->force_rows;
  }
  // device time of the last polar_ewald_field_at call: [0] the real-space kernel, [1] the reciprocal kernels and the fold
  if (strcmp(name, "ewald_field_at_ms") == 0) { if (dim) *dim = 1; return h->ew_fa_ms; }
  // device time of the last polar_ewald step's field half (structure factors and k_ew_field), the part of ms_kspace before the solve
  if (strcmp(name, "ewald_field_ms") == 0) { if (dim) *dim = 0; return &h->ew_field_ms; }   // (a scalar, as "cut_coul")
  if (dim) *dim = 2;
  if (strcmp(name, "epsilon") == 0) return h->ph.epsilon.data();
  if (strcmp(name, "sigma") == 0) return h->ph.sigma.data();
  if (strcmp(name, "cut_lj") == 0) return h->ph.cut_lj.data();
  return nullptr;
}
int polar_get_settings(const polar_handle *h, polar_settings *out) {
  if (!h || !out) return POLAR_ERR_STATE;
  *out = h->ph.st;
  return POLAR_OK;
}
int polar_restart_pack(const polar_handle *h, void *buf, int max_bytes) {
  if (!h) return POLAR_ERR_STATE;
  return restart_pack(h->ph.st, buf, max_bytes);
}
int polar_restart_unpack(polar_handle *h, const void *buf, int nbytes) {
  return guarded(h, [&]() {
    h->ph.st = restart_unpack(h->ph.st, buf, nbytes);
    h->reset_plan();
    return POLAR_OK;
  });
}
int polar_set_settings(polar_handle *h, const polar_settings *s) {
  return guarded(h, [&]() {
    check_solver_choice(*s);
    polar_settings v = *s;
    if (v.polar_sor == 0.0) v.polar_sor = 1.0;   // a zero-initialised struct means "the reference's update", not "freeze the dipoles"
    if (!(v.polar_sor > 0.0 && v.polar_sor < 2.0)) throw InputError("polar_sor must lie in (0, 2)");
    if (v.polar_accel < 0 || v.polar_accel > POLAR_ACCEL_MAX) throw InputError("polar_accel must lie in 0 .. 8");
    if (!(v.polar_ewald >= 0.0 && v.polar_ewald < 1.0)) throw InputError("polar_ewald must lie in [0, 1)");
    h->ph.st = v;
    h->colors_valid = false;
    h->field_ready = false;
    return POLAR_OK;
  });
}
int polar_set_types(polar_handle *h, int ntypes, const double *lj1, const double *lj2, const double *lj3,
                    const double *lj4, const double *offset, const double *cut_ljsq, const double *cutsq) {
  return guarded(h, [&]() {
    HIPCHECK(hipSetDevice(h->device));
    const double *t[7] = {lj1, lj2, lj3, lj4, offset, cut_ljsq, cutsq};
    upload_types(h, ntypes, t);
    return POLAR_OK;
  });
}
int polar_set_coul(polar_handle *h, double g_ewald, double qqrd2e, const double special_lj[4],
                   const double special_coul[4], int nbits, int mask, int shift, double tabinnersq,
                   const double *rtable, const double *drtable, const double *ftable, const double *dftable,
                   const double *ctable, const double *dctable, const double *etable, const double *detable) {
  return guarded(h, [&]() {
    const double *c[8] = {rtable, drtable, ftable, dftable, ctable, dctable, etable, detable};
    h->ph.set_tables(nbits, mask, shift, tabinnersq, c);  // host copy: polar_pair_single reads the same table
    h->field_ready = false;   // (qqrd2e, as in polar_pair_init)
    h->ph.g_ewald = g_ewald; h->ph.qqrd2e = qqrd2e;
    for (int k = 0; k < 4; k++) { h->ph.special_lj[k] = special_lj[k]; h->ph.special_coul[k] = special_coul[k]; }
    if (h->have_device) {
      HIPCHECK(hipSetDevice(h->device));
      double dummy = 0.0;
      if (nbits <= 0) for (int k = 0; k < 8; k++) c[k] = &dummy;
      upload_coul(h, g_ewald, qqrd2e, special_lj, special_coul, nbits > 0 ? nbits : 0, mask, shift, tabinnersq, c);
    }
    return POLAR_OK;
  });
}

int polar_set_box(polar_handle *h, const double boxlo[3], const double prd[3], const double tilt[3],
                  const int periodic[3], int triclinic) {
  return guarded(h, [&]() {
    // triclinic boxes: supported by the exact (all-pairs) kernels through the triclinic branch of
    // closest_image; the list mode's cell grid is orthogonal only
    const bool tri = triclinic != 0;
    Box nb{};
    nb.triclinic = tri ? 1 : 0;
    nb.xy = tri && tilt ? tilt[0] : 0.0;
    nb.xz = tri && tilt ? tilt[1] : 0.0;
    nb.yz = tri && tilt ? tilt[2] : 0.0;
    bool same = h->box_set;
    for (int k = 0; k < 3; k++) {
      if (!(prd[k] > 0.0) || !std::isfinite(prd[k])) throw InputError("box lengths must be positive and finite");
      nb.prd[k] = prd[k]; nb.half[k] = 0.5 * prd[k]; nb.inv[k] = 1.0 / prd[k]; nb.periodic[k] = periodic[k] ? 1 : 0;
      same = same && h->boxlo[k] == boxlo[k] && h->box.prd[k] == nb.prd[k] && h->box.periodic[k] == nb.periodic[k];
      h->boxlo[k] = boxlo[k];
    }
    same = same && h->box.triclinic == nb.triclinic && h->box.xy == nb.xy && h->box.xz == nb.xz && h->box.yz == nb.yz;
    h->box = nb;
    h->box_set = true;
    h->field_ready = false;   // (polar_field_at: the records belong to the box they were made in)
    // a shim hands the box over every step: the colour phases (host-side colouring, rank metric) are rebuilt only when
    // the box really changed -- and on reneighbor steps, through polar_set_neighbors* / polar_build_neighbors
    if (!same) h->colors_valid = false;
    return POLAR_OK;
  });
}

int polar_set_atoms(polar_handle *h, int nlocal, int nghost, const double *x, const double *q, const double *alpha,
                    const int *type, const int *molecule) {
  return guarded(h, [&]() {
    need_device(h);
    HIPCHECK(hipSetDevice(h->device));
    if (nlocal < 0 || nghost < 0) throw InputError("negative atom count");
    h->force_ran = false;   // "nl_entries" / "force_rows" describe a compute call on THESE atoms: 0 until the next one (inert_counters)
    h->field_ready = false;
    const size_t nall = (size_t)nlocal + nghost;
    // the checks and the copies into the pinned staging area by the helper threads (a reneighbor step of an MD run hands all
    // five arrays over: single-threaded checks + five copies out of pageable memory cost 1.3 ms at 258k atoms)
    const size_t words = 3 * nall + nall + nall + (nall + 1) / 2 + (nall + 1) / 2 + 8;
    double *st = staging(h, std::max(words, 3 * nall + 6 * (size_t)nlocal));
    double *sx = st, *sq = sx + 3 * nall, *sa = sq + nall;
    int *stype = reinterpret_cast<int *>(sa + nall), *smol = stype + 2 * ((nall + 1) / 2);
    struct Ext { double lo[3], hi[3]; int bad, neg; char pad[56]; };
    const int nparts = nall < (1u << 14) ? 1 : std::min(8, HostPool::get().width());
    Ext ext[8];
    for (auto &e : ext) { for (int k = 0; k < 3; k++) { e.lo[k] = 1e300; e.hi[k] = -1e300; } e.bad = e.neg = 0; }
    const size_t per = ((nall + nparts - 1) / nparts + 3) / 4 * 4;
    HostPool::get().run([&](int part) {
      Ext &e = ext[part];
      const size_t a0 = std::min(nall, (size_t)part * per), a1 = std::min(nall, ((size_t)part + 1) * per);
      if (!scan_positions(x, sx, a0, a1, e.lo, e.hi)) e.bad = 1;
      memcpy(sq + a0, q + a0, (a1 - a0) * sizeof(double));
      memcpy(sa + a0, alpha + a0, (a1 - a0) * sizeof(double));
      memcpy(stype + a0, type + a0, (a1 - a0) * sizeof(int));
      memcpy(smol + a0, molecule + a0, (a1 - a0) * sizeof(int));
      double amin = 0.0;
      for (size_t k = a0; k < a1; k++) amin = alpha[k] < amin ? alpha[k] : amin;
      if (amin < 0.0) e.neg = 1;
    }, nparts);
    for (const auto &e : ext) {
      if (e.bad) throw InputError("non-finite atom coordinate");
      if (e.neg) throw InputError("Invalid value in set command");  // src/set.cpp:174-184 rejects negatives
    }
    if (nlocal != h->nlocal) { h->colors_valid = false; h->mu_resident = false; }
    else if (h->colors_valid) {  // the rows of the colour phases are the polarizable atoms: same atoms, same rows
      for (int k = 0; k < nlocal; k++)
        if ((alpha[k] != 0.0) != (h->halpha[k] != 0.0)) { h->colors_valid = false; break; }
    }
    h->nlocal = nlocal; h->nghost = nghost;
    // a symmetrised LJ/Coulomb list made for the arrays replaced here keeps no distance classes: the rows are walked whole until
    // the next list (a list uploaded but not yet symmetrised takes its classes from the new arrays)
    if (h->sym_valid) h->skin_valid = false;
    h->d_x.ensure(3 * nall + 3); h->d_q.ensure(nall + 1); h->d_alpha.ensure(nall + 1); h->d_type.ensure(nall + 1); h->d_mol.ensure(nall + 1);
    hipStream_t s = h->stream;
    HIPCHECK(hipMemcpyAsync(h->d_x.p, sx, 3 * nall * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(h->d_q.p, sq, nall * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(h->d_alpha.p, sa, nall * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(h->d_type.p, stype, nall * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(h->d_mol.p, smol, nall * sizeof(int), hipMemcpyHostToDevice, s));
    h->hx.assign(x, x + 3 * (size_t)nlocal);
    h->halpha.assign(alpha, alpha + nlocal);
    for (int k = 0; k < 3; k++) { h->bbox_lo[k] = 1e300; h->bbox_hi[k] = -1e300; }
    for (const auto &e : ext)
      for (int k = 0; k < 3; k++) { h->bbox_lo[k] = std::min(h->bbox_lo[k], e.lo[k]); h->bbox_hi[k] = std::max(h->bbox_hi[k], e.hi[k]); }
    HIPCHECK(hipStreamSynchronize(s));
    h->atoms_set = true;
    h->mu_host_in_sync = false;  // the atoms may sit in a new order
    return POLAR_OK;
  });
}

int polar_set_positions(polar_handle *h, int nlocal, int nghost, const double *x) {
  return guarded(h, [&]() {
    need_device(h);
    HIPCHECK(hipSetDevice(h->device));
    if (!h->atoms_set || nlocal != h->nlocal || nghost != h->nghost) throw InputError("polar_set_positions: atom counts differ from the last polar_set_atoms");
    if (!x) throw InputError("polar_set_positions: null pointer");
    h->field_ready = false;
    const size_t nall = (size_t)nlocal + nghost;
    // through the pinned staging area: a pageable source is staged by the runtime in small pieces at a third of the rate
    // (the caller's array is NOT registered in place, as VERDICT r2 suggested: a registration outlives a free + malloc that
    //  returns the same address with other pages behind it -- LAMMPS re-creates its per-atom arrays between runs -- and the
    //  next DMA would then land in the stale pages.  A copy by four threads costs 0.1 ms at 260k atoms.)
    double *st = staging(h, 3 * nall + 6 * (size_t)nlocal);
    // one pass: the copy, the check polar_set_atoms makes (non-finite coordinates must not reach the cell build) and the
    // bounding box polar_build_neighbors lays its grid over -- so that polar_set_positions -> polar_build_neighbors is as
    // good as polar_set_atoms -> polar_build_neighbors
    struct Ext { double lo[3], hi[3]; int bad; char pad[64]; };
    const int nparts = nall < (1u << 14) ? 1 : std::min(8, HostPool::get().width());
    Ext ext[8];
    for (auto &e : ext) { for (int k = 0; k < 3; k++) { e.lo[k] = 1e300; e.hi[k] = -1e300; } e.bad = 0; }
    const size_t per = ((nall + nparts - 1) / nparts + 3) / 4 * 4;
    HostPool::get().run([&](int part) {
      Ext &e = ext[part];
      const size_t a0 = std::min(nall, (size_t)part * per), a1 = std::min(nall, ((size_t)part + 1) * per);
      if (!scan_positions(x, st, a0, a1, e.lo, e.hi)) e.bad = 1;
    }, nparts);
    for (int k = 0; k < 3; k++) { h->bbox_lo[k] = 1e300; h->bbox_hi[k] = -1e300; }
    for (const auto &e : ext) {
      if (e.bad) throw InputError("non-finite atom coordinate");
      for (int k = 0; k < 3; k++) { h->bbox_lo[k] = std::min(h->bbox_lo[k], e.lo[k]); h->bbox_hi[k] = std::max(h->bbox_hi[k], e.hi[k]); }
    }
    if (h->hx.size() == 3 * (size_t)nlocal) memcpy(h->hx.data(), st, 3 * (size_t)nlocal * sizeof(double));
    HIPCHECK(hipMemcpyAsync(h->d_x.p, st, 3 * nall * sizeof(double), hipMemcpyHostToDevice, h->stream));
    // (no synchronisation: the staging area is next written by the downloads of the compute call, which wait for the stream)
    return POLAR_OK;
  });
}

int polar_set_neighbors_csr(polar_handle *h, int inum, const int *ilist, const int *numneigh,
                            const long long *firstneigh, const int *neigh) {
  return guarded(h, [&]() {
    need_device(h);
    HIPCHECK(hipSetDevice(h->device));
    if (!h->atoms_set) throw std::runtime_error("polar_set_neighbors before polar_set_atoms");
    if (inum < 0 || (inum > 0 && (!ilist || !numneigh || !firstneigh || !neigh))) throw InputError("polar_set_neighbors_csr: null pointer");
    for (int ii = 0; ii < inum; ii++) {
      const int i = ilist[ii];
      if (i < 0 || i >= h->nlocal) throw InputError("neighbor list row index out of range");
      if (firstneigh[i] < 0) throw InputError("negative neighbor count/offset");
    }
    upload_neighbor_rows(h, inum, ilist, numneigh, [&](int i) { return neigh + firstneigh[i]; });
    return POLAR_OK;
  });
}

int polar_build_neighbors(polar_handle *h, const double *cutneighsq, const int *tag, const int *nspecial,
                          const int *special, int maxspecial, const int special_flag[4], int exclude_molecule_intra) {
  return guarded(h, [&]() {
    need_device(h);
    HIPCHECK(hipSetDevice(h->device));
    if (h->list_up_pending) { HIPCHECK(hipStreamSynchronize(h->up_stream)); h->list_up_pending = false; }   // (an uploaded list still on its way into the arrays rebuilt here)
    if (!h->atoms_set || !h->box_set) throw std::runtime_error("polar_build_neighbors before polar_set_box/polar_set_atoms");
    if (!h->types_set) throw std::runtime_error("polar_build_neighbors before the pair tables were set");
    if (!cutneighsq || !special_flag) throw InputError("polar_build_neighbors: null cutneighsq/special_flag");
    if ((nspecial == nullptr) != (special == nullptr) || (special && maxspecial <= 0)) throw InputError("polar_build_neighbors: nspecial/special/maxspecial are inconsistent");
    const int n = h->nlocal, nall = h->nlocal + h->nghost, w = h->ntypes + 1;
    // a sharded handle (polar_set_row_range) holds [own | halo | ghosts]: only the own atoms get list rows -- the halo
    // atoms are somebody else's rows and would otherwise be counted into this rank's energies and virial
    const int nown = own_n(h);
    hipStream_t s = h->stream;
    double cutmax2 = 0.0;
    for (int a = 1; a < w; a++) for (int b = 1; b < w; b++) cutmax2 = std::max(cutmax2, cutneighsq[a * w + b]);
    if (!(cutmax2 > 0.0)) throw InputError("polar_build_neighbors: no positive neighbor cutoff");
    const double cutmax = std::sqrt(cutmax2);
    // grid over the bounding box of locals + ghosts (recorded by polar_set_atoms), cell edge >= cutmax / 2
    LJGrid g;
    const long long ncell = lj_grid(h->bbox_lo, h->bbox_hi, cutmax, g);
    h->d_ljcell_id.ensure(nall + 1); h->d_ljcell_cnt.ensure(ncell + 1); h->d_ljcell_fill.ensure(ncell + 1); h->d_ljcell_first.ensure(ncell + 2);
    h->d_ljpos.ensure(nall + 1); h->d_ljaux.ensure(nall + 1); h->d_cutneighsq.ensure((size_t)w * w);
    HIPCHECK(hipMemcpyAsync(h->d_cutneighsq.p, cutneighsq, (size_t)w * w * sizeof(double), hipMemcpyHostToDevice, s));
    const int *d_tag = nullptr, *d_nsp = nullptr, *d_sp = nullptr;
    if (tag) { h->d_tag.ensure(nall + 1); HIPCHECK(hipMemcpyAsync(h->d_tag.p, tag, (size_t)nall * sizeof(int), hipMemcpyHostToDevice, s)); d_tag = h->d_tag.p; }
    if (special) {
      if (!tag) throw InputError("polar_build_neighbors: special lists need the atom tags");
      h->d_nspecial.ensure(3 * (size_t)n + 3); h->d_special.ensure((size_t)n * maxspecial + 1);
      HIPCHECK(hipMemcpyAsync(h->d_nspecial.p, nspecial, 3 * (size_t)n * sizeof(int), hipMemcpyHostToDevice, s));
      HIPCHECK(hipMemcpyAsync(h->d_special.p, special, (size_t)n * maxspecial * sizeof(int), hipMemcpyHostToDevice, s));
      d_nsp = h->d_nspecial.p; d_sp = h->d_special.p;
    }
    HIPCHECK(hipMemsetAsync(h->d_ljcell_cnt.p, 0, (ncell + 1) * sizeof(int), s));
    HIPCHECK(hipMemsetAsync(h->d_ljcell_fill.p, 0, (ncell + 1) * sizeof(int), s));
    k_lj_cell_count<<<nblk(nall, 256), 256, 0, s>>>(nall, h->d_x.p, g, h->d_ljcell_id.p, h->d_ljcell_cnt.p);
    launch_scan(ncell, h->d_ljcell_cnt.p, h->d_ljcell_first.p, h->d_scan_a, s);
    k_lj_cell_fill<<<nblk(nall, 256), 256, 0, s>>>(nall, h->d_ljcell_id.p, h->d_ljcell_first.p, h->d_ljcell_fill.p, h->d_x.p,
                                                    h->d_type.p, h->d_mol.p, d_tag, h->d_ljpos.p, h->d_ljaux.p);
    if (h->lj_pitch == 0 && getenv("POLAR_INIT_PITCH")) h->lj_pitch = pitch_forced(atoi(getenv("POLAR_INIT_PITCH")));  // tests: force the overflow path
    if (h->lj_pitch == 0) h->lj_pitch = lj_first_pitch(h->bbox_lo, h->bbox_hi, cutmax2, nall);  // first build: 1.3x the mean sphere population
    h->d_numneigh.ensure(n + 1); h->d_ilist.ensure(n + 1); h->d_first.ensure(n + 1);
    h->dev_typed = h->lj_typed && nall < (1 << 24) && h->ntypes < 64;
    const size_t lds = (size_t)w * w * sizeof(double);
    if (lds > 64 * 1024) throw InputError("too many atom types for the LDS-resident cutoff table");
    for (int attempt = 0;; attempt++) {
      h->d_neigh.ensure((size_t)std::max(n, 1) * h->lj_pitch + 64);
      HIPCHECK(hipMemsetAsync(h->d_overflow.p, 0, 16 * sizeof(int), s));
      HIPCHECK(hipMemsetAsync(h->d_ddtot.p, 0, 64 * 16 * sizeof(unsigned long long), s));
      k_lj_nl_build<<<nblk(nown, POLAR_ROWS_PER_BLOCK), POLAR_BLOCK, lds, s>>>(
          own_lo(h), nown, h->ntypes, h->d_x.p, h->d_type.p, h->d_mol.p, h->d_ljpos.p, h->d_ljaux.p, g, h->d_ljcell_first.p,
          h->d_cutneighsq.p, h->box, exclude_molecule_intra, d_nsp, d_sp, maxspecial, special_flag[1], special_flag[2],
          special_flag[3], h->lj_pitch, h->d_numneigh.p, h->d_neigh.p, h->d_overflow.p, h->d_ddtot.p, h->dev_typed ? 1 : 0);
      HIPCHECK(hipMemcpyAsync(h->h_flags.p, h->d_overflow.p, sizeof(int), hipMemcpyDeviceToHost, s));
      HIPCHECK(hipMemcpyAsync(h->h_ddtot.p, h->d_ddtot.p, 64 * 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
      HIPCHECK(hipStreamSynchronize(s));
      HIPCHECK(hipGetLastError());
      if (h->h_flags.p[0] == 0) break;
      if (attempt >= 3) throw std::runtime_error("polar_build_neighbors: row pitch overflow persists");
      h->lj_pitch = pitch_grown(h->h_flags.p[0]);
    }
    unsigned long long tot = 0;
    for (int k = 0; k < 64; k++) tot += h->h_ddtot.p[16 * k];
    h->h_flags.p[0] = 0;
    k_lj_rows<<<nblk(nown, 256), 256, 0, s>>>(own_lo(h), nown, h->lj_pitch, h->d_ilist.p, h->d_first.p);
    h->inum = nown; h->nneigh = (long long)tot;
    h->neigh_set = true; h->sym_valid = false; h->lj_ran = false;
    if (h->colors_valid) h->colors_recheck = true;
    h->device_list = true; h->full_list = 1;
    return POLAR_OK;
  });
}

int polar_set_neighbors(polar_handle *h, int inum, const int *ilist, const int *numneigh, int *const *firstneigh) {
  return guarded(h, [&]() {
    need_device(h);
    HIPCHECK(hipSetDevice(h->device));
    if (!h->atoms_set) throw std::runtime_error("polar_set_neighbors before polar_set_atoms");
    if (inum < 0 || (inum > 0 && (!ilist || !numneigh || !firstneigh))) throw InputError("polar_set_neighbors: null pointer");
    // LAMMPS' paged int** rows, packed straight into the pinned upload buffers (no flat copy in between)
    upload_neighbor_rows(h, inum, ilist, numneigh, [&](int i) { return (const int *)firstneigh[i]; });
    return POLAR_OK;
  });
}

int polar_compute(polar_handle *h, int eflag, int vflag, double *f, double *mu, double *ef_static, polar_result *out) {
  return guarded(h, [&]() {
    if (!f || !mu || !out) throw std::runtime_error("polar_compute: null output pointer");
    if (eflag / 2 || vflag / 4) throw InputError("per-atom tallies (eflag & 2, vflag & 4) are returned by polar_compute_peratom");
    need_device(h);
    HIPCHECK(hipSetDevice(h->device));
    const size_t n = h->nlocal, nall = (size_t)h->nlocal + h->nghost;
    // results come back through one pinned staging area (pageable destinations cost ~3x the PCIe time):
    // [f nall*3 | mu n*3 | ef n*3]; mu and ef leave as soon as the solve is over (phase_finish, their own stream, beside the
    // force kernel), f after the force kernel; the host adds the forces in while whatever is left still travels
    double *st = staging(h, 3 * nall + 6 * n);
    struct Early {  // (cleared on every way out: the stepwise interface shares phase_finish)
      polar_handle *h;
      ~Early() { h->early_mu = h->early_ef = h->user_mu = h->user_ef = nullptr; }
    } early{h};
    h->early_mu = st + 3 * nall;
    h->early_ef = ef_static ? st + 3 * nall + 3 * n : nullptr;
    h->user_mu = mu; h->user_ef = ef_static;
    const bool dbg = getenv("POLAR_DEBUG") != nullptr;
    auto t0 = std::chrono::steady_clock::now();
    auto lap = [&](const char *what) {
      if (!dbg) return;
      const auto t1 = std::chrono::steady_clock::now();
      fprintf(stderr, "[polar] compute: %-22s %7.3f ms\n", what, std::chrono::duration<double, std::milli>(t1 - t0).count());
      t0 = t1;
    };
    int rc = do_compute(h, eflag, vflag, mu, out);
    if (rc < 0) return rc;
    lap("device step + sync");
    // the forces: four pieces, each added into the caller's array while the next one travels
    const size_t tot = 3 * nall, piece = (tot + 3) / 4;
    for (int k = 0; k < 4; k++) {
      const size_t a = std::min(tot, k * piece), b = std::min(tot, (k + 1) * piece);
      if (b > a) HIPCHECK(hipMemcpyAsync(st + a, h->d_f.p + a, (b - a) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
      HIPCHECK(hipEventRecord(h->ev_fchunk[k], h->stream));
    }
    for (int k = 0; k < 4; k++) {
      const size_t a = std::min(tot, k * piece), b = std::min(tot, (k + 1) * piece);
      HIPCHECK(hipEventSynchronize(h->ev_fchunk[k]));
      host_chunks(b - a, [&](size_t lo, size_t hi) { for (size_t i = a + lo; i < a + hi; i++) f[i] += st[i]; });
    }
    lap("f arrived and added");
    h->mu_host_in_sync = true;
    h->field_ready = true;
    return rc;
  });
}

int polar_compute_peratom(polar_handle *h, int eflag, int vflag, double *f, double *mu, double *ef_static,
                          double *eatom, double *vatom, polar_result *out) {
  return guarded(h, [&]() {
    if (!f || !mu || !out) throw std::runtime_error("polar_compute_peratom: null output pointer");
    if ((eflag / 2 && !eatom) || (vflag / 4 && !vatom)) throw InputError("polar_compute_peratom: eflag & 2 needs eatom, vflag & 4 needs vatom");
    need_device(h);
    HIPCHECK(hipSetDevice(h->device));
    int rc = do_compute(h, eflag, vflag, mu, out);
    if (rc < 0) return rc;
    const size_t n = h->nlocal, nall = (size_t)h->nlocal + h->nghost;
    auto add_from = [&](const double *dev, double *host, size_t cnt) {
      h->h_tmp.resize(cnt);
      HIPCHECK(hipMemcpy(h->h_tmp.data(), dev, cnt * sizeof(double), hipMemcpyDeviceToHost));
      for (size_t k = 0; k < cnt; k++) host[k] += h->h_tmp[k];
    };
    add_from(h->d_f.p, f, 3 * nall);
    if (eflag / 2) add_from(h->d_eatom.p, eatom, nall);
    if (vflag / 4) add_from(h->d_vatom.p, vatom, 6 * nall);
    HIPCHECK(hipMemcpy(mu, h->d_mu.p, 3 * n * sizeof(double), hipMemcpyDeviceToHost));
    if (ef_static) HIPCHECK(hipMemcpy(ef_static, h->d_ef.p, 3 * n * sizeof(double), hipMemcpyDeviceToHost));
    h->mu_host_in_sync = true;
    h->field_ready = true;
    return rc;
  });
}

int polar_compute_resident(polar_handle *h, int eflag, int vflag, polar_result *out) {
  return guarded(h, [&]() {
    if (!out) throw std::runtime_error("polar_compute_resident: null result pointer");
    need_device(h);
    HIPCHECK(hipSetDevice(h->device));
    const int rc = do_compute(h, eflag, vflag, nullptr, out);
    if (rc >= 0) h->field_ready = true;
    return rc;
  });
}

void *polar_dev_ptr(polar_handle *h, const char *name) {
  if (!h || !name || !h->have_device) return nullptr;
  if (strcmp(name, "f") == 0) return h->d_f.p;
  if (strcmp(name, "mu") == 0) return h->d_mu.p;
  if (strcmp(name, "ef_static") == 0) return h->d_ef.p;
  if (strcmp(name, "x") == 0) return h->d_x.p;
  if (strcmp(name, "eatom") == 0) return h->d_eatom.p;
  if (strcmp(name, "vatom") == 0) return h->d_vatom.p;
  return nullptr;
}
int polar_download(polar_handle *h, const char *name, double *dst, long long n) {
  return guarded(h, [&]() {
    need_device(h);
    void *p = polar_dev_ptr(h, name);
    if (!p) throw std::runtime_error("polar_download: unknown array name");
    HIPCHECK(hipMemcpy(dst, p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    return POLAR_OK;
  });
}
int polar_upload_mu(polar_handle *h, const double *mu, long long n) {
  return guarded(h, [&]() {
    need_device(h);
    h->d_mu.ensure((size_t)n);
    HIPCHECK(hipMemcpy(h->d_mu.p, mu, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
    h->mu_resident = true;
    return POLAR_OK;
  });
}

/* ---- field and potential of the polarized box at arbitrary points (polar_field_at.hpp) -------- */
int polar_field_at(polar_handle *h, long long npoints, const double *x, const int *skip_atom, const int *molecule,
                   double *e_static, double *e_induced, double *phi_static, double *phi_induced, double *device_ms) {
  return guarded(h, [&]() {
    need_device(h);
    if (ewald_on(h)) throw Unsupported("polar_field_at: with polar_ewald the static field is not the shifted-force one");
    if (!point_call_begin(h, "polar_field_at", true, npoints, x, skip_atom, device_ms)) return (int)POLAR_OK;
    HIPCHECK(hipSetDevice(h->device));
    point_passes(npoints, [&](long long p0, int m) {
      field_at_pass(h, m, x + 3 * p0, from(skip_atom, p0), from(molecule, p0), from(e_static, p0, 3), from(e_induced, p0, 3),
                    from(phi_static, p0), from(phi_induced, p0), device_ms);
    });
    return (int)POLAR_OK;
  });
}

/* ---- ... and with polar_ewald: the Ewald field and potential (polar_ewald_field_at.hpp) -------- */
int polar_ewald_field_at(polar_handle *h, long long npoints, const double *x, const int *skip_atom, const int *molecule,
                         double *e_static, double *e_induced, double *phi_static, double *phi_induced, double *device_ms) {
  return guarded(h, [&]() {
    need_device(h);
    if (!ewald_on(h)) throw Unsupported("polar_ewald_field_at: the handle runs without polar_ewald; polar_field_at maps its shifted-force field");
    if (!point_call_begin(h, "polar_ewald_field_at", false, npoints, x, skip_atom, device_ms)) return (int)POLAR_OK;
    HIPCHECK(hipSetDevice(h->device));
    point_passes(npoints, [&](long long p0, int m) {
      ewald_field_at_pass(h, m, x + 3 * p0, from(skip_atom, p0), from(molecule, p0), from(e_static, p0, 3), from(e_induced, p0, 3),
                          from(phi_static, p0), from(phi_induced, p0), device_ms);
    });
    return (int)POLAR_OK;
  });
}

/* ---- LJ, Coulomb and induction energy of test sites (polar_probe_at.hpp) -------- */
int polar_probe_at(polar_handle *h, long long npoints, const double *x, const int *type, const double *q, const double *alpha,
                   const int *skip_atom, const int *molecule, double *e_lj, double *e_coul, double *e_pol, double *f_lj,
                   double *e_total, double *device_ms) {
  return guarded(h, [&]() {
    need_device(h);
    const polar_settings &st = h->ph.st;
    const bool lj = e_lj || f_lj, field = e_coul || e_pol || e_total;
    if (!point_call_begin(h, "polar_probe_at", true, npoints, x, skip_atom, device_ms)) return (int)POLAR_OK;
    check_probe_sites(npoints, type, h->ntypes, q, alpha, lj);
    if (lj) {
      double width[3];
      box_widths(h->box, width);
      check_probe_reach(st.dd_cutoff > 0.0, h->probe_reach_max, st.cut_coul, st.dd_cutoff, width, h->box.periodic);
    }
    if (!lj && !field) return (int)POLAR_OK;
    HIPCHECK(hipSetDevice(h->device));
    point_passes(npoints, [&](long long p0, int m) {
      probe_at_pass(h, m, x + 3 * p0, from(type, p0), from(q, p0), from(alpha, p0), from(skip_atom, p0), from(molecule, p0), from(e_lj, p0),
                    from(e_coul, p0), from(e_pol, p0), from(f_lj, p0, 3), from(e_total, p0, 3), device_ms);
    });
    return (int)POLAR_OK;
  });
}

/* ---- the gradient of the field at arbitrary points (polar_field_grad_at.hpp) -------- */
int polar_field_grad_at(polar_handle *h, long long npoints, const double *x, const int *skip_atom, const int *molecule,
                        double *g_static, double *g_induced, double *e_static, double *e_induced, double *device_ms) {
  return guarded(h, [&]() {
    need_device(h);
    if (ewald_on(h)) throw Unsupported("polar_field_grad_at: with polar_ewald the static field is not the shifted-force one; polar_ewald_field_grad_at gives the gradient of the Ewald field");
    if (!point_call_begin(h, "polar_field_grad_at", true, npoints, x, skip_atom, device_ms)) return (int)POLAR_OK;
    HIPCHECK(hipSetDevice(h->device));
    point_passes(npoints, [&](long long p0, int m) {
      field_grad_at_pass(h, m, x + 3 * p0, from(skip_atom, p0), from(molecule, p0), from(g_static, p0, 6), from(g_induced, p0, 6),
                         from(e_static, p0, 3), from(e_induced, p0, 3), device_ms);
    });
    return (int)POLAR_OK;
  });
}

/* ---- ... and the force on a test site: LJ, Coulomb, induction (polar_field_grad_at.hpp, polar_probe_at.hpp) -------- */
// what polar_probe_force_at and polar_ewald_probe_force_at do behind their refusals: the pass takes the handle's own gradient
static int probe_force_call(polar_handle *h, const char *name, long long npoints, const double *x, const int *type, const double *q,
                            const double *alpha, const int *skip_atom, const int *molecule, double *f_lj, double *f_coul, double *f_pol,
                            double *device_ms) {
  const polar_settings &st = h->ph.st;
  const bool lj = f_lj != nullptr, field = f_coul || f_pol;
  if (!point_call_begin(h, name, true, npoints, x, skip_atom, device_ms)) return (int)POLAR_OK;
  check_probe_sites(npoints, type, h->ntypes, q, alpha, lj);
  if (lj) {   // (polar_probe_at's reach check: f_lj is that call's)
    double width[3];
    box_widths(h->box, width);
    check_probe_reach(st.dd_cutoff > 0.0, h->probe_reach_max, st.cut_coul, st.dd_cutoff, width, h->box.periodic);
  }
  if (!lj && !field) return (int)POLAR_OK;
  HIPCHECK(hipSetDevice(h->device));
  point_passes(npoints, [&](long long p0, int m) {
    probe_force_at_pass(h, m, x + 3 * p0, from(type, p0), from(q, p0), from(alpha, p0), from(skip_atom, p0), from(molecule, p0),
                        from(f_lj, p0, 3), from(f_coul, p0, 3), from(f_pol, p0, 3), device_ms);
  });
  return (int)POLAR_OK;
}
int polar_probe_force_at(polar_handle *h, long long npoints, const double *x, const int *type, const double *q, const double *alpha,
                         const int *skip_atom, const int *molecule, double *f_lj, double *f_coul, double *f_pol, double *device_ms) {
  return guarded(h, [&]() {
    need_device(h);
    if (ewald_on(h)) throw Unsupported("polar_probe_force_at: with polar_ewald the static field is not the shifted-force one; polar_ewald_probe_force_at gives the force in the Ewald field");
    return probe_force_call(h, "polar_probe_force_at", npoints, x, type, q, alpha, skip_atom, molecule, f_lj, f_coul, f_pol, device_ms);
  });
}

/* ---- ... and with polar_ewald: the gradient of the Ewald field and the force in it (polar_ewald_field_grad_at.hpp) -------- */
int polar_ewald_field_grad_at(polar_handle *h, long long npoints, const double *x, const int *skip_atom, const int *molecule,
                              double *g_static, double *g_induced, double *e_static, double *e_induced, double *device_ms) {
  return guarded(h, [&]() {
    need_device(h);
    if (!ewald_on(h)) throw Unsupported("polar_ewald_field_grad_at: the handle runs without polar_ewald; polar_field_grad_at gives the gradient of its shifted-force field");
    if (!point_call_begin(h, "polar_ewald_field_grad_at", false, npoints, x, skip_atom, device_ms)) return (int)POLAR_OK;
    HIPCHECK(hipSetDevice(h->device));
    point_passes(npoints, [&](long long p0, int m) {
      ewald_field_grad_at_pass(h, m, x + 3 * p0, from(skip_atom, p0), from(molecule, p0), from(g_static, p0, 6), from(g_induced, p0, 6),
                               from(e_static, p0, 3), from(e_induced, p0, 3), device_ms);
    });
    return (int)POLAR_OK;
  });
}

int polar_ewald_probe_force_at(polar_handle *h, long long npoints, const double *x, const int *type, const double *q, const double *alpha,
                               const int *skip_atom, const int *molecule, double *f_lj, double *f_coul, double *f_pol, double *device_ms) {
  return guarded(h, [&]() {
    need_device(h);
    if (!ewald_on(h)) throw Unsupported("polar_ewald_probe_force_at: the handle runs without polar_ewald; polar_probe_force_at gives the force in its shifted-force field");
    return probe_force_call(h, "polar_ewald_probe_force_at", npoints, x, type, q, alpha, skip_atom, molecule, f_lj, f_coul, f_pol, device_ms);
  });
}

/* ---- ... on a regular grid of the cell: the reciprocal sums as three 1-D transforms (polar_ewald_field_grid.hpp) -------- */
int polar_ewald_field_grid(polar_handle *h, const int n[3], const double offset[3], double *x_out, double *e_static, double *e_induced,
                           double *phi_static, double *phi_induced, double *device_ms) {
  return guarded(h, [&]() {
    need_device(h);
    if (!ewald_on(h)) throw Unsupported("polar_ewald_field_grid: the handle runs without polar_ewald; polar_field_at maps its shifted-force field");
    point_call_state(h, "polar_ewald_field_grid");
    double off[3];
    const long long npoints = check_grid(n, offset, off);
    if (device_ms) *device_ms = 0.0;
    h->ew_fa_ms[0] = h->ew_fa_ms[1] = 0.0;
    HIPCHECK(hipSetDevice(h->device));
    EwGridCall call;
    ewald_field_grid_begin(h, n, off, call, device_ms);
    point_passes(npoints, [&](long long p0, int m) {
      ewald_field_grid_pass(h, call, p0, m, from(x_out, p0, 3), from(e_static, p0, 3), from(e_induced, p0, 3), from(phi_static, p0),
                            from(phi_induced, p0), device_ms);
    });
    return (int)POLAR_OK;
  });
}

/* ---- ... and the gradient of that field on the grid: nine coefficient sets through the transforms (polar_ewald_field_grad_grid.hpp) -------- */
int polar_ewald_field_grad_grid(polar_handle *h, const int n[3], const double offset[3], double *x_out, double *g_static, double *g_induced,
                                double *e_static, double *e_induced, double *device_ms) {
  return guarded(h, [&]() {
    need_device(h);
    if (!ewald_on(h)) throw Unsupported("polar_ewald_field_grad_grid: the handle runs without polar_ewald; polar_field_grad_at gives the gradient of its shifted-force field");
    point_call_state(h, "polar_ewald_field_grad_grid");
    double off[3];
    const long long npoints = check_grid(n, offset, off);
    if (device_ms) *device_ms = 0.0;
    h->ew_fa_ms[0] = h->ew_fa_ms[1] = 0.0;
    HIPCHECK(hipSetDevice(h->device));
    EwGridCall call;
    ewald_field_grad_grid_begin(h, n, off, call, device_ms);
    point_passes(npoints, [&](long long p0, int m) {
      ewald_field_grad_grid_pass(h, call, p0, m, from(x_out, p0, 3), from(g_static, p0, 6), from(g_induced, p0, 6), from(e_static, p0, 3),
                                 from(e_induced, p0, 3), device_ms);
    });
    return (int)POLAR_OK;
  });
}

/* ---- stepwise / sharded interface (multi-GPU driver, parallel.py) --------------------------- */
int polar_set_stream(polar_handle *h, void *hip_stream) {
  return guarded(h, [&]() {
    need_device(h);
    if (h->stream.own_stream && h->stream) HIPCHECK(hipStreamSynchronize(h->stream));
    h->stream.borrow((hipStream_t)hip_stream);   // (lets go of the stream it replaces, if that one was the library's)
    return POLAR_OK;
  });
}
int polar_set_row_range(polar_handle *h, int lo, int hi) {
  return guarded(h, [&]() {
    if (lo < 0 || (hi >= 0 && hi < lo)) throw InputError("bad row range");
    h->row_lo = lo; h->row_hi = hi;
    h->force_ran = false;   // (the rows of the last force launch are not the handle's rows any more: inert_counters)
    return POLAR_OK;
  });
}
int polar_set_global_count(polar_handle *h, long long natoms) {
  if (!h) return POLAR_ERR_STATE;
  if (natoms < 0 || natoms > 2147483647LL) return fail(h, POLAR_ERR_INPUT, "bad global atom count");
  h->global_count = natoms;
  return POLAR_OK;
}
int polar_get_debug_trace(polar_handle *h, double *u_polar, int max) {
  if (!h) return POLAR_ERR_STATE;
  int n = 0;
  int rc = guarded(h, [&]() {
    need_device(h);
    n = std::min(h->ntrace, max);
    if (n > 0) HIPCHECK(hipMemcpy(u_polar, h->d_trace.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    return (int)POLAR_OK;
  });
  return rc < 0 ? rc : n;
}
int polar_get_colors(polar_handle *h, int *color, int n) {
  if (!h) return POLAR_ERR_STATE;
  int nc = 0;
  int rc = guarded(h, [&]() {
    need_device(h);
    if (!color || n < 0) throw InputError("polar_get_colors: null pointer");
    const int m = std::min(n, h->nlocal);
    for (int k = 0; k < n; k++) color[k] = -1;
    if (!h->colors_valid || (int)h->color_off.size() < 2) return (int)POLAR_OK;
    nc = (int)h->color_off.size() - 1;
    if (h->d_color_orig.p && h->d_color_orig.cap >= (size_t)m && m > 0)   // colours by original index (both colourings leave them here)
      HIPCHECK(hipMemcpy(color, h->d_color_orig.p, (size_t)m * sizeof(int), hipMemcpyDeviceToHost));
    return (int)POLAR_OK;
  });
  return rc < 0 ? rc : nc;
}
int polar_get_debug_forces(polar_handle *h, double *out6) {
  return guarded(h, [&]() {
    need_device(h);
    if (!out6) throw InputError("polar_get_debug_forces: null pointer");
    for (int k = 0; k < 6; k++) out6[k] = 0.0;
    if (!h->ph.st.debug || !h->d_dbgf.p) return 0;
    HIPCHECK(hipMemcpy(out6, h->d_dbgf.p, 6 * sizeof(double), hipMemcpyDeviceToHost));
    return 1;
  });
}
int polar_set_newton(polar_handle *h, int newton_pair) {
  if (!h) return POLAR_ERR_STATE;
  h->newton_pair = newton_pair ? 1 : 0;
  return POLAR_OK;
}
int polar_set_list_style(polar_handle *h, int full) {
  if (!h) return POLAR_ERR_STATE;
  h->user_full_list = full ? 1 : 0;
  if (!h->device_list) h->full_list = h->user_full_list;
  return POLAR_OK;
}
int polar_step_begin(polar_handle *h, int eflag, int vflag) {
  return guarded(h, [&]() {
    step_begin_lists(h, eflag, vflag);
    step_begin_finish(h);
    return POLAR_OK;
  });
}
int polar_step_sweep_phase(polar_handle *h, int color, int part) {
  return guarded(h, [&]() {
    if (!h->in_step) throw std::runtime_error("polar_step_sweep_phase outside polar_step_begin/finish");
    const polar_settings &st = h->ph.st;
    if (!(st.dd_cutoff > 0.0 && (st.polar_gs || st.polar_gs_ranked) && h->sweep_kernel == 2)) throw InputError("polar_step_sweep_phase: colour phases exist for the Gauss-Seidel sweep of list mode only");
    if (color < 0 || color >= (int)h->color_off.size() - 1 || part < 0 || part > 2) throw InputError("polar_step_sweep_phase: bad colour or part");
    sweep_phase(h, color, part);
    return POLAR_OK;
  });
}
int polar_set_colors(polar_handle *h, const int *color, int n) {
  return guarded(h, [&]() {
    if (!color && n != 0) throw InputError("polar_set_colors: null pointer");
    if (n == 0) { h->user_colors.clear(); h->user_colors_clashed = false; h->colors_valid = false; return POLAR_OK; }
    if (!h->atoms_set || n != h->nlocal) throw InputError("polar_set_colors: one colour per local atom of the last polar_set_atoms");
    for (int k = 0; k < n; k++) {
      if (color[k] < -1 || color[k] > 63) throw InputError("polar_set_colors: colours are -1 (none) or 0 .. 63");
      if ((color[k] >= 0) != (h->halpha[k] != 0.0)) throw InputError("polar_set_colors: exactly the polarizable atoms carry a colour");
    }
    h->user_colors.assign(color, color + n);
    h->user_colors_clashed = false;
    h->colors_valid = false;
    return POLAR_OK;
  });
}
int polar_set_positions_range(polar_handle *h, int lo, int hi, const double *x) {
  return guarded(h, [&]() {
    need_device(h);
    HIPCHECK(hipSetDevice(h->device));
    if (!h->atoms_set || lo < 0 || hi < lo || hi > h->nlocal + h->nghost) throw InputError("polar_set_positions_range: range outside the atoms of the last polar_set_atoms");
    if (hi > lo && !x) throw InputError("polar_set_positions_range: null pointer");
    h->field_ready = false;
    const size_t cnt = 3 * (size_t)(hi - lo);
    double *st = staging(h, 3 * ((size_t)h->nlocal + h->nghost) + 6 * (size_t)h->nlocal);
    if (cnt) {
      // the box the handle has keeps growing (the other atoms are where they were); a refused range leaves it as it was
      double blo[3] = {h->bbox_lo[0], h->bbox_lo[1], h->bbox_lo[2]}, bhi[3] = {h->bbox_hi[0], h->bbox_hi[1], h->bbox_hi[2]};
      if (!scan_positions(x, st, 0, (size_t)(hi - lo), blo, bhi)) throw InputError("non-finite atom coordinate");
      for (int k = 0; k < 3; k++) { h->bbox_lo[k] = blo[k]; h->bbox_hi[k] = bhi[k]; }
      HIPCHECK(hipMemcpyAsync(h->d_x.p + 3 * (size_t)lo, st, cnt * sizeof(double), hipMemcpyHostToDevice, h->stream));
      for (int a = lo; a < std::min(hi, h->nlocal); a++) for (int k = 0; k < 3; k++) h->hx[3 * (size_t)a + k] = x[3 * (size_t)(a - lo) + k];
      HIPCHECK(hipStreamSynchronize(h->stream));   // (the staging area is the caller's to reuse)
    }
    return POLAR_OK;
  });
}
int polar_step_sweep(polar_handle *h) {
  return guarded(h, [&]() {
    if (!h->in_step) throw std::runtime_error("polar_step_sweep outside polar_step_begin/finish");
    sweep_once(h, false);
    return POLAR_OK;
  });
}
int polar_step_sweep_part(polar_handle *h, int part, int nparts) {
  return guarded(h, [&]() {
    if (!h->in_step) throw std::runtime_error("polar_step_sweep_part outside polar_step_begin/finish");
    if (nparts < 1 || part < 0 || part >= nparts) throw InputError("polar_step_sweep_part: bad part");
    const polar_settings &st = h->ph.st;
    if (nparts > 1 && !(st.dd_cutoff > 0.0 && (st.polar_gs || st.polar_gs_ranked) && (h->sweep_kernel == 2 || h->sweep_kernel == 4)))
      throw InputError("polar_step_sweep_part: parts exist for the colour-phase Gauss-Seidel sweep of list mode only");
    struct Window {  // restored on every way out: a failed launch must not leave the next full sweep truncated
      polar_handle *h;
      ~Window() { h->part_k = 0; h->part_n = 1; }
    } window{h};
    h->part_k = part; h->part_n = nparts;
    sweep_once(h, false);
    return POLAR_OK;
  });
}
int polar_step_sweep_end_n(polar_handle *h, const double *dev_global_change, int count) {
  return guarded(h, [&]() {
    if (!h->in_step) throw std::runtime_error("polar_step_sweep_end outside polar_step_begin/finish");
    if (count < 1) throw InputError("polar_step_sweep_end_n: count must be >= 1");
    const polar_settings &st = h->ph.st;
    const bool gs = st.polar_gs || st.polar_gs_ranked;
    if (count > 1 && !(gs && st.fixed_iteration)) throw InputError("polar_step_sweep_end_n: count > 1 needs fixed-iteration Gauss-Seidel");
    launch_solver_step(h, dev_global_change, count);
    return POLAR_OK;
  });
}
int polar_step_sweep_end(polar_handle *h, const double *dev_global_change) { return polar_step_sweep_end_n(h, dev_global_change, 1); }
int polar_step_state(polar_handle *h, int *done, int *iterations, int *status) {
  return guarded(h, [&]() {
    need_device(h);
    read_scal(h);
    if (done) *done = h->h_scal.p->done;
    if (iterations) *iterations = h->h_scal.p->iterations;
    if (status) *status = h->h_scal.p->status;
    return POLAR_OK;
  });
}
int polar_step_finish(polar_handle *h, polar_result *out) {
  return guarded(h, [&]() {
    if (!h->in_step) throw std::runtime_error("polar_step_finish without polar_step_begin");
    memset(out, 0, sizeof(*out));
    int rc = phase_finish(h, out);
    out->ncolors = (h->ph.st.polar_gs || h->ph.st.polar_gs_ranked) ? (tile_mode(h) ? (int)h->tile_launches.size() : (int)h->color_off.size() - 1) : 0;
    h->in_step = false;
    if (grow_pitches(h)) {  // the driver must redo the step (all ranks see their own flag)
      out->status = POLAR_RETRY_STEP;
      h->warn = "neighbor list pitch overflow: pitch enlarged, repeat the step";
      return POLAR_RETRY_STEP;
    }
    h->field_ready = true;
    return rc;
  });
}
int polar_mu_gather(polar_handle *h, long long lo, long long hi, double *dev_dst) {
  return guarded(h, [&]() {
    need_device(h);
    if (hi > lo) k_mu_gather<<<nblk(hi - lo, 256), 256, 0, h->stream>>>(lo, hi, h->sorted ? h->d_inv.p : nullptr, h->d_scal.p, mu_view(h), dev_dst);
    return POLAR_OK;
  });
}
int polar_mu_scatter(polar_handle *h, long long lo, long long hi, const double *dev_src) {
  return guarded(h, [&]() {
    need_device(h);
    h->field_ready = false;   // (the records' dipoles are no longer those of the finished step)
    if (hi > lo) k_mu_scatter<<<nblk(hi - lo, 256), 256, 0, h->stream>>>(lo, hi, h->sorted ? h->d_inv.p : nullptr, h->d_scal.p, mu_view(h), dev_src);
    return POLAR_OK;
  });
}
int polar_mu_gather_idx(polar_handle *h, const int *dev_idx, long long n, double *dev_dst) {
  return guarded(h, [&]() {
    need_device(h);
    if (n > 0) k_mu_gather_idx<<<nblk(n, 256), 256, 0, h->stream>>>(n, dev_idx, h->sorted ? h->d_inv.p : nullptr, h->d_scal.p, mu_view(h), dev_dst);
    return POLAR_OK;
  });
}
int polar_mu_scatter_idx(polar_handle *h, const int *dev_idx, long long n, const double *dev_src) {
  return guarded(h, [&]() {
    need_device(h);
    h->field_ready = false;
    if (n > 0) k_mu_scatter_idx<<<nblk(n, 256), 256, 0, h->stream>>>(n, dev_idx, h->sorted ? h->d_inv.p : nullptr, h->d_scal.p, mu_view(h), dev_src, own_lo(h), own_lo(h) + own_n(h));
    return POLAR_OK;
  });
}
int polar_change_export(polar_handle *h, double *dev_dst) {
  return guarded(h, [&]() {
    need_device(h);
    k_fold_change<<<1, POLAR_NSLOT, 0, h->stream>>>(h->d_scal.p, h->d_slots.p, dev_dst, det_part(h), det_npart(h));
    return POLAR_OK;
  });
}

int polar_step_mu_get(polar_handle *h, long long lo, long long hi, double *mu_host) {
  return guarded(h, [&]() {
    need_device(h);
    if (!mu_host || lo < 0 || hi < lo || hi > h->nlocal) throw InputError("polar_step_mu_get: bad range or null pointer");
    const size_t cnt = 3 * (size_t)(hi - lo);
    if (cnt == 0) return (int)POLAR_OK;
    h->d_xchg.ensure(cnt);
    k_mu_gather<<<nblk(hi - lo, 256), 256, 0, h->stream>>>(lo, hi, h->sorted ? h->d_inv.p : nullptr, h->d_scal.p, mu_view(h), h->d_xchg.p);
    HIPCHECK(hipMemcpyAsync(mu_host, h->d_xchg.p, cnt * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    return (int)POLAR_OK;
  });
}
int polar_step_mu_put_idx(polar_handle *h, long long n, const int *idx_host, const double *mu_host) {
  return guarded(h, [&]() {
    need_device(h);
    if (n < 0 || (n > 0 && (!idx_host || !mu_host))) throw InputError("polar_step_mu_put_idx: null pointer");
    if (n == 0) return (int)POLAR_OK;
    h->field_ready = false;
    for (long long k = 0; k < n; k++)
      if (idx_host[k] >= h->nlocal) throw InputError("polar_step_mu_put_idx: atom index out of range");
    h->d_xchg.ensure(3 * (size_t)n); h->d_xidx.ensure((size_t)n);
    HIPCHECK(hipMemcpyAsync(h->d_xidx.p, idx_host, (size_t)n * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIPCHECK(hipMemcpyAsync(h->d_xchg.p, mu_host, 3 * (size_t)n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    k_mu_scatter_idx<<<nblk(n, 256), 256, 0, h->stream>>>(n, h->d_xidx.p, h->sorted ? h->d_inv.p : nullptr, h->d_scal.p, mu_view(h), h->d_xchg.p, own_lo(h), own_lo(h) + own_n(h));
    HIPCHECK(hipStreamSynchronize(h->stream));  // the host buffers may be reused by the caller
    return (int)POLAR_OK;
  });
}
int polar_step_change_get(polar_handle *h, double *sum) {
  return guarded(h, [&]() {
    need_device(h);
    if (!sum) throw InputError("polar_step_change_get: null pointer");
    h->d_xchg.ensure(8);
    k_fold_change<<<1, POLAR_NSLOT, 0, h->stream>>>(h->d_scal.p, h->d_slots.p, h->d_xchg.p, det_part(h), det_npart(h));
    HIPCHECK(hipMemcpyAsync(sum, h->d_xchg.p, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    return (int)POLAR_OK;
  });
}
int polar_step_sweep_end_host(polar_handle *h, double global_change) {
  if (!h) return POLAR_ERR_STATE;
  int rc = guarded(h, [&]() {
    need_device(h);
    h->d_xchg.ensure(8);
    HIPCHECK(hipMemcpyAsync(h->d_xchg.p + 4, &global_change, sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));  // global_change lives on the caller's stack
    return (int)POLAR_OK;
  });
  if (rc < 0) return rc;
  return polar_step_sweep_end(h, h->d_xchg.p + 4);
}


}  // extern "C"
