// polar_step.hip -- one PairLJCutCoulLongPolarization::compute (PS.cpp:125-645) on one MI355X: cell order and the pitched
// lists, a3 on its side stream, static field, the solve (DipoleSolverIterative, PS.cpp:1113-1238) with its sweep launchers,
// forces and tallies.  All arithmetic of the hot path runs in the kernels of polar_kernels.hpp.
#include "polar_handle.hpp"

// exclusive scan of n ints (out: n + 1 long longs), polar_lists.hpp
void launch_scan(long long n, const int *in, long long *out, DBuf<long long> &tot, hipStream_t s) {
  const int nb = (int)std::max<long long>(1, (n + POLAR_SCAN_ITEMS - 1) / POLAR_SCAN_ITEMS);
  tot.ensure((size_t)nb + 1);
  k_scan_block<<<nb, 1024, 0, s>>>(n, in, out, tot.p);
  if (nb > 1) {
    k_scan_totals<<<1, 1024, 0, s>>>(nb, tot.p, out + n);
    k_scan_add<<<nblk(n - POLAR_SCAN_ITEMS, 256), 256, 0, s>>>(n, out, tot.p);
  }
}

void build_cells(polar_handle *h) {
  const polar_settings &st = h->ph.st;
  const int n = h->nlocal;
  const double cutall = std::max(st.cut_coul, st.dd_cutoff);
  double width[3];
  box_widths(h->box, width);
  CellGrid &g = h->grid;
  if (!list_grid(width, h->box.periodic, cutall, g.nc))
    throw InputError("dd_cutoff mode needs box lengths >= 2*max(cut_coul,dd_cutoff); use exact mode (dd_cutoff 0)");
  g.trim = 1;
#ifdef POLAR_LAB
  if (const char *e = getenv("POLAR_NL_TRIM")) g.trim = atoi(e);
#endif
  if (h->box.triclinic) g.trim = 0;  // the per-atom stencil trimming measures orthogonal distances
  long long ncell = 1;
  for (int k = 0; k < 3; k++) {
    // tile sweep: the launches are the parity classes of the cells; an even count in a periodic dimension needs no third
    // class for the seam (cells grow by at most 1/6)
    if (h->sweep_kernel == 4 && k == 0 && h->tile_wide) g.nc[k] = std::max(1, (int)std::floor(width[k] / cutall));
    if (h->sweep_kernel == 4 && h->box.periodic[k] && g.nc[k] >= 7 && (g.nc[k] & 1)) g.nc[k] -= 1;
    h->tile_sw[k] = std::max(1, std::min(2, (int)std::ceil(st.dd_cutoff / (width[k] / g.nc[k]) - 1e-9)));
    g.lo[k] = h->boxlo[k];
    g.inv[k] = g.nc[k] / h->box.prd[k];
    ncell *= g.nc[k];
  }
  h->ncell = ncell;
  if (h->sweep_kernel == 4) {  // tile colours: per dimension the even cells, the odd cells and -- odd count, periodic -- the last cell
    struct Cls { int start, stride, count; };
    std::vector<Cls> cls[3];
    for (int k = 0; k < 3; k++) {
      const int nc = g.nc[k];
      const bool seam = h->box.periodic[k] && (nc & 1) && nc > 1;
      const int lim = seam ? nc - 1 : nc;
      if ((lim + 1) / 2 > 0) cls[k].push_back(Cls{0, 2, (lim + 1) / 2});
      if (lim / 2 > 0) cls[k].push_back(Cls{1, 2, lim / 2});
      if (seam) cls[k].push_back(Cls{nc - 1, 1, 1});
    }
    h->tile_launches.clear();
    for (const Cls &cz : cls[2]) for (const Cls &cy : cls[1]) for (const Cls &cx : cls[0]) {
      TileLaunch L;
      L.start[0] = cx.start; L.stride[0] = cx.stride; L.count[0] = cx.count;
      L.start[1] = cy.start; L.stride[1] = cy.stride; L.count[1] = cy.count;
      L.start[2] = cz.start; L.stride[2] = cz.stride; L.count[2] = cz.count;
      for (int k = 0; k < 3; k++) L.nc[k] = g.nc[k];
      h->tile_launches.push_back(L);
    }
    for (int k = 0; k < 3; k++) { h->tile_all.start[k] = 0; h->tile_all.stride[k] = 1; h->tile_all.count[k] = g.nc[k]; h->tile_all.nc[k] = g.nc[k]; }
  }
  hipStream_t s = h->stream;
  // inert sites (no charge, no polarizability) are binned behind the grid, into a second copy of it (cell_bin, polar_plan.hpp):
  // cell_first[0 .. ncell], all that the candidate walks and the colouring read, spans the other sites alone, and the record
  // table holds no inert record between two cells.  On exactly when the lists leave the inert sites out (nl_inert).
  const bool split = h->nl_inert && h->cell_inert;
  if (!cell_bins_fit(ncell, split)) throw InputError("the list grid has more cells than a 32-bit bin index holds");
  const CellBins cb = cell_bins(ncell, split);
  const bool pol_first = h->pol_first || h->sweep_kernel == 4;
  h->cell_split = split;
  h->d_cell_id.ensure(n); h->d_cell_cnt.ensure(cb.cnt); h->d_cell_fill.ensure(cb.fill);
  h->d_cell_first.ensure(cb.first); h->d_perm.ensure(n + 1); h->d_inv.ensure(n + 1);
  zero_many(s, {{h->d_cell_cnt.p, (size_t)cb.cnt * sizeof(int)}, {h->d_cell_fill.p, (size_t)cb.fill * sizeof(int)}});
  k_cell_count<<<nblk(n, 256), 256, 0, s>>>(n, h->d_x.p, h->d_q.p, h->d_alpha.p, g, h->box, split ? ncell : 0, h->d_cell_id.p, h->d_cell_cnt.p);
  launch_scan(cb.nbins, h->d_cell_cnt.p, h->d_cell_first.p, h->d_scan_a, s);
  k_cell_fill<<<nblk(n, 256), 256, 0, s>>>(n, h->d_cell_id.p, h->d_cell_first.p, h->d_cell_fill.p,
                                           pol_first ? h->d_cell_fill.p + cb.fill_back : nullptr, h->d_alpha.p, h->d_perm.p, h->d_inv.p);
  // the order inside a cell follows the atomics of k_cell_fill: put it into atom order -- always, not only for `deterministic
  // yes` (reproducible sums): the device colouring breaks its ties by position in the cell, and a colouring that changed from
  // run to run would make unconverged (`fixed_iteration`) results differ at 1e-6 instead of the 1e-9 of the in-place race
  k_cell_sort<<<nblk(cb.nbins, 4), 256, 0, s>>>(cb.nbins, h->d_cell_first.p, pol_first ? h->d_cell_fill.p : nullptr, h->d_perm.p, h->d_inv.p);
  h->sorted = true;
  if (sharded(h)) {
    h->d_ownrows.ensure(own_n(h) + 1);
    k_map_range<<<nblk(own_n(h), 256), 256, 0, s>>>(own_lo(h), own_n(h), h->d_inv.p, h->d_ownrows.p);
  }
}

// lp sweep: where k_nl_build stores every atom's dd row = its row in launch order (colour phases back to back for GS,
// own rows for Jacobi).  While no colouring exists yet (first step, or after a clash) the rows are laid out in atom
// order and the lists are built once more after the colouring (solve / polar_step_begin).
void compute_slots(polar_handle *h) {
  const polar_settings &st = h->ph.st;
  const bool gs = st.polar_gs || st.polar_gs_ranked;
  const int n = h->nlocal;
  hipStream_t s = h->stream;
  h->d_slot.ensure(n + 1);
  HIPCHECK(hipMemsetAsync(h->d_slot.p, 0xFF, (size_t)(n + 1) * sizeof(int), s));
  if (gs && h->colors_valid) {
    const int tot = h->color_off.empty() ? 0 : h->color_off.back();
    if (tot > 0) k_slot_from_rows<<<nblk(tot, 256), 256, 0, s>>>(tot, h->d_rows.p, h->d_slot.p);
    h->slots_by_color = true;
    h->slots_epoch = h->color_epoch;
  } else {
    k_slot_from_rows<<<nblk(own_n(h), 256), 256, 0, s>>>(own_n(h), own_rows(h), h->d_slot.p);
    h->slots_by_color = false;
  }
}

void build_lists(polar_handle *h) {
  const polar_settings &st = h->ph.st;
  const int n = h->nlocal;
  const double cutall = std::max(st.cut_coul, st.dd_cutoff);
  hipStream_t s = h->stream;
  const CellGrid &g = h->grid;
  if (h->nl_pitch == 0 && getenv("POLAR_INIT_PITCH")) h->nl_pitch = h->dd_pitch = pitch_forced(atoi(getenv("POLAR_INIT_PITCH")));  // tests: force the overflow path
  if (h->nl_pitch == 0) {  // first build: 1.5x the mean sphere population, at the density of the OCCUPIED part of the box
    const double vol = occupied_volume(n, h->hx.data(), g.lo, h->box.prd, cutall);
    h->dens = n / vol;
    double mean = n / vol * 4.18879020478639 * cutall * cutall * cutall;
    h->nl_pitch = h->dd_pitch = pitch_first(mean, 1.5);
  }
  if (h->sweep_kernel == 2) h->dd_pitch = ((h->dd_pitch + 255) / 256) * 256;  // whole 4-trip chunks (k_field_lp)
  // the lp / cluster index streams hold byte offsets j << 6 in 32-bit words: the record table must stay below 2^31 bytes
  if ((h->sweep_kernel == 2 || h->sweep_kernel == 3) && ((long long)n + 1) * (long long)sizeof(AtomRec) >= (1ll << 31))
    throw InputError("more than 2^25 atoms on one handle: the 32-bit record offsets of the sweep's index stream would wrap (shard the system)");
  h->d_nl_cnt.ensure(n + 1); h->d_dd_cnt.ensure(n + 1);
  h->d_nl_j.ensure((size_t)n * h->nl_pitch + 64);
  if (h->sweep_kernel < 3) h->d_dd_j.ensure((size_t)n * h->dd_pitch + 1024);  // slack: k_field_lp requests two index chunks per row up front
  else h->d_dd_j.ensure(64);
  // what the sweep streams per pair (3: k_field_lp, the index alone; 4: the dd lists are the clusters' union lists
  // (build_cluster_lists) or the tiles' (build_tiles))
  const int mode = h->stream_mode = stream_mode(h->cache_r2, h->sweep_kernel, h->dd_pairs, own_n(h), h->dd_pitch);
  const bool r2c = mode == 1;
  if (mode == 1) h->d_dd_r2.ensure((size_t)n * h->dd_pitch + 64);
  else if (mode == 0) h->d_dd_s.ensure((size_t)n * h->dd_pitch + 64);
  double *r2p = r2c ? h->d_dd_r2.p : nullptr;
  double2 *sp = mode == 0 ? h->d_dd_s.p : nullptr;
  bool fuse = mode != 0 && mode != 4;  // r^2 and padding written by k_nl_build (no k_dd_scalars pass)
#ifdef POLAR_LAB
  if (getenv("POLAR_NO_FUSE_R2")) fuse = false;
#endif
  const double cutallsq = cutall * cutall, ddsq = mode == 4 ? -1.0 : st.dd_cutoff * st.dd_cutoff;
  const int nr = own_n(h);
  const int *rows = own_rows(h);
  zero_many(s, {{h->d_nl_cnt.p, (size_t)(n + 1) * sizeof(int)}, {h->d_dd_cnt.p, (size_t)(n + 1) * sizeof(int)},
                {h->d_overflow.p, 16 * sizeof(int)}, {h->d_ddtot.p, 64 * 16 * sizeof(unsigned long long)}});
  const bool lp = mode == 3;
  if (lp) h->d_dd_wrap.ensure(n + 1);
  const bool recheck = h->colors_valid && h->colors_recheck && h->sweep_kernel < 3 && (int)h->h_color.size() == n;
  if (h->colors_recheck && !recheck) { h->colors_valid = false; h->colors_recheck = false; }
  if (recheck) {
    h->d_color_s.ensure(n + 1);
    k_color_map<<<nblk(n, 256), 256, 0, s>>>(n, h->d_perm.p, h->d_color_orig.p, h->d_color_s.p);
  }
  // the list build addresses the 32-byte position entries with 32-bit byte offsets
  if (((long long)n + 1) * (long long)sizeof(double4) >= (1ll << 32))
    throw InputError("more than 2^27 atoms on one handle: the 32-bit position offsets of the list build would wrap (shard the system)");
#define NLB3(TRI, RC, DENSE)                                                                                                  \
  k_nl_build<TRI, RC, DENSE><<<nblk(nr, POLAR_ROWS_PER_BLOCK), POLAR_BLOCK, 0, s>>>(                                          \
      rows, nr, h->d_pos4.p, h->box, g, h->d_cell_first.p, cutallsq, ddsq, h->nl_pitch, h->dd_pitch, h->d_nl_cnt.p,            \
      h->d_dd_cnt.p, h->d_nl_j.p, h->d_dd_j.p, fuse ? r2p : nullptr, fuse ? 1 : 0, lp ? (6 | (h->lp_quad_major << 8)) : 0,    \
      lp ? n : -1, lp ? h->d_dd_wrap.p : nullptr, recheck ? h->d_color_s.p : nullptr, h->color_keep * h->color_keep,           \
      h->d_overflow.p + 8, lp ? h->d_slot.p : nullptr, h->d_overflow.p, h->d_ddtot.p)
#ifdef POLAR_LAB
#define NLB(TRI, RC) do { if (h->nl_dense) NLB3(TRI, RC, true); else NLB3(TRI, RC, false); } while (0)
  h->nl_dense_used = h->nl_dense ? 1.0 : 0.0;
#else
#define NLB(TRI, RC) NLB3(TRI, RC, true)
#endif
  // the box shape and "colours are being re-validated" are compile-time: the kernel is bound by its vector instructions
  if (h->box.triclinic) { if (recheck) NLB(true, true); else NLB(true, false); }
  else                  { if (recheck) NLB(false, true); else NLB(false, false); }
#undef NLB
#undef NLB3
  const RowList ddl{h->d_dd_cnt.p, h->dd_pitch};
  if (fuse || mode == 4) {
    // modes 1 and 2: the list build wrote r^2 (mode 1) and the padding itself; mode 4: no per-atom dd rows at all
  }
#ifdef POLAR_LAB
  else if (st.damping_type == POLAR_DAMP_EXPONENTIAL)
    k_dd_scalars<0><<<nblk(nr, POLAR_ROWS_PER_BLOCK), POLAR_BLOCK, 0, s>>>(rows, nr, h->d_rec0.p, h->box, ddl, h->d_dd_j.p, st.polar_damp, sp, r2p);
  else
    k_dd_scalars<1><<<nblk(nr, POLAR_ROWS_PER_BLOCK), POLAR_BLOCK, 0, s>>>(rows, nr, h->d_rec0.p, h->box, ddl, h->d_dd_j.p, st.polar_damp, sp, r2p);
#endif
  // overflow flag and dd total come back with the end-of-step read (no sync here)
  HIPCHECK(hipMemcpyAsync(h->h_flags.p, h->d_overflow.p, sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHECK(hipMemcpyAsync(h->h_ddtot.p, h->d_ddtot.p, 64 * 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
}
template <bool AP>
static void launch_rank(polar_handle *h, int pass) {
  const int n = h->nlocal, ntot = h->nlocal + h->nghost;
  dim3 grid(nblk(n, POLAR_ROWS_PER_BLOCK)), block(POLAR_BLOCK);
  if (pass == 2) k_fold_scal<<<1, POLAR_NSLOT, 0, h->stream>>>(h->d_scal.p, h->d_slots.p, 1);
  // pass 1 of the all-pairs form: the partners of an atom over several waves while there are few atoms (a minimum: any order)
  const int nchunk = (AP && pass == 1) ? std::max(1, std::min(16, 8192 / std::max(n, 1))) : 1;
  if (pass == 1)
    k_rank<AP, 1><<<nblk((long long)n * nchunk, POLAR_ROWS_PER_BLOCK), block, 0, h->stream>>>(n, ntot, h->d_x.p, h->d_alpha.p, h->d_mol.p, h->box, RowList{h->d_nl_cnt.p, h->nl_pitch},
                                                 h->d_nl_j.p, h->d_rec0.p, h->d_mol_s.p, h->d_scal.p, h->d_slots.p, h->d_rank.p, nchunk);
  else
    k_rank<AP, 2><<<grid, block, 0, h->stream>>>(n, ntot, h->d_x.p, h->d_alpha.p, h->d_mol.p, h->box, RowList{h->d_nl_cnt.p, h->nl_pitch},
                                                 h->d_nl_j.p, h->d_rec0.p, h->d_mol_s.p, h->d_scal.p, h->d_slots.p, h->d_rank.p, 1);
}

void launch_rank_pass(polar_handle *h, bool allpairs, int pass) {
  if (allpairs) launch_rank<true>(h, pass); else launch_rank<false>(h, pass);
}

template <bool AP, int DAMP, int EP>
void launch_field(polar_handle *h, int nrows, const int *rows) {
  const polar_settings &st = h->ph.st;
  if (nrows <= 0) return;
  const int fb = h->field_block;  // threads per workgroup = 64 x rows that share one L1
  const size_t lds = AP ? 0 : (size_t)(fb / 64) * 64 * 5 * sizeof(double2);  // per-wave staging tiles (list mode)
  k_field<AP, DAMP, EP><<<nblk(nrows, fb / 64), fb, lds, h->stream>>>(
      nrows, rows, h->nlocal, h->d_rec0.p, h->d_rec1.p, h->box, RowList{h->d_dd_cnt.p, h->dd_pitch}, h->d_dd_j.p, h->d_dd_s.p,
      st.dd_cutoff * st.dd_cutoff, st.polar_damp, h->d_ef_s.p, h->d_F.p, h->d_scal.p, h->d_slots.p
#ifdef POLAR_LAB
      , h->ablate
#endif
      );
}
template <int EP>
void launch_field_dyn(polar_handle *h, bool ap, int nrows, const int *rows) {
  const bool expd = h->ph.st.damping_type == POLAR_DAMP_EXPONENTIAL;
  if (ap) { if (expd) launch_field<true, 0, EP>(h, nrows, rows); else launch_field<true, 1, EP>(h, nrows, rows); }
#ifdef POLAR_LAB
  else    { if (expd) launch_field<false, 0, EP>(h, nrows, rows); else launch_field<false, 1, EP>(h, nrows, rows); }
#else
  else throw std::logic_error("k_field's list branch exists in the lab build only");
#endif
}

#ifdef POLAR_LAB
#include "lab/launch_quad.inc"
#else
template <int EP> inline void launch_field_quad(polar_handle *, int, const int *) { throw std::logic_error("lab build only"); }
#endif  // POLAR_LAB

// list-mode sweep, lane-per-pair with LDS-DMA gathers (k_field_lp), one wave per row
// row descriptors of this step for k_field_lp: the colour phases back to back (GS), or the own rows (Jacobi)
void prepare_lp(polar_handle *h) {
  const polar_settings &st = h->ph.st;
  const bool gs = st.polar_gs || st.polar_gs_ranked;
  const int tot = gs ? (h->color_off.empty() ? 0 : h->color_off.back()) : own_n(h);
  h->d_lpdesc.ensure((size_t)tot + 1);
  h->lp_npart = 0;
  if (deterministic(h)) {  // one partial sum per 256 rows of every launch; launches are 256-aligned in the array
    h->d_lp_pend.ensure(4 * (size_t)tot + 4);
    const int nlaunch = gs ? (int)h->color_off.size() - 1 : 1;
    h->lp_npart = tot / 256 + nlaunch + 1;
    h->d_lp_part.ensure((size_t)h->lp_npart + 1);
    HIPCHECK(hipMemsetAsync(h->d_lp_part.p, 0, (size_t)h->lp_npart * sizeof(double), h->stream));
  }
  if (tot > 0)
    k_lp_desc<<<nblk(tot, 256), 256, 0, h->stream>>>(tot, gs ? h->d_rows.p : own_rows(h), RowList{h->d_dd_cnt.p, h->dd_pitch},
                                                     h->d_dd_wrap.p, h->d_lpdesc.p);
}
template <int EP>
void launch_field_lp(polar_handle *h, int nrows, const int2 *desc) {
  const long long row0 = desc - h->d_lpdesc.p;  // launch row of the first descriptor = its dd row
  if (nrows <= 0) return;
  const polar_settings &st = h->ph.st;
  const int qb = h->quad_block;
  const bool det = deterministic(h);
  const int nt = det ? 2 : h->lp_tiles;   // (the one-tile instance is a lab variant of the in-place sweep only: the LDS request must match the instance launched)
  size_t lds = (size_t)(qb / 64) * nt * POLAR_LP_TILE;
  if (h->lp_wg_per_cu > 0) lds = std::max(lds, std::min((size_t)64 * 1024, (size_t)160 * 1024 / h->lp_wg_per_cu));  // lab: cap the residency
  // the launch requests dynamic LDS without raising the kernel's limit: beyond 64 KB (workgroups of more than 512 threads
  // with two tiles per wave) it would fail, and the failure would only surface at the next read of the loop state
  if (lds > (size_t)64 * 1024) throw InputError("k_field_lp: workgroup size x tiles needs more than 64 KB of LDS (POLAR_QUAD_BLOCK <= 512 with two tiles)");
  const double omega = EP == EP_INPLACE ? st.polar_sor : 1.0;
#ifdef POLAR_LAB
#define POLAR_LAB_ARG , h->ablate
#else
#define POLAR_LAB_ARG
#endif
#define FL(D, NT, DT) k_field_lp<EP, D, NT, DT><<<nblk_xcd(nrows, qb / 64), qb, lds, h->stream>>>(                   \
      nrows, row0, desc, h->d_rec0.p, h->d_rec1.p, h->box, h->dd_pitch, h->d_dd_j.p,                               \
      st.polar_damp, make_expcoef(), h->d_ef_s.p, h->d_scal.p, h->d_slots.p, omega, h->d_lp_pend.p POLAR_LAB_ARG)
  const bool expd = st.damping_type == POLAR_DAMP_EXPONENTIAL;
#ifdef POLAR_LAB
#include "lab/launch_lpa.inc"
#endif
#ifdef POLAR_LAB
#include "lab/launch_lpr.inc"
#endif
  if (det) {
    if (expd) FL(0, 2, true); else FL(1, 2, true);
    // the launch only read the record table: its rows' new dipoles and the sum of their changes are folded in now
    // (launch `l` of the sweep starts at row0: its partial sums start at slot row0 / 256 + l -- disjoint for every launch)
    int launch_no = 0;
    if (EP == EP_INPLACE) while (launch_no + 1 < (int)h->color_off.size() && h->color_off[launch_no] < row0) launch_no++;
    k_lp_commit<<<nblk(nrows, 256), 256, 0, h->stream>>>(nrows, row0, desc, h->d_lp_pend.p, h->d_rec0.p, h->d_rec1.p, EP == EP_JACOBI ? 1 : 0,
                                                      h->d_scal.p, h->d_lp_part.p + row0 / 256 + launch_no);
  } else {
    if (expd) FL(0, 2, false); else FL(1, 2, false);
  }
#undef FL
#undef POLAR_LAB_ARG
}

#ifdef POLAR_LAB
#include "lab/launch_cluster_tile.inc"
#else
template <int EP> inline void launch_field_cl(polar_handle *, int, int) { throw std::logic_error("lab build only"); }
inline size_t tile_lds_bytes(int) { return 0; }
inline int tile_lds_cap() { return 0; }
inline void build_tiles(polar_handle *) { throw std::logic_error("lab build only"); }
template <int EP> inline void launch_field_tile(polar_handle *, const TileLaunch &) { throw std::logic_error("lab build only"); }
#endif  // POLAR_LAB

// one sweep over the rows this handle owns (Jacobi, or the colour phases)
#ifdef POLAR_LAB
#include "lab/build_units_paired_rows.inc"
#endif

void sweep_once(polar_handle *h, bool ap) {
  const polar_settings &st = h->ph.st;
  const bool gs = st.polar_gs || st.polar_gs_ranked;
  if (!ap && h->sweep_kernel == 4) {
    if (!gs) { launch_field_tile<EP_JACOBI>(h, h->tile_all); return; }
    const int ncol = (int)h->tile_launches.size();
    const int c0 = h->part_n > 1 ? ncol * h->part_k / h->part_n : 0, c1 = h->part_n > 1 ? ncol * (h->part_k + 1) / h->part_n : ncol;
    for (int c = c0; c < c1; c++) launch_field_tile<EP_INPLACE>(h, h->tile_launches[c]);  // (polar_step_sweep_part: a window of the tile colours)
    return;
  }
  if (!ap && h->sweep_kernel == 3) {
    const int ncol = (int)h->color_off.size() - 1;
    for (int c = 0; c < ncol; c++) {
      if (gs) launch_field_cl<EP_INPLACE>(h, h->color_off[c + 1] - h->color_off[c], h->color_off[c]);
      else launch_field_cl<EP_JACOBI>(h, h->color_off[c + 1] - h->color_off[c], h->color_off[c]);
    }
    return;
  }
#ifdef POLAR_LAB
  if (!ap && h->sweep_kernel == 2 && h->lp_pairs && !deterministic(h) && h->part_n <= 1) {
    if (!gs) { launch_field_lp2<EP_JACOBI>(h, 0); return; }
    for (int c = 0; c + 1 < (int)h->unit_off.size(); c++) launch_field_lp2<EP_INPLACE>(h, c);
    return;
  }
#endif
  if (!ap && h->sweep_kernel == 2) {
    if (!gs) { launch_field_lp<EP_JACOBI>(h, own_n(h), h->d_lpdesc.p); return; }
    const int ncol = (int)h->color_off.size() - 1;
    const int c0 = h->part_n > 1 ? ncol * h->part_k / h->part_n : 0, c1 = h->part_n > 1 ? ncol * (h->part_k + 1) / h->part_n : ncol;
    for (int c = c0; c < c1; c++)  // (polar_step_sweep_part: a window of the colour phases)
      launch_field_lp<EP_INPLACE>(h, h->color_off[c + 1] - h->color_off[c], h->d_lpdesc.p + h->color_off[c]);
    return;
  }
  if (!ap && h->sweep_kernel == 0) {
    if (!gs) { launch_field_quad<EP_JACOBI>(h, own_n(h), own_rows(h)); return; }
    const int ncol = (int)h->color_off.size() - 1;
    for (int c = 0; c < ncol; c++)
      launch_field_quad<EP_INPLACE>(h, h->color_off[c + 1] - h->color_off[c], h->d_rows.p + h->color_off[c]);
    return;
  }
  if (!gs) {
    launch_field_dyn<EP_JACOBI>(h, ap, own_n(h), own_rows(h));
    return;
  }
  const int ncol = (int)h->color_off.size() - 1;
  for (int c = 0; c < ncol; c++) {
    const int cnt = h->color_off[c + 1] - h->color_off[c];
    if (cnt <= 0) continue;
    launch_field_dyn<EP_INPLACE>(h, false, cnt, h->d_rows.p + h->color_off[c]);
  }
}

// one colour phase of the list-mode Gauss-Seidel (row sweep): part 0 = all its rows, 1 = its boundary rows (rows whose
// dipoles a peer of a multi-GPU run receives: they come first in the phase), 2 = its interior rows.  `deterministic yes`
// keeps a phase in one launch (its partial sums are laid out per launch): part 1 = everything, part 2 = nothing.
void sweep_phase(polar_handle *h, int c, int part) {
  const int ncol = (int)h->color_off.size() - 1;
  if (c < 0 || c >= ncol) throw std::logic_error("sweep_phase: no such colour");
  const int a = h->color_off[c], b = h->color_off[c + 1];
  const int m = (h->color_nsub == 2 && !deterministic(h)) ? h->color_sub[2 * c + 1] : b;
  const int lo = part == 2 ? m : a, hi = part == 1 ? m : b;
  launch_field_lp<EP_INPLACE>(h, hi - lo, h->d_lpdesc.p + lo);
}
template <bool AP, int DAMP>
void launch_force(polar_handle *h, int eflag, int vglobal, double *vatom, double *fdst) {
  const bool vpair = vglobal || vatom;
  const polar_settings &st = h->ph.st;
  dim3 grid(nblk(own_n(h), POLAR_ROWS_PER_BLOCK)), block(POLAR_BLOCK);
  const double ccs = st.cut_coul * st.cut_coul, dds = st.dd_cutoff * st.dd_cutoff, e2s = std::sqrt(h->P.qqrd2e);
  double *dbg6 = nullptr;   // `debug yes`: polarization force on the caller's atom 0 and its dipole-dipole part (PS.cpp:637-638)
  if (st.debug) {
    h->d_dbgf.ensure(8);
    HIPCHECK(hipMemsetAsync(h->d_dbgf.p, 0, 8 * sizeof(double), h->stream));
    dbg6 = h->d_dbgf.p;
  }
  const bool ew = ewald_on(h);
  const double g = h->P.g_ewald;
#ifdef POLAR_LAB
#define POLAR_LIT_ARG , h->force_literal
#else
#define POLAR_LIT_ARG
#endif
#define LF(E, V)                                                                                                    \
  if (ew) k_ew_polar_force<AP, DAMP, E, V><<<grid, block, 0, h->stream>>>(own_rows(h), own_n(h), h->sorted ? h->d_perm.p : nullptr, h->nlocal, h->d_scal.p, h->d_rec0.p, h->d_rec1.p,  \
                                                               h->d_mol_s.p, h->box, RowList{h->d_nl_cnt.p, h->nl_pitch}, h->d_nl_j.p,  \
                                                               ccs, dds, st.polar_damp, e2s, fdst, h->d_slots.p, vatom, vglobal, make_expcoef(),  \
                                                               dbg6, g, h->nl_inert POLAR_LIT_ARG);             \
  else k_polar_force<AP, DAMP, E, V><<<grid, block, 0, h->stream>>>(own_rows(h), own_n(h), h->sorted ? h->d_perm.p : nullptr, h->nlocal, h->d_scal.p, h->d_rec0.p, h->d_rec1.p,  \
                                                               h->d_mol_s.p, h->box, RowList{h->d_nl_cnt.p, h->nl_pitch}, h->d_nl_j.p,  \
                                                               ccs, dds, st.polar_damp, e2s, fdst, h->d_slots.p, vatom, vglobal, make_expcoef(),  \
                                                               dbg6, h->nl_inert POLAR_LIT_ARG)
  h->force_ran = true; h->force_listed = !AP; h->force_nrows = own_n(h);   // (polar_pair_extract "force_rows")
  if (eflag) { if (vpair) { LF(true, true); } else { LF(true, false); } }
  else       { if (vpair) { LF(false, true); } else { LF(false, false); } }
#undef LF
#undef POLAR_LIT_ARG
}

// ---- `polar_ewald <accuracy>`: the reciprocal-space half of the Ewald static field and of its forces (polar_ewald.hpp) ----
static_assert(sizeof(PlanD4) == sizeof(double4) && sizeof(PlanI4) == sizeof(int4), "polar_plan.hpp's vectors go to the device as bytes");

// the k-vector table (polar_plan.hpp) on the device; rebuilt when the box, g_ewald or the accuracy changed
void ewald_upload_kvectors(polar_handle *h) {
  const Box &b = h->box;
  const double g = h->P.g_ewald, acc = h->ph.st.polar_ewald;
  std::vector<double> key = {b.prd[0], b.prd[1], b.prd[2], b.xy, b.xz, b.yz, g, acc};
  if (key == h->ew_key) return;
  const EwaldPlan p = ewald_kvectors(b, g, acc);
  const auto &kv = p.kv; const auto &hkl = p.hkl; const auto &rows = p.rows;
  h->ew_nk = p.nk; h->ew_nrow = p.nrow; h->ew_nm = p.nm;
  std::copy(p.cell, p.cell + 6, h->ew_cell);
  h->d_ew_kv.ensure(kv.size() + 1); h->d_ew_hkl.ensure(hkl.size() + 1); h->d_ew_rows.ensure(rows.size());
  h->d_ew_s.ensure(kv.size() + 1); h->d_ew_m.ensure(kv.size() + 1);
  if (!kv.empty()) {
    HIPCHECK(hipMemcpyAsync(h->d_ew_kv.p, kv.data(), kv.size() * sizeof(double4), hipMemcpyHostToDevice, h->stream));
    HIPCHECK(hipMemcpyAsync(h->d_ew_hkl.p, hkl.data(), hkl.size() * sizeof(int4), hipMemcpyHostToDevice, h->stream));
  }
  HIPCHECK(hipMemcpyAsync(h->d_ew_rows.p, rows.data(), rows.size() * sizeof(int4), hipMemcpyHostToDevice, h->stream));
  HIPCHECK(hipStreamSynchronize(h->stream));  // (the host vectors go out of scope)
  h->ew_key = key;
}

// what the keyword is not offered with (POLAR_ERR_UNSUPPORTED); thrown before the step touches anything
void ewald_check(polar_handle *h, int vflag) {
  const polar_settings &st = h->ph.st;
  if (sharded(h)) throw Unsupported("polar_ewald needs one handle over all atoms: on a row-sharded handle the structure factors would need an all-reduce across the ranks");
  if (st.rccl_halo) throw Unsupported("polar_ewald is not offered with rccl_halo yes: the structure factors would need an all-reduce across the ranks");
  if (!(h->box.periodic[0] && h->box.periodic[1] && h->box.periodic[2])) throw Unsupported("polar_ewald needs a box periodic in x, y and z");
  if (vflag & 4) throw Unsupported("polar_ewald offers no per-atom virial (vflag & 4): the reciprocal-space virial has no pairwise definition");
  if (!(h->P.g_ewald > 0.0)) throw InputError("polar_ewald needs g_ewald > 0 (polar_pair_init / polar_set_coul)");
  ewald_upload_kvectors(h);   // (host work and a synchronous upload, when the box, g_ewald or the accuracy changed)
  if ((size_t)ewald_tile(h->ew_nm) * ewald_lds_per_atom(h->ew_nm) > 64 * 1024)
    throw Unsupported("polar_ewald: the k-vector range per box axis is too large for the structure-factor kernel (raise the accuracy value or g_ewald)");
}

bool ewald_short_box(const polar_handle *h) {
  double width[3];
  box_widths(h->box, width);
  return ewald_short_box(width, h->ph.st.cut_coul);
}

EwCell ew_cell(const polar_handle *h) {
  const double *c = h->ew_cell;
  return EwCell{c[0], c[1], c[2], c[3], c[4], c[5]};
}

// S(k) (mu = false) or M(k) (mu = true) of the n atoms of the s-space records -> out[nk]
void ewald_sfac(polar_handle *h, bool mu, double2 *out) {
  const int n = h->nlocal, nk = h->ew_nk, nm = h->ew_nm;
  if (nk == 0) return;
  const int tile = ewald_tile(nm);
  const size_t lds = (size_t)tile * ewald_lds_per_atom(nm);
  const SfacChunks ck = ewald_sfac_chunks(n, nk, tile);
  const int kb = ck.kb, nchunk = ck.nchunk, chunk = ck.chunk;
  h->d_ew_part.ensure((size_t)nchunk * nk);
  dim3 grid(kb, nchunk);
  if (mu) k_ew_sfac<true><<<grid, 256, lds, h->stream>>>(nk, h->d_ew_hkl.p, h->d_ew_kv.p, n, chunk, tile, nm, ew_cell(h), h->d_scal.p, h->d_rec0.p, h->d_rec1.p, h->d_ew_part.p);
  else    k_ew_sfac<false><<<grid, 256, lds, h->stream>>>(nk, h->d_ew_hkl.p, h->d_ew_kv.p, n, chunk, tile, nm, ew_cell(h), nullptr, h->d_rec0.p, h->d_rec1.p, h->d_ew_part.p);
  k_ew_fold<<<kb, 256, 0, h->stream>>>(nk, nchunk, h->d_ew_part.p, out);
}

// before the static-field kernel: S(k), then the reciprocal field of every atom into d_ew_erec (s space)
void ewald_field(polar_handle *h) {
  const int n = h->nlocal;
  HIPCHECK(hipEventRecord(h->ev_ks[0], h->stream));   // (the k-vector set is current: ewald_check)
  h->d_ew_erec.ensure(3 * (size_t)n + 3);
  ewald_sfac(h, false, h->d_ew_s.p);
  if (n > 0) {
    if (h->ew_nk > 0)
      k_ew_field<<<nblk(n, 256), 256, 0, h->stream>>>(n, h->ew_nrow, h->d_ew_rows.p, h->d_ew_kv.p, h->d_ew_s.p, ew_cell(h), std::sqrt(h->P.qqrd2e), h->d_rec0.p, h->d_ew_erec.p);
    else HIPCHECK(hipMemsetAsync(h->d_ew_erec.p, 0, 3 * (size_t)n * sizeof(double), h->stream));
  }
  HIPCHECK(hipEventRecord(h->ev_ks[1], h->stream));
}

// after the real-space forces (and the fdotr virial, which must not see these forces: the reciprocal virial has its own
// formula): M(k), the reciprocal forces into d_f, and [u_ef, virial[6]] into d_ew_out
void ewald_forces(polar_handle *h) {
  const int n = h->nlocal, nk = h->ew_nk;
  hipStream_t s = h->stream;
  HIPCHECK(hipEventRecord(h->ev_ks[2], s));
  ewald_sfac(h, true, h->d_ew_m.p);
  const int nba = nblk(std::max(n, 1), 256), nbk = nk > 0 ? nblk(nk, 256) : 0;
  h->d_ew_vpart.ensure(8 * (size_t)(nba + nbk)); h->d_ew_out.ensure(8);
  const double e2s = std::sqrt(h->P.qqrd2e), g = h->P.g_ewald;
  k_ew_force<<<nba, 256, 0, s>>>(n, nk > 0 ? h->ew_nrow : 0, h->d_ew_rows.p, h->d_ew_kv.p, h->d_ew_s.p, h->d_ew_m.p, ew_cell(h), e2s, h->d_scal.p,
                                 h->d_rec0.p, h->d_rec1.p, h->sorted ? h->d_perm.p : nullptr, h->d_ef_s.p, h->d_ew_erec.p, h->d_f.p, h->d_ew_vpart.p);
  if (nbk) k_ew_kvirial<<<nbk, 256, 0, s>>>(nk, h->d_ew_kv.p, h->d_ew_s.p, h->d_ew_m.p, e2s, 1.0 / (4.0 * g * g), h->d_ew_vpart.p + 8 * (size_t)nba);
  k_ew_finish<<<1, 256, 0, s>>>(nba + nbk, h->d_ew_vpart.p, h->d_ew_out.p);
  HIPCHECK(hipEventRecord(h->ev_ks[3], s));
}

void read_scal(polar_handle *h) {
  HIPCHECK(hipGetLastError());  // a failed kernel launch must not go unnoticed
  HIPCHECK(hipMemcpyAsync(h->h_scal.p, h->d_scal.p, sizeof(Scal), hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(hipStreamSynchronize(h->stream));
}
#ifdef POLAR_LAB
#include "lab/build_cluster_lists.inc"
#else
void build_cluster_lists(polar_handle *) { throw std::logic_error("lab build only"); }
#endif  // POLAR_LAB
// `debug yes` (PS.cpp:1182-1191): u_polar after sweep `sw`, kept on the device until polar_get_debug_trace
void debug_trace(polar_handle *h, int sw) {
  if (!h->ph.st.debug) return;
  h->d_trace.ensure((size_t)h->ph.st.iterations_max + 8);
  if (sw > h->ph.st.iterations_max + 1) return;
  const MuView mv = mu_view(h);
  k_debug_upolar<<<1, 1024, 0, h->stream>>>(h->nlocal, h->d_scal.p, mv.a, mv.b, mv.stride, h->d_ef_s.p, h->d_trace.p, sw, 0);  // Jacobi: like the reference, the value is formed BEFORE "mu = mu_new"
  h->ntrace = sw + 1;
}

// `polar_accel m` (extension keyword): Anderson mixing of depth m on the sweep map of the list-mode Gauss-Seidel
// (kernels and formulas: polar_accel.hpp, k_accel_*).  accel_begin: buffers, x_0 = the initial guess of the own rows; returns
// whether the keyword applies to this solve.  accel_step: after a sweep (and its end-of-sweep decision) -- differences and
// their dot products, the m x m solve, the mixed iterate into the records.  `global_dots`: multi-GPU, the all-reduced dot
// products in device memory ([2 * POLAR_ACCEL_MAXM] doubles); the local ones are then exported first (accel_export).
bool accel_begin(polar_handle *h, bool ap) {
  const polar_settings &st = h->ph.st;
  const bool gs = st.polar_gs || st.polar_gs_ranked;
  if (st.polar_accel <= 0) return false;
  if (ap || !gs || h->sweep_kernel != 2) throw InputError("polar_accel needs the Gauss-Seidel sweep of list mode (dd_cutoff > 0 with polar_gs or polar_gs_ranked)");
  if (deterministic(h)) throw InputError("polar_accel and `deterministic yes` exclude each other");
  const int tot = h->color_off.empty() ? 0 : h->color_off.back();
  const long long pitch = ((long long)tot + 255) / 256 * 256;
  const int M = POLAR_ACCEL_MAXM;
  h->acc_pitch = pitch; h->acc_rows = tot;
  const bool fresh = h->d_acc_dF.cap < (size_t)M * 3 * pitch + 1;
  h->d_acc_x.ensure(3 * pitch + 1); h->d_acc_f.ensure(3 * pitch + 1); h->d_acc_g.ensure(3 * pitch + 1);
  h->d_acc_dF.ensure((size_t)M * 3 * pitch + 1); h->d_acc_dG.ensure((size_t)M * 3 * pitch + 1);
  h->d_acc_part.ensure((size_t)2 * M * nblk(tot, 256) + 2 * M); h->d_acc_state.ensure(1);
  if (fresh) {  // (slots outside the window are multiplied by zero, never skipped: no NaN may sit there)
    HIPCHECK(hipMemsetAsync(h->d_acc_dF.p, 0, h->d_acc_dF.cap * sizeof(double), h->stream));
    HIPCHECK(hipMemsetAsync(h->d_acc_dG.p, 0, h->d_acc_dG.cap * sizeof(double), h->stream));
  }
  k_accel_init<<<nblk(tot, 256), 256, 0, h->stream>>>(tot, pitch, h->d_lpdesc.p, h->d_rec0.p, h->d_acc_x.p, h->d_acc_state.p);
  return true;
}
// the two launches over the own rows that the forms of the mixing share: differences and their partial dot products
// (launch_accel_diff); the mixed iterate into the records (launch_accel_mix)
static void launch_accel_diff(polar_handle *h, int tot, int nb, int ring) {
  k_accel_diff<POLAR_ACCEL_MAXM><<<nb, 256, 0, h->stream>>>(tot, h->acc_pitch, h->d_lpdesc.p, h->d_rec0.p, h->d_scal.p, h->d_acc_state.p, h->d_acc_x.p,
                                                           h->d_acc_f.p, h->d_acc_g.p, h->d_acc_dF.p, h->d_acc_dG.p, h->d_acc_part.p, ring);
}
static void launch_accel_mix(polar_handle *h, int tot, int nb);   // (defined after its callers: the kernels keep their order in the code object)
void accel_export(polar_handle *h, double *dev_local_dots) {
  const int tot = h->acc_rows, nb = nblk(tot, 256), ring = std::min(h->ph.st.polar_accel, POLAR_ACCEL_MAXM);
  launch_accel_diff(h, tot, nb, ring);
  k_accel_solve<POLAR_ACCEL_MAXM><<<1, 256, 0, h->stream>>>(nb, h->d_acc_part.p, h->d_scal.p, h->d_acc_state.p, dev_local_dots, nullptr, ring);
}
// Round 5, precision mode: the single-workgroup launches around the mixing folded together (polar_accel.hpp).
// accel_export_fused: differences + partial dots, then this rank's sum (dmu)^2 into ared[0] and its dot products into ared[1 ..]
// (multi-GPU, before the all-reduce).  accel_decide_mix: the end-of-sweep decision -- on ared[0] if given -- and the mixing
// coefficients in one launch, then the mix; `diff_first`: single handle, where nothing has formed the differences yet.
void accel_export_fused(polar_handle *h, double *ared) {
  const int tot = h->acc_rows, nb = nblk(tot, 256), ring = std::min(h->ph.st.polar_accel, POLAR_ACCEL_MAXM);
  launch_accel_diff(h, tot, nb, ring);
  k_accel_export<POLAR_ACCEL_MAXM><<<1, POLAR_NSLOT, 0, h->stream>>>(h->d_scal.p, h->d_slots.p, ared, 1, nb, h->d_acc_part.p, h->d_acc_state.p, ring);
}
void accel_decide_mix(polar_handle *h, const double *ared, bool diff_first) {
  const polar_settings &st = h->ph.st;
  const int tot = h->acc_rows, nb = nblk(tot, 256), ring = std::min(st.polar_accel, POLAR_ACCEL_MAXM);
  if (diff_first) launch_accel_diff(h, tot, nb, ring);
  k_solver_accel<POLAR_ACCEL_MAXM><<<1, POLAR_NSLOT, 0, h->stream>>>(h->d_scal.p, h->d_slots.p, norm_count(h), st.iterations_max, st.polar_precision, ared, 1, nb,
                                                                     h->d_acc_part.p, h->d_acc_state.p, ring);
  launch_accel_mix(h, tot, nb);
}
void accel_step(polar_handle *h, const double *global_dots) {
  const int tot = h->acc_rows, nb = nblk(tot, 256), ring = std::min(h->ph.st.polar_accel, POLAR_ACCEL_MAXM);
  if (!global_dots) launch_accel_diff(h, tot, nb, ring);
  k_accel_solve<POLAR_ACCEL_MAXM><<<1, 256, 0, h->stream>>>(nb, h->d_acc_part.p, h->d_scal.p, h->d_acc_state.p, nullptr, global_dots, ring);
  launch_accel_mix(h, tot, nb);
}
static void launch_accel_mix(polar_handle *h, int tot, int nb) {
  k_accel_mix<POLAR_ACCEL_MAXM><<<nb, 256, 0, h->stream>>>(tot, h->acc_pitch, h->d_lpdesc.p, h->d_rec0.p, h->d_scal.p, h->d_acc_state.p, h->d_acc_x.p,
                                                          h->d_acc_g.p, h->d_acc_dG.p);
}

// end of a sweep in solve(): where the host is due a look at the device-resident loop state (look_at_state; never in a
// fixed-iteration run) it reads it; true = the stop rule has fired
static bool sweep_stops(polar_handle *h, int sw, int check_every) {
  if (h->ph.st.fixed_iteration || !look_at_state(h->last_sweeps, sw, check_every)) return false;
  read_scal(h);
  return h->h_scal.p->done != 0;
}
void launch_solver_step(polar_handle *h, const double *global_change, int count, const double *part, int npart) {
  const polar_settings &st = h->ph.st;
  k_solver_step<<<1, POLAR_NSLOT, 0, h->stream>>>(h->d_scal.p, h->d_slots.p, norm_count(h), st.fixed_iteration, st.iterations_max, st.polar_precision,
                                                  (st.polar_gs || st.polar_gs_ranked) ? 0 : 1, global_change, count, part, npart);
}

void solve(polar_handle *h, bool ap, polar_result *out) {
  const polar_settings &st = h->ph.st;
  const int n = h->nlocal;
  hipStream_t s = h->stream;
  const bool gs = st.polar_gs || st.polar_gs_ranked;
  const bool expd = st.damping_type == POLAR_DAMP_EXPONENTIAL;
  const int max_sweeps = st.iterations_max + 1;
  const int check_every = 4;
  out->ncolors = 0;
  if (st.polar_accel > 0 && (ap || !gs)) throw InputError("polar_accel needs the Gauss-Seidel sweep of list mode (dd_cutoff > 0 with polar_gs or polar_gs_ranked)");

  if (!gs || !ap) {  // Jacobi (reference "polar_gs no") or colour-phase Gauss-Seidel over the dd list
    const bool clm = !ap && h->sweep_kernel == 3, tile = !ap && h->sweep_kernel == 4;  // tile sweep: no host-side colours at all
    if (!ap && !tile) resolve_colors(h);
    if (!tile && (gs || clm) && !h->colors_valid) { ensure_colors(h); if (clm) build_cluster_lists(h); else map_color_rows(h); }
    if (!ap && gs && h->sweep_kernel == 2 && !slots_current(h)) { compute_slots(h); build_lists(h); }  // rows into launch order
    if (gs) out->ncolors = tile ? (int)h->tile_launches.size() : (int)h->color_off.size() - 1;
    if (!ap && h->sweep_kernel == 2) prepare_lp(h);
#ifdef POLAR_LAB
    if (!ap && h->sweep_kernel == 2 && h->lp_pairs && !deterministic(h)) build_units(h);
#endif
    const bool accel = accel_begin(h, ap);   // `polar_accel m`: Anderson mixing between the sweeps
    for (int sw = 0; sw < max_sweeps; sw++) {
      sweep_once(h, ap);
      debug_trace(h, sw);
      const SweepEnd e = sweep_end(sw, max_sweeps, st.fixed_iteration != 0, gs, accel, 0);
      if (e.mix && e.decide_in_mix) accel_decide_mix(h, nullptr, true);   // differences, [decision + coefficients], mix: the mix is a no-op once the stop rule has fired (the result is G(x_k) of the last sweep)
      else if (e.mix) accel_step(h, nullptr);   // (fixed-iteration GS: no decision to wait for; nothing after the last sweep)
      if (e.count > 0) launch_solver_step(h, nullptr, e.count);
      if (sweep_stops(h, sw, check_every)) break;
    }
  } else if (h->dense_gs) {  // exact-order blocked Gauss-Seidel on the HBM-resident tensor
    const long long np = ((long long)n + 63) / 64 * 64;   // row pitch of the component-major tensor
    h->d_T6.ensure((size_t)n * 6 * np + 64);
    if (expd) k_build_T6<0><<<nblk(n, POLAR_ROWS_PER_BLOCK), POLAR_BLOCK, 0, s>>>(n, np, h->d_rec0.p, h->box, st.polar_damp, h->d_T6.p);
    else      k_build_T6<1><<<nblk(n, POLAR_ROWS_PER_BLOCK), POLAR_BLOCK, 0, s>>>(n, np, h->d_rec0.p, h->box, st.polar_damp, h->d_T6.p);
    k_dense_field<<<nblk(n, POLAR_ROWS_PER_BLOCK), POLAR_BLOCK, 0, s>>>(n, np, h->d_T6.p, h->d_rec0.p, h->d_F.p);
    // ONE launch per block of B atoms, nothing sequential inside it: d = G cb - N d' (polar_exact.hpp, k_gs_blk).  G and N
    // are formed here, once per step.
    const int B = dense_gs_block(n), R = 3 * B, nb = (n + B - 1) / B;
    const size_t RR = (size_t)R * R;
    h->d_Minv.ensure(nb * RR); h->d_gsN.ensure(nb * RR); h->d_gsAT.ensure(nb * RR); h->d_cb.ensure(3 * (size_t)n + 3);
    h->d_dmu.ensure(2 * (size_t)R + 8);
    if (B > 64) HIPCHECK(hipMemsetAsync(h->d_Minv.p, 0, nb * RR * sizeof(double), s));   // (what lies right of the diagonal pieces)
    k_gs_blockinv<<<nb * (B / 64) * (POLAR_GS64 / POLAR_GSB_COLS), 64, 0, s>>>(n, np, h->d_T6.p, h->d_rec0.p, h->d_Minv.p, R, (long long)RR, B / 64);
    for (int m = 64; m < B; m *= 2) {
      // two triangles of m atoms side by side on G's diagonal become one of 2 m: G = [[G1, 0], [-G2 (A T21) G1, G2]];
      // Y = (A T21) G1, then the piece below G1 = -G2 Y.  All pairs of all blocks in one batch.
      const int per = B / (2 * m), nz = nb * per, q = 3 * m;
      const long long inner = (long long)2 * q * (R + 1), qq = (long long)q * q;
      double *AT21 = h->d_gsAT.p, *Y = h->d_gsN.p;   // (scratch here; filled for good below)
      const GsBatch dense{qq, 0, 1}, diag{(long long)RR, inner, per};
      k_gs_expand<<<dim3(m / 64, m / 4, nz), 256, 0, s>>>(n, np, h->d_T6.p, h->d_rec0.p, B, nb, 1, m, AT21, q, qq);
      k_gs_gemm<false><<<dim3(q / 64, q / 64, nz), 256, 0, s>>>(q, 1.0, AT21, q, dense, h->d_Minv.p, R, diag, Y, q, dense);
      k_gs_gemm<true><<<dim3(q / 64, q / 64, nz), 256, 0, s>>>(q, -1.0, h->d_Minv.p + (size_t)q * (R + 1), R, diag, Y, q, dense, h->d_Minv.p + (size_t)q * R, R, diag);
    }
    const GsBatch whole{(long long)RR, 0, 1};
    k_gs_expand<<<dim3(B / 64, B / 4, nb), 256, 0, s>>>(n, np, h->d_T6.p, h->d_rec0.p, B, nb, 0, B, h->d_gsAT.p, R, (long long)RR);
    k_gs_gemm<true><<<dim3(R / 64, R / 64, nb), 256, 0, s>>>(R, 1.0, h->d_Minv.p, R, whole, h->d_gsAT.p, R, whole, h->d_gsN.p, R, whole);
    k_gs_cb_init<<<nblk(n, 256), 256, 0, s>>>(n, h->d_rec0.p, h->d_ef_s.p, h->d_F.p, h->d_cb.p);
    int prev = -1, flip = 0;
    const int grid = R / POLAR_GS_WAVES + nblk(n, POLAR_GS_WAVES), npart = nb * (R / POLAR_GS_WAVES);
    h->d_gs_part.ensure((size_t)npart + 1);
    HIPCHECK(hipMemsetAsync(h->d_gs_part.p, 0, (size_t)npart * sizeof(double), s));
    // the sweep's last launch carries the end-of-sweep logic (GsTail) unless something has to happen between the two (`debug yes`)
    const bool tail_on = !st.debug;
    if (tail_on && !h->d_gs_cnt.p) { h->d_gs_cnt.ensure(8); HIPCHECK(hipMemsetAsync(h->d_gs_cnt.p, 0, 8 * sizeof(int), s)); }
    for (int sw = 0; sw < max_sweeps; sw++) {
      for (int b0 = 0; b0 < n; b0 += B) {
        const int next0 = b0 + B < n ? b0 + B : 0;
        const GsTail tail = (tail_on && b0 + B >= n) ? GsTail{h->d_gs_cnt.p, npart, norm_count(h), st.fixed_iteration, st.iterations_max, st.polar_precision}
                                                     : GsTail{nullptr, 0, 0, 0, 0, 0.0};
#define POLAR_GS_BLK(BB) k_gs_blk<BB><<<grid, 64 * POLAR_GS_WAVES, 0, s>>>(n, np, b0, prev, next0, h->d_T6.p, h->d_Minv.p, h->d_gsN.p, h->d_rec0.p, h->d_ef_s.p, h->d_F.p, h->d_cb.p, \
                                                            h->d_dmu.p + R * flip, h->d_dmu.p + R * (flip ^ 1), h->d_scal.p, h->d_gs_part.p, tail)
        if (B == 256) POLAR_GS_BLK(256); else if (B == 128) POLAR_GS_BLK(128); else POLAR_GS_BLK(64);
#undef POLAR_GS_BLK
        prev = b0; flip ^= 1;
      }
      debug_trace(h, sw);
      if (!tail_on) launch_solver_step(h, nullptr, 1, h->d_gs_part.p, npart);
      if (sweep_stops(h, sw, check_every)) break;
    }
  } else {  // exact-order blocked Gauss-Seidel, matrix-free (systems whose tensor does not fit)
    std::vector<int> order(n), pos(n);
    std::iota(order.begin(), order.end(), 0);
    if (st.polar_gs_ranked) {  // stable descending sort == the reference's bubble sort (PS.cpp:1130-1143)
      std::vector<double> rk(n);
      HIPCHECK(hipMemcpyAsync(rk.data(), h->d_rank.p, n * sizeof(double), hipMemcpyDeviceToHost, s));
      HIPCHECK(hipStreamSynchronize(s));
      std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return rk[a] > rk[b]; });
    }
    for (int k = 0; k < n; k++) pos[order[k]] = k;
    h->d_order.ensure(n); h->d_pos.ensure(n); h->d_dmu.ensure(3 * 64);
    HIPCHECK(hipMemcpyAsync(h->d_order.p, order.data(), n * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(h->d_pos.p, pos.data(), n * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHECK(hipStreamSynchronize(s));  // order/pos are stack vectors
    launch_field_dyn<EP_FIELD>(h, true, n, nullptr);
    for (int sw = 0; sw < max_sweeps; sw++) {
      for (int b0 = 0; b0 < n; b0 += 64) {
        if (expd) {
          k_gs_block_seq<0><<<1, 64, 0, s>>>(n, b0, h->d_order.p, h->d_rec0.p, h->box, st.polar_damp, h->d_ef_s.p, h->d_F.p, h->d_dmu.p, h->d_scal.p, h->d_slots.p);
          k_gs_block_push<0><<<nblk(n, POLAR_ROWS_PER_BLOCK), POLAR_BLOCK, 0, s>>>(n, b0, h->d_order.p, h->d_pos.p, h->d_rec0.p, h->box, st.polar_damp, h->d_dmu.p, h->d_F.p, h->d_scal.p);
        } else {
          k_gs_block_seq<1><<<1, 64, 0, s>>>(n, b0, h->d_order.p, h->d_rec0.p, h->box, st.polar_damp, h->d_ef_s.p, h->d_F.p, h->d_dmu.p, h->d_scal.p, h->d_slots.p);
          k_gs_block_push<1><<<nblk(n, POLAR_ROWS_PER_BLOCK), POLAR_BLOCK, 0, s>>>(n, b0, h->d_order.p, h->d_pos.p, h->d_rec0.p, h->box, st.polar_damp, h->d_dmu.p, h->d_F.p, h->d_scal.p);
        }
      }
      debug_trace(h, sw);
      launch_solver_step(h, nullptr, 1, nullptr, 0);
      if (sweep_stops(h, sw, check_every)) break;
    }
  }
}

// PS.cpp:125-386: everything before the solve
void phase_begin(polar_handle *h, int eflag, int vflag, const double *mu_host) {
  need_device(h);
  h->field_ready = false;   // (polar_field_at: the records are being rewritten until the step has finished)
  h->d_fa_x.release(); h->d_fa_idx.release(); h->d_fa_out.release();   // a probe's pass buffers (100 bytes per point) do not outlive the step it looked at
  h->d_fa_part.release(); h->ew_q_valid = false;   // (polar_ewald_field_at: its chunk partials; the charges may be other ones)
  h->d_eg_tab.release(); h->d_eg_t.release(); h->d_eg_v.release(); h->d_eg_first.release();   // (polar_ewald_field_grid: tables, T, V)
  h->d_pr_qa.release(); h->d_pr_type.release(); h->d_pr_out.release(); h->d_pr_type_s.release(); h->pr_types_valid = false;   // (polar_probe_at: sites, results, the records' types)
  h->d_fg_out.release();   // (polar_field_grad_at)
  if (!h->types_set || !h->coul_set) throw std::runtime_error("polar_compute before the pair tables were set: polar_pair_init (or polar_set_types), then polar_set_coul with the Coulomb tables of Pair::init_tables unless pair_modify table 0");
  if (!h->box_set || !h->atoms_set || !h->neigh_set) throw std::runtime_error("polar_compute before polar_set_box/polar_set_atoms/polar_set_neighbors");
  const polar_settings &st = h->ph.st;
  const int n = h->nlocal, nall = h->nlocal + h->nghost;
  const bool ap = !(st.dd_cutoff > 0.0);
  if (ap && own_n(h) != n) throw InputError("row sharding needs dd_cutoff > 0 (exact all-pairs mode runs as replicas only)");
  if (!ap && h->box.triclinic && !(h->sweep_kernel == 4 || (h->sweep_kernel == 2 && h->lp_depth == 0)))
    throw InputError("dd_cutoff (list) mode in a triclinic box needs the row sweep (k_field_lp) or, in the lab build, the tile sweep");
  if (ewald_on(h)) ewald_check(h, vflag);
  const int vmode = vflag % 4;
  hipStream_t s = h->stream;
  h->warn.clear();
  if (ewald_on(h) && ewald_short_box(h))
    h->warn = "polar_ewald: cut_coul exceeds half a box width, and the real-space sum takes the minimum image only: the field is "
              "the Ewald field only where erfc(g_ewald * half the box width) is negligible";
  h->ntrace = 0;
  h->step_eflag = eflag; h->step_vflag = vflag;

  h->d_f.ensure(3 * (size_t)nall); h->d_ef.ensure(3 * (size_t)n); h->d_F.ensure(3 * (size_t)n);
  h->d_mu.ensure(3 * (size_t)n); h->d_rank.ensure(n); h->d_rec0.ensure(n + 1); h->d_rec1.ensure(n + 1);  // + the dummy record
  h->d_ef_s.ensure(3 * (size_t)n); h->d_mol_s.ensure(n + 1);
  HIPCHECK(hipEventRecord(h->ev[0], s));
  HIPCHECK(hipMemsetAsync(h->d_f.p, 0, 3 * (size_t)nall * sizeof(double), s));
  // per-atom tallies (eflag/2, vflag/4: src/pair.cpp:760-764), zeroed like ev_setup does (:789-806)
  double *eatom = nullptr, *vatom = nullptr;
  if (eflag / 2) { h->d_eatom.ensure(nall + 1); eatom = h->d_eatom.p; HIPCHECK(hipMemsetAsync(eatom, 0, (size_t)nall * sizeof(double), s)); }
  if (vflag / 4) { h->d_vatom.ensure(6 * (size_t)nall + 6); vatom = h->d_vatom.p; HIPCHECK(hipMemsetAsync(vatom, 0, 6 * (size_t)nall * sizeof(double), s)); }
  // (on a row-sharded handle every kernel tallies into the rows it walks -- half of each pair per row atom -- so the
  //  shards' arrays add up to the unsharded ones: LJ/Coulomb over the rows of the list the shard was given, polarization
  //  over the own rows)
  k_zero_slots<<<nblk(POLAR_NSLOT, 256), 256, 0, s>>>(h->d_slots.p, h->d_scal.p);
  auto launch_lj = [&]() {  // a3 -- on a low-priority side stream when overlap is on: it depends on nothing below, and fills
    // whatever the list build, the static field and the latency-bound solver launches leave idle
    hipStream_t ms = s;
    h->lj_forked = h->overlap_lj && h->inum > 0;
    if (h->lj_forked) {
      HIPCHECK(hipEventRecord(h->ev_fork, ms));
      HIPCHECK(hipStreamWaitEvent(h->lj_stream, h->ev_fork, 0));
    }
    hipStream_t s = h->lj_forked ? h->lj_stream : ms;  // shadows the main stream inside this block
    if (h->list_up_pending) {   // the uploaded list may still be on its way (upload_neighbor_rows returns before its transfer has ended)
      HIPCHECK(hipStreamWaitEvent(s, h->ev_list_up, 0));   // (every step until the next list: free once the event has fired)
    }
    HIPCHECK(hipEventRecord(h->ev_lj0, s));
    LJCoulParams P = h->P;
    P.newton_pair = h->newton_pair; P.nlocal = n; P.cut_coulsq = st.cut_coul * st.cut_coul; P.full_list = h->full_list; P.ablate = 0;
    h->d_xq.ensure(nall + 1);
    const size_t ljlds = (size_t)(h->ntypes + 1) * (h->ntypes + 1) * 8 * sizeof(double);
    if (ljlds > 64 * 1024) throw InputError("too many atom types for the LDS-resident LJ table (max 31)");
    dim3 block(POLAR_BLOCK);
    bool symmetrise = !h->full_list;
#ifdef POLAR_LAB
    if (getenv("POLAR_LJ_ATOMICS")) symmetrise = false;  // round 1's FP64 atomics on f[j]
#endif
    // A full (newton-off) list puts no force on ghosts, so sum f.x over locals+ghosts (fdotr) would miss
    // the image terms: the LJ/Coulomb virial is then tallied pairwise (the same number), and only the
    // polarization forces -- local atoms, minimum-image displacements -- go through f.x (phase_finish)
    const bool lj_pairwise_virial = h->full_list && vmode == 2;
    if ((eatom || vatom) && !symmetrise && !h->full_list) throw InputError("per-atom tallies need the row-complete pair list");
    const bool sym_build = symmetrise && !h->sym_valid && h->inum > 0;
    // Between two builds of the symmetrised list its rows keep the distance classes and the positions they were made from
    // (polar_skin.hpp): the pack folds the largest displacement since into one device scalar, which never reaches the host
    const bool skin_kept = symmetrise && !sym_build && h->sym_valid && h->skin_valid && h->skin_nall == nall;
    if (skin_kept && h->lj_skin) {
      HIPCHECK(hipMemsetAsync(h->d_lj_drift.p, 0, sizeof(unsigned long long), s));
      k_pack_lj<<<nblk(nall, 256), 256, 0, s>>>(nall, h->d_x.p, h->d_q.p, h->d_xq.p, h->d_xq_snap.p, h->d_lj_drift.p);
    } else k_pack_lj<<<nblk(nall, 256), 256, 0, s>>>(nall, h->d_x.p, h->d_q.p, h->d_xq.p, nullptr, nullptr);
    if (sym_build) {  // once per uploaded list (reneighbor steps)
      dim3 g0(nblk(h->inum, POLAR_ROWS_PER_BLOCK));
      // POLAR_LJ_SKIN=0: one class -- the rows, and the cost of this build, as they were before the distance classes
      const int nclass = h->lj_skin ? SKIN_CLASSES : 1;
      const size_t nk = (size_t)nall * nclass;   // (row, class) pairs
      h->d_sym_cnt.ensure(nk + 4); h->d_sym_fill.ensure(nk + 4); h->d_sym_cfirst.ensure(nk + 2); h->d_sym_first.ensure(nall + 2);
      h->d_sym_j.ensure(2 * (size_t)h->nneigh + 64);
      if (h->lj_skin) {
        h->d_sym_cend.ensure(nk + 1); h->d_lj_walk.ensure(nall + 1); h->d_sym_cls.ensure((size_t)h->nneigh + 64);
        h->d_xq_snap.ensure(nall + 1); h->d_lj_drift.ensure(2);
      }
      HIPCHECK(hipMemsetAsync(h->d_sym_cnt.p, 0, (nk + 4) * sizeof(int), s));
      HIPCHECK(hipMemsetAsync(h->d_sym_fill.p, 0, (nk + 4) * sizeof(int), s));
      h->sym_typed = h->lj_typed && nall < (1 << 24) && h->ntypes < 64;
      const int *ty = h->sym_typed ? h->d_type.p : nullptr;
      if (h->lj_skin) {
        k_sym_count<SKIN_CLASSES><<<g0, block, 0, s>>>(h->inum, h->d_ilist.p, h->d_numneigh.p, h->d_first.p, h->d_neigh.p, h->d_xq.p, h->r_cmax,
                                                     h->d_sym_cnt.p, h->d_sym_cls.p, h->d_sym_fill.p);
        launch_scan((long long)nk, h->d_sym_cnt.p, h->d_sym_cfirst.p, h->d_scan_b, s);
        k_sym_ends<SKIN_CLASSES><<<nblk(nall + 1, 256), 256, 0, s>>>(nall, h->d_sym_cfirst.p, h->d_sym_first.p, h->d_sym_cend.p);
        k_sym_fill<SKIN_CLASSES><<<g0, block, 0, s>>>(h->inum, h->d_ilist.p, h->d_numneigh.p, h->d_first.p, h->d_neigh.p, h->d_sym_cfirst.p,
                                                    h->d_sym_fill.p, h->d_sym_j.p, ty, h->d_sym_cls.p);
        // the snapshot the drift is measured from: the records the classes were made from (no displacement yet)
        HIPCHECK(hipMemcpyAsync(h->d_xq_snap.p, h->d_xq.p, (size_t)nall * sizeof(double4), hipMemcpyDeviceToDevice, s));
        HIPCHECK(hipMemsetAsync(h->d_lj_drift.p, 0, sizeof(unsigned long long), s));
      } else {
        k_sym_count<1><<<g0, block, 0, s>>>(h->inum, h->d_ilist.p, h->d_numneigh.p, h->d_first.p, h->d_neigh.p, nullptr, 0.0,
                                          h->d_sym_cnt.p, nullptr, h->d_sym_fill.p);
        launch_scan((long long)nk, h->d_sym_cnt.p, h->d_sym_cfirst.p, h->d_scan_b, s);
        k_sym_ends<1><<<nblk(nall + 1, 256), 256, 0, s>>>(nall, h->d_sym_cfirst.p, h->d_sym_first.p, nullptr);
        k_sym_fill<1><<<g0, block, 0, s>>>(h->inum, h->d_ilist.p, h->d_numneigh.p, h->d_first.p, h->d_neigh.p, h->d_sym_cfirst.p,
                                         h->d_sym_fill.p, h->d_sym_j.p, ty, nullptr);
      }
      h->sym_valid = true; h->skin_valid = h->lj_skin != 0; h->skin_nall = nall;
    }
    // newton off: ghosts receive no force and tally nothing (PS.cpp:293, ev_tally's 0.5 per LOCAL atom), so only the
    // local rows of the symmetrised list are walked: a local-ghost pair then counts 0.5, a local-local pair 0.5 + 0.5
    const int nrows_lj = symmetrise ? (h->newton_pair ? nall : n) : h->inum;
    dim3 grid(nblk(nrows_lj, POLAR_ROWS_PER_BLOCK));
    if (symmetrise) P.full_list = 1;  // rows of the symmetrised list: force on the row atom only, tallies halved
    P.typed_list = symmetrise ? (h->sym_typed ? 1 : 0) : (h->device_list && h->dev_typed ? 1 : 0);
    // a row of the symmetrised list is walked up to the end of the last class the drift can have brought inside a cutoff
    // (k_lj_walk; the force loop takes the length as a row's numneigh); POLAR_LJ_SKIN=0, or classes that no longer belong to
    // the atoms: the whole row
    const bool walk = (sym_build || skin_kept) && h->lj_skin && h->skin_valid && h->inum > 0;
    if (walk) k_lj_walk<<<nblk(nall, 256), 256, 0, s>>>(nall, h->d_sym_cend.p, h->d_lj_drift.p, h->r_cmax, h->d_lj_walk.p);
    h->lj_sym_last = symmetrise; h->lj_walk_last = walk; h->lj_rows_last = nrows_lj; h->lj_ran = h->inum > 0;
    const int *il = symmetrise ? nullptr : h->d_ilist.p;
    const int *nn = symmetrise ? (walk ? h->d_lj_walk.p : nullptr) : h->d_numneigh.p;
    const long long *fi = symmetrise ? h->d_sym_first.p : h->d_first.p;
    const int *nj = symmetrise ? h->d_sym_j.p : h->d_neigh.p;
    if (h->inum > 0) {
      const bool vrow = vmode == 1 || vatom || lj_pairwise_virial;
      // the persistent form with the Coulomb bins in LDS (k_ljcoul_pers) where the bins fit beside the LJ table and there are
      // rows enough to fill the chip's 16 waves per CU; else one wave per row with the bins in memory
      const size_t ljlds_al = ((ljlds / sizeof(double) + 3) & ~(size_t)3) * sizeof(double);
      const size_t plds = ljlds_al + ((size_t)32 << P.ncoultablebits);
      const bool pers = h->lj_pers && P.ncoultablebits > 0 && plds <= (size_t)160 * 1024 && h->ncu > 0 && (nrows_lj >= 16 * h->ncu || h->lj_pers >= 2);   // (POLAR_LJ_PERS=2: also for small systems -- tests)
      if (pers) {
#define LJP(E, V, T) do {                                                                                                              \
          static size_t raised[64] = {0};   /* (per template instance and device: the attribute belongs to the function ON a device) */ \
          size_t &rs = raised[h->device & 63];                                                                                          \
          if (rs < plds) { HIPCHECK(hipFuncSetAttribute((const void *)k_ljcoul_pers<E, V, T>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)plds)); rs = plds; } \
          k_ljcoul_pers<E, V, T><<<h->ncu, h->lj_pers_threads, plds, s>>>(P, nrows_lj, il, nn, fi, nj, h->d_xq.p, h->d_type.p, h->d_f.p, h->d_slots.p, eatom, vatom, vmode == 1 || lj_pairwise_virial); \
        } while (0)
#define LJPT(E, V) do { if (h->lj_tab_arith) LJP(E, V, 2); else LJP(E, V, 1); } while (0)
        if (eflag) { if (vrow) LJPT(true, true); else LJPT(true, false); }
        else       { if (vrow) LJPT(false, true); else LJPT(false, false); }
#undef LJPT
#undef LJP
      } else {
#define LJ(E, V) k_ljcoul<E, V><<<grid, block, ljlds, s>>>(P, nrows_lj, il, nn, fi, nj, h->d_xq.p, h->d_type.p, h->d_f.p, h->d_slots.p, eatom, vatom, vmode == 1 || lj_pairwise_virial)
        if (eflag) { if (vrow) LJ(true, true); else LJ(true, false); }
        else       { if (vrow) LJ(false, true); else LJ(false, false); }
#undef LJ
      }
    }
    HIPCHECK(hipEventRecord(h->ev_lj1, s));
    if (h->lj_forked) HIPCHECK(hipEventRecord(h->ev_join, s));
  };
  bool lj_late = false;
#ifdef POLAR_LAB
  lj_late = getenv("POLAR_LJ_LATE") != nullptr;  // fork a3 after the static field instead
#endif
  if (!lj_late) launch_lj();
  const double *mu0 = nullptr;
  if (st.use_previous) {
    // the caller's mu_induced (PS.cpp:376-386 reads atom->mu_induced).  Between two polar_set_atoms calls the atoms keep
    // their places and the caller's array is what the last compute call wrote into it: the resident copy is the same
    // numbers (a caller that edits mu_induced in between goes through polar_upload_mu or polar_set_atoms)
    if (h->attempt > 0) {
      // a retry after an outgrown pitch starts from the SAME guess as the first attempt: the failed attempt has overwritten
      // d_mu (k_unpack) and, through the early download, the caller's array
      if (h->mu0_saved) { HIPCHECK(hipMemcpyAsync(h->d_mu.p, h->d_mu0.p, 3 * (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, s)); mu0 = h->d_mu.p; }
    } else {
      if (mu_host && !(h->mu_resident && h->mu_host_in_sync)) {
        HIPCHECK(hipMemcpyAsync(h->d_mu.p, mu_host, 3 * (size_t)n * sizeof(double), hipMemcpyHostToDevice, s));
        mu0 = h->d_mu.p;
      } else if (h->mu_resident) mu0 = h->d_mu.p;
      h->mu0_saved = mu0 != nullptr;
      if (mu0) { h->d_mu0.ensure(3 * (size_t)n + 3); HIPCHECK(hipMemcpyAsync(h->d_mu0.p, h->d_mu.p, 3 * (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, s)); }
    }
  }
  h->sorted = false;
  h->dense_gs = false;
  const bool gs_mode = (st.polar_gs || st.polar_gs_ranked) && !st.zodid;
  bool ranked_done = false;
  if (ap && gs_mode && dense_gs_fits(n) && !getenv("POLAR_NO_DENSE_GS")) {
    // exact-order Gauss-Seidel on the HBM-resident tensor: put the atoms in SWEEP order first
    // (s space = ranked order), so blocks of the sweep are contiguous rows/columns of T6
    h->dense_gs = true;
    if (st.polar_gs_ranked) {
      launch_rank<true>(h, 1); launch_rank<true>(h, 2);  // a2 (orig space: needs only x/alpha/mol)
      ranked_done = true;
      // stable descending sort == the reference's bubble sort (PS.cpp:1130-1143), on the device: no host round trip
      h->d_perm.ensure(n + 1); h->d_inv.ensure(n + 1);
      k_rank_order<<<nblk(n, POLAR_ROWS_PER_BLOCK), POLAR_BLOCK, 0, s>>>(n, h->d_rank.p, h->d_perm.p, h->d_inv.p);
      h->sorted = true;
    }
  }
  if (!ap) { build_cells(h); h->d_pos4.ensure(n + 1); if (h->static_xq) h->d_xq_s.ensure(n + 2); }  // cell order: perm / inv
  k_pack<<<nblk(n + 1, 256), 256, 0, s>>>(n, h->sorted ? h->d_perm.p : nullptr, h->d_x.p, h->d_q.p, h->d_alpha.p, h->d_mol.p, mu0,
                                      h->d_rec0.p, h->d_rec1.p, h->d_mol_s.p, ap ? nullptr : h->d_pos4.p, (!ap && h->static_xq) ? h->d_xq_s.p : nullptr,
                                      (!ap && h->sweep_kernel == 4) ? 1 : 0, h->box, h->boxlo[0], h->boxlo[1], h->boxlo[2], h->nl_inert ? 0 : 1);
  if (!ap) {
    if (h->colors_valid && h->sweep_kernel < 3) map_color_rows(h);  // the colour rows in this step's cell order
    if (h->sweep_kernel == 2) compute_slots(h);
    build_lists(h);
    if (h->colors_valid && h->sweep_kernel == 3) build_cluster_lists(h);
    if (h->sweep_kernel == 4) build_tiles(h);
  }
  HIPCHECK(hipEventRecord(h->ev[1], s));

  // a2: every step in exact mode (reference); in cutoff mode only when the colour phases are rebuilt
  if (st.polar_gs_ranked && (ap || (!h->colors_valid && h->sweep_kernel != 4)) && !ranked_done) {
    if (ap) { launch_rank<true>(h, 1); launch_rank<true>(h, 2); }
    else    { launch_rank<false>(h, 1); launch_rank<false>(h, 2); }
  }
  HIPCHECK(hipEventRecord(h->ev[2], s));

  HIPCHECK(hipEventRecord(h->ev[3], s));

  {  // a4 + a5
    dim3 grid(nblk(own_n(h), POLAR_ROWS_PER_BLOCK)), block(POLAR_BLOCK);
    const double ccs = st.cut_coul * st.cut_coul, e2s = std::sqrt(h->P.qqrd2e);
    if (ewald_on(h)) {  // `polar_ewald`: reciprocal field first, then the real-space kernel adds it in before the initial guess
      ewald_field(h);
      const double g = h->P.g_ewald;
      if (ap) k_ew_static_field<true><<<grid, block, 0, s>>>(nullptr, n, n, h->d_rec0.p, h->d_mol_s.p, h->box, RowList{nullptr, 0}, nullptr, ccs, e2s, st.polar_gamma, st.use_previous, h->d_ef_s.p, h->d_rec0.p, h->d_rec1.p, nullptr, g, h->d_ew_erec.p);
      else    k_ew_static_field<false><<<grid, block, 0, s>>>(own_rows(h), own_n(h), n, h->d_rec0.p, h->d_mol_s.p, h->box, RowList{h->d_nl_cnt.p, h->nl_pitch}, h->d_nl_j.p, ccs, e2s, st.polar_gamma, st.use_previous, h->d_ef_s.p, h->d_rec0.p, h->d_rec1.p, h->static_xq ? h->d_xq_s.p : nullptr, g, h->d_ew_erec.p);
    } else if (ap) k_static_field<true><<<grid, block, 0, s>>>(nullptr, n, n, h->d_rec0.p, h->d_mol_s.p, h->box, RowList{nullptr, 0}, nullptr, ccs, e2s, st.polar_gamma, st.use_previous, h->d_ef_s.p, h->d_rec0.p, h->d_rec1.p, nullptr);
    else    k_static_field<false><<<grid, block, 0, s>>>(own_rows(h), own_n(h), n, h->d_rec0.p, h->d_mol_s.p, h->box, RowList{h->d_nl_cnt.p, h->nl_pitch}, h->d_nl_j.p, ccs, e2s, st.polar_gamma, st.use_previous, h->d_ef_s.p, h->d_rec0.p, h->d_rec1.p, h->static_xq ? h->d_xq_s.p : nullptr);
  }
  // tile sweep: the solve works on 48-byte sweep records {position, dipole}; the initial dipoles are in the AtomRecs now
#ifdef POLAR_LAB
  if (!ap && h->sweep_kernel == 4 && !st.zodid)
    k_srec_pack<<<nblk(n, 256), 256, 0, s>>>(n, h->d_rec0.p, h->d_srec0.p, h->d_srec1.p);
#endif
  HIPCHECK(hipEventRecord(h->ev[4], s));
  if (lj_late) launch_lj();
}

// PS.cpp:406-645: everything after the solve
int phase_finish(polar_handle *h, polar_result *out) {
  const polar_settings &st = h->ph.st;
  const int n = h->nlocal, nall = h->nlocal + h->nghost;
  const bool ap = !(st.dd_cutoff > 0.0);
  const bool expd = st.damping_type == POLAR_DAMP_EXPONENTIAL;
  const int eflag = h->step_eflag, vmode = h->step_vflag % 4;
  hipStream_t s = h->stream;
#ifdef POLAR_LAB
  if (!ap && h->sweep_kernel == 4 && !st.zodid)  // the solved dipoles back into the AtomRecs the remaining kernels read
    k_srec_unpack<<<nblk(n, 256), 256, 0, s>>>(n, h->d_scal.p, h->d_srec0.p, h->d_srec1.p, h->d_rec0.p, h->d_rec1.p);
#endif
  k_fallback<<<nblk(n, 256), 256, 0, s>>>(n, h->d_scal.p, h->d_rec0.p, h->d_rec1.p, h->d_ef_s.p);
  HIPCHECK(hipEventRecord(h->ev[5], s));
  // the dipoles and the static field are final: back into the caller's atom order now, so that polar_compute can send them
  // to the host while the force kernel runs (nothing below writes the records)
  k_unpack<<<nblk(n, 256), 256, 0, s>>>(n, h->sorted ? h->d_perm.p : nullptr, h->d_scal.p, h->d_rec0.p, h->d_rec1.p, h->d_ef_s.p, h->d_mu.p, h->d_ef.p);
  if (h->early_mu && n > 0) {
    HIPCHECK(hipEventRecord(h->ev_mu_ready, s));
    HIPCHECK(hipStreamWaitEvent(h->dl_stream, h->ev_mu_ready, 0));
    HIPCHECK(hipMemcpyAsync(h->early_mu, h->d_mu.p, 3 * (size_t)n * sizeof(double), hipMemcpyDeviceToHost, h->dl_stream));
    if (h->early_ef) HIPCHECK(hipMemcpyAsync(h->early_ef, h->d_ef.p, 3 * (size_t)n * sizeof(double), hipMemcpyDeviceToHost, h->dl_stream));
    HIPCHECK(hipEventRecord(h->ev_dl1, h->dl_stream));
  }
  double *vatom = (h->step_vflag / 4) ? h->d_vatom.p : nullptr;
  // join a3: before the force kernel when both write the (non-atomic) per-atom virial rows,
  // otherwise only before the accumulators are read
  auto join_lj = [&]() { if (h->lj_forked) { HIPCHECK(hipStreamWaitEvent(s, h->ev_join, 0)); h->lj_forked = false; } };
  if (vatom) join_lj();
  // full-list mode with an fdotr virial: the polarization forces go to their own array first, so that
  // sum f_pol . x can be formed without the LJ forces (whose virial was tallied pairwise)
  const bool split_f = h->full_list && vmode == 2;
  double *fdst = h->d_f.p;
  if (split_f) {
    h->d_fpol.ensure(3 * (size_t)n + 3);
    HIPCHECK(hipMemsetAsync(h->d_fpol.p, 0, 3 * (size_t)n * sizeof(double), s));
    fdst = h->d_fpol.p;
  }
  if (ap) { if (expd) launch_force<true, 0>(h, eflag, vmode == 1, vatom, fdst); else launch_force<true, 1>(h, eflag, vmode == 1, vatom, fdst); }
  else    { if (expd) launch_force<false, 0>(h, eflag, vmode == 1, vatom, fdst); else launch_force<false, 1>(h, eflag, vmode == 1, vatom, fdst); }
  join_lj();
  if (split_f) {
    k_virial_fdotr<<<std::min(1024, nblk(n, 256)), 256, 0, s>>>(n, h->d_x.p, h->d_fpol.p, h->d_slots.p);
    k_add_into<<<nblk(3 * (long long)n, 256), 256, 0, s>>>(3 * (long long)n, h->d_fpol.p, h->d_f.p);
  } else if (vmode == 2) k_virial_fdotr<<<std::min(1024, nblk(nall, 256)), 256, 0, s>>>(nall, h->d_x.p, h->d_f.p, h->d_slots.p);  // a10
  if (ewald_on(h)) ewald_forces(h);  // (after the fdotr virial: the reciprocal forces are not pair forces)
  k_fold_scal<<<1, POLAR_NSLOT, 0, s>>>(h->d_scal.p, h->d_slots.p, 0);
  HIPCHECK(hipEventRecord(h->ev[6], s));
  if (h->early_mu && h->user_mu && n > 0) {  // the force kernel is still running: the dipoles and the field, on the host by now, go into the caller's arrays meanwhile
    HIPCHECK(hipEventSynchronize(h->ev_dl1));
    const double *sm = h->early_mu, *se = h->early_ef;
    double *um = h->user_mu, *ue = h->user_ef;
    host_chunks(3 * (size_t)n, [&](size_t a, size_t b) {
      memcpy(um + a, sm + a, (b - a) * sizeof(double));
      if (ue && se) memcpy(ue + a, se + a, (b - a) * sizeof(double));
    });
  }
  read_scal(h);
  h->mu_resident = true;
  h->mu_host_in_sync = false;  // d_mu has new numbers; polar_compute / polar_compute_peratom set this again once the caller's array holds them

  const Scal &sc = *h->h_scal.p;
  out->eng_vdwl = sc.eng_vdwl; out->eng_coul = sc.eng_coul;
  out->u_self = sc.u_self; out->u_ef = sc.u_ef; out->u_dd = sc.u_dd;
  out->eng_pol = sc.u_self + sc.u_ef + sc.u_dd;  // PS.cpp:632 (all zero when eflag == 0)
  for (int k = 0; k < 6; k++) out->virial[k] = sc.virial[k];
  if (ewald_on(h)) {  // u_ef = -sum mu . E_static over the whole Ewald field; the reciprocal virial by its k-space formula
    double ew[7];
    HIPCHECK(hipMemcpyAsync(ew, h->d_ew_out.p, sizeof(ew), hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    if (eflag) { out->u_ef = ew[0]; out->eng_pol = sc.u_self + ew[0] + sc.u_dd; }
    if (vmode) for (int k = 0; k < 6; k++) out->virial[k] += ew[1 + k];
    float a = 0.f, b = 0.f;
    HIPCHECK(hipEventElapsedTime(&a, h->ev_ks[0], h->ev_ks[1]));
    HIPCHECK(hipEventElapsedTime(&b, h->ev_ks[2], h->ev_ks[3]));
    out->ms_kspace = (double)a + (double)b;
    h->ew_field_ms = (double)a;   // (polar_pair_extract "ewald_field_ms": the field half alone, the yardstick of tools/ewald_field_at_cost.py)
    out->nkvec = h->ew_nk;
  }
  long long rb = (long long)sc.rmin_bits;
  memcpy(&out->rmin, &rb, sizeof(double));
  out->rms_dmu = std::sqrt(std::max(0.0, sc.last_change));
  h->ntrace = std::min(h->ntrace, sc.sweeps);
  out->iterations = sc.iterations; out->sweeps = sc.sweeps; out->status = sc.status ? POLAR_WARN_NOT_CONVERGED : POLAR_OK;
  h->last_sweeps = (!st.fixed_iteration && !st.zodid && !sc.status && sc.done) ? sc.sweeps : 0;   // (where the next solve's first look at the loop state goes)
  if (!ap) {
    unsigned long long tot = 0;
    for (int k = 0; k < 64; k++) tot += h->h_ddtot.p[16 * k];
    h->dd_pairs = (long long)tot;
  }
  out->dd_pairs = ap ? (long long)n * (n - 1) : h->dd_pairs;
  out->ms_color_host = h->ms_color_host;
  h->ms_color_host = 0.0;
  float ms;
  auto el = [&](int a, int b) { HIPCHECK(hipEventElapsedTime(&ms, h->ev[a], h->ev[b])); return (double)ms; };
  out->ms_list = el(0, 1); out->ms_rank = el(1, 2); out->ms_static = el(3, 4);
  HIPCHECK(hipEventElapsedTime(&ms, h->ev_lj0, h->ev_lj1));
  out->ms_ljcoul = ms;  // on its own stream: overlaps the other phases, so the parts no longer add up to ms_total
  out->ms_solve = el(4, 5); out->ms_force = el(5, 6); out->ms_total = el(0, 6);
  if (sc.status) h->warn = "Number of iterations exceeding max_iterations, setting dipoles to alpha*E";  // PS.cpp:1233
  return out->status;
}

// end-of-step flags of the pitched lists (pinned, copied at the end of the list builds): true = a list did not fit, the
// pitches have been enlarged and the step must be repeated
void clear_flags(polar_handle *h) { for (int k = 0; k < 16; k++) h->h_flags.p[k] = 0; }
void tile_fallback(polar_handle *h) {
  h->sweep_kernel = 2;
  h->colors_valid = false; h->slots_by_color = false;
  h->nl_pitch = h->dd_pitch = 0;  // the cell grid changes with the sweep kernel
  h->warn = "tile sweep unavailable for this system (cell neighbourhood beyond the LDS, or a cell beyond the builder's limits): row sweep in use";
}
bool grow_pitches(polar_handle *h) {
  bool again = false;
  if (h->h_flags.p[0] != 0) {
    h->nl_pitch = h->dd_pitch = std::max(pitch_grown(h->h_flags.p[0]), h->nl_pitch + 64);
    again = true;
  }
  if (h->h_flags.p[4] != 0) { h->cl_pitch = (((long long)(1.25 * h->h_flags.p[4]) + 255) / 256) * 256; again = true; }
  if (h->sweep_kernel == 4) {
    if (h->h_flags.p[7] != 0) { tile_fallback(h); return true; }
    if (h->h_flags.p[5] != 0) {  // a union list beyond the pitch, or beyond what the sweep's LDS request holds
      const int need = (int)(((long long)(1.15 * h->h_flags.p[5]) + 16 + 63) / 64 * 64);
      if (need > tile_lds_cap()) { tile_fallback(h); return true; }
      h->un_pitch = std::max(h->un_pitch, need); h->un_lds = h->un_pitch;
      again = true;
    }
    if (h->h_flags.p[6] != 0) { h->pitch16 = ((long long)(1.25 * h->h_flags.p[6]) + 511) / 512 * 512; again = true; }
    if (!again && h->h_flags.p[9] > 0) {  // next step: ask only for the LDS the unions need (two workgroups per CU below 80 KB)
      h->tile_max_u = h->h_flags.p[9];
      h->un_lds = std::min(h->un_pitch, (int)((long long)(1.06 * (h->tile_max_u + 1)) + 8 + 7) / 8 * 8);
      if (getenv("POLAR_DEBUG") && !h->tile_reported) {
        h->tile_reported = true;
        fprintf(stderr, "[polar] tile sweep: %lld cells (%d x %d x %d), %d launches per sweep, largest union %d records, union pitch %d, "
                "LDS request %zu bytes (%d records), row pitch %lld entries\n", h->ncell, h->grid.nc[0], h->grid.nc[1], h->grid.nc[2],
                (int)h->tile_launches.size(), h->tile_max_u, h->un_pitch, tile_lds_bytes(std::min(h->un_pitch, h->un_lds)), h->un_lds, h->pitch16);
      }
    }
  }
  return again;
}

int do_compute(polar_handle *h, int eflag, int vflag, const double *mu_host, polar_result *out) {
  memset(out, 0, sizeof(*out));
  const bool ap = !(h->ph.st.dd_cutoff > 0.0);
  int rc = 0;
  bool done = false;
  struct Attempt { polar_handle *h; ~Attempt() { h->attempt = 0; } } guard{h};
  for (int attempt = 0; attempt < 5; attempt++) {
    clear_flags(h);
    h->attempt = attempt;
    try {
      phase_begin(h, eflag, vflag, mu_host);
    } catch (const TileUnavailable &) {  // density beyond what a workgroup can stage: the row sweep takes over
      tile_fallback(h);
      continue;
    }
    if (!h->ph.st.zodid) solve(h, ap, out);  // a6 + a7 (PS.cpp:389)
    const int nc = out->ncolors;
    rc = phase_finish(h, out);
    out->ncolors = nc;
    if (ap || !grow_pitches(h)) { done = true; break; }
    memset(out, 0, sizeof(*out));  // a row did not fit its pitch: the pitches have grown, redo the step
  }
  if (!done) throw std::runtime_error("neighbor list pitch overflow persists");
  return rc;
}

// polar_step_begin in two halves, so that a multi-GPU driver can agree on failures and on a common colouring in between:
// step_begin_lists = everything up to the point where the colour phases are needed (PS.cpp:125-386: lists, a3 forked, static
// field, initial guess; on reneighbor steps the verdict on the colouring in use); step_begin_finish = the colouring if it is
// still missing (this handle's own), rows into launch order, descriptors.
void step_begin_lists(polar_handle *h, int eflag, int vflag) {
  HIPCHECK(hipSetDevice(h->device));
  clear_flags(h);
  try {
    phase_begin(h, eflag, vflag, nullptr);
  } catch (const TileUnavailable &) {
    tile_fallback(h);
    phase_begin(h, eflag, vflag, nullptr);
  }
  if (h->ph.st.dd_cutoff > 0.0 && !tile_mode(h)) resolve_colors(h);
}
bool step_needs_colors(const polar_handle *h) {
  const polar_settings &st = h->ph.st;
  const bool clm = st.dd_cutoff > 0.0 && h->sweep_kernel == 3;
  return st.dd_cutoff > 0.0 && !tile_mode(h) && !st.zodid && (st.polar_gs || st.polar_gs_ranked || clm) && !h->colors_valid;
}
void step_begin_finish(polar_handle *h) {
  const polar_settings &st = h->ph.st;
  const bool clm = st.dd_cutoff > 0.0 && h->sweep_kernel == 3;
  if (step_needs_colors(h)) { ensure_colors(h); if (clm) build_cluster_lists(h); else map_color_rows(h); }
  if (!st.zodid && st.dd_cutoff > 0.0 && (st.polar_gs || st.polar_gs_ranked) && h->sweep_kernel == 2 && !slots_current(h)) { compute_slots(h); build_lists(h); }
  if (!st.zodid && st.dd_cutoff > 0.0 && h->sweep_kernel == 2) prepare_lp(h);
  h->in_step = true;
}

// ---- what the passes of the point calls share ------------------------------------------------------------------------------
// The points of a pass go up into d_fa_x, skip_atom and molecule (either may be null) into the halves of d_fa_idx; the event
// pair of the passes exists from here on.  Returns where the two index arrays went (null: not given).
struct PointIdx { int *skip, *pmol; };
static PointIdx point_upload(polar_handle *h, int m, const double *x, const int *skip_atom, const int *molecule) {
  hipStream_t s = h->stream;
  const size_t mm = (size_t)m;
  h->d_fa_x.ensure(3 * mm); h->d_fa_idx.ensure(2 * mm);
  if (!h->ev_fa[0].e) { h->ev_fa[0].create(); h->ev_fa[1].create(); }
  HIPCHECK(hipMemcpyAsync(h->d_fa_x.p, x, 3 * mm * sizeof(double), hipMemcpyHostToDevice, s));
  PointIdx idx{nullptr, nullptr};
  if (skip_atom) { idx.skip = h->d_fa_idx.p; HIPCHECK(hipMemcpyAsync(idx.skip, skip_atom, mm * sizeof(int), hipMemcpyHostToDevice, s)); }
  if (molecule) { idx.pmol = h->d_fa_idx.p + mm; HIPCHECK(hipMemcpyAsync(idx.pmol, molecule, mm * sizeof(int), hipMemcpyHostToDevice, s)); }
  return idx;
}

// The list grid with the box origin in it (exact mode has built no grid: the point kernels take the origin from it in both
// modes) ...
static CellGrid point_grid(const polar_handle *h) {
  CellGrid cg = h->grid;
  for (int k = 0; k < 3; k++) cg.lo[k] = h->boxlo[k];
  return cg;
}
// ... and with it the other by-value arguments of the field kernels: the cutoffs, e2s, the exponential's constants.
struct PointParm { PointCut cut; double e2s; ExpCoef K; CellGrid cg; };
static PointParm point_parm(const polar_handle *h) {
  const polar_settings &st = h->ph.st;
  const double rc = st.cut_coul;
  return PointParm{PointCut{rc * rc, st.dd_cutoff * st.dd_cutoff, 1.0 / (rc * rc), 2.0 / rc, st.polar_damp}, std::sqrt(h->P.qqrd2e), make_expcoef(),
                   point_grid(h)};
}

// The end of a pass: the results the caller asked for come back (a null host pointer: not asked for), the stream is waited
// for, and the device time between ev_fa[0] and ev_fa[1] is added to *ms -- with `ewald` also that between ev_fa[1] and
// ev_fa_k, and both to the handle's ew_fa_ms.
struct PointBack { double *host; const double *dev; size_t count; };
static void point_finish(polar_handle *h, std::initializer_list<PointBack> back, bool ewald, double *ms) {
  hipStream_t s = h->stream;
  for (const PointBack &b : back)
    if (b.host) HIPCHECK(hipMemcpyAsync(b.host, b.dev, b.count * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  float t = 0.f, tk = 0.f;
  HIPCHECK(hipEventElapsedTime(&t, h->ev_fa[0], h->ev_fa[1]));
  if (ewald) {
    HIPCHECK(hipEventElapsedTime(&tk, h->ev_fa[1], h->ev_fa_k));
    h->ew_fa_ms[0] += (double)t; h->ew_fa_ms[1] += (double)tk;
  }
  if (ms) *ms += ewald ? (double)t + (double)tk : (double)t;
}
// ... of a pass whose results are the field block in d_fa_out
static void field_out_finish(polar_handle *h, int m, double *e_static, double *e_induced, double *phi_static, double *phi_induced, bool ewald,
                             double *ms) {
  const size_t mm = (size_t)m;
  const FieldAtOut out{h->d_fa_out.p};
  point_finish(h, {{e_static, out.es(), 3 * mm}, {e_induced, out.ei(mm), 3 * mm}, {phi_static, out.ps(mm), mm}, {phi_induced, out.pi(mm), mm}}, ewald, ms);
}

// polar_field_at, one pass: the points go up, one launch of k_field_at (polar_field_at.hpp) on the handle's stream reads the
// records, the molecule ids and -- list mode -- the cell table the finished step left, the results the caller asked for come
// back.  Nothing of the handle's step state is written.
void field_at_pass(polar_handle *h, int m, const double *x, const int *skip_atom, const int *molecule, double *e_static,
                   double *e_induced, double *phi_static, double *phi_induced, double *ms, bool phi_on_device) {
  const polar_settings &st = h->ph.st;
  const bool ap = !(st.dd_cutoff > 0.0);
  const bool expd = st.damping_type == POLAR_DAMP_EXPONENTIAL;
  const bool phi = phi_static || phi_induced || phi_on_device;
  hipStream_t s = h->stream;
  h->d_fa_out.ensure(8 * (size_t)m);
  const PointIdx idx = point_upload(h, m, x, skip_atom, molecule);
  const PointParm pp = point_parm(h);
  const FieldAtOut out{h->d_fa_out.p};
  const dim3 grid(nblk(m, POLAR_ROWS_PER_BLOCK)), block(POLAR_BLOCK);
  HIPCHECK(hipEventRecord(h->ev_fa[0], s));
#define FA(AP, D, P)                                                                                                            \
  k_field_at<AP, D, P><<<grid, block, 0, s>>>(m, h->d_fa_x.p, idx.skip, idx.pmol, h->sorted ? h->d_inv.p : nullptr, h->nlocal,  \
                                              h->d_scal.p, h->d_rec0.p, h->d_rec1.p, h->d_mol_s.p, h->box, pp.cg,               \
                                              AP ? nullptr : h->d_cell_first.p, pp.cut, pp.e2s, pp.K, out)
#define FAP(AP, D) do { if (phi) FA(AP, D, true); else FA(AP, D, false); } while (0)
  if (ap) { if (expd) FAP(true, 0); else FAP(true, 1); }
  else    { if (expd) FAP(false, 0); else FAP(false, 1); }
#undef FAP
#undef FA
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipEventRecord(h->ev_fa[1], s));
  field_out_finish(h, m, e_static, e_induced, phi_static, phi_induced, false, ms);
}

// The launch of k_ew_point_real (polar_ewald_field_at.hpp) on the m points in d_fa_x, between the events ev_fa[0] and ev_fa[1],
// behind Q of the neutralising-background term (once per call window): what polar_ewald_field_at and polar_ewald_field_grid share.
static void ew_point_real_launch(polar_handle *h, int m, const int *d_skip, const int *d_pmol, bool phi) {
  const polar_settings &st = h->ph.st;
  const bool ap = !(st.dd_cutoff > 0.0);
  const bool expd = st.damping_type == POLAR_DAMP_EXPONENTIAL;
  hipStream_t s = h->stream;
  const PointParm pp = point_parm(h);
  const EwPointParm ewp = make_ew_point_parm(h->P.g_ewald);
  const FieldAtOut out{h->d_fa_out.p};
  if (!h->ew_q_valid) {   // Q of the neutralising-background term, once per call window
    h->d_fa_q.ensure(1);
    k_ew_point_qsum<<<1, 256, 0, s>>>(h->nlocal, h->d_rec0.p, h->d_fa_q.p);
    HIPCHECK(hipGetLastError());   // (a launch that failed leaves no Q marked valid)
    h->ew_q_valid = true;
  }
  const dim3 grid(nblk(m, POLAR_ROWS_PER_BLOCK)), block(POLAR_BLOCK);
  HIPCHECK(hipEventRecord(h->ev_fa[0], s));
#define FA(AP, D, P)                                                                                                               \
  k_ew_point_real<AP, D, P><<<grid, block, 0, s>>>(m, h->d_fa_x.p, d_skip, d_pmol, h->sorted ? h->d_inv.p : nullptr, h->nlocal,    \
                                                   h->d_scal.p, h->d_rec0.p, h->d_rec1.p, h->d_mol_s.p, h->box, pp.cg,             \
                                                   AP ? nullptr : h->d_cell_first.p, pp.cut, ewp, pp.e2s, pp.K, out)
#define FAP(AP, D) do { if (phi) FA(AP, D, true); else FA(AP, D, false); } while (0)
  if (ap) { if (expd) FAP(true, 0); else FAP(true, 1); }
  else    { if (expd) FAP(false, 0); else FAP(false, 1); }
#undef FAP
#undef FA
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipEventRecord(h->ev_fa[1], s));
}

// polar_ewald_field_at, one pass: k_ew_point_real (polar_ewald_field_at.hpp) writes the real-space static sums and the induced
// sums of the m points; then, for runs of points sized so that the chunk partials stay within 64 MB, k_ew_point_recip over
// (points, row chunks of the step's k-vector table) and k_ew_point_fold.  S(k) in d_ew_s is the finished step's: nothing writes
// it after ewald_field.  Nothing of the handle's step state is written.
void ewald_field_at_pass(polar_handle *h, int m, const double *x, const int *skip_atom, const int *molecule, double *e_static,
                         double *e_induced, double *phi_static, double *phi_induced, double *ms, bool phi_on_device) {
  const bool phi = phi_static || phi_induced || phi_on_device;
  hipStream_t s = h->stream;
  const size_t mm = (size_t)m;
  h->d_fa_out.ensure(8 * mm);
  if (!h->ev_fa_k.e) h->ev_fa_k.create();
  const PointIdx idx = point_upload(h, m, x, skip_atom, molecule);
  ew_point_real_launch(h, m, idx.skip, idx.pmol, phi);
  const double g = h->P.g_ewald, e2s = std::sqrt(h->P.qqrd2e);
  const FieldAtOut out{h->d_fa_out.p};
  const double *lo = h->boxlo;
  // reciprocal space
  const int nk = h->ew_nk, nrow = nk > 0 ? h->ew_nrow : 0;
  const int nchunk = ew_point_chunks(nrow, nk), rpc = ew_point_rows_per_chunk(nrow, nk);
  const double vol = h->box.prd[0] * h->box.prd[1] * h->box.prd[2];
  const double qterm = -3.14159265358979323846 / (g * g * vol);
  const size_t per_point = (size_t)std::max(nchunk, 1) * 4 * sizeof(double);
  const int run = (int)std::max<size_t>(256, std::min<size_t>(mm, ((size_t)64 << 20) / per_point / 256 * 256));
  h->d_fa_part.ensure((size_t)std::max(nchunk, 1) * 4 * std::min<size_t>(mm, (size_t)run));
  for (int p0 = 0; p0 < m; p0 += run) {
    const int np = std::min(run, m - p0);
    if (nchunk > 0) {
      const dim3 gk(nblk(np, 256), nchunk);
      if (phi) k_ew_point_recip<true><<<gk, 256, 0, s>>>(np, p0, h->d_fa_x.p, h->box, lo[0], lo[1], lo[2], ew_cell(h), nrow, rpc, h->d_ew_rows.p, h->d_ew_kv.p, h->d_ew_s.p, h->d_fa_part.p);
      else     k_ew_point_recip<false><<<gk, 256, 0, s>>>(np, p0, h->d_fa_x.p, h->box, lo[0], lo[1], lo[2], ew_cell(h), nrow, rpc, h->d_ew_rows.p, h->d_ew_kv.p, h->d_ew_s.p, h->d_fa_part.p);
    }
    if (phi) k_ew_point_fold<true><<<nblk(np, 256), 256, 0, s>>>(np, p0, m, nchunk, h->d_fa_part.p, e2s, qterm, h->d_fa_q.p, out);
    else     k_ew_point_fold<false><<<nblk(np, 256), 256, 0, s>>>(np, p0, m, nchunk, h->d_fa_part.p, e2s, qterm, h->d_fa_q.p, out);
  }
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipEventRecord(h->ev_fa_k, s));
  field_out_finish(h, m, e_static, e_induced, phi_static, phi_induced, true, ms);
}

// polar_probe_at, one pass.  The field half is a pass of the handle's own field call with no host output: it leaves the points,
// skip_atom and molecule in d_fa_x / d_fa_idx and the field block (potentials included) in d_fa_out, and has synchronised.  Then
// one launch: k_probe_lj (polar_probe_at.hpp), whose lane 0 also combines the field block with the site's q and alpha, or
// k_probe_combine alone.  Nothing of the handle's step state is written; the records' types (d_pr_type_s) are made by the first
// pass of a call window.
void probe_at_pass(polar_handle *h, int m, const double *x, const int *type, const double *q, const double *alpha, const int *skip_atom,
                   const int *molecule, double *e_lj, double *e_coul, double *e_pol, double *f_lj, double *e_total, double *ms) {
  const polar_settings &st = h->ph.st;
  const bool ap = !(st.dd_cutoff > 0.0);
  const bool lj = e_lj || f_lj, field = e_coul || e_pol || e_total;
  hipStream_t s = h->stream;
  const size_t mm = (size_t)m;
  if (field) {
    if (ewald_on(h)) ewald_field_at_pass(h, m, x, skip_atom, molecule, nullptr, nullptr, nullptr, nullptr, ms, true);
    else field_at_pass(h, m, x, skip_atom, molecule, nullptr, nullptr, nullptr, nullptr, ms, true);
  } else {
    point_upload(h, m, x, skip_atom, molecule);
  }
  const int *d_skip = skip_atom ? h->d_fa_idx.p : nullptr, *d_pmol = molecule ? h->d_fa_idx.p + mm : nullptr;
  h->d_pr_out.ensure(9 * mm); h->d_pr_qa.ensure(2 * mm); h->d_pr_type.ensure(mm);
  const double *d_q = nullptr, *d_a = nullptr;
  if (field && q) { d_q = h->d_pr_qa.p; HIPCHECK(hipMemcpyAsync(h->d_pr_qa.p, q, mm * sizeof(double), hipMemcpyHostToDevice, s)); }
  if (field && alpha) { d_a = h->d_pr_qa.p + mm; HIPCHECK(hipMemcpyAsync(h->d_pr_qa.p + mm, alpha, mm * sizeof(double), hipMemcpyHostToDevice, s)); }
  if (lj) HIPCHECK(hipMemcpyAsync(h->d_pr_type.p, type, mm * sizeof(int), hipMemcpyHostToDevice, s));
  if (lj && !h->pr_types_valid) {   // the records' types, once per call window
    h->d_pr_type_s.ensure((size_t)h->nlocal + 1);
    k_probe_types<<<nblk(h->nlocal, 256), 256, 0, s>>>(h->nlocal, h->sorted ? h->d_perm.p : nullptr, h->d_type.p, h->d_pr_type_s.p);
    HIPCHECK(hipGetLastError());
    h->pr_types_valid = true;
  }
  const ProbeOut out{h->d_pr_out.p};
  const ProbeField fld{FieldAtOut{field ? h->d_fa_out.p : nullptr}, d_q, d_a, std::sqrt(h->P.qqrd2e)};
  HIPCHECK(hipEventRecord(h->ev_fa[0], s));
  if (lj) {
    ProbeGrid pg;
    pg.g = point_grid(h);
    pg.ncell_inert = (!ap && h->cell_split) ? h->ncell : 0;
    double width[3];
    box_widths(h->box, width);
    probe_dfrac_scale(width, pg.dscale);
    const dim3 grid(nblk(m, POLAR_ROWS_PER_BLOCK)), block(POLAR_BLOCK);
#define PR(AP, F)                                                                                                                   \
  k_probe_lj<AP, F><<<grid, block, 0, s>>>(m, h->d_fa_x.p, h->d_pr_type.p, d_skip, d_pmol, h->sorted ? h->d_inv.p : nullptr, h->nlocal, \
                                           h->d_scal.p, h->d_rec0.p, h->d_rec1.p, h->d_pr_type_s.p, h->d_mol_s.p, h->box, pg,        \
                                           AP ? nullptr : h->d_cell_first.p, h->d_lj.p, h->ntypes, h->d_pr_reach.p, fld, out)
    if (ap) { if (f_lj) PR(true, true); else PR(true, false); }
    else    { if (f_lj) PR(false, true); else PR(false, false); }
#undef PR
  } else {
    k_probe_combine<<<nblk(m, 256), 256, 0, s>>>(m, fld, out);
  }
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipEventRecord(h->ev_fa[1], s));
  point_finish(h, {{e_lj, out.elj(), mm}, {f_lj, out.flj(mm), 3 * mm}, {e_total, out.et(mm), 3 * mm}, {e_coul, out.ec(mm), mm}, {e_pol, out.ep(mm), mm}}, false, ms);
}

// polar_field_grad_at, one pass: field_at_pass with k_field_grad_at (polar_field_grad_at.hpp) and the block of 18 doubles per
// point in d_fg_out, where it stays for polar_probe_force_at.  Nothing of the handle's step state is written.
void field_grad_at_pass(polar_handle *h, int m, const double *x, const int *skip_atom, const int *molecule, double *g_static,
                        double *g_induced, double *e_static, double *e_induced, double *ms) {
  const polar_settings &st = h->ph.st;
  const bool ap = !(st.dd_cutoff > 0.0);
  const bool expd = st.damping_type == POLAR_DAMP_EXPONENTIAL;
  hipStream_t s = h->stream;
  const size_t mm = (size_t)m;
  h->d_fg_out.ensure(POLAR_FIELD_GRAD_DOUBLES * mm);
  const PointIdx idx = point_upload(h, m, x, skip_atom, molecule);
  const PointParm pp = point_parm(h);
  const FieldGradOut out{h->d_fg_out.p};
  const dim3 grid(nblk(m, POLAR_ROWS_PER_BLOCK)), block(POLAR_BLOCK);
  HIPCHECK(hipEventRecord(h->ev_fa[0], s));
#define FG(AP, D)                                                                                                                  \
  k_field_grad_at<AP, D><<<grid, block, 0, s>>>(m, h->d_fa_x.p, idx.skip, idx.pmol, h->sorted ? h->d_inv.p : nullptr, h->nlocal,   \
                                                h->d_scal.p, h->d_rec0.p, h->d_rec1.p, h->d_mol_s.p, h->box, pp.cg,                \
                                                AP ? nullptr : h->d_cell_first.p, pp.cut, pp.e2s, pp.K, out)
  if (ap) { if (expd) FG(true, 0); else FG(true, 1); }
  else    { if (expd) FG(false, 0); else FG(false, 1); }
#undef FG
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipEventRecord(h->ev_fa[1], s));
  point_finish(h, {{e_static, out.es(), 3 * mm}, {e_induced, out.ei(mm), 3 * mm}, {g_static, out.gs(mm), 6 * mm}, {g_induced, out.gi(mm), 6 * mm}}, false, ms);
}

// The launch of k_ew_grad_real (polar_ewald_field_grad_at.hpp) on the m points in d_fa_x, between the events ev_fa[0] and ev_fa[1],
// into the block in d_fg_out: what polar_ewald_field_grad_at and polar_ewald_field_grad_grid share.
static void ew_grad_real_launch(polar_handle *h, int m, const int *d_skip, const int *d_pmol) {
  const polar_settings &st = h->ph.st;
  const bool ap = !(st.dd_cutoff > 0.0);
  const bool expd = st.damping_type == POLAR_DAMP_EXPONENTIAL;
  hipStream_t s = h->stream;
  const PointParm pp = point_parm(h);
  const EwPointParm ewp = make_ew_point_parm(h->P.g_ewald);
  const FieldGradOut out{h->d_fg_out.p};
  const dim3 grid(nblk(m, POLAR_ROWS_PER_BLOCK)), block(POLAR_BLOCK);
  HIPCHECK(hipEventRecord(h->ev_fa[0], s));
#define FG(AP, D)                                                                                                                 \
  k_ew_grad_real<AP, D><<<grid, block, 0, s>>>(m, h->d_fa_x.p, d_skip, d_pmol, h->sorted ? h->d_inv.p : nullptr, h->nlocal,       \
                                               h->d_scal.p, h->d_rec0.p, h->d_rec1.p, h->d_mol_s.p, h->box, pp.cg,                \
                                               AP ? nullptr : h->d_cell_first.p, pp.cut, ewp, pp.e2s, pp.K, out)
  if (ap) { if (expd) FG(true, 0); else FG(true, 1); }
  else    { if (expd) FG(false, 0); else FG(false, 1); }
#undef FG
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipEventRecord(h->ev_fa[1], s));
}

// polar_ewald_field_grad_at, one pass: k_ew_grad_real (polar_ewald_field_grad_at.hpp) writes the real-space static sums and
// the induced sums of the m points into the block of 18 doubles per point in d_fg_out; then, for runs of points sized so that
// the chunk partials (9 doubles per point and chunk) stay within 64 MB, k_ew_grad_recip over (points, row chunks of the step's
// k-vector table) and k_ew_grad_fold.  The block stays in d_fg_out for polar_ewald_probe_force_at.  Nothing of the handle's
// step state is written.
void ewald_field_grad_at_pass(polar_handle *h, int m, const double *x, const int *skip_atom, const int *molecule, double *g_static,
                              double *g_induced, double *e_static, double *e_induced, double *ms) {
  hipStream_t s = h->stream;
  const size_t mm = (size_t)m;
  h->d_fg_out.ensure(POLAR_FIELD_GRAD_DOUBLES * mm);
  if (!h->ev_fa_k.e) h->ev_fa_k.create();
  const PointIdx idx = point_upload(h, m, x, skip_atom, molecule);
  ew_grad_real_launch(h, m, idx.skip, idx.pmol);
  const double e2s = std::sqrt(h->P.qqrd2e);
  const FieldGradOut out{h->d_fg_out.p};
  // reciprocal space
  const double *lo = h->boxlo;
  const int nk = h->ew_nk, nrow = nk > 0 ? h->ew_nrow : 0;
  const int nchunk = ew_point_chunks(nrow, nk), rpc = ew_point_rows_per_chunk(nrow, nk);
  const size_t per_point = (size_t)std::max(nchunk, 1) * 9 * sizeof(double);
  const int run = (int)std::max<size_t>(256, std::min<size_t>(mm, ((size_t)64 << 20) / per_point / 256 * 256));
  h->d_fa_part.ensure((size_t)std::max(nchunk, 1) * 9 * std::min<size_t>(mm, (size_t)run));
  for (int p0 = 0; p0 < m; p0 += run) {
    const int np = std::min(run, m - p0);
    if (nchunk > 0) {
      const dim3 gk(nblk(np, 256), nchunk);
      k_ew_grad_recip<<<gk, 256, 0, s>>>(np, p0, h->d_fa_x.p, h->box, lo[0], lo[1], lo[2], ew_cell(h), nrow, rpc, h->d_ew_rows.p, h->d_ew_kv.p, h->d_ew_s.p, h->d_fa_part.p);
      k_ew_grad_fold<<<nblk(np, 256), 256, 0, s>>>(np, p0, m, nchunk, h->d_fa_part.p, e2s, out);
    }
  }
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipEventRecord(h->ev_fa_k, s));
  point_finish(h, {{e_static, out.es(), 3 * mm}, {e_induced, out.ei(mm), 3 * mm}, {g_static, out.gs(mm), 6 * mm}, {g_induced, out.gi(mm), 6 * mm}}, true, ms);
}

// polar_probe_force_at and polar_ewald_probe_force_at, one pass.  f_lj: a pass of polar_probe_at that asks for nothing but the
// LJ force (k_probe_lj's FORCE instance: the bits of that call).  f_coul, f_pol: a gradient pass of the handle's own model with
// no host output, which leaves the block in d_fg_out and has synchronised; then k_probe_force_combine, one thread per point,
// behind the site's q and alpha.
void probe_force_at_pass(polar_handle *h, int m, const double *x, const int *type, const double *q, const double *alpha,
                         const int *skip_atom, const int *molecule, double *f_lj, double *f_coul, double *f_pol, double *ms) {
  hipStream_t s = h->stream;
  const size_t mm = (size_t)m;
  if (f_lj) probe_at_pass(h, m, x, type, nullptr, nullptr, skip_atom, molecule, nullptr, nullptr, nullptr, f_lj, nullptr, ms);
  if (!f_coul && !f_pol) return;
  if (ewald_on(h)) ewald_field_grad_at_pass(h, m, x, skip_atom, molecule, nullptr, nullptr, nullptr, nullptr, ms);
  else field_grad_at_pass(h, m, x, skip_atom, molecule, nullptr, nullptr, nullptr, nullptr, ms);
  h->d_pr_qa.ensure(2 * mm);
  const double *d_q = nullptr, *d_a = nullptr;
  if (f_coul && q) { d_q = h->d_pr_qa.p; HIPCHECK(hipMemcpyAsync(h->d_pr_qa.p, q, mm * sizeof(double), hipMemcpyHostToDevice, s)); }
  if (f_pol && alpha) { d_a = h->d_pr_qa.p + mm; HIPCHECK(hipMemcpyAsync(h->d_pr_qa.p + mm, alpha, mm * sizeof(double), hipMemcpyHostToDevice, s)); }
  const FieldGradOut out{h->d_fg_out.p};
  HIPCHECK(hipEventRecord(h->ev_fa[0], s));
  k_probe_force_combine<<<nblk(m, 256), 256, 0, s>>>(m, d_q, d_a, std::sqrt(h->P.qqrd2e), out);
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipEventRecord(h->ev_fa[1], s));
  point_finish(h, {{f_coul, out.fc(mm), 3 * mm}, {f_pol, out.fp(mm), 3 * mm}}, false, ms);
}

// polar_ewald_field_grid and polar_ewald_field_grad_grid (`name`), once per call: the layout from the k-vector table (its rows
// come back from the device: 16 bytes per (h, k) row) with nset coefficient sets per element of T and V, then the phase tables
// (k_ew_grid_tab) and stage 1 -- k_ew_grid_l of polar_ewald_field_grid.hpp with four sets, k_ew_gg_l of
// polar_ewald_field_grad_grid.hpp with EW_GG_SETS.  Their device time is reciprocal time.
static void ew_grid_call_begin(polar_handle *h, const std::string &name, int nset, const int n[3], const double off[3], EwGridCall &c,
                               double *ms) {
  hipStream_t s = h->stream;
  const int nk = h->ew_nk, nrow = nk > 0 ? h->ew_nrow : 0;
  std::vector<PlanI4> rows((size_t)nrow + 1, PlanI4{0, 0, 0, 0});
  if (nrow > 0) {
    HIPCHECK(hipMemcpyAsync(rows.data(), h->d_ew_rows.p, rows.size() * sizeof(int4), hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
  }
  c.plan = ew_grid_plan(rows.data(), nrow);
  if (!c.plan.ok) throw std::runtime_error(name + ": the k-vector table is not in (h, k) order");
  EwGrid &g = c.g;
  for (int a = 0; a < 3; a++) { g.n[a] = n[a]; g.off[a] = off[a]; g.lo[a] = h->boxlo[a]; }
  g.ax = h->box.prd[0]; g.bx = h->box.xy; g.by = h->box.prd[1]; g.cx = h->box.xz; g.cy = h->box.yz; g.cz = h->box.prd[2];
  ew_grid_slo(h->ew_cell, h->boxlo, g.slo);
  c.sz = ew_grid_sizes(c.plan, nrow, n, nset);
  c.lines_per_run = ew_grid_lines_per_run(c.sz.v_line_bytes);
  const int nzb = nblk(n[2], 64);
  if ((long long)nrow * nzb > 2147483647LL || (c.sz.tab + 255) / 256 > (size_t)2147483647)
    throw InputError(name + ": the grid is too large for the k-vector table's stage-1 launch");
  h->d_eg_tab.ensure(c.sz.tab); h->d_eg_t.ensure(c.sz.t); h->d_eg_first.ensure(c.plan.first.size());
  if (!h->ev_fa[0].e) { h->ev_fa[0].create(); h->ev_fa[1].create(); }
  if (!h->ev_fa_k.e) h->ev_fa_k.create();
  HIPCHECK(hipMemcpyAsync(h->d_eg_first.p, c.plan.first.data(), c.plan.first.size() * sizeof(int), hipMemcpyHostToDevice, s));
  HIPCHECK(hipEventRecord(h->ev_fa[1], s));
  k_ew_grid_tab<<<(unsigned)((c.sz.tab + 255) / 256), 256, 0, s>>>(c.sz.tab, g, c.plan.kmax, c.plan.lmax, c.sz.off_y, c.sz.off_z, h->d_eg_tab.p);
  if (nrow > 0) {
    if (nset == EW_GG_SETS) k_ew_gg_l<<<nrow * nzb, 64, 0, s>>>(nrow, n[2], nzb, c.plan.lmax, h->d_ew_rows.p, h->d_ew_kv.p, h->d_ew_s.p, h->d_eg_tab.p + c.sz.off_z, h->d_eg_t.p);
    else                    k_ew_grid_l<<<nrow * nzb, 64, 0, s>>>(nrow, n[2], nzb, c.plan.lmax, h->d_ew_rows.p, h->d_ew_kv.p, h->d_ew_s.p, h->d_eg_tab.p + c.sz.off_z, h->d_eg_t.p);
  }
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipEventRecord(h->ev_fa_k, s));
  HIPCHECK(hipStreamSynchronize(s));   // (c.plan.first has gone up)
  float tk = 0.f;
  HIPCHECK(hipEventElapsedTime(&tk, h->ev_fa[1], h->ev_fa_k));
  h->ew_fa_ms[1] += (double)tk;
  if (ms) *ms += (double)tk;
}
void ewald_field_grid_begin(polar_handle *h, const int n[3], const double off[3], EwGridCall &c, double *ms) {
  ew_grid_call_begin(h, "polar_ewald_field_grid", 4, n, off, c, ms);
}
void ewald_field_grad_grid_begin(polar_handle *h, const int n[3], const double off[3], EwGridCall &c, double *ms) {
  ew_grid_call_begin(h, "polar_ewald_field_grad_grid", EW_GG_SETS, n, off, c, ms);
}

// ... and one pass, the points [p0, p0 + m) of the flat order: k_ew_grid_points writes them into d_fa_x, k_ew_point_real adds
// the real-space static sums and the induced sums as for polar_ewald_field_at; then, per run of whole lines whose V stays within
// 64 MB (ew_grid_runs), stage 2 (k_ew_grid_k) and stage 3 with the fold (k_ew_grid_h).  Nothing of the handle's step state is
// written.
void ewald_field_grid_pass(polar_handle *h, const EwGridCall &c, long long p0, int m, double *x_out, double *e_static, double *e_induced,
                           double *phi_static, double *phi_induced, double *ms) {
  const bool phi = phi_static || phi_induced;
  hipStream_t s = h->stream;
  const size_t mm = (size_t)m;
  h->d_fa_x.ensure(3 * mm); h->d_fa_out.ensure(8 * mm);
  k_ew_grid_points<<<nblk(m, 256), 256, 0, s>>>(m, p0, c.g, h->d_fa_x.p);
  HIPCHECK(hipGetLastError());
  ew_point_real_launch(h, m, nullptr, nullptr, phi);
  const double g = h->P.g_ewald, e2s = std::sqrt(h->P.qqrd2e);
  const FieldAtOut out{h->d_fa_out.p};
  const double vol = h->box.prd[0] * h->box.prd[1] * h->box.prd[2];
  const double qterm = -3.14159265358979323846 / (g * g * vol);
  const int nx = c.g.n[0], ny = c.g.n[1], nz = c.g.n[2], hmax = c.plan.hmax;
  const std::vector<EwGridRun> runs = ew_grid_runs(p0, m, nx, c.lines_per_run);
  long long nl_max = 1;
  for (const EwGridRun &r : runs) nl_max = std::max(nl_max, r.lb - r.la);
  h->d_eg_v.ensure((size_t)nl_max * (size_t)(hmax + 1) * 4);
  const int nyb = nblk(ny, 64), nxb = nblk(nx, 64);
  for (const EwGridRun &r : runs) {
    const int nl = (int)(r.lb - r.la), gz0 = (int)(r.la / ny), ngz = (int)((r.lb - 1) / ny) - gz0 + 1;
    const long long bk = (long long)(hmax + 1) * ngz * nyb, bh = (long long)nl * nxb;
    if (bk > 2147483647LL || bh > 2147483647LL) throw InputError("polar_ewald_field_grid: a run of lines is too large for one launch");
    k_ew_grid_k<<<(unsigned)bk, 64, 0, s>>>(r.la, r.lb, gz0, ngz, nyb, nz, ny, c.plan.kmax, h->d_eg_first.p, h->d_ew_rows.p, h->d_eg_t.p,
                                           h->d_eg_tab.p + c.sz.off_y, h->d_eg_v.p);
    if (phi) k_ew_grid_h<true><<<(unsigned)bh, 64, 0, s>>>(r.q0, r.q1, r.la, nl, nx, nxb, hmax, h->d_eg_v.p, h->d_eg_tab.p, p0, m, e2s, qterm, h->d_fa_q.p, out);
    else     k_ew_grid_h<false><<<(unsigned)bh, 64, 0, s>>>(r.q0, r.q1, r.la, nl, nx, nxb, hmax, h->d_eg_v.p, h->d_eg_tab.p, p0, m, e2s, qterm, h->d_fa_q.p, out);
  }
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipEventRecord(h->ev_fa_k, s));
  if (x_out) HIPCHECK(hipMemcpyAsync(x_out, h->d_fa_x.p, 3 * mm * sizeof(double), hipMemcpyDeviceToHost, s));
  field_out_finish(h, m, e_static, e_induced, phi_static, phi_induced, true, ms);
}

// polar_ewald_field_grad_grid, one pass, the points [p0, p0 + m) of the flat order: k_ew_grid_points writes them into d_fa_x,
// k_ew_grad_real adds the real-space static sums and the induced sums into the block in d_fg_out as for
// polar_ewald_field_grad_at; then, per run of whole lines whose V -- nine sets -- stays within 64 MB (ew_grid_runs), stage 2
// (k_ew_gg_k) and stage 3 with the fold (k_ew_gg_h) of polar_ewald_field_grad_grid.hpp.  T and V live in the buffers of
// polar_ewald_field_grid (d_eg_*: the two calls do not overlap).  Nothing of the handle's step state is written.
void ewald_field_grad_grid_pass(polar_handle *h, const EwGridCall &c, long long p0, int m, double *x_out, double *g_static,
                                double *g_induced, double *e_static, double *e_induced, double *ms) {
  hipStream_t s = h->stream;
  const size_t mm = (size_t)m;
  h->d_fa_x.ensure(3 * mm); h->d_fg_out.ensure(POLAR_FIELD_GRAD_DOUBLES * mm);
  k_ew_grid_points<<<nblk(m, 256), 256, 0, s>>>(m, p0, c.g, h->d_fa_x.p);
  HIPCHECK(hipGetLastError());
  ew_grad_real_launch(h, m, nullptr, nullptr);
  const double e2s = std::sqrt(h->P.qqrd2e);
  const FieldGradOut out{h->d_fg_out.p};
  const int nx = c.g.n[0], ny = c.g.n[1], nz = c.g.n[2], hmax = c.plan.hmax;
  const std::vector<EwGridRun> runs = ew_grid_runs(p0, m, nx, c.lines_per_run);
  long long nl_max = 1;
  for (const EwGridRun &r : runs) nl_max = std::max(nl_max, r.lb - r.la);
  h->d_eg_v.ensure((size_t)nl_max * (size_t)(hmax + 1) * EW_GG_SETS);
  const int nyb = nblk(ny, 64), nxb = nblk(nx, 64);
  for (const EwGridRun &r : runs) {
    const int nl = (int)(r.lb - r.la), gz0 = (int)(r.la / ny), ngz = (int)((r.lb - 1) / ny) - gz0 + 1;
    const long long bk = (long long)(hmax + 1) * ngz * nyb, bh = (long long)nl * nxb;
    if (bk > 2147483647LL || bh > 2147483647LL) throw InputError("polar_ewald_field_grad_grid: a run of lines is too large for one launch");
    k_ew_gg_k<<<(unsigned)bk, 64, 0, s>>>(r.la, r.lb, gz0, ngz, nyb, nz, ny, c.plan.kmax, h->d_eg_first.p, h->d_ew_rows.p, h->d_eg_t.p,
                                         h->d_eg_tab.p + c.sz.off_y, h->d_eg_v.p);
    if (e_static) k_ew_gg_h<true><<<(unsigned)bh, 64, 0, s>>>(r.q0, r.q1, r.la, nl, nx, nxb, hmax, h->d_eg_v.p, h->d_eg_tab.p, p0, m, e2s, out);
    else          k_ew_gg_h<false><<<(unsigned)bh, 64, 0, s>>>(r.q0, r.q1, r.la, nl, nx, nxb, hmax, h->d_eg_v.p, h->d_eg_tab.p, p0, m, e2s, out);
  }
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipEventRecord(h->ev_fa_k, s));
  if (x_out) HIPCHECK(hipMemcpyAsync(x_out, h->d_fa_x.p, 3 * mm * sizeof(double), hipMemcpyDeviceToHost, s));
  point_finish(h, {{e_static, out.es(), 3 * mm}, {e_induced, out.ei(mm), 3 * mm}, {g_static, out.gs(mm), 6 * mm}, {g_induced, out.gi(mm), 6 * mm}}, true, ms);
}
