// lab/launch_cluster_tile.inc -- LAB BUILD ONLY (-DPOLAR_LAB, libpolar_mi355x_lab.so): code that was built, measured and did not become the
// product path (DESIGN.md section 4).  Included by polar_step.hip inside `#ifdef POLAR_LAB`; the product library never sees it.
// No include guard: it is a fragment of polar_step.hip, textually in that file's scope.
// cluster sweep (k_field_cl): one wave per cluster, clusters [first, first + ncl) of the colour-sorted table
template <int EP>
void launch_field_cl(polar_handle *h, int ncl, int first) {
  if (ncl <= 0) return;
  const polar_settings &st = h->ph.st;
  const int qb = std::min(h->quad_block, 256);
  const int nt = h->lp_tiles;
  const size_t lds = (size_t)(qb / 64) * nt * POLAR_LP_TILE;
#define FC(D, NT) k_field_cl<EP, D, NT><<<nblk_xcd(ncl, qb / 64), qb, lds, h->stream>>>(                              \
      ncl, first, h->d_cl_s.p, h->d_cl_tw.p, h->d_rec0.p, h->d_rec1.p, h->box, h->cl_pitch, h->d_dd_j.p,              \
      st.dd_cutoff * st.dd_cutoff, st.polar_damp, make_expcoef(), h->d_ef_s.p, h->d_scal.p, h->d_slots.p, h->ablate)
  const bool expd = st.damping_type == POLAR_DAMP_EXPONENTIAL;
  if (nt == 1) { if (expd) FC(0, 1); else FC(1, 1); }
  else         { if (expd) FC(0, 2); else FC(1, 2); }
#undef FC
}

// ---- tile sweep: per-step tables (polar_tiles.hpp) ---------------------------------------------------
inline size_t tile_lds_bytes(int records) { return POLAR_TILE_LDS_REC + (size_t)(records + 1) * sizeof(SRec) + POLAR_TILE_LDS_SLACK; }
inline int tile_lds_cap() { return (int)((160 * 1024 - POLAR_TILE_LDS_REC - POLAR_TILE_LDS_SLACK - 256) / sizeof(SRec)) - 1; }  // records one workgroup can stage at all
void build_tiles(polar_handle *h) {
  const polar_settings &st = h->ph.st;
  const int n = h->nlocal;
  hipStream_t s = h->stream;
  const double rc = st.dd_cutoff;
  if (h->un_pitch == 0) {
    long long npol = 0;
    for (int a = 0; a < n; a++) npol += h->halpha[a] != 0.0;
    const double dens = (h->dens > 0.0 ? h->dens : n / (h->box.prd[0] * h->box.prd[1] * h->box.prd[2])) * (double)npol / std::max(n, 1);
    double e[3];
    for (int k = 0; k < 3; k++) e[k] = h->box.prd[k] / h->grid.nc[k];
    // what a cell's rows can see: the cell widened by the cutoff (Minkowski sum of a box and a sphere)
    const double vol = e[0] * e[1] * e[2] + 2.0 * (e[0] * e[1] + e[1] * e[2] + e[0] * e[2]) * rc + M_PI * (e[0] + e[1] + e[2]) * rc * rc +
                       4.18879020478639 * rc * rc * rc;
    h->un_pitch = (int)(((long long)(1.25 * dens * vol) + 64 + 63) / 64 * 64);
    h->pitch16 = ((long long)(1.5 * dens * 4.18879020478639 * rc * rc * rc) + 64 + 511) / 512 * 512;
    if (const char *ip = getenv("POLAR_INIT_PITCH")) {  // tests: force the overflow paths
      h->un_pitch = std::max(64, atoi(ip) / 64 * 64);
      h->pitch16 = 512;
    }
    h->un_lds = 0;
  }
  if (h->un_pitch > tile_lds_cap()) throw TileUnavailable("tile sweep: a cell's neighbourhood does not fit the LDS of a compute unit");
  if (h->un_lds <= 0 || h->un_lds > h->un_pitch) h->un_lds = h->un_pitch;
  const long long ncell = h->ncell;
  h->d_thdr.ensure((size_t)ncell + 1); h->d_trow.ensure((size_t)n + 1);
  {  // the sweep requests entry words before it knows how many a tile holds: the table never contains stale garbage
    const int *before = h->d_un_j.p;
    h->d_un_j.ensure((size_t)ncell * h->un_pitch + 64);
    if (h->d_un_j.p != before) HIPCHECK(hipMemsetAsync(h->d_un_j.p, 0, h->d_un_j.cap * sizeof(int), s));
  }
  h->d_dd16.ensure((size_t)std::max(n, 1) * h->pitch16 + 1024);
  h->d_srec0.ensure((size_t)n + 1); h->d_srec1.ensure((size_t)n + 1);
  if (deterministic(h)) h->d_pend.ensure(3 * (size_t)n + 3);
  // (build_lists has just zeroed the flag words and the pair totals; its own k_nl_build lists no dd pair in this mode)
  const size_t lds = 24 * (size_t)h->un_pitch + (4 * 128 + 2 * POLAR_TILE_MAXROWS) * sizeof(int) + 24 * sizeof(double) + 12 * sizeof(int) + 16;
  if (lds > h->tile_build_lds_attr) {
    HIPCHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_tile_build), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    h->tile_build_lds_attr = lds;
  }
  const int cap = std::min(h->un_pitch, h->un_lds);
  k_tile_build<<<(int)ncell, 256, lds, s>>>(h->grid, h->box, h->d_pos4.p, h->d_cell_first.p, h->d_cell_fill.p, h->d_perm.p, own_lo(h),
                                            own_lo(h) + own_n(h), rc * rc, h->color_dist * h->color_dist, h->tile_waves, h->tile_sw[0], h->tile_sw[1], h->tile_sw[2], cap, h->d_un_j.p, h->pitch16,
                                            h->d_dd16.p, h->d_thdr.p, h->d_trow.p, h->d_rec0.p, h->d_overflow.p, h->d_ddtot.p);
  HIPCHECK(hipMemcpyAsync(h->h_flags.p + 5, h->d_overflow.p + 5, 5 * sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHECK(hipMemcpyAsync(h->h_ddtot.p, h->d_ddtot.p, 64 * 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
}
// NOTE: the builder indexes the union lists with the pitch it is given (`cap`), so the sweep must use the same value
inline int tile_pitch(const polar_handle *h) { return std::min(h->un_pitch, h->un_lds); }

template <int EP>
void launch_field_tile(polar_handle *h, const TileLaunch &L) {
  const polar_settings &st = h->ph.st;
  const long long nt = (long long)L.count[0] * L.count[1] * L.count[2];
  if (nt <= 0) return;
  const bool expd = st.damping_type == POLAR_DAMP_EXPONENTIAL;
  const bool det = deterministic(h) && EP == EP_INPLACE;
  size_t lds = tile_lds_bytes(tile_pitch(h));
  if (const char *e = getenv("POLAR_TILE_LDS_PAD")) lds += (size_t)atoi(e);  // LAB (temporary): residency experiment
  const int inst = ((EP == EP_JACOBI ? 0 : (det ? 2 : 1)) * 2 + (expd ? 0 : 1)) * 2 + (h->tile_waves == 8 ? 1 : 0);
#define FT(D, DT, W)                                                                                                           \
  {                                                                                                                            \
    if (lds > h->tile_lds_attr[inst]) {                                                                                        \
      HIPCHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_field_tile<EP, D, DT, W>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); \
      h->tile_lds_attr[inst] = lds;                                                                                            \
    }                                                                                                                          \
    k_field_tile<EP, D, DT, W><<<nblk_xcd(nt, 1), 64 * W, lds, h->stream>>>(L, h->d_thdr.p, h->d_trow.p, h->d_un_j.p, tile_pitch(h),   \
        h->d_dd16.p, h->pitch16, h->d_srec0.p, h->d_srec1.p, h->d_pend.p, h->d_ef_s.p, h->box, st.polar_damp,       \
        make_expcoef(), h->d_scal.p, h->d_slots.p, h->nlocal);                                                                   \
  }
#define FW(D, DT) { if (h->tile_waves == 8) FT(D, DT, 8) else FT(D, DT, 4) }
  if (det) { if (expd) FW(0, true) else FW(1, true) }
  else     { if (expd) FW(0, false) else FW(1, false) }
#undef FW
#undef FT
  if (det) k_tile_commit<<<(int)nt, 64, 0, h->stream>>>(L, h->d_thdr.p, h->d_trow.p, h->d_pend.p, h->d_srec0.p, h->d_scal.p);
}

