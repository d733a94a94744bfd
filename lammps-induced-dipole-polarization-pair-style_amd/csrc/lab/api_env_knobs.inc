// lab/api_env_knobs.inc -- LAB BUILD ONLY (-DPOLAR_LAB, libpolar_mi355x_lab.so): code that was built, measured and did not become the
// product path (DESIGN.md section 4).  Included by polar_api.hip inside `#ifdef POLAR_LAB`; the product library never sees it.
// No include guard: it is a fragment of polar_api.hip, textually in that file's scope.
  if (const char *e = getenv("POLAR_ABLATE")) h->ablate = atoi(e);
  if (const char *e = getenv("POLAR_HOST_COLORS")) h->host_colors = atoi(e) != 0;
  if (const char *e = getenv("POLAR_SWEEP_KERNEL")) h->sweep_kernel = atoi(e);
  if (const char *e = getenv("POLAR_TILE_WAVES")) h->tile_waves = atoi(e) == 8 ? 8 : 4;
  if (const char *e = getenv("POLAR_TILE_WIDE")) h->tile_wide = atoi(e) != 0;
  if (const char *e = getenv("POLAR_CACHE_R2")) h->cache_r2 = atoi(e);
  if (const char *e = getenv("POLAR_LJ_TYPED")) h->lj_typed = atoi(e) != 0;
  if (const char *e = getenv("POLAR_STATIC_XQ")) h->static_xq = atoi(e) != 0;
  if (const char *e = getenv("POLAR_POL_FIRST")) h->pol_first = atoi(e) != 0;
  if (const char *e = getenv("POLAR_LP_WG_PER_CU")) h->lp_wg_per_cu = atoi(e);
  if (const char *e = getenv("POLAR_LP_QM")) h->lp_quad_major = atoi(e) != 0;
  if (const char *e = getenv("POLAR_LP_TILES")) h->lp_tiles = atoi(e) == 1 ? 1 : 2;
  if (const char *e = getenv("POLAR_LP_ROWS")) h->lp_rows = std::max(1, std::min(64, atoi(e)));
  if (const char *e = getenv("POLAR_LP_PAIRS")) h->lp_pairs = atoi(e) != 0;
  if (const char *e = getenv("POLAR_CLUSTER_DIST")) h->cluster_dist = atof(e);
  if (const char *e = getenv("POLAR_CLUSTER_MAX")) h->cluster_max = std::max(1, std::min(4, atoi(e)));
  if (const char *e = getenv("POLAR_LP_DEPTH")) { int v = atoi(e); h->lp_depth = (v == 2 || v == 3) ? v : 0; }
  if (const char *e = getenv("POLAR_QUAD_BLOCK")) { int v = atoi(e); if (v >= 64 && v <= 1024 && v % 64 == 0) h->quad_block = v; }
  if (const char *e = getenv("POLAR_FIELD_BLOCK")) { int v = atoi(e); if (v >= 64 && v <= 1024 && v % 64 == 0) h->field_block = v; }
  if (const char *e = getenv("POLAR_FORCE_LITERAL")) h->force_literal = atoi(e) != 0;
  if (const char *e = getenv("POLAR_NL_DENSE")) h->nl_dense = atoi(e) != 0;
