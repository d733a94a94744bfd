// lab/build_cluster_lists.inc -- LAB BUILD ONLY (-DPOLAR_LAB, libpolar_mi355x_lab.so): code that was built, measured and did not become the
// product path (DESIGN.md section 4).  Included by polar_step.hip inside `#ifdef POLAR_LAB`; the product library never sees it.
// No include guard: it is a fragment of polar_step.hip, textually in that file's scope.
// cluster mode, per step: members -> s space, union lists, descriptors (needs the colours AND this step's cell order)
void build_cluster_lists(polar_handle *h) {
  const polar_settings &st = h->ph.st;
  hipStream_t s = h->stream;
  const int ncl = h->ncl;
  if (h->cl_pitch == 0) h->cl_pitch = ((h->dd_pitch * 5 / 4 + 255) / 256) * 256;
  h->d_cl_cnt.ensure(ncl + 1); h->d_cl_wrap.ensure(ncl + 1); h->d_cl_tw.ensure(ncl + 1);
  h->d_dd_j.ensure((size_t)std::max(ncl, 1) * h->cl_pitch + 256);
  if (ncl <= 0) return;
  k_map_rows_pad<<<nblk(4 * (long long)ncl, 256), 256, 0, s>>>(4 * ncl, h->d_inv.p, h->d_cl_orig.p, reinterpret_cast<int *>(h->d_cl_s.p));
  zero_many(s, {{h->d_overflow.p + 4, 4 * sizeof(int)}, {h->d_ddtot.p, 64 * 16 * sizeof(unsigned long long)}});
  k_cl_build<<<nblk(ncl, POLAR_ROWS_PER_BLOCK), POLAR_BLOCK, 0, s>>>(
      ClusterRows{h->d_cl_s.p, ncl}, h->d_pos4.p, h->box, h->grid, h->d_cell_first.p, st.dd_cutoff * st.dd_cutoff, h->cl_pitch,
      h->d_cl_cnt.p, h->d_dd_j.p, h->nlocal, h->d_cl_wrap.p, h->d_overflow.p + 4, h->d_ddtot.p);
  k_cl_desc<<<nblk(ncl, 256), 256, 0, s>>>(ncl, h->d_cl_cnt.p, h->cl_pitch, h->d_cl_wrap.p, h->d_cl_tw.p);
  HIPCHECK(hipMemcpyAsync(h->h_flags.p + 4, h->d_overflow.p + 4, sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHECK(hipMemcpyAsync(h->h_ddtot.p, h->d_ddtot.p, 64 * 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
}

