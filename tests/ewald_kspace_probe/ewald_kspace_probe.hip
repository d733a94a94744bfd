// ewald_kspace_probe.hip -- TEST INFRASTRUCTURE (tests/test_gpu_ewald_kspace.py compiles it into its tmp_path).
//
// The six reciprocal-space kernels of csrc/polar_ewald.hpp, launched as polar_step.hip launches them, on records filled
// from plain arrays: k_ew_sfac<false> + k_ew_fold (S), k_ew_field, k_ew_sfac<true> + k_ew_fold (M), k_ew_force,
// k_ew_kvirial, k_ew_finish.  No arithmetic of its own: the k-vector table is polar::ewald_kvectors', the tiling
// ewald_tile / ewald_lds_per_atom / ewald_sfac_chunks' (polar_plan.hpp) unless the caller overrides tile or chunk.
//
// The launch geometry mirrors csrc/polar_step.hip line for line (line numbers as of this file's writing):
//   sfac()   below = ewald_sfac,   lines 468-480 (tile, lds, chunks, grid(kb, nchunk), the null scal of the <false> launch,
//                                  k_ew_fold<<<kb, 256>>>; nothing when nk == 0)
//   stage 1  below = ewald_field,  lines 483-494 (S, then k_ew_field<<<nblk(n, 256), 256>>> on the first records when n > 0
//                                  and nk > 0, a memset of erec when nk == 0)
//   stage 2  below = ewald_forces, lines 498-511 (M, nba = nblk(max(n, 1), 256), nbk = nk > 0 ? nblk(nk, 256) : 0, k_ew_force
//                                  with nrow 0 when nk == 0, k_ew_kvirial behind the atom partials, k_ew_finish<<<1, 256>>>)
// The overrides replace `tile` and `chunk` alone (nchunk follows as in ewald_sfac_chunks); everything else is as above.
//
// Every device output buffer (part, S, M, erec, f, vpart, out) ends in GUARD doubles of a fixed bit pattern and starts
// filled with it (f: with f0), so a write past the end and an entry never written both show.  The records carry `pad`
// more atoms with unit charge and dipole behind the n real ones, which no correct kernel reads.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "polar_common.hpp"
#include "polar_ewald.hpp"
#include "polar_plan.hpp"

using namespace polar;

static_assert(sizeof(PlanD4) == sizeof(double4) && sizeof(PlanI4) == sizeof(int4), "polar_plan.hpp's vectors go to the device as bytes");

namespace {

constexpr int GUARD = 64;
constexpr unsigned long long GUARD_BITS = 0x7ff8c0dedeadbeefull;   // a quiet NaN that no kernel produces

Box make_box(const double *prd, const double *tilt) {
  Box b;
  for (int k = 0; k < 3; k++) { b.prd[k] = prd[k]; b.half[k] = 0.5 * prd[k]; b.inv[k] = 1.0 / prd[k]; b.periodic[k] = 1; }
  b.xy = tilt[0]; b.xz = tilt[1]; b.yz = tilt[2];
  b.triclinic = (tilt[0] != 0.0 || tilt[1] != 0.0 || tilt[2] != 0.0) ? 1 : 0;
  return b;
}

// a device array of `count` doubles and GUARD more, all holding GUARD_BITS
struct Guarded {
  double *p = nullptr;
  size_t count = 0;
  hipError_t alloc(size_t n) {
    count = n;
    std::vector<unsigned long long> fill(n + GUARD, GUARD_BITS);
    hipError_t e = hipMalloc(&p, sizeof(double) * (n + GUARD));
    if (e == hipSuccess) e = hipMemcpy(p, fill.data(), sizeof(double) * (n + GUARD), hipMemcpyHostToDevice);
    return e;
  }
  // copies the first `count` doubles to dst (if any) and says through `ok` whether the guard words are as they were
  hipError_t fetch(double *dst, bool &ok) const {
    unsigned long long g[GUARD];
    hipError_t e = hipMemcpy(g, p + count, sizeof(g), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return e;
    for (int k = 0; k < GUARD; k++) ok = ok && g[k] == GUARD_BITS;
    if (dst && count) e = hipMemcpy(dst, p, sizeof(double) * count, hipMemcpyDeviceToHost);
    return e;
  }
  void release() { if (p) (void)hipFree(p); p = nullptr; }
};

}  // namespace

// the k-vector table's sizes and the plan's own tiling for n atoms; host only
extern "C" int ewald_kspace_probe_plan(const double *prd, const double *tilt, double g, double acc, int n, int *nk, int *nrow, int *nm,
                                       int *tile, int *kb, int *nchunk, int *chunk) {
  const EwaldPlan p = ewald_kvectors(make_box(prd, tilt), g, acc);
  *nk = p.nk; *nrow = p.nrow; *nm = p.nm;
  *tile = ewald_tile(p.nm);
  const SfacChunks ck = ewald_sfac_chunks(n, p.nk, *tile);
  *kb = ck.kb; *nchunk = ck.nchunk; *chunk = ck.chunk;
  return 0;
}

// x [n][3], q [n], muA [n][3], muB [n][3], perm [n] or NULL, ef_s [n][3], f0 [n][3] in; tile_override / chunk_override: 0 = the
// plan's.  kv [nk][4], hkl [nk][4], rows [nrow + 1][4], S [nk][2], M [nk][2], erec [n][3], f [n][3], out [7] out (host arrays
// sized from ewald_kspace_probe_plan).  Returns 0, a HIP error code (> 0; nothing is launched after the first), or -1
// when every call succeeded and a guard word behind one of the device buffers changed.
extern "C" int ewald_kspace_probe_run(const double *prd, const double *tilt, double g, double acc, double e2s, int n, const double *x,
                                      const double *q, const double *muA, const double *muB, int cur, const int *perm,
                                      const double *ef_s, const double *f0, int tile_override, int chunk_override, double *kv_out,
                                      int *hkl_out, int *rows_out, double *S_out, double *M_out, double *erec_out, double *f_out,
                                      double *out_out) {
  const EwaldPlan plan = ewald_kvectors(make_box(prd, tilt), g, acc);
  const int nk = plan.nk, nrow = plan.nrow, nm = plan.nm;
  const EwCell cell{plan.cell[0], plan.cell[1], plan.cell[2], plan.cell[3], plan.cell[4], plan.cell[5]};
  if (nk) {
    std::memcpy(kv_out, plan.kv.data(), sizeof(PlanD4) * (size_t)nk);
    std::memcpy(hkl_out, plan.hkl.data(), sizeof(PlanI4) * (size_t)nk);
  }
  std::memcpy(rows_out, plan.rows.data(), sizeof(PlanI4) * ((size_t)nrow + 1));

  // tiling: the plan's (ewald_sfac), or the caller's
  const int tile = tile_override > 0 ? tile_override : ewald_tile(nm);
  const size_t lds = (size_t)tile * ewald_lds_per_atom(nm);
  SfacChunks ck = ewald_sfac_chunks(n, nk, tile);
  if (chunk_override > 0) { ck.chunk = chunk_override; ck.nchunk = nblk(std::max(n, 1), ck.chunk); }
  const int kb = ck.kb, nchunk = ck.nchunk, chunk = ck.chunk;
  if (lds > 64 * 1024) return (int)hipErrorInvalidValue;   // (ewald_check's limit)

  // records: recA with muA, recB with muB, the same x, q, a; behind them `pad` atoms that nothing may read
  const int pad = std::max(tile, 32);
  std::vector<AtomRec> ra((size_t)n + pad), rb((size_t)n + pad);
  for (int i = 0; i < n + pad; i++) {
    AtomRec r;
    if (i < n) { r.x = x[3 * i]; r.y = x[3 * i + 1]; r.z = x[3 * i + 2]; r.q = q[i]; r.a = 1.0; r.mx = muA[3 * i]; r.my = muA[3 * i + 1]; r.mz = muA[3 * i + 2]; }
    else { r.x = 0.3 * i; r.y = 0.7 * i; r.z = 1.1 * i; r.q = 1.0; r.a = 1.0; r.mx = r.my = r.mz = 1.0; }
    ra[i] = r;
    if (i < n) { r.mx = muB[3 * i]; r.my = muB[3 * i + 1]; r.mz = muB[3 * i + 2]; }
    rb[i] = r;
  }
  Scal scal;
  std::memset(&scal, 0, sizeof(scal));
  scal.cur = cur;

  const int nba = nblk(std::max(n, 1), 256), nbk = nk > 0 ? nblk(nk, 256) : 0;
  AtomRec *d_recA = nullptr, *d_recB = nullptr;
  Scal *d_scal = nullptr;
  double4 *d_kv = nullptr;
  int4 *d_hkl = nullptr, *d_rows = nullptr;
  int *d_perm = nullptr;
  double *d_efs = nullptr;
  Guarded part, S, M, erec, f, vpart, out;
  hipError_t e = hipSuccess;
  bool intact = true;
#define PROBE_TRY(call) if (e == hipSuccess) e = (call)
#define PROBE_LAUNCH(...) if (e == hipSuccess) { __VA_ARGS__; e = hipGetLastError(); }
  PROBE_TRY(hipMalloc(&d_recA, sizeof(AtomRec) * ra.size()));
  PROBE_TRY(hipMalloc(&d_recB, sizeof(AtomRec) * rb.size()));
  PROBE_TRY(hipMalloc(&d_scal, sizeof(Scal)));
  PROBE_TRY(hipMalloc(&d_kv, sizeof(double4) * ((size_t)nk + 1)));
  PROBE_TRY(hipMalloc(&d_hkl, sizeof(int4) * ((size_t)nk + 1)));
  PROBE_TRY(hipMalloc(&d_rows, sizeof(int4) * ((size_t)nrow + 1)));
  PROBE_TRY(hipMalloc(&d_efs, sizeof(double) * (3 * (size_t)n + 3)));
  PROBE_TRY(hipMemcpy(d_recA, ra.data(), sizeof(AtomRec) * ra.size(), hipMemcpyHostToDevice));
  PROBE_TRY(hipMemcpy(d_recB, rb.data(), sizeof(AtomRec) * rb.size(), hipMemcpyHostToDevice));
  PROBE_TRY(hipMemcpy(d_scal, &scal, sizeof(Scal), hipMemcpyHostToDevice));
  if (nk) {
    PROBE_TRY(hipMemcpy(d_kv, plan.kv.data(), sizeof(double4) * (size_t)nk, hipMemcpyHostToDevice));
    PROBE_TRY(hipMemcpy(d_hkl, plan.hkl.data(), sizeof(int4) * (size_t)nk, hipMemcpyHostToDevice));
  }
  PROBE_TRY(hipMemcpy(d_rows, plan.rows.data(), sizeof(int4) * ((size_t)nrow + 1), hipMemcpyHostToDevice));
  if (n) PROBE_TRY(hipMemcpy(d_efs, ef_s, sizeof(double) * 3 * (size_t)n, hipMemcpyHostToDevice));
  if (perm && n) {
    PROBE_TRY(hipMalloc(&d_perm, sizeof(int) * (size_t)n));
    PROBE_TRY(hipMemcpy(d_perm, perm, sizeof(int) * (size_t)n, hipMemcpyHostToDevice));
  }
  PROBE_TRY(part.alloc(2 * (size_t)nchunk * nk));
  PROBE_TRY(S.alloc(2 * (size_t)nk));
  PROBE_TRY(M.alloc(2 * (size_t)nk));
  PROBE_TRY(erec.alloc(3 * (size_t)n));
  PROBE_TRY(f.alloc(3 * (size_t)n));
  PROBE_TRY(vpart.alloc(8 * (size_t)(nba + nbk)));
  PROBE_TRY(out.alloc(7));
  if (n) PROBE_TRY(hipMemcpy(f.p, f0, sizeof(double) * 3 * (size_t)n, hipMemcpyHostToDevice));

  double2 *d_part = reinterpret_cast<double2 *>(part.p), *d_S = reinterpret_cast<double2 *>(S.p), *d_M = reinterpret_cast<double2 *>(M.p);
  auto sfac = [&](bool mu, double2 *dst) {   // ewald_sfac
    if (nk == 0) return;
    dim3 grid(kb, nchunk);
    if (mu) { PROBE_LAUNCH(k_ew_sfac<true><<<grid, 256, lds, 0>>>(nk, d_hkl, d_kv, n, chunk, tile, nm, cell, d_scal, d_recA, d_recB, d_part)); }
    else    { PROBE_LAUNCH(k_ew_sfac<false><<<grid, 256, lds, 0>>>(nk, d_hkl, d_kv, n, chunk, tile, nm, cell, nullptr, d_recA, d_recB, d_part)); }
    PROBE_LAUNCH(k_ew_fold<<<kb, 256, 0, 0>>>(nk, nchunk, d_part, dst));
  };
  // stage 1: ewald_field
  sfac(false, d_S);
  if (n > 0) {
    if (nk > 0) { PROBE_LAUNCH(k_ew_field<<<nblk(n, 256), 256, 0, 0>>>(n, nrow, d_rows, d_kv, d_S, cell, e2s, d_recA, erec.p)); }
    else PROBE_TRY(hipMemsetAsync(erec.p, 0, 3 * (size_t)n * sizeof(double), 0));
  }
  // stage 2: ewald_forces
  sfac(true, d_M);
  PROBE_LAUNCH(k_ew_force<<<nba, 256, 0, 0>>>(n, nk > 0 ? nrow : 0, d_rows, d_kv, d_S, d_M, cell, e2s, d_scal, d_recA, d_recB, d_perm, d_efs,
                                              erec.p, f.p, vpart.p));
  if (nbk) { PROBE_LAUNCH(k_ew_kvirial<<<nbk, 256, 0, 0>>>(nk, d_kv, d_S, d_M, e2s, 1.0 / (4.0 * g * g), vpart.p + 8 * (size_t)nba)); }
  PROBE_LAUNCH(k_ew_finish<<<1, 256, 0, 0>>>(nba + nbk, vpart.p, out.p));
  PROBE_TRY(hipDeviceSynchronize());
  PROBE_TRY(hipGetLastError());

  PROBE_TRY(part.fetch(nullptr, intact));
  PROBE_TRY(S.fetch(S_out, intact));
  PROBE_TRY(M.fetch(M_out, intact));
  PROBE_TRY(erec.fetch(erec_out, intact));
  PROBE_TRY(f.fetch(f_out, intact));
  PROBE_TRY(vpart.fetch(nullptr, intact));
  PROBE_TRY(out.fetch(out_out, intact));
#undef PROBE_LAUNCH
#undef PROBE_TRY
  part.release(); S.release(); M.release(); erec.release(); f.release(); vpart.release(); out.release();
  if (d_recA) (void)hipFree(d_recA);
  if (d_recB) (void)hipFree(d_recB);
  if (d_scal) (void)hipFree(d_scal);
  if (d_kv) (void)hipFree(d_kv);
  if (d_hkl) (void)hipFree(d_hkl);
  if (d_rows) (void)hipFree(d_rows);
  if (d_efs) (void)hipFree(d_efs);
  if (d_perm) (void)hipFree(d_perm);
  if (e != hipSuccess) return (int)e;
  return intact ? 0 : -1;
}
