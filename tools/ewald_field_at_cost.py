#!/usr/bin/env python
"""Cost of polar_ewald_field_at on the MI355X, measured and printed -- not part of the test suite, no threshold.

Two workloads of bench.py with `polar_ewald 1e-6`: BASELINE configs[2] (the MOF5+H2 cell replicated 5x5x4 = 134,900 atoms, list
mode, dd_cutoff = cut_coul) and configs[0] (the 1,349-atom cell, exact mode), each with a 64^3 grid.  Each: warm-up steps and one
warm-up grid, then five grids; the device time of the real-space kernel and of the reciprocal kernels (HIP events) separately.

Beside them:
  * ns per (point, k) term of the reciprocal kernels, and ns per (atom, k) term of the same handle's step: the field half of the
    step's reciprocal work (structure factors and k_ew_field), timed by the event pair around it in the same run
    (polar_pair_extract "ewald_field_ms") -- not ms_kspace, which includes the forces;
  * the real-space kernel against k_field_at on the same handle, the same grid, with the keyword off (polar_ewald 0).
Prints one JSON line per workload.

    python tools/ewald_field_at_cost.py [--grid-list 64] [--grid-exact 64] [--repeats 5] [--only list|exact]"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "lammps-induced-dipole-polarization-pair-style_amd"
CUT = 12.8345
ACC = "1e-6"


def _extract(p, name):
    ptr = p.L.polar_pair_extract(p.h, name.encode(), C.byref(C.c_int()))
    return C.cast(C.c_void_p(ptr), C.POINTER(C.c_double))[0]


def measure(pkg, s, shape, repeats, label, device_neigh):
    p = pkg.pair_from_system(s, device_neigh=device_neigh)
    for _ in range(2):
        p.compute_resident(eflag=1, vflag=2)
    steps, field_ms = [], []
    for _ in range(3):
        steps.append(p.compute_resident(eflag=1, vflag=2))
        field_ms.append(_extract(p, "ewald_field_ms"))
    step = steps[-1]
    nk = step["nkvec"]
    pts = p.grid_points(shape)
    npts = len(pts)
    p.ewald_field_at(pts)                                   # warm-up: buffers, code objects
    runs = [p.ewald_field_at(pts) for _ in range(repeats)]
    runs_field_only = [p.ewald_field_at(pts, potential=False) for _ in range(repeats)]
    med = lambda key, rr=runs: float(np.median([r[key] for r in rr]))   # noqa: E731
    ms_real, ms_recip = med("ms_real"), med("ms_recip")
    step_field = float(np.median(field_ms))
    # the same handle with the keyword off: k_field_at on the same grid
    st = p.get_settings()
    st.polar_ewald = 0.0
    p._ck(p.L.polar_set_settings(p.h, C.byref(st)))
    p.compute_resident(eflag=1, vflag=2)
    p.field_at(pts)
    ms_plain = float(np.median([p.field_at(pts)["ms"] for _ in range(repeats)]))
    out = dict(workload=label, natoms=s.nlocal, grid=list(shape), points=npts, nkvec=nk, accuracy=float(ACC),
               ms_real=[round(r["ms_real"], 3) for r in runs], ms_recip=[round(r["ms_recip"], 3) for r in runs],
               ms_real_median=ms_real, ms_recip_median=ms_recip, ms_total_median=med("ms"),
               ms_real_field_only_median=med("ms_real", runs_field_only), ms_recip_field_only_median=med("ms_recip", runs_field_only),
               point_k_terms=float(npts) * nk, ns_per_point_k=1e6 * ms_recip / (float(npts) * nk),
               step_ewald_field_ms=step_field, atom_k_terms=float(s.nlocal) * nk, ns_per_atom_k=1e6 * step_field / (float(s.nlocal) * nk),
               step_ms_kspace=step["ms_kspace"], k_field_at_ms_keyword_off=ms_plain, real_over_k_field_at=ms_real / ms_plain,
               us_per_point=1e3 * med("ms") / npts)
    p.close()
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid-list", type=int, default=64)
    ap.add_argument("--grid-exact", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", choices=["list", "exact"], default=None)
    a = ap.parse_args()
    pkg = importlib.import_module(PKG)
    wl = importlib.import_module(PKG + ".workload")
    if pkg.device_count() < 1:
        raise SystemExit("ewald_field_at_cost.py needs an MI355X: there is nothing to measure without one")
    fixture = os.path.join(ROOT, "tests", "golden", "mof5_h2.npz")
    if a.only != "exact":
        s = wl.replicate_fixture(fixture, 5, 5, 4, extra_args=["use_previous", "no", "polar_gs_ranked", "yes", "dd_cutoff", repr(CUT), "fixed_iteration", "no",
                                                               "precision", "1e-11", "max_iterations", "100", "polar_ewald", ACC], build_list=False)
        g = a.grid_list
        measure(pkg, s, (g, g, g), a.repeats, "BASELINE configs[2]: MOF5+H2 5x5x4, list mode, polar_ewald 1e-6", True)
    if a.only != "list":
        s, _ = wl.load_fixture(fixture, extra_args=["use_previous", "no", "polar_gs_ranked", "yes", "precision", "1e-11", "max_iterations", "30", "polar_ewald", ACC])
        g = a.grid_exact
        measure(pkg, s, (g, g, g), a.repeats, "BASELINE configs[0]: MOF5+H2 1,349 atoms, exact mode, polar_ewald 1e-6", False)


if __name__ == "__main__":
    main()
