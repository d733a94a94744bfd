#!/usr/bin/env python
"""Cost of polar_ewald_field_grad_at on the MI355X beside polar_ewald_field_at on the same handle and grid in the same run,
alternating, measured and printed -- not part of the test suite, no threshold.

The workloads of tools/ewald_field_at_cost.py, with `polar_ewald 1e-6`: BASELINE configs[2] (the MOF5+H2 cell replicated 5x5x4 =
134,900 atoms, list mode, dd_cutoff = cut_coul) and configs[0] (the 1,349-atom cell, exact mode), each with a 64^3 grid.  Each:
two warm-up steps and one warm-up grid per call, then five rounds of (gradient call, field call); the device time of the
real-space kernel and of the reciprocal kernels (HIP events) separately.  ewald_field_at runs without the potentials: the
gradient call computes none.  Prints one JSON line per workload with the medians and the two ratios.

    python tools/ewald_field_grad_at_cost.py [--grid-list 64] [--grid-exact 64] [--repeats 5] [--only list|exact]"""
import argparse
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


def measure(pkg, s, shape, repeats, label, device_neigh):
    p = pkg.pair_from_system(s, device_neigh=device_neigh)
    for _ in range(2):
        step = p.compute_resident(eflag=1, vflag=2)
    pts = p.grid_points(shape)
    p.ewald_field_grad_at(pts, field=False)                 # warm-up: buffers, code objects
    p.ewald_field_at(pts, potential=False)
    grad, field = [], []
    for _ in range(repeats):
        grad.append(p.ewald_field_grad_at(pts, field=False))
        field.append(p.ewald_field_at(pts, potential=False))
    p.close()
    med = lambda rr, key: float(np.median([r[key] for r in rr]))   # noqa: E731
    out = dict(workload=label, natoms=s.nlocal, grid=list(shape), points=len(pts), nkvec=step["nkvec"], accuracy=float(ACC))
    for key in ("ms_real", "ms_recip", "ms"):
        out["grad_" + key] = [round(r[key], 3) for r in grad]
        out["field_" + key] = [round(r[key], 3) for r in field]
        out["grad_%s_median" % key], out["field_%s_median" % key] = med(grad, key), med(field, key)
        out["ratio_" + key] = med(grad, key) / med(field, key)
    out["ns_per_point_k"] = 1e6 * med(grad, "ms_recip") / (float(len(pts)) * step["nkvec"])
    out["us_per_point"] = 1e3 * med(grad, "ms") / len(pts)
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
        raise SystemExit("ewald_field_grad_at_cost.py needs an MI355X: there is nothing to measure without one")
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
