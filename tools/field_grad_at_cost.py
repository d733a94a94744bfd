#!/usr/bin/env python
"""Cost of polar_field_grad_at on the MI355X beside polar_field_at on the same grids in the same run, measured and printed -- not
part of the test suite, no threshold.

The workloads of tools/field_at_cost.py: BASELINE configs[2] (the MOF5+H2 cell replicated 5x5x4 = 134,900 atoms, list mode,
dd_cutoff = cut_coul) with a 64^3 and a 128^3 grid, and configs[0] (the 1,349-atom cell, exact mode) with a 64^3 grid.  Each:
two warm-up steps and one warm-up grid per call, then five grids per call; device_ms is the device time of the call's kernel (HIP
events).  field_at runs without the potentials: the gradient call computes none.  Prints one JSON line per (workload, grid) with
both medians and their ratio.

    python tools/field_grad_at_cost.py [--repeats 5] [--only list|exact]"""
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


def measure(pkg, s, shapes, repeats, label, device_neigh):
    p = pkg.pair_from_system(s, device_neigh=device_neigh)
    for _ in range(2):
        p.compute_resident(eflag=1, vflag=2)
    for shape in shapes:
        pts = p.grid_points(shape)
        p.field_grad_at(pts, field=False)              # warm-up: buffers, code objects
        p.field_at(pts, potential=False)
        ms_g = [p.field_grad_at(pts, field=False)["ms"] for _ in range(repeats)]
        ms_f = [p.field_at(pts, potential=False)["ms"] for _ in range(repeats)]
        mg, mf = float(np.median(ms_g)), float(np.median(ms_f))
        print(json.dumps(dict(workload=label, natoms=s.nlocal, grid=list(shape), points=len(pts), field_grad_at_ms=[round(v, 3) for v in ms_g],
                              field_at_ms=[round(v, 3) for v in ms_f], field_grad_at_ms_median=mg, field_at_ms_median=mf,
                              ratio=mg / mf, us_per_point=1e3 * mg / len(pts))), flush=True)
    p.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", choices=["list", "exact"], default=None)
    a = ap.parse_args()
    pkg = importlib.import_module(PKG)
    wl = importlib.import_module(PKG + ".workload")
    if pkg.device_count() < 1:
        raise SystemExit("field_grad_at_cost.py needs an MI355X: there is nothing to measure without one")
    fixture = os.path.join(ROOT, "tests", "golden", "mof5_h2.npz")
    if a.only != "exact":
        s = wl.replicate_fixture(fixture, 5, 5, 4, extra_args=["use_previous", "no", "polar_gs_ranked", "yes", "dd_cutoff", repr(CUT), "fixed_iteration", "no",
                                                               "precision", "1e-11", "max_iterations", "100"], build_list=False)
        measure(pkg, s, [(64, 64, 64), (128, 128, 128)], a.repeats, "BASELINE configs[2]: MOF5+H2 5x5x4, list mode", True)
    if a.only != "list":
        s, _ = wl.load_fixture(fixture, extra_args=["use_previous", "no", "polar_gs_ranked", "yes", "precision", "1e-11", "max_iterations", "30"])
        measure(pkg, s, [(64, 64, 64)], a.repeats, "BASELINE configs[0]: MOF5+H2 1,349 atoms, exact mode", False)


if __name__ == "__main__":
    main()
