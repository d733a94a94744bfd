#!/usr/bin/env python
"""Cost of polar_field_at on the MI355X, measured and printed -- not part of the test suite, no threshold.

Two workloads of bench.py: BASELINE configs[2] (the MOF5+H2 cell replicated 5x5x4 = 134,900 atoms, list mode,
dd_cutoff = cut_coul) with a 128^3 grid, and configs[0] (the 1,349-atom cell, exact mode) with a 64^3 grid.  Each: two warm-up
steps and one warm-up grid, then five grids; device_ms is the device time of the call's kernels (HIP events), points/s and
candidate pairs/s follow from it.  Candidate pairs per point: every atom in exact mode; in list mode the records of the +-2
cell stencil, estimated as atoms / cells x 125.

The yardstick beside them: a probe point's work is one static-field row plus one sweep row, so ms_static + one sweep
(ms_solve / sweeps) of a step of the same handle, per atom row, is what a point would cost if the probe ran at the step
kernels' rate.  Prints one JSON line per workload.

    python tools/field_at_cost.py [--grid-list 128] [--grid-exact 64] [--repeats 5]"""
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


def measure(pkg, s, shape, repeats, label, device_neigh):
    p = pkg.pair_from_system(s, device_neigh=device_neigh)
    for _ in range(2):
        step = p.compute_resident(eflag=1, vflag=2)
    steps = [p.compute_resident(eflag=1, vflag=2) for _ in range(3)]
    step = steps[-1]
    ms_static = float(np.median([o["ms_static"] for o in steps]))
    ms_sweep = float(np.median([o["ms_solve"] / max(o["sweeps"], 1) for o in steps]))
    pts = p.grid_points(shape)
    npts = len(pts)
    p.field_at(pts)                                   # warm-up: buffers, code objects
    ms = [p.field_at(pts)["ms"] for _ in range(repeats)]
    ms_field_only = [p.field_at(pts, potential=False)["ms"] for _ in range(repeats)]
    st = s.settings
    if st.dd_cutoff > 0:
        cutall = max(st.cut_coul, st.dd_cutoff)
        ncell = int(np.prod([max(1, int(np.floor(w / (0.5 * cutall)))) for w in s.prd]))
        cand = s.nlocal / ncell * 125.0
    else:
        cand = float(s.nlocal)
    med = float(np.median(ms))
    out = dict(workload=label, natoms=s.nlocal, grid=list(shape), points=npts, device_ms=[round(v, 3) for v in ms], device_ms_median=med,
               device_ms_field_only_median=float(np.median(ms_field_only)), points_per_s=npts / (med * 1e-3),
               candidate_pairs_per_point=cand, candidate_pairs_per_s=npts * cand / (med * 1e-3),
               us_per_point=1e3 * med / npts, yardstick_ms_static=ms_static, yardstick_ms_one_sweep=ms_sweep,
               yardstick_us_per_row=1e3 * (ms_static + ms_sweep) / s.nlocal,
               ratio_point_over_row=(med / npts) / ((ms_static + ms_sweep) / s.nlocal), sweeps=step["sweeps"], dd_pairs=step["dd_pairs"])
    p.close()
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid-list", type=int, default=128)
    ap.add_argument("--grid-exact", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", choices=["list", "exact"], default=None)
    a = ap.parse_args()
    pkg = importlib.import_module(PKG)
    wl = importlib.import_module(PKG + ".workload")
    if pkg.device_count() < 1:
        raise SystemExit("field_at_cost.py needs an MI355X: there is nothing to measure without one")
    fixture = os.path.join(ROOT, "tests", "golden", "mof5_h2.npz")
    if a.only != "exact":
        s = wl.replicate_fixture(fixture, 5, 5, 4, extra_args=["use_previous", "no", "polar_gs_ranked", "yes", "dd_cutoff", repr(CUT), "fixed_iteration", "no",
                                                               "precision", "1e-11", "max_iterations", "100"], build_list=False)
        g = a.grid_list
        measure(pkg, s, (g, g, g), a.repeats, "BASELINE configs[2]: MOF5+H2 5x5x4, list mode", True)
    if a.only != "list":
        s, _ = wl.load_fixture(fixture, extra_args=["use_previous", "no", "polar_gs_ranked", "yes", "precision", "1e-11", "max_iterations", "30"])
        g = a.grid_exact
        measure(pkg, s, (g, g, g), a.repeats, "BASELINE configs[0]: MOF5+H2 1,349 atoms, exact mode", False)


if __name__ == "__main__":
    main()
