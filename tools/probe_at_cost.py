#!/usr/bin/env python
"""Cost of polar_probe_at on the MI355X, measured and printed -- not part of the test suite, no threshold.

Two workloads of bench.py, as tools/field_at_cost.py: BASELINE configs[2] (the MOF5+H2 cell replicated 5x5x4 = 134,900 atoms,
list mode, dd_cutoff = cut_coul) with a 64^3 and a 128^3 `probe_grid`, and configs[0] (the 1,349-atom cell, exact mode) with a
64^3 one.  Each: two warm-up steps and one warm-up grid, then five grids of the LJ half alone (q = alpha = None), five of the
field half alone (type = None) and five of the whole call; beside them `field_at` on the same grid from the same run.
device_ms is the device time of the call's kernels (HIP events).  The probe type is 8, the centre site of the fixture's H2 model
(its pair cutoffs are 2.5 sigma: a reach of 8.23 A against the 12.83 A of cutall; --type picks another).  Prints one JSON line per
grid.

    python tools/probe_at_cost.py [--grids-list 64 128] [--grid-exact 64] [--repeats 5] [--type T]"""
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


def measure(pkg, s, shapes, repeats, label, device_neigh, ptype):
    p = pkg.pair_from_system(s, device_neigh=device_neigh)
    for _ in range(2):
        p.compute_resident(eflag=1, vflag=2)
    tb = s.tables
    reach = float(np.sqrt(tb["cut_ljsq"][ptype, 1:].max()))
    for shape in shapes:
        pts = p.grid_points(shape)
        npts = len(pts)
        p.probe_at(pts, ptype, 0.0, 0.0)                  # warm-up: buffers, code objects, the records' types
        p.field_at(pts)
        med = lambda f: float(np.median([f()["ms"] for _ in range(repeats)]))
        ms_lj = med(lambda: p.probe_at(pts, ptype, None, None))
        ms_lj_force = med(lambda: p.probe_at(pts, ptype, None, None, force=True))
        ms_field = med(lambda: p.probe_at(pts, None, 0.3, 1.0))
        ms_all = med(lambda: p.probe_at(pts, ptype, 0.3, 1.0))
        ms_field_at = med(lambda: p.field_at(pts))
        out = dict(workload=label, natoms=s.nlocal, grid=list(shape), points=npts, probe_type=int(ptype), reach=reach,
                   device_ms_lj=ms_lj, device_ms_lj_with_force=ms_lj_force, device_ms_field_half=ms_field, device_ms_whole_call=ms_all,
                   device_ms_field_at=ms_field_at, ns_per_point_lj=1e6 * ms_lj / npts, ns_per_point_field_half=1e6 * ms_field / npts)
        print(json.dumps(out), flush=True)
    p.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grids-list", type=int, nargs="*", default=[64, 128])
    ap.add_argument("--grid-exact", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--type", type=int, default=8, help="probe type (default: 8, the H2 centre site)")
    ap.add_argument("--only", choices=["list", "exact"], default=None)
    a = ap.parse_args()
    pkg = importlib.import_module(PKG)
    wl = importlib.import_module(PKG + ".workload")
    if pkg.device_count() < 1:
        raise SystemExit("probe_at_cost.py needs an MI355X: there is nothing to measure without one")
    fixture = os.path.join(ROOT, "tests", "golden", "mof5_h2.npz")
    if a.only != "exact" and a.grids_list:
        s = wl.replicate_fixture(fixture, 5, 5, 4, extra_args=["use_previous", "no", "polar_gs_ranked", "yes", "dd_cutoff", repr(CUT), "fixed_iteration", "no",
                                                               "precision", "1e-11", "max_iterations", "100"], build_list=False)
        measure(pkg, s, [(g, g, g) for g in a.grids_list], a.repeats, "BASELINE configs[2]: MOF5+H2 5x5x4, list mode", True, a.type)
    if a.only != "list":
        s, _ = wl.load_fixture(fixture, extra_args=["use_previous", "no", "polar_gs_ranked", "yes", "precision", "1e-11", "max_iterations", "30"])
        g = a.grid_exact
        measure(pkg, s, [(g, g, g)], a.repeats, "BASELINE configs[0]: MOF5+H2 1,349 atoms, exact mode", False, a.type)


if __name__ == "__main__":
    main()
