#!/usr/bin/env python
"""Cost of polar_ewald_field_grad_grid on the MI355X beside the per-point path, measured and printed -- not part of the test suite,
no threshold.

The two workloads of tools/ewald_field_at_cost.py with `polar_ewald 1e-6`: BASELINE configs[2] (the MOF5+H2 cell replicated
5x5x4 = 134,900 atoms, list mode, dd_cutoff = cut_coul) and configs[0] (the 1,349-atom cell, exact mode), each with a 64^3 and a
128^3 grid.  Per workload one handle; per grid a warm-up grid of each path, then `--repeats` grids of
ewald_field_grad_grid(recip="points") and of ewald_field_grad_grid(recip="grid"), interleaved in the same run.  Reported per path: the
device time (HIP events) of the real-space kernel and of the reciprocal kernels, medians and the spread (min .. max) of the
repeats, the wall time of a call, and the largest difference of the two paths' outputs over the grid, as a fraction of the
output's maximum, and the share of the device time that is reciprocal.  Prints one JSON line per (workload, grid).

    python tools/ewald_field_grad_grid_cost.py [--grids 64,128] [--repeats 5] [--only list|exact]"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "lammps-induced-dipole-polarization-pair-style_amd"
CUT = 12.8345
ACC = "1e-6"
NAMES = ("g_static", "g_induced", "e_static", "e_induced")


def _timed(fn):
    t0 = time.perf_counter()
    out = fn()
    out["wall_ms"] = 1e3 * (time.perf_counter() - t0)
    return out


def _stats(runs, key):
    v = [r[key] for r in runs]
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))


def measure(pkg, s, grids, repeats, label, device_neigh):
    p = pkg.pair_from_system(s, device_neigh=device_neigh)
    for _ in range(3):
        step = p.compute_resident(eflag=1, vflag=2)
    nk = step["nkvec"]
    for g in grids:
        shape = (g, g, g)
        calls = {"points": lambda: p.ewald_field_grad_grid(shape, recip="points"), "grid": lambda: p.ewald_field_grad_grid(shape, recip="grid")}
        warm = {k: f() for k, f in calls.items()}                # warm-up: buffers, code objects; and the two paths side by side
        diff = {k: float(np.max(np.abs(warm["grid"][k] - warm["points"][k])) / np.max(np.abs(warm["points"][k]))) for k in NAMES}
        runs = {"points": [], "grid": []}
        for _ in range(repeats):
            for k, f in calls.items():
                r = _timed(f)
                runs[k].append({key: r[key] for key in ("ms", "ms_real", "ms_recip", "wall_ms")})
        out = dict(workload=label, natoms=s.nlocal, shape=list(shape), points=g ** 3, nkvec=nk, accuracy=float(ACC), repeats=repeats,
                   grid_against_points_of_max=diff)
        for k in ("points", "grid"):
            out[k] = {key: _stats(runs[k], key) for key in ("ms_real", "ms_recip", "ms", "wall_ms")}
        for k in ("points", "grid"):
            out[k]["recip_share"] = out[k]["ms_recip"]["median"] / out[k]["ms"]["median"]
        out["recip_speedup"] = out["points"]["ms_recip"]["median"] / out["grid"]["ms_recip"]["median"]
        out["real_ratio_grid_over_points"] = out["grid"]["ms_real"]["median"] / out["points"]["ms_real"]["median"]
        out["real_spread_points"] = (out["points"]["ms_real"]["max"] - out["points"]["ms_real"]["min"]) / out["points"]["ms_real"]["median"]
        out["real_spread_grid"] = (out["grid"]["ms_real"]["max"] - out["grid"]["ms_real"]["min"]) / out["grid"]["ms_real"]["median"]
        print(json.dumps(out), flush=True)
    p.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grids", default="64,128")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", choices=["list", "exact"], default=None)
    a = ap.parse_args()
    grids = [int(v) for v in a.grids.split(",")]
    pkg = importlib.import_module(PKG)
    wl = importlib.import_module(PKG + ".workload")
    if pkg.device_count() < 1:
        raise SystemExit("ewald_field_grad_grid_cost.py needs an MI355X: there is nothing to measure without one")
    fixture = os.path.join(ROOT, "tests", "golden", "mof5_h2.npz")
    if a.only != "exact":
        s = wl.replicate_fixture(fixture, 5, 5, 4, extra_args=["use_previous", "no", "polar_gs_ranked", "yes", "dd_cutoff", repr(CUT), "fixed_iteration", "no",
                                                               "precision", "1e-11", "max_iterations", "100", "polar_ewald", ACC], build_list=False)
        measure(pkg, s, grids, a.repeats, "BASELINE configs[2]: MOF5+H2 5x5x4, list mode, polar_ewald 1e-6", True)
    if a.only != "list":
        s, _ = wl.load_fixture(fixture, extra_args=["use_previous", "no", "polar_gs_ranked", "yes", "precision", "1e-11", "max_iterations", "30", "polar_ewald", ACC])
        measure(pkg, s, grids, a.repeats, "BASELINE configs[0]: MOF5+H2 1,349 atoms, exact mode, polar_ewald 1e-6", False)


if __name__ == "__main__":
    main()
