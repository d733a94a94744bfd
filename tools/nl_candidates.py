#!/usr/bin/env python3
"""What a row of the list build walks, emulated in NumPy: runs, candidates and dense 64-candidate trips per row atom of a
replicated MOF-5 + H2 box, with the inert sites between the others in cell order and with them behind the grid.

Follows k_nl_build (csrc/polar_lists.hpp) for an orthogonal periodic box: the list grid of list_grid (cells at least half a
cutoff high), the +-2 stencil as up to 25 rows of cells, the per-atom trimming of a row of cells to what a sphere of the
cutoff (+ 1e-6) can reach, one or two contiguous runs per stencil row, all runs of a row atom laid end to end and walked 64
at a time.  The candidates of a run are the atoms between two entries of cell_first: every atom of those cells, or -- inert
sites behind the grid (build_cells) -- the ones that carry a charge or a polarizability.  No GPU and no library are needed.

    python tools/nl_candidates.py 5 5 4
    python tools/nl_candidates.py 3 3 3 --rows 600 --seed 1
"""
import argparse
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def replicate(z, reps):
    x0, prd0 = np.asarray(z["x"], float) - np.asarray(z["boxlo"], float), np.asarray(z["prd"], float)
    shifts = np.array([[i, j, k] for k in range(reps[2]) for j in range(reps[1]) for i in range(reps[0])], float) * prd0
    x = (x0[None, :, :] + shifts[:, None, :]).reshape(-1, 3)
    q, alpha = np.tile(np.asarray(z["q"], float), len(shifts)), np.tile(np.asarray(z["alpha"], float), len(shifts))
    return x, q, alpha, prd0 * np.array(reps, float)


def rows_walked(x, prd, nc, first, cut, rows):
    """(runs, candidates, trips) per row atom for the scan `first` over the cells (x fastest)"""
    n0, n1, n2 = (int(v) for v in nc)
    edge = prd / nc
    reach2 = (cut + 1e-6) ** 2
    out = np.zeros((len(rows), 3), np.int64)
    for r, i in enumerate(rows):
        fr = x[i] / prd
        fr -= np.floor(fr)
        t = fr * nc
        cc = np.minimum(t.astype(np.int64), nc - 1)
        uu = t - cc
        zs = range(cc[2] - 2, cc[2] + 3) if n2 >= 5 else range(n2)
        ys = range(cc[1] - 2, cc[1] + 3) if n1 >= 5 else range(n1)
        runs = cand = 0
        for zz in zs:
            for yy in ys:
                dz = zz - cc[2] if n2 >= 5 else 0
                dy = yy - cc[1] if n1 >= 5 else 0
                dzmin = (dz - uu[2]) * edge[2] if dz > 0 else ((uu[2] - (dz + 1)) * edge[2] if dz < 0 else 0.0)
                dymin = (dy - uu[1]) * edge[1] if dy > 0 else ((uu[1] - (dy + 1)) * edge[1] if dy < 0 else 0.0)
                rem2 = reach2 - dzmin * dzmin - dymin * dymin
                if rem2 < 0.0:
                    continue
                xlo, xhi = (cc[0] - 2, cc[0] + 2) if n0 >= 5 else (0, n0 - 1)
                if n0 >= 5:
                    xr = np.sqrt(rem2) / edge[0]
                    xlo, xhi = cc[0] + max(int(np.floor(uu[0] - xr)), -2), cc[0] + min(int(np.floor(uu[0] + xr)), 2)
                base = ((zz % n2) * n1 + (yy % n1)) * n0
                xa, xb = max(xlo, 0), min(xhi, n0 - 1)
                pieces = [(first[base + xa], first[base + xb + 1])]
                if xlo < 0:
                    pieces.append((first[base + xlo + n0], first[base + n0]))
                elif xhi >= n0:
                    pieces.append((first[base], first[base + xhi - n0 + 1]))
                for a, b in pieces:
                    if b > a:
                        runs += 1
                        cand += int(b - a)
        out[r] = (runs, cand, -(-cand // 64))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("reps", type=int, nargs=3, help="replicate nx ny nz of tests/golden/mof5_h2.npz")
    ap.add_argument("--cutoff", type=float, default=12.8345, help="max(cut_coul, dd_cutoff)")
    ap.add_argument("--rows", type=int, default=600, help="random row atoms")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    z = np.load(os.path.join(ROOT, "tests", "golden", "mof5_h2.npz"))
    x, q, alpha, prd = replicate(z, a.reps)
    n = len(x)
    nc = np.maximum(1, np.floor(prd / (0.5 * a.cutoff))).astype(np.int64)
    assert np.all(prd >= 2.0 * a.cutoff * (1 - 1e-12)), "a periodic dimension is narrower than two cutoffs"
    fr = x / prd
    fr -= np.floor(fr)
    c3 = np.minimum((fr * nc).astype(np.int64), nc - 1)
    cell = (c3[:, 2] * nc[1] + c3[:, 1]) * nc[0] + c3[:, 0]
    ncell = int(nc.prod())
    inert = (q == 0.0) & (alpha == 0.0)
    scan = lambda m: np.concatenate([[0], np.cumsum(np.bincount(cell[m], minlength=ncell))])
    rows = np.random.default_rng(a.seed).choice(n, min(a.rows, n), replace=False)
    print("%d x %d x %d: %d atoms, %d inert (%.1f %%), grid %d x %d x %d, cells of %.3f x %.3f x %.3f A, %.1f atoms per cell (%.1f not inert)" % (
        *a.reps, n, inert.sum(), 100.0 * inert.mean(), *nc, *(prd / nc), n / ncell, (~inert).sum() / ncell))
    res = {}
    for name, m in (("inert sites between the others", np.ones(n, bool)), ("inert sites behind the grid", ~inert)):
        w = rows_walked(x, prd, nc, scan(m), a.cutoff, rows)
        res[name] = w.mean(axis=0)
        print("  %-31s runs %.1f  candidates %.0f  trips %.1f  (lane slots %.0f, %.0f %% empty)" % (
            name + ":", *res[name], 64 * res[name][2], 100.0 * (1.0 - res[name][1] / (64 * res[name][2]))))
    b, s = res["inert sites between the others"], res["inert sites behind the grid"]
    print("  ratio: candidates x %.3f, trips x %.3f  (%d random rows, inert rows included: they keep their rows)" % (s[1] / b[1], s[2] / b[2], len(rows)))


if __name__ == "__main__":
    main()
