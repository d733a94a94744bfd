"""Reference for polar_probe_at's Lennard-Jones half, written from the definition (include/polar_mi355x.h), not from the
library's headers.

A point p carries a type t_p, optionally a skip_atom and a molecule id.  With d = x_p - x_j(image), r = |d| and the style's tables
(lj1 .. lj4, offset, cut_ljsq, indexed [t_p][t_j]):

    e_lj = sum_j [ r^-6 (lj3 r^-6 - lj4) - offset ]         r^2 < cut_ljsq (strict), r^2 > 0
    f_lj = sum_j (lj1 r^-6 - lj2) r^-6 r^-2 d               the same atoms: the force on the probe

over ALL atoms -- charged, polarizable or neither -- but the skip_atom and the atoms of the point's non-zero molecule id.
special_lj does not enter.

Two levels, as tests/point_ref.py:
  * probe_pair: ONE atom's terms at 40 digits on the backends of tests/pair_ref.py, each with its scale;
  * probe_lj_numpy: whole points in FP64, brute force over the 27 nearest lattice images of every atom (every image within
    reach counts once; with the box widths polar_probe_at accepts that is at most one), value and per-point scale:
    sum_j (|lj3| r^-12 + |lj4| r^-6 + |offset|) for the energy, sum_j (|lj1| r^-12 + |lj2| r^-6) / r for the force."""
import numpy as np

import pair_ref as pr
from point_ref import cell_matrix


def probe_pair(d, lj1, lj2, lj3, lj4, offset, cut_ljsq, be=None):
    """One atom per row: d [n, 3]; the table entries of the row's type pair [n].  The cutoff is decided on the FP64 rsq the kernel
    sees (fma(dx, dx, fma(dy, dy, dz dz)) is within an ulp of it: callers keep their pairs off the shell).  Returns dict(on, e,
    f = [fx, fy, fz]) of Sums, empty where the pair is off."""
    be = be or pr.backend()
    d = np.asarray(d, np.float64)
    z = np.zeros(len(d))
    rsq64 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
    on = (rsq64 > 0) & (rsq64 < cut_ljsq)
    safe = np.where((rsq64 > 0)[:, None], d, 1.0)
    dl = [pr.leaf(be, safe[:, k]) for k in range(3)]
    L1, L2, L3, L4, OF = (pr.leaf(be, v + z) for v in (lj1, lj2, lj3, lj4, offset))
    rsq = dl[0] * dl[0] + dl[1] * dl[1] + dl[2] * dl[2]
    r2inv = pr._inv(rsq)
    r6inv = r2inv * r2inv * r2inv
    e = L3 * r6inv * r6inv - L4 * r6inv - OF
    fp = (L1 * r6inv * r6inv - L2 * r6inv) * r2inv
    return dict(on=on, e=e.where(on), f=[(fp * dl[k]).where(on) for k in range(3)])


def _image_shifts(prd, tilt):
    H = cell_matrix(prd, tilt)
    n = np.array([(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)], np.float64)
    return H, n @ H.T


def probe_lj_numpy(points, type, skip, pmol, x, typ, mol, tables, prd, tilt=None):
    """Brute force.  points [m, 3]; type [m] (1 .. ntypes); skip [m] or None (-1: none); pmol [m] or None (0: none); x [n, 3],
    typ, mol [n]: the atoms; tables: dict with lj1 .. lj4, offset, cut_ljsq as [ntypes + 1, ntypes + 1] arrays.
    Returns dict(e_lj, e_scale [m], f_lj [m, 3], f_scale [m], shell [m]: the smallest |r - cut_lj| over all images met)."""
    points = np.asarray(points, np.float64)
    m, n = len(points), len(x)
    skip = np.full(m, -1) if skip is None else np.asarray(skip)
    pmol = np.zeros(m, int) if pmol is None else np.asarray(pmol)
    type = np.broadcast_to(np.asarray(type), (m,))
    H, shifts = _image_shifts(prd, tilt)
    idx = np.arange(n)
    e, es, f, fs, shell = np.zeros(m), np.zeros(m), np.zeros((m, 3)), np.zeros(m), np.full(m, np.inf)
    tb = {k: np.asarray(tables[k], np.float64) for k in ("lj1", "lj2", "lj3", "lj4", "offset", "cut_ljsq")}
    for p in range(m):
        d0 = points[p] - x
        d0 = d0 - np.round(np.linalg.solve(H, d0.T).T) @ H.T          # near the origin cell
        d = (d0[:, None, :] + shifts[None, :, :]).reshape(-1, 3)       # the 27 images of every atom
        j = np.repeat(idx, 27)
        rsq = np.sum(d * d, axis=1)
        t = type[p]
        c2 = tb["cut_ljsq"][t, typ[j]]
        keep = (j != skip[p]) & ((pmol[p] == 0) | (pmol[p] != mol[j])) & (rsq > 0)
        shell[p] = np.min(np.abs(np.sqrt(rsq[keep]) - np.sqrt(c2[keep]))) if np.any(keep) else np.inf
        on = keep & (rsq < c2)
        r2i = 1.0 / rsq[on]
        r6i = r2i ** 3
        tj = typ[j][on]
        l1, l2, l3, l4, of = (tb[k][t, tj] for k in ("lj1", "lj2", "lj3", "lj4", "offset"))
        e[p] = np.sum(r6i * (l3 * r6i - l4) - of)
        es[p] = np.sum(np.abs(l3) * r6i * r6i + np.abs(l4) * r6i + np.abs(of))
        f[p] = np.sum(((l1 * r6i - l2) * r6i * r2i)[:, None] * d[on], axis=0)
        fs[p] = np.sum((np.abs(l1) * r6i * r6i + np.abs(l2) * r6i) * np.sqrt(r2i))
    return dict(e_lj=e, e_scale=es, f_lj=f, f_scale=fs, shell=shell)
