"""Reference for polar_field_at: the field and the potential of the polarized box at a point, written from the definition
(include/polar_mi355x.h), not from the library's headers.

With d = x_p - x_j(image), r = |d|, e2s = sqrt(qqrd2e), rc = cut_coul and the style's tensor scalars s3, s5 (PS.cpp:1287-1297):

    e_static   = e2s sum_j q_j (1/r^2 - 1/rc^2) d / r     r^2 <= rc^2, molecule rule (mol_p != mol_j or mol_p == 0)
    phi_static = e2s sum_j q_j (1/r + r/rc^2 - 2/rc)      the same atoms
    e_induced  = -sum_j (s3 mu_j - s5 (mu_j.d) d)         every atom (exact mode) or r^2 < dd_cutoff^2; alpha_j != 0
    phi_induced = sum_j s3 (mu_j.d)                        the same atoms

Two levels:
  * point_terms / point_pair: ONE atom's terms at 40 digits on the backends of tests/pair_ref.py, each with its scale (the sum
    of the absolute values of the terms added to form it), as that module returns its quantities;
  * field_at_numpy: whole points, an FP64 brute-force sum over all atoms, value and per-point scale sum_j |term_j| (per
    component for the fields).  Orthogonal boxes take the per-axis nearest image, tilted boxes the nearest of the 27
    neighbouring lattice images (legitimate in list mode: the cutoffs are below half the cell widths)."""
import numpy as np

import pair_ref as pr


def point_terms(d, q, mu, alpha, cut_coul, pd, e2s, damp, be=None):
    """One atom per row, before the cutoffs select: d [n, 3] = x_p - x_j; q, alpha [n]; mu [n, 3].  Returns a dict of Sums:
    es, ei (lists of three), ps, pi."""
    be = be or pr.backend()
    d = np.asarray(d, np.float64)
    z = np.zeros(len(d))
    dl = [pr.leaf(be, d[:, k]) for k in range(3)]
    mj = [pr.leaf(be, np.where(np.asarray(alpha) != 0, np.asarray(mu)[:, k], 0.0)) for k in range(3)]
    q_, e2s_, rc = pr.leaf(be, q + z), pr.leaf(be, e2s + z), pr.leaf(be, cut_coul + z)
    rsq = dl[0] * dl[0] + dl[1] * dl[1] + dl[2] * dl[2]
    r = pr._sqrt(rsq)
    rinv = pr._inv(r)
    rc2inv, rcinv = pr._inv(rc * rc), pr._inv(rc)
    ef = (pr._inv(rsq) - rc2inv) * rinv
    es = [e2s_ * q_ * ef * dl[k] for k in range(3)]
    ps = e2s_ * q_ * (rinv + r * rc2inv - 2 * rcinv)
    s3, s5 = pr._tensor_scalars(rsq, pd, damp)
    md = pr._dot(mj, dl)
    ei = [s5 * md * dl[k] - s3 * mj[k] for k in range(3)]
    pi = s3 * md
    return dict(es=es, ps=ps, ei=ei, pi=pi)


def point_pair(d, q, mu, alpha, molok, cut_coul, dd_cutoff, pd, e2s, damp, be=None):
    """The same with the cutoffs applied (decided on the FP64 rsq the kernel sees); dd_cutoff None: every pair (exact mode).
    Returns the dict of point_terms plus st_on, in_on."""
    d = np.asarray(d, np.float64)
    rsq64 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
    st_on = (rsq64 > 0) & (rsq64 <= cut_coul * cut_coul) & np.asarray(molok, bool)
    in_on = (rsq64 > 0) & (np.asarray(alpha) != 0)
    if dd_cutoff is not None:
        in_on = in_on & (rsq64 < dd_cutoff * dd_cutoff)
    safe = np.where((rsq64 > 0)[:, None], d, 1.0)            # (a pair at r = 0 adds nothing: keep the reference finite there)
    t = point_terms(safe, q, mu, alpha, cut_coul, pd, e2s, damp, be)
    return dict(st_on=st_on, in_on=in_on, es=[c.where(st_on) for c in t["es"]], ps=t["ps"].where(st_on),
                ei=[c.where(in_on) for c in t["ei"]], pi=t["pi"].where(in_on))


# ---------------------------------------------------------------------------------------------------------------------
# whole points in FP64

def cell_matrix(prd, tilt=None):
    lx, ly, lz = prd
    xy, xz, yz = (0.0, 0.0, 0.0) if tilt is None else tilt
    return np.array([[lx, xy, xz], [0.0, ly, yz], [0.0, 0.0, lz]], dtype=np.float64)


def images(dr, prd, tilt=None):
    """minimum image of the displacements dr [n, 3]"""
    prd = np.asarray(prd, np.float64)
    if tilt is None or not np.any(np.asarray(tilt) != 0.0):
        return dr - prd * np.round(dr / prd)
    H = cell_matrix(prd, tilt)
    fr = np.linalg.solve(H, dr.T).T
    dr = dr - np.round(fr) @ H.T                             # near the origin cell; then the nearest of the 27 around it
    best, bn = dr, np.sum(dr * dr, axis=1)
    for a in (-1, 0, 1):
        for b in (-1, 0, 1):
            for c in (-1, 0, 1):
                cand = dr + np.array([a, b, c], np.float64) @ H.T
                cn = np.sum(cand * cand, axis=1)
                take = cn < bn
                best, bn = np.where(take[:, None], cand, best), np.where(take, cn, bn)
    return best


def tensor_scalars64(r, pd, damp):
    r3, r5 = r ** -3, r ** -5
    if damp == 0:
        a = pd * r
        e = np.exp(-a)
        p2 = 1 + a + 0.5 * a * a
        p3 = p2 + a * a * a / 6
        return (1 - e * p2) * r3, 3 * (1 - e * p3) * r5, (1 + e * p2) * r3, 3 * (1 + e * p3) * r5
    return r3, 3 * r5, r3, 3 * r5


def field_at_numpy(points, skip_atom, molecule, x, q, alpha, mol, mu, prd, tilt, cut_coul, dd_cutoff, pd, damp, e2s):
    """Brute force over all atoms.  dd_cutoff None: exact mode.  Returns {name: (value, scale)} for e_static, e_induced
    ([m, 3]) and phi_static, phi_induced ([m])."""
    points = np.asarray(points, np.float64)
    m = len(points)
    skip_atom = np.full(m, -1) if skip_atom is None else np.asarray(skip_atom)
    molecule = np.zeros(m, int) if molecule is None else np.asarray(molecule)
    mu = np.where((np.asarray(alpha) != 0)[:, None], mu, 0.0)
    out = {k: (np.zeros((m, 3)), np.zeros((m, 3))) for k in ("e_static", "e_induced")}
    out.update({k: (np.zeros(m), np.zeros(m)) for k in ("phi_static", "phi_induced")})
    idx = np.arange(len(x))
    for p in range(m):
        d = images(points[p] - x, prd, tilt)
        rsq = np.sum(d * d, axis=1)
        keep = (idx != skip_atom[p]) & (rsq > 0)
        r = np.sqrt(np.where(rsq > 0, rsq, 1.0))
        st = keep & (rsq <= cut_coul * cut_coul) & ((molecule[p] != mol) | (molecule[p] == 0))
        t = (e2s * q * (1 / rsq.clip(1e-300) - 1 / cut_coul ** 2) / r)[:, None] * d
        ta = (e2s * np.abs(q) * (1 / rsq.clip(1e-300) + 1 / cut_coul ** 2) / r)[:, None] * np.abs(d)
        out["e_static"][0][p], out["e_static"][1][p] = t[st].sum(0), ta[st].sum(0)
        out["phi_static"][0][p] = np.sum((e2s * q * (1 / r + r / cut_coul ** 2 - 2 / cut_coul))[st])
        out["phi_static"][1][p] = np.sum((e2s * np.abs(q) * (1 / r + r / cut_coul ** 2 + 2 / cut_coul))[st])
        ind = keep & (alpha != 0)
        if dd_cutoff is not None:
            ind = ind & (rsq < dd_cutoff * dd_cutoff)
        s3, s5, s3a, s5a = tensor_scalars64(r, pd, damp)
        md, mda = np.sum(mu * d, axis=1), np.sum(np.abs(mu * d), axis=1)
        ti = (s5 * md)[:, None] * d - s3[:, None] * mu
        tia = (s5a * mda)[:, None] * np.abs(d) + s3a[:, None] * np.abs(mu)
        out["e_induced"][0][p], out["e_induced"][1][p] = ti[ind].sum(0), tia[ind].sum(0)
        out["phi_induced"][0][p], out["phi_induced"][1][p] = np.sum((s3 * md)[ind]), np.sum((s3a * mda)[ind])
    return out
