"""Reference for polar_field_grad_at: the gradient G_ab = d e_a / d x_b of the two fields of tests/point_ref.py at a point,
written from the definition (include/polar_mi355x.h), not from the library's headers.  Six components, xx, yy, zz, xy, xz, yz.

With d = x_p - x_j(image), r = |d|, e2s = sqrt(qqrd2e), rc = cut_coul and the style's tensor scalars s3, s5:

    g_static_ab  = e2s sum_j q_j [ (r^-3 - rc^-2 r^-1) delta_ab + (rc^-2 r^-3 - 3 r^-5) d_a d_b ]
    g_induced_ab = sum_j [ s5 (mu_a d_b + d_a mu_b + (mu.d) delta_ab) - s7 (mu.d) d_a d_b ],   s7 = -(1/r) d s5 / d r
    damping none: s7 = 15 r^-7;  exponential, a = pd r:  s7 = 15 r^-7 (1 - e^-a (1 + a + a^2/2 + a^3/6 + a^4/30))

over the atoms of point_ref's sums.  Two levels, as there:
  * grad_terms / grad_pair: ONE atom's terms at 40 digits on the `Sum` backends of tests/pair_ref.py, each with its scale;
  * field_grad_numpy: whole points in FP64 by brute force, value and per-component scale sum_j |term_j|."""
import numpy as np

import pair_ref as pr
from point_ref import images, tensor_scalars64

COMP = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))


def _s7(rsq, pd, damp):
    """15 / r^7, times 1 - e^-a (1 + a + a^2/2 + a^3/6 + a^4/30) with exponential damping -- term by term"""
    be = rsq.be
    r = pr._sqrt(rsq)
    r7 = pr._inv(r * r * r * r * r * r * r)
    if damp == 0:
        pd = pr.leaf(be, pd + np.zeros_like(rsq.s))
        a = pd * r
        e = pr._exp(-a, damp=True)
        thirtieth = pr.Sum(be, be.arr(1.0) / 30)
        d3 = 1 - e * (a * a * a * a * thirtieth + a * a * a * pr._sixth(be) + a * a * 0.5 + a + 1)
        return 15 * (d3 * r7)
    return 15 * r7


def grad_terms(d, q, mu, alpha, cut_coul, pd, e2s, damp, be=None):
    """One atom per row, before the cutoffs select (arguments as point_ref.point_terms).  Returns dict(gs, gi): lists of six Sums."""
    be = be or pr.backend()
    d = np.asarray(d, np.float64)
    z = np.zeros(len(d))
    dl = [pr.leaf(be, d[:, k]) for k in range(3)]
    mj = [pr.leaf(be, np.where(np.asarray(alpha) != 0, np.asarray(mu)[:, k], 0.0)) for k in range(3)]
    q_, e2s_, rc = pr.leaf(be, q + z), pr.leaf(be, e2s + z), pr.leaf(be, cut_coul + z)
    rsq = dl[0] * dl[0] + dl[1] * dl[1] + dl[2] * dl[2]
    r = pr._sqrt(rsq)
    rinv, r3inv, r5inv = pr._inv(r), pr._inv(r * r * r), pr._inv(r * r * r * r * r)
    rc2inv = pr._inv(rc * rc)
    iso = r3inv - rc2inv * rinv
    ani = rc2inv * r3inv - 3 * r5inv
    s3, s5 = pr._tensor_scalars(rsq, pd, damp)
    s7 = _s7(rsq, pd, damp)
    md = pr._dot(mj, dl)
    gs, gi = [], []
    for a, b in COMP:
        t = e2s_ * q_ * (ani * dl[a] * dl[b])
        u = s5 * (mj[a] * dl[b] + dl[a] * mj[b]) - s7 * md * dl[a] * dl[b]
        if a == b:
            t = t + e2s_ * q_ * iso
            u = u + s5 * md
        gs.append(t)
        gi.append(u)
    return dict(gs=gs, gi=gi)


def grad_pair(d, q, mu, alpha, molok, cut_coul, dd_cutoff, pd, e2s, damp, be=None):
    """The same with the cutoffs applied (decided on the FP64 rsq the kernel sees), as point_ref.point_pair."""
    d = np.asarray(d, np.float64)
    rsq64 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
    st_on = (rsq64 > 0) & (rsq64 <= cut_coul * cut_coul) & np.asarray(molok, bool)
    in_on = (rsq64 > 0) & (np.asarray(alpha) != 0)
    if dd_cutoff is not None:
        in_on = in_on & (rsq64 < dd_cutoff * dd_cutoff)
    safe = np.where((rsq64 > 0)[:, None], d, 1.0)
    t = grad_terms(safe, q, mu, alpha, cut_coul, pd, e2s, damp, be)
    return dict(st_on=st_on, in_on=in_on, gs=[c.where(st_on) for c in t["gs"]], gi=[c.where(in_on) for c in t["gi"]])


def s7_64(r, pd, damp):
    """(s7, its scale) in FP64"""
    r7 = r ** -7
    if damp == 0:
        a = pd * r
        e = np.exp(-a)
        p4 = 1 + a + 0.5 * a * a + a ** 3 / 6 + a ** 4 / 30
        return 15 * (1 - e * p4) * r7, 15 * (1 + e * p4) * r7
    return 15 * r7, 15 * r7


def closest_image_del(dr, prd, tilt):
    """x_p - closest_image(x_j) for a tilted box in exact mode, where the induced sum has no cutoff and the image of a far pair
    matters: Domain::closest_image reduces z first (carrying yz, xz into y and x), then y (carrying xy), then x, each into
    [-L/2, L/2] -- which is not always the nearest of the 27 images that point_ref.images takes."""
    d = np.array(dr, np.float64)
    xy, xz, yz = tilt
    n2 = np.round(d[:, 2] / prd[2])
    d -= n2[:, None] * np.array([xz, yz, prd[2]])
    n1 = np.round(d[:, 1] / prd[1])
    d -= n1[:, None] * np.array([xy, prd[1], 0.0])
    d[:, 0] -= prd[0] * np.round(d[:, 0] / prd[0])
    return d


def field_grad_numpy(points, skip_atom, molecule, x, q, alpha, mol, mu, prd, tilt, cut_coul, dd_cutoff, pd, damp, e2s):
    """Brute force over all atoms (arguments as point_ref.field_at_numpy).  Returns {name: (value, scale)} for g_static and
    g_induced, [m, 6] each."""
    points = np.asarray(points, np.float64)
    m = len(points)
    skip_atom = np.full(m, -1) if skip_atom is None else np.asarray(skip_atom)
    molecule = np.zeros(m, int) if molecule is None else np.asarray(molecule)
    mu = np.where((np.asarray(alpha) != 0)[:, None], mu, 0.0)
    out = {k: (np.zeros((m, 6)), np.zeros((m, 6))) for k in ("g_static", "g_induced")}
    idx = np.arange(len(x))
    rc2 = cut_coul ** 2
    for p in range(m):
        # (exact mode in a tilted box: the image rule of the mode's atom loops, see closest_image_del)
        tilted = tilt is not None and np.any(np.asarray(tilt) != 0.0)
        d = closest_image_del(points[p] - x, prd, tilt) if (tilted and dd_cutoff is None) else images(points[p] - x, prd, tilt)
        rsq = np.sum(d * d, axis=1)
        keep = (idx != skip_atom[p]) & (rsq > 0)
        r = np.sqrt(np.where(rsq > 0, rsq, 1.0))
        st = keep & (rsq <= rc2) & ((molecule[p] != mol) | (molecule[p] == 0))
        ind = keep & (alpha != 0)
        if dd_cutoff is not None:
            ind = ind & (rsq < dd_cutoff * dd_cutoff)
        iso, isa = e2s * q * (r ** -3 - 1 / (rc2 * r)), e2s * np.abs(q) * (r ** -3 + 1 / (rc2 * r))
        ani, ana = e2s * q * (r ** -3 / rc2 - 3 * r ** -5), e2s * np.abs(q) * (r ** -3 / rc2 + 3 * r ** -5)
        s3, s5, s3a, s5a = tensor_scalars64(r, pd, damp)
        s7, s7a = s7_64(r, pd, damp)
        md, mda = np.sum(mu * d, axis=1), np.sum(np.abs(mu * d), axis=1)
        for k, (a, b) in enumerate(COMP):
            dd = d[:, a] * d[:, b]
            t, ta = ani * dd, ana * np.abs(dd)
            u = s5 * (mu[:, a] * d[:, b] + d[:, a] * mu[:, b]) - s7 * md * dd
            ua = s5a * (np.abs(mu[:, a] * d[:, b]) + np.abs(d[:, a] * mu[:, b])) + s7a * mda * np.abs(dd)
            if a == b:
                t, ta = t + iso, ta + isa
                u, ua = u + s5 * md, ua + s5a * mda
            out["g_static"][0][p, k], out["g_static"][1][p, k] = t[st].sum(), ta[st].sum()
            out["g_induced"][0][p, k], out["g_induced"][1][p, k] = u[ind].sum(), ua[ind].sum()
    return out
