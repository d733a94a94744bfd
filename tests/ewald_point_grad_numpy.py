"""NumPy reference for polar_ewald_field_grad_at: the gradient G_ab = d e_a / d x_b of the Ewald field of the polarized box at
points, written from the definition (include/polar_mi355x.h), not from the library's headers.  Six
components, xx, yy, zz, xy, xz, yz.  The field itself is tests/ewald_point_numpy.py's.

With d = x_p - x_j (minimum image), r = |d|, g = g_ewald, rc = cut_coul, G(r) = 2g/sqrt(pi) e^(-g^2 r^2), ph = erfc(gr)/r for a
kept atom and -erf(gr)/r for an excluded one, B1 = (ph + G) / r^2, B2 = (3 B1 + 2 g^2 G) / r^2, the half-space k-vectors and c_k
of ewald_numpy.kvectors and S(k) = sum_j q_j e^{ik.x_j}:

    g_static_ab = e2s [ sum_{r^2 <= rc^2} q_j (B1 delta_ab - B2 d_a d_b) + sum_k c_k k_a k_b Re(e^{ik.p} conj S) ]

Excluded: the point's (non-zero) molecule, the point's skip_atom, an atom on the point -- which adds the r -> 0 limit of the erf
form, -(2/3) g^2 (2g/sqrt(pi)) q_j on the diagonal.  In FP64 the erf form cancels at small gr ((gr)^2 of its terms survive in
B1, (gr)^4 in B2, and the division by r^2 magnifies the rest): below gr = 1/8 this reference sums the two Taylor series in
x = gr instead,
    B1 = g^3 2/sqrt(pi) sum_{n>=1} (-1)^n x^(2n-2) 2n / ((2n+1) n!),     B2 = g^5 2/sqrt(pi) sum_{n>=2} (-1)^n x^(2n-4) 4n(1-n) / ((2n+1) n!)
(from erf(x)/x = 2/sqrt(pi) sum (-1)^n x^2n / (n! (2n+1)) and e^(-x^2) = sum (-1)^n x^2n / n!), twelve terms each.
The induced gradient is that of tests/point_grad_ref.py with the image rule handed over, as ewald_point_numpy.induced_at."""
import math

import numpy as np
from scipy.special import erf, erfc

import ewald_point_numpy as epn
import point_ref as ptr
from ewald_numpy import kvectors
from point_grad_ref import COMP, s7_64

SERIES_BELOW = 0.125    # gr


def excluded_b12(g, r):
    """(B1, B2) of the erf form, r > 0: closed form from gr = 1/8 on, the series below"""
    x = g * r
    lo = x < SERIES_BELOW
    xs = np.where(lo, x, SERIES_BELOW)
    b1s, b2s = np.zeros_like(xs), np.zeros_like(xs)
    for n in range(12, 0, -1):      # smallest terms first
        f = (-1.0) ** n / ((2 * n + 1) * math.factorial(n))
        b1s += f * 2 * n * xs ** (2 * n - 2)
        if n >= 2:
            b2s += f * 4 * n * (1 - n) * xs ** (2 * n - 4)
    c = 2 / math.sqrt(math.pi)
    rr = np.where(lo, 1.0, r)
    gauss = g * c * np.exp(-(g * rr) ** 2)
    b1c = (-erf(g * rr) / rr + gauss) / rr ** 2
    b2c = (3 * b1c + 2 * g * g * gauss) / rr ** 2
    return np.where(lo, g ** 3 * c * b1s, b1c), np.where(lo, g ** 5 * c * b2s, b2c)


def recip_grad_sums(points, x, q, H, g, accuracy):
    """(g [m, 6], scale [6], sum_k c_k |k|^2 |S(k)|) of the reciprocal sums without e2s; scale_ab = sum_k c_k |k_a k_b| |S(k)|"""
    k, c = kvectors(H, g, accuracy)
    m = len(points)
    if len(k) == 0:
        return np.zeros((m, 6)), np.zeros(6), 0.0
    S = epn.structure_factors(x, q, k)
    re = np.real(np.exp(1j * (np.asarray(points) @ k.T)) * np.conj(S)[None, :]) * c[None, :]
    kk = np.stack([k[:, a] * k[:, b] for a, b in COMP], axis=1)
    return re @ kk, (c * np.abs(S)) @ np.abs(kk), float(np.sum(c * np.sum(k * k, axis=1) * np.abs(S)))


def static_grad_at(points, skip_atom, molecule, x, q, mol, prd, tilt, cut, g, accuracy, e2s=1.0):
    """(g_static [m, 6], scale [m, 6]): scale = the sum of the absolute terms"""
    points = np.asarray(points, np.float64).reshape(-1, 3)
    x, q, mol = np.asarray(x, np.float64), np.asarray(q, np.float64), np.asarray(mol)
    m = len(points)
    skip_atom = np.full(m, -1) if skip_atom is None else np.asarray(skip_atom)
    molecule = np.zeros(m, int) if molecule is None else np.asarray(molecule)
    H = ptr.cell_matrix(prd, tilt)
    G0 = 2 * g / math.sqrt(math.pi)
    idx = np.arange(len(x))
    val, sc = np.zeros((m, 6)), np.zeros((m, 6))
    for p in range(m):
        d = ptr.images(points[p] - x, prd, tilt)
        rsq = np.sum(d * d, axis=1)
        inr = rsq <= cut * cut
        on = rsq == 0
        excl = ((mol == molecule[p]) & (molecule[p] != 0)) | (idx == skip_atom[p]) | on
        r = np.sqrt(np.where(on, 1.0, rsq))
        gauss = G0 * np.exp(-g * g * r * r)
        b1k = (erfc(g * r) / r + gauss) / r ** 2
        b2k = (3 * b1k + 2 * g * g * gauss) / r ** 2
        b1x, b2x = excluded_b12(g, r)
        b1, b2 = np.where(excl, b1x, b1k), np.where(excl, b2x, b2k)
        # the terms as they are added: |ph| / r^2 and G / r^2 in B1, three of those and 2 g^2 G in B2 r^2
        a1 = (np.where(excl, erf(g * r), erfc(g * r)) / r + gauss) / r ** 2
        a2 = (3 * a1 + 2 * g * g * gauss) / r ** 2
        sel = inr & ~on
        lim = (2.0 / 3.0) * g * g * G0 * np.sum(q[inr & on])
        lima = (2.0 / 3.0) * g * g * G0 * np.sum(np.abs(q[inr & on]))
        for k, (a, b) in enumerate(COMP):
            t, ta = -q * b2 * d[:, a] * d[:, b], np.abs(q) * a2 * np.abs(d[:, a] * d[:, b])
            if a == b:
                t, ta = t + q * b1, ta + np.abs(q) * a1
            val[p, k], sc[p, k] = t[sel].sum(), ta[sel].sum()
            if a == b:
                val[p, k] -= lim
                sc[p, k] += lima
    gr, grs, _ = recip_grad_sums(points, x, q, H, g, accuracy)
    return e2s * (val + gr), e2s * (sc + grs[None, :])


def induced_grad_at(points, skip_atom, x, alpha, mu, pd, damp, image, dd_cutoff=None):
    """(g_induced [m, 6], scale [m, 6]): polar_field_grad_at's induced sums (tests/point_grad_ref.py) with the image rule
    handed over: image(p) -> d [n, 3]"""
    points = np.asarray(points, np.float64).reshape(-1, 3)
    m = len(points)
    skip_atom = np.full(m, -1) if skip_atom is None else np.asarray(skip_atom)
    alpha = np.asarray(alpha)
    mu = np.where((alpha != 0)[:, None], mu, 0.0)
    idx = np.arange(len(x))
    val, sc = np.zeros((m, 6)), np.zeros((m, 6))
    for p in range(m):
        d = image(points[p])
        rsq = np.sum(d * d, axis=1)
        ind = (idx != skip_atom[p]) & (rsq > 0) & (alpha != 0)
        if dd_cutoff is not None:
            ind = ind & (rsq < dd_cutoff * dd_cutoff)
        r = np.sqrt(np.where(rsq > 0, rsq, 1.0))
        _, s5, _, s5a = ptr.tensor_scalars64(r, pd, damp)
        s7, s7a = s7_64(r, pd, damp)
        md, mda = np.sum(mu * d, axis=1), np.sum(np.abs(mu * d), axis=1)
        for k, (a, b) in enumerate(COMP):
            dd = d[:, a] * d[:, b]
            u = s5 * (mu[:, a] * d[:, b] + d[:, a] * mu[:, b]) - s7 * md * dd
            ua = s5a * (np.abs(mu[:, a] * d[:, b]) + np.abs(d[:, a] * mu[:, b])) + s7a * mda * np.abs(dd)
            if a == b:
                u, ua = u + s5 * md, ua + s5a * mda
            val[p, k], sc[p, k] = u[ind].sum(), ua[ind].sum()
    return val, sc


def field_grad_numpy(points, skip_atom, molecule, x, q, alpha, mol, mu, prd, tilt, cut_coul, dd_cutoff, pd, damp, e2s, g, accuracy):
    """{name: (value, scale)} for g_static and g_induced, [m, 6] each.  dd_cutoff None: exact mode, whose uncut induced sums take
    Domain::closest_image's image in a tilted cell (ewald_point_numpy.closest_image_del), as ewald_point_numpy.field_at_numpy."""
    if dd_cutoff is None and tilt is not None and np.any(np.asarray(tilt) != 0.0):
        image = lambda p: epn.closest_image_del(p, x, prd, tilt)   # noqa: E731
    else:
        image = lambda p: ptr.images(p - np.asarray(x, np.float64), prd, tilt)   # noqa: E731
    return dict(g_static=static_grad_at(points, skip_atom, molecule, x, q, mol, prd, tilt, cut_coul, g, accuracy, e2s),
                g_induced=induced_grad_at(points, skip_atom, x, alpha, mu, pd, damp, image, dd_cutoff))
