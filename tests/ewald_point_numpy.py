"""NumPy reference for polar_ewald_field_at: the Ewald field and potential of the polarized box at points, written from the
definition (include/polar_mi355x.h), not from the library's headers.

With d = x_p - x_j (minimum image), r = |d|, g = g_ewald, rc = cut_coul, G(r) = 2g/sqrt(pi) e^(-g^2 r^2),
B1 = (erfc(gr)/r + G) / r^2, the half-space k-vectors and c_k of ewald_numpy.kvectors, S(k) = sum_j q_j e^{ik.x_j}, Q = sum_j q_j:

    e_static   = e2s [ sum_kept q_j B1 d + sum_excl q_j (B1 - 1/r^3) d + sum_k c_k k Im(e^{ik.p} conj S) ]
    phi_static = e2s [ sum_kept q_j erfc(gr)/r - sum_excl q_j erf(gr)/r + sum_k c_k Re(e^{ik.p} conj S) - pi Q / (g^2 V) ]

over the atoms with r^2 <= rc^2.  Excluded: the point's (non-zero) molecule, the point's skip_atom, an atom on the point
(r^2 == 0: nothing in the field, -q_j 2g/sqrt(pi) in the potential).  The induced sums are those of point_ref.field_at_numpy;
in exact mode in a tilted cell, where they are uncut, with the image Domain::closest_image takes (closest_image_del)."""
import math

import numpy as np
from scipy.special import erf, erfc

import point_ref as ptr
from ewald_numpy import kvectors


def structure_factors(x, q, k):
    return (np.asarray(q)[:, None] * np.exp(1j * (np.asarray(x) @ k.T))).sum(0)


def recip_sums(points, x, q, H, g, accuracy):
    """(e [m, 3], phi [m], scale) of the reciprocal sums without e2s and without the Q term; scale = sum_k c_k |k| |S(k)|."""
    k, c = kvectors(H, g, accuracy)
    if len(k) == 0:
        return np.zeros((len(points), 3)), np.zeros(len(points)), 0.0
    S = structure_factors(x, q, k)
    z = np.exp(1j * (np.asarray(points) @ k.T)) * np.conj(S)[None, :]
    return (np.imag(z) * c[None, :]) @ k, (np.real(z) * c[None, :]).sum(1), float(np.sum(c * np.linalg.norm(k, axis=1) * np.abs(S)))


def static_at(points, skip_atom, molecule, x, q, mol, prd, tilt, cut, g, accuracy, e2s=1.0, background=True):
    """(e_static [m, 3], phi_static [m]).  background=False leaves the Q term out (what the g-independence test shows it is for)."""
    points = np.asarray(points, np.float64).reshape(-1, 3)
    x, q, mol = np.asarray(x, np.float64), np.asarray(q, np.float64), np.asarray(mol)
    m = len(points)
    skip_atom = np.full(m, -1) if skip_atom is None else np.asarray(skip_atom)
    molecule = np.zeros(m, int) if molecule is None else np.asarray(molecule)
    H = ptr.cell_matrix(prd, tilt)
    G = 2 * g / math.sqrt(math.pi)
    idx = np.arange(len(x))
    e, phi = np.zeros((m, 3)), np.zeros(m)
    for p in range(m):
        d = ptr.images(points[p] - x, prd, tilt)
        rsq = np.sum(d * d, axis=1)
        inr = rsq <= cut * cut
        on = rsq == 0
        excl = ((mol == molecule[p]) & (molecule[p] != 0)) | (idx == skip_atom[p]) | on
        r = np.sqrt(np.where(on, 1.0, rsq))
        gauss = G * np.exp(-g * g * rsq)
        ph = np.where(excl, -erf(g * r) / r, erfc(g * r) / r)
        b1 = (ph + gauss) / np.where(on, 1.0, rsq)
        sel = inr & ~on
        e[p] = ((q * b1)[:, None] * d)[sel].sum(0)
        phi[p] = np.sum((q * ph)[sel]) - G * np.sum(q[inr & on])
    er, pr_, _ = recip_sums(points, x, q, H, g, accuracy)
    e += er
    phi += pr_
    if background:
        phi -= math.pi * q.sum() / (g * g * abs(np.linalg.det(H)))
    return e2s * e, e2s * phi


def closest_image_del(p, x, prd, tilt, lo=(0.0, 0.0, 0.0)):
    """d = p - x_j(image) [n, 3] by the rule of exact mode in a tilted cell: whole lattice vectors off the point first (floor of its
    fractional coordinates, as the kernels wrap it), then the triclinic branch of Domain::closest_image (domain.cpp:1258-1305,
    restated in oracle/polar_oracle.c orc_closest_image) for every atom: along z, then y, then x, a negative separation has the
    lattice vector added until it is not negative and taken off once if it then exceeds half the edge (a positive one the
    other way round), z carrying yz and xz along, y carrying xy.  Not always the nearest image (tests/test_closest_image.py)."""
    lx, ly, lz = (float(v) for v in prd)
    xy, xz, yz = (float(v) for v in tilt)
    H = ptr.cell_matrix(prd, tilt)
    fr = np.linalg.solve(H, np.asarray(p, np.float64) - np.asarray(lo, np.float64))
    p = np.asarray(p, np.float64) - H @ np.floor(fr)
    d = np.asarray(x, np.float64) - p                      # x_j - x_i, as the reference forms it
    for ax, edge, carry in ((2, lz, ((1, yz), (0, xz))), (1, ly, ((0, xy),)), (0, lx, ())):
        vec = np.zeros(3)
        vec[ax] = edge
        for c, t in carry:
            vec[c] = t
        neg = d[:, ax] < 0.0
        for sign, rows in ((1.0, neg), (-1.0, ~neg)):
            while True:
                todo = rows & (sign * d[:, ax] < 0.0)
                if not np.any(todo):
                    break
                d[todo] += sign * vec
            back = rows & (sign * d[:, ax] > 0.5 * edge)
            d[back] -= sign * vec
    return -d


def induced_at(points, skip_atom, x, alpha, mu, pd, damp, image, dd_cutoff=None):
    """(e_induced [m, 3], phi_induced [m]): polar_field_at's sums (tests/point_ref.py) with the image rule handed over:
    image(p) -> d [n, 3]"""
    points = np.asarray(points, np.float64).reshape(-1, 3)
    m = len(points)
    skip_atom = np.full(m, -1) if skip_atom is None else np.asarray(skip_atom)
    mu = np.where((np.asarray(alpha) != 0)[:, None], mu, 0.0)
    idx = np.arange(len(x))
    e, phi = np.zeros((m, 3)), np.zeros(m)
    for p in range(m):
        d = image(points[p])
        rsq = np.sum(d * d, axis=1)
        ind = (idx != skip_atom[p]) & (rsq > 0) & (np.asarray(alpha) != 0)
        if dd_cutoff is not None:
            ind = ind & (rsq < dd_cutoff * dd_cutoff)
        s3, s5, _, _ = ptr.tensor_scalars64(np.sqrt(np.where(rsq > 0, rsq, 1.0)), pd, damp)
        md = np.sum(mu * d, axis=1)
        e[p] = ((s5 * md)[:, None] * d - s3[:, None] * mu)[ind].sum(0)
        phi[p] = np.sum((s3 * md)[ind])
    return e, phi


def field_at_numpy(points, skip_atom, molecule, x, q, alpha, mol, mu, prd, tilt, cut_coul, dd_cutoff, pd, damp, e2s, g, accuracy):
    """{name: value} for e_static, e_induced [m, 3] and phi_static, phi_induced [m].  dd_cutoff None: exact mode, whose uncut
    induced sums take Domain::closest_image's image in a tilted cell (closest_image_del) -- beyond half the shortest edge not
    always the nearest one, which the static sums (within cut_coul) and list mode (within dd_cutoff) never meet."""
    es, ps = static_at(points, skip_atom, molecule, x, q, mol, prd, tilt, cut_coul, g, accuracy, e2s)
    if dd_cutoff is None and tilt is not None and np.any(np.asarray(tilt) != 0.0):
        ei, pi = induced_at(points, skip_atom, x, alpha, mu, pd, damp, lambda p: closest_image_del(p, x, prd, tilt))
    else:
        ind = ptr.field_at_numpy(points, skip_atom, molecule, x, q, alpha, mol, mu, prd, tilt, cut_coul, dd_cutoff, pd, damp, e2s)
        ei, pi = ind["e_induced"][0], ind["phi_induced"][0]
    return dict(e_static=es, phi_static=ps, e_induced=ei, phi_induced=pi)
