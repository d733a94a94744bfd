"""Independent NumPy implementation of the `polar_ewald` static field, the charge-dipole energy at fixed dipoles, its
forces and its virial.  Used by test_polar_ewald_host.py (checked against itself: g-independence,
a brute-force lattice sum, finite differences) and by test_gpu_polar_ewald.py (the device against it).

Units as the library's: fields and forces carry the factor e2s = sqrt(qqrd2e) once, energies mu . E."""
import math

import numpy as np
from scipy.special import erf, erfc


def cell(prd, tilt=(0.0, 0.0, 0.0)):
    """H = [a b c] of a LAMMPS box (a = (lx,0,0), b = (xy,ly,0), c = (xz,yz,lz))."""
    lx, ly, lz = prd
    xy, xz, yz = tilt
    return np.array([[lx, xy, xz], [0.0, ly, yz], [0.0, 0.0, lz]], dtype=np.float64)


def kvectors(H, g, accuracy):
    """Half-space k-vectors with |k| <= 2 g sqrt(-ln accuracy) and c_k = (8 pi / V) exp(-k^2/4g^2) / k^2."""
    Hi = np.linalg.inv(H)
    kcut = 2.0 * g * math.sqrt(-math.log(accuracy))
    lens = np.linalg.norm(H, axis=0)
    nm = [int(math.floor(kcut * L / (2 * math.pi))) for L in lens]
    hh, kk, ll = np.meshgrid(np.arange(0, nm[0] + 1), np.arange(-nm[1], nm[1] + 1), np.arange(-nm[2], nm[2] + 1), indexing="ij")
    n = np.stack([hh.ravel(), kk.ravel(), ll.ravel()], 1)
    half = (n[:, 0] > 0) | ((n[:, 0] == 0) & (n[:, 1] > 0)) | ((n[:, 0] == 0) & (n[:, 1] == 0) & (n[:, 2] > 0))
    n = n[half]
    k = 2 * math.pi * n @ Hi            # k = 2 pi H^-T n  (row vectors: n^T H^-1)
    k2 = np.einsum("ij,ij->i", k, k)
    keep = (k2 <= kcut * kcut) & (k2 > 0)
    k, k2 = k[keep], k2[keep]
    vol = abs(np.linalg.det(H))
    return k, 8 * math.pi / vol * np.exp(-k2 / (4 * g * g)) / k2


def _pairs(x, H, cut):
    """All i != j minimum-image pairs within cut (each ordered pair once): i, j, d = x_i - x_j(image)."""
    Hi = np.linalg.inv(H)
    n = len(x)
    I, J = np.nonzero(~np.eye(n, dtype=bool))
    d = x[I] - x[J]
    s = d @ Hi.T
    s -= np.rint(s)
    d = s @ H.T
    r2 = np.einsum("ij,ij->i", d, d)
    m = r2 <= cut * cut
    return I[m], J[m], d[m], r2[m]


def _b12(r2, g, kept):
    r = np.sqrt(r2)
    e = 2 * g / math.sqrt(math.pi) * np.exp(-g * g * r2)
    b1 = np.where(kept, (erfc(g * r) / r + e) / r2, -(erf(g * r) / r - e) / r2)
    b2 = (3 * b1 + 2 * g * g * e) / r2
    return b1, b2


def _excluded(mol, I, J):
    return (mol[I] == mol[J]) & (mol[I] != 0)


def _kblocks(nk, kblock):
    """slices of at most kblock k-vectors (the dense [n, nk] phase arrays of a large box would not fit in memory)"""
    return [slice(a, min(nk, a + kblock)) for a in range(0, nk, kblock)]


def field(x, q, mol, H, cut, g, accuracy, e2s=1.0, parts=False, kblock=None):
    """Static field E_i (times e2s): real space + exclusion correction + reciprocal space.
    kblock: the reciprocal sum in blocks of that many k-vectors (S(k) of a block needs all atoms and no other k: the same
    terms, the partial sums of the blocks added in order); None, the default: all k-vectors at once."""
    x = np.asarray(x, np.float64)
    I, J, d, r2 = _pairs(x, H, cut)
    b1, _ = _b12(r2, g, ~_excluded(mol, I, J))
    ereal = np.zeros_like(x)
    np.add.at(ereal, I, (b1 * q[J])[:, None] * d)
    k, c = kvectors(H, g, accuracy)
    if kblock is None:
        ph = x @ k.T                                        # [n, nk]
        S = (q[:, None] * np.exp(1j * ph)).sum(0)
        erec = (np.imag(np.exp(1j * ph) * np.conj(S)[None, :]) * c[None, :]) @ k
    else:
        erec = np.zeros_like(x)
        for b in _kblocks(len(k), kblock):
            e = np.exp(1j * (x @ k[b].T))
            S = (q[:, None] * e).sum(0)
            erec += (np.imag(e * np.conj(S)[None, :]) * c[None, b]) @ k[b]
    if parts:
        return e2s * ereal, e2s * erec
    return e2s * (ereal + erec)


def energy(x, q, mol, mu, H, cut, g, accuracy, e2s=1.0):
    """Charge-dipole energy at fixed dipoles: -sum mu . E."""
    return -np.sum(mu * field(x, q, mol, H, cut, g, accuracy, e2s))


def forces_virial(x, q, mol, mu, H, cut, g, accuracy, e2s=1.0, parts=False, kblock=None):
    """Analytic forces -dU/dx at fixed mu and the virial [xx, yy, zz, xy, xz, yz] in LAMMPS' convention (sum r_a F_b).
    parts=True: (real-space forces, reciprocal forces, pairwise real-space virial, reciprocal virial) instead.
    kblock: as in field()."""
    x = np.asarray(x, np.float64)
    I, J, d, r2 = _pairs(x, H, cut)
    b1, b2 = _b12(r2, g, ~_excluded(mol, I, J))
    mi, mj = mu[I], mu[J]
    pi = np.einsum("ij,ij->i", mi, d)[:, None]
    pj = np.einsum("ij,ij->i", mj, d)[:, None]
    fp = e2s * (q[J][:, None] * (b1[:, None] * mi - b2[:, None] * pi * d) - q[I][:, None] * (b1[:, None] * mj - b2[:, None] * pj * d))
    f = np.zeros_like(x)
    np.add.at(f, I, fp)
    w = 0.5 * np.einsum("pa,pb->ab", d, fp)            # every pair seen from both atoms
    k_all, c_all = kvectors(H, g, accuracy)
    f_real, w_real = f.copy(), w.copy()
    f_rec = None
    for b in ([slice(None)] if kblock is None else _kblocks(len(k_all), kblock)):
        k, c = k_all[b], c_all[b]
        e = np.exp(1j * (x @ k.T))
        S = (q[:, None] * e).sum(0)
        kmu = mu @ k.T
        M = (kmu * e).sum(0)
        res = np.real(e * np.conj(S)[None, :])
        rem = np.real(e * np.conj(M)[None, :])
        f_blk = e2s * ((kmu * res - q[:, None] * rem) * c[None, :]) @ k
        f_rec = f_blk if f_rec is None else f_rec + f_blk
        erec = e2s * (np.imag(e * np.conj(S)[None, :]) * c[None, :]) @ k
        U = -e2s * c * np.imag(M * np.conj(S))
        k2 = np.einsum("ij,ij->i", k, k)
        bb = 2 * (1 / k2 + 1 / (4 * g * g))
        w += np.einsum("k,ab->ab", U, np.eye(3)) - np.einsum("k,ka,kb->ab", U * bb, k, k)
        w -= np.einsum("ia,ib->ab", mu, erec)
    if f_rec is None:
        f_rec = np.zeros_like(x)
    f += f_rec
    six = lambda m: np.array([m[0, 0], m[1, 1], m[2, 2], m[0, 1], m[0, 2], m[1, 2]])  # noqa: E731
    if parts:
        return f_real, f_rec, six(w_real), six(w) - six(w_real)
    return f, six(w)


def fdotr(x, f):
    """sum x_i f_i in LAMMPS' order [xx, yy, zz, xy, xz, yz] (Pair::virial_fdotr_compute)."""
    m = np.einsum("ia,ib->ab", x, f)
    return np.array([m[0, 0], m[1, 1], m[2, 2], m[0, 1], m[0, 2], m[1, 2]])


def brute_field(x, q, mol, H, cut, nshell):
    """Tin-foil lattice sum by brute force: sum over images in spherical shells |n| <= nshell of q_j d / r^3, minus the
    excluded minimum-image pairs.  Converges (conditionally, in spherical order) for a
    neutral cubic box; the spherical sum lacks the tin-foil surface term 4 pi P / 3V, which is added."""
    x = np.asarray(x, np.float64)
    n = len(x)
    rng = np.arange(-nshell, nshell + 1)
    img = np.stack(np.meshgrid(rng, rng, rng, indexing="ij"), -1).reshape(-1, 3)
    img = img[np.einsum("ij,ij->i", img, img) <= nshell * nshell]
    shifts = img @ H.T
    E = np.zeros_like(x)
    for i in range(n):
        d = x[i][None, None, :] - (x[None, :, :] + shifts[:, None, :])   # [img, j, 3]
        r2 = np.einsum("ijk,ijk->ij", d, d)
        r2[r2 == 0] = np.inf
        E[i] = np.einsum("ij,ijk->k", q[None, :] / r2 ** 1.5, d)
    I, J, d, r2 = _pairs(x, H, cut)
    ex = _excluded(mol, I, J)
    np.add.at(E, I[ex], -(q[J[ex]] / r2[ex] ** 1.5)[:, None] * d[ex])
    vol = abs(np.linalg.det(H))
    P = (q[:, None] * x).sum(0)
    return E + 4 * math.pi / (3 * vol) * P
