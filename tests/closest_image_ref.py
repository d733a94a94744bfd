"""What tests/test_closest_image.py (CPU) and tests/test_gpu_closest_image.py (GPU) share: the recorded images of the
reference's compiled Domain::closest_image (tests/golden/ref_closest_image.npz, written by
oracle/ref_seam/gen_closest_image_golden.py), lattice helpers, and a plain NumPy float64 statement of the static field,
the damped dipole tensor and the dipole solve, built from GIVEN pair displacements (so that the image rule is an input)."""
import copy
import os

import numpy as np

from helpers import GOLD

_Z = None


def fixture():
    global _Z
    if _Z is None:
        with np.load(os.path.join(GOLD, "ref_closest_image.npz")) as z:
            _Z = {k: z[k] for k in z.files}
        for v in _Z.values():
            v.setflags(write=False)   # one copy, shared by every test
    return _Z


def box_names():
    return [str(s) for s in fixture()["box_name"]]


def box(name):
    z = fixture()
    b = box_names().index(name)
    lo, hi = int(z["first"][b]), int(z["first"][b + 1])
    return dict(name=name, prd=z["box_prd"][b], tilt=z["box_tilt"][b], periodic=z["box_periodic"][b],
                triclinic=int(z["box_triclinic"][b]), xi=z["xi"][lo:hi], xj=z["xj"][lo:hi], xjimage=z["xjimage"][lo:hi],
                klass=z["klass"][lo:hi])


def system(name):
    z = fixture()
    k = [str(s) for s in z["sys_name"]].index(name)
    return dict(name=name, prd=z["sys_prd"][k], tilt=z["sys_tilt"][k], x=z["sys_x"][k], xjimage=z["sys_xjimage"][k])


def cell(prd, tilt):
    """rows a, b, c of a LAMMPS cell with tilt = (xy, xz, yz)"""
    return np.array([[prd[0], 0.0, 0.0], [tilt[0], prd[1], 0.0], [tilt[1], tilt[2], prd[2]]])


def widths(prd, tilt, periodic=(1, 1, 1)):
    """distance between opposite faces, per periodic lattice vector: the distance of the vector from the span of the
    other periodic ones = 1 / sqrt((G^-1)_kk), G the Gram matrix of the periodic vectors; inf where not periodic"""
    h = cell(prd, tilt)
    idx = [k for k in range(3) if periodic[k]]
    w = np.full(3, np.inf)
    if idx:
        hp = h[idx]
        gi = np.linalg.inv(hp @ hp.T)
        w[idx] = 1.0 / np.sqrt(np.diag(gi))
    return w


def image_shifts(prd, tilt, periodic=(1, 1, 1), reach=2):
    h = cell(prd, tilt)
    r = [np.arange(-reach, reach + 1) if p else np.array([0]) for p in periodic]
    return np.array([i * h[0] + j * h[1] + k * h[2] for i in r[0] for j in r[1] for k in r[2]], dtype=np.float64)


def nearest(prd, tilt, periodic, d, reach=2):
    """brute force over the (2 reach + 1)^3 images d + i a + j b + k c: the shortest one and its length"""
    sh = image_shifts(prd, tilt, periodic, reach)
    c = d[:, None, :] + sh[None, :, :]
    k = (c ** 2).sum(-1).argmin(-1)
    best = c[np.arange(len(d)), k]
    return best, np.sqrt((best ** 2).sum(-1))


def mini_system(wl, x, prd, tilt, triclinic, cut_coul, extra=()):
    """The system of tests/test_gpu_edges.py::test_triclinic_box_exact_mode on given positions: charges, polarizabilities,
    types and molecules of its _mini(seed 11), no LJ / Coulomb list and no ghosts (the polarization loops are the ones that
    use the minimum image)."""
    n = len(x)
    rng = np.random.default_rng(11)
    x0 = rng.uniform(2.0, float(min(prd)) - 2.0, (n, 3))   # make_system lays its lists out on these; replaced below
    typ = rng.integers(1, 3, n).astype(np.int32)
    q = rng.normal(0, 0.4, n)
    q -= q.mean()
    alpha = np.where(rng.uniform(size=n) < 0.7, rng.uniform(0.3, 1.2, n), 0.0)
    mol = (np.arange(n) // 2 + 1).astype(np.int32)
    st = wl.parse_pair_style_args(["8.0", repr(float(cut_coul)), "damp_type", "exponential"] + list(extra))
    rows = [["1", "1", "0.10", "3.0"], ["1", "2", "0.08", "3.2"], ["2", "2", "0.06", "3.4"]]
    s = wl.make_system(x0, q, alpha, typ, mol, np.zeros(3), np.array(prd, float), 2, rows, st, 0.25,
                       name="closest_image")
    s2 = copy.copy(s)
    s2.tilt, s2.triclinic = tuple(float(t) for t in tilt), int(triclinic)
    s2.x = np.ascontiguousarray(x, dtype=np.float64)
    s2.nghost = 0
    for k in ("q", "alpha", "type", "molecule"):
        setattr(s2, k, np.ascontiguousarray(getattr(s, k)[:n]))
    s2.owner = np.arange(n)
    s2.ilist = np.zeros(0, np.int32); s2.numneigh = np.zeros(n, np.int32)
    s2.firstneigh = np.zeros(n, np.int64); s2.neigh = np.zeros(0, np.int32)
    return s2


def pair_del(x, xjimage):
    """del[i, j] = x_i - image_j for i < j and its negative for j > i: the reference asks closest_image once per pair i < j
    and uses that displacement for both atoms (PS.cpp:324-361, 1243-1316)"""
    return upper_antisymmetric(x[:, None, :] - xjimage)


def upper_antisymmetric(d):
    """d[i, j] for i < j, -d[j, i] for i > j, 0 on the diagonal"""
    iu = np.triu(np.ones(d.shape[:2], bool), 1)
    out = np.where(iu[:, :, None], d, 0.0)
    return out - out.transpose(1, 0, 2)


def static_field(D, q, mol, cut_coul, qqrd2e):
    """PS.cpp:324-386: shifted-force field of the charges, rsq <= cut_coul^2, not inside a molecule (id 0 aside)"""
    n = len(q)
    r2 = (D ** 2).sum(-1)
    ok = (r2 <= cut_coul * cut_coul) & ~np.eye(n, dtype=bool) & ((mol[:, None] != mol[None, :]) | (mol[:, None] == 0))
    r2s = np.where(ok, r2, 1.0)
    ef = np.where(ok, (1.0 / r2s - 1.0 / (cut_coul * cut_coul)) / np.sqrt(r2s), 0.0)
    return (ef[:, :, None] * q[None, :, None] * D).sum(1) * np.sqrt(qqrd2e)


def dipole_matrix(D, alpha, polar_damp):
    """PS.cpp:1243-1316 with exponential damping: [3n, 3n], 1 / alpha on the diagonal (inf where alpha = 0), the tensor
    blocks off it, no cutoff"""
    n = len(alpha)
    r2 = (D ** 2).sum(-1) + np.eye(n)
    r = np.sqrt(r2)
    pd = polar_damp
    e = np.exp(-pd * r)
    d1 = 1.0 - e * (0.5 * pd * pd * r2 + pd * r + 1.0)
    d2 = 1.0 - e * (pd * pd * pd * r2 * r / 6.0 + 0.5 * pd * pd * r2 + pd * r + 1.0)
    r3, r5 = 1.0 / (r * r * r), 1.0 / (r * r * r * r * r)
    T = -3.0 * D[:, :, :, None] * D[:, :, None, :] * (d2 * r5)[:, :, None, None]
    T = T + (d1 * r3)[:, :, None, None] * np.eye(3)[None, None]
    T[np.arange(n), np.arange(n)] = 0.0
    M = T.transpose(0, 2, 1, 3).reshape(3 * n, 3 * n).copy()
    with np.errstate(divide="ignore"):
        M[np.arange(3 * n), np.arange(3 * n)] = np.repeat(1.0 / alpha, 3)
    return M


def solve_dipoles(M, ef, alpha):
    """mu_i = alpha_i (E_i - sum_j T_ij mu_j) at its fixed point, directly: (1 / alpha + T) mu = E over the polarizable
    atoms, mu = 0 elsewhere; eng_pol = -1/2 sum mu . E"""
    n = len(alpha)
    pol = np.repeat(alpha != 0.0, 3)
    mu = np.zeros(3 * n)
    mu[pol] = np.linalg.solve(M[np.ix_(pol, pol)], ef.reshape(-1)[pol])
    mu = mu.reshape(n, 3)
    return mu, -0.5 * float((mu * ef).sum())
