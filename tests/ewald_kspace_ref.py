"""Long-double reference of the reciprocal-space sums of `polar_ewald`, for the kernels of
csrc/polar_ewald.hpp: S(k), M(k), E_rec, F_rec, u_ef and the two halves of the reciprocal virial, each with its scale
(the sum of the absolute values of its terms, times e2s where the value carries it).

Plain NumPy in np.longdouble (64-bit mantissa: `available()`).  The cell, its inverse and the fractional coordinates
s = H^-1 r are formed in long double; a phase is 2 pi frac(h s_x + k s_y + l s_z) from the INTEGER (h, k, l), reduced modulo
1 before the multiplication by 2 pi.  So nothing here is shared with the kernels' recurrences or with the x @ k.T of
tests/ewald_numpy.py.  The k-vectors and c_k are taken as given (the table itself is pinned by tests/test_plan_host.py);
`kvectors_check` says how far they are from 2 pi hkl H^-1.  tests/test_ewald_kspace_ref_host.py pins this module to
ewald_numpy."""
import numpy as np

LD = np.longdouble
PHASES = 2_000_000        # phases held at once: the sums are blocked over k


def available():
    return np.finfo(LD).eps < 2e-19


def two_pi():
    return 8 * np.arctan(LD(1))


def cell(prd, tilt=(0.0, 0.0, 0.0)):
    """H = [a b c] of a LAMMPS box and H^-1 (both upper triangular), in long double"""
    lx, ly, lz = (LD(v) for v in prd)
    xy, xz, yz = (LD(v) for v in tilt)
    z = LD(0)
    H = np.array([[lx, xy, xz], [z, ly, yz], [z, z, lz]], dtype=LD)
    Hi = np.array([[1 / lx, -xy / (lx * ly), (xy * yz - ly * xz) / (lx * ly * lz)], [z, 1 / ly, -yz / (ly * lz)], [z, z, 1 / lz]], dtype=LD)
    return H, Hi


def frac(x, Hi, shift=None):
    """s = H^-1 (x + shift) per atom, [n][3]; the products written out (no BLAS for long double, and the order is fixed)"""
    x = np.asarray(x, dtype=LD).reshape(-1, 3)
    if shift is not None:
        x = x + np.asarray(shift, dtype=LD)
    return np.stack([Hi[0, 0] * x[:, 0] + Hi[0, 1] * x[:, 1] + Hi[0, 2] * x[:, 2], Hi[1, 1] * x[:, 1] + Hi[1, 2] * x[:, 2], Hi[2, 2] * x[:, 2]], 1)


def _cis(hkl, s):
    """cos and sin of 2 pi frac(h s_x + k s_y + l s_z), [n][nk]"""
    n3 = np.asarray(hkl)[:, :3].astype(LD)
    t = s[:, 0, None] * n3[None, :, 0] + s[:, 1, None] * n3[None, :, 1] + s[:, 2, None] * n3[None, :, 2]
    t -= np.floor(t)
    t *= two_pi()
    return np.cos(t), np.sin(t)


def structure_factors(prd, tilt, x, q, hkl, shift=None):
    """S(k) alone as (re, im) [nk][2] and its scale sum_j |q_j| (the lattice-shift invariant of the host test)"""
    _, Hi = cell(prd, tilt)
    s = frac(x, Hi, shift)
    q = np.asarray(q, dtype=LD)
    hkl = np.asarray(hkl).reshape(-1, 4)
    S = np.zeros((len(hkl), 2), dtype=LD)
    step = max(1, PHASES // max(len(s), 1))
    for a in range(0, len(hkl), step):
        c, sn = _cis(hkl[a:a + step], s)
        S[a:a + step, 0] = (q[:, None] * c).sum(0)
        S[a:a + step, 1] = (q[:, None] * sn).sum(0)
    return S, np.abs(q).sum()


def kvectors_check(prd, tilt, g, hkl, kv):
    """How far the table is from its formulas.  Returns (dk, dc):
    dk = max |kv_a - 2 pi (hkl H^-1)_a| over sum_b 2 pi |n_b H^-1_ba|, the k-vector against long double, of the sum of its terms;
    dc = max relative distance of c_k from (8 pi / V) exp(-k^2 / 4 g^2) / k^2 evaluated in FP64 from the table's own k^2 =
    kx kx + ky ky + kz kz (a rounding of k^2 moves the exponential by up to k^2 / 4 g^2 = -ln accuracy roundings, so c_k
    can follow the formula to a few ulp only from the same k^2).  Both in units of eps = 2^-52."""
    hkl, kv = np.asarray(hkl).reshape(-1, 4), np.asarray(kv, dtype=np.float64).reshape(-1, 4)
    if len(kv) == 0:
        return 0.0, 0.0
    _, Hi = cell(prd, tilt)
    n3 = hkl[:, :3].astype(LD)
    terms = two_pi() * n3[:, :, None] * Hi[None, :, :]             # [nk][b][a]
    dk = np.max(np.abs(kv[:, :3].astype(LD) - terms.sum(1)) / np.abs(terms).sum(1).clip(min=np.finfo(np.float64).tiny))
    k2 = kv[:, 0] * kv[:, 0] + kv[:, 1] * kv[:, 1] + kv[:, 2] * kv[:, 2]
    vol = float(prd[0]) * float(prd[1]) * float(prd[2])
    want = 8.0 * np.pi / vol * np.exp(-k2 / (4.0 * g * g)) / k2
    dc = np.max(np.abs(kv[:, 3] - want) / want)
    eps = np.finfo(np.float64).eps
    return float(dk / eps), float(dc / eps)


SIX = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))       # LAMMPS' order xx, yy, zz, xy, xz, yz


def reference(prd, tilt, g, e2s, x, q, mu, ef_s, hkl, kv):
    """Every output of the k-space kernels for n atoms (positions x, charges q, dipoles mu, static field ef_s) and the
    table (hkl [nk][4] integers, kv [nk][4] = kx, ky, kz, c_k).  A dict of long-double arrays, value and `<name>_scale`:
      S, M [nk][2]        sum_j q_j e^{ik.r_j}, sum_j (k.mu_j) e^{ik.r_j};          scales: sum_j |q_j| (a number), sum_j sum_a |k_a mu_j,a| [nk]
      erec [n][3]         e2s sum_k c_k k Im(e^{ik.r_i} conj S);                     scale: e2s sum_k c_k |k| |S| (a number)
      f [n][3]            e2s sum_k c_k k [(k.mu_i) Re(e conj S) - q_i Re(e conj M)]; scale [n]: e2s sum_k c_k |k| (|k.mu_i| |S| + |q_i| |M|)
      u_ef                -sum_i mu_i . ef_s,i;                                      scale: sum_i sum_a |mu_i,a ef_s,i,a|
      w_atom [6]          -sum_i mu_i,a erec_i,b;                                    scale: sum_i |mu_i,a| erec_scale
      w_k [6]             sum_k U_k (delta_ab - 2 k_a k_b (1/k^2 + 1/4g^2)), U_k = -e2s c_k Im(M conj S);
                          scale: sum_k e2s c_k (|M_y S_x| + |M_x S_y|) (delta_ab + 2 |k_a k_b| (1/k^2 + 1/4g^2))"""
    _, Hi = cell(prd, tilt)
    s = frac(x, Hi)
    n = len(s)
    q = np.asarray(q, dtype=LD).reshape(n)
    mu = np.asarray(mu, dtype=LD).reshape(n, 3)
    ef_s = np.asarray(ef_s, dtype=LD).reshape(n, 3)
    hkl = np.asarray(hkl).reshape(-1, 4)
    kv = np.asarray(kv, dtype=np.float64).reshape(-1, 4).astype(LD)
    nk = len(kv)
    e2s, g = LD(e2s), LD(g)
    S, M = np.zeros((nk, 2), dtype=LD), np.zeros((nk, 2), dtype=LD)
    M_scale = np.zeros(nk, dtype=LD)
    erec, f = np.zeros((n, 3), dtype=LD), np.zeros((n, 3), dtype=LD)
    erec_scale, f_scale = LD(0), np.zeros(n, dtype=LD)
    w_k, w_k_scale = np.zeros(6, dtype=LD), np.zeros(6, dtype=LD)
    step = max(1, PHASES // max(n, 1))
    for a in range(0, nk, step):
        k, ck = kv[a:a + step, :3], kv[a:a + step, 3]
        c, sn = _cis(hkl[a:a + step], s)                                    # [n][kb]
        kmu = mu[:, 0, None] * k[None, :, 0] + mu[:, 1, None] * k[None, :, 1] + mu[:, 2, None] * k[None, :, 2]
        sx, sy = (q[:, None] * c).sum(0), (q[:, None] * sn).sum(0)
        mx, my = (kmu * c).sum(0), (kmu * sn).sum(0)
        S[a:a + step, 0], S[a:a + step, 1], M[a:a + step, 0], M[a:a + step, 1] = sx, sy, mx, my
        M_scale[a:a + step] = (np.abs(mu[:, 0, None] * k[None, :, 0]) + np.abs(mu[:, 1, None] * k[None, :, 1])
                               + np.abs(mu[:, 2, None] * k[None, :, 2])).sum(0)
        knorm = np.sqrt((k * k).sum(1))
        sabs, mabs = np.sqrt(sx * sx + sy * sy), np.sqrt(mx * mx + my * my)
        im_s = sn * sx[None, :] - c * sy[None, :]                            # Im(e conj S)
        re_s = c * sx[None, :] + sn * sy[None, :]
        re_m = c * mx[None, :] + sn * my[None, :]
        ve = im_s * ck[None, :]
        vf = (kmu * re_s - q[:, None] * re_m) * ck[None, :]
        for b in range(3):
            erec[:, b] += e2s * (ve * k[None, :, b]).sum(1)
            f[:, b] += e2s * (vf * k[None, :, b]).sum(1)
        erec_scale += e2s * (ck * knorm * sabs).sum()
        f_scale += e2s * ((np.abs(kmu) * sabs[None, :] + np.abs(q)[:, None] * mabs[None, :]) * (ck * knorm)[None, :]).sum(1)
        u = -e2s * ck * (my * sx - mx * sy)
        us = e2s * ck * (np.abs(my * sx) + np.abs(mx * sy))
        bb = 2 * (1 / (knorm * knorm) + 1 / (4 * g * g))
        for j, (p, r) in enumerate(SIX):
            w_k[j] += (u * ((1 if p == r else 0) - bb * k[:, p] * k[:, r])).sum()
            w_k_scale[j] += (us * ((1 if p == r else 0) + bb * np.abs(k[:, p] * k[:, r]))).sum()
    w_atom = np.array([-(mu[:, p] * erec[:, r]).sum() for p, r in SIX], dtype=LD)
    w_atom_scale = np.array([np.abs(mu[:, p]).sum() * erec_scale for p, r in SIX], dtype=LD)
    return dict(S=S, S_scale=np.abs(q).sum(), M=M, M_scale=M_scale, erec=erec, erec_scale=erec_scale, f=f, f_scale=f_scale,
                u_ef=-(mu * ef_s).sum(), u_ef_scale=np.abs(mu * ef_s).sum(), w_atom=w_atom, w_atom_scale=w_atom_scale,
                w_k=w_k, w_k_scale=w_k_scale)


def hkl_of(k, prd, tilt):
    """the integer (h, k, l, 0) of k-vectors k = 2 pi n H^-1 given in FP64 (ewald_numpy.kvectors): n = k H / 2 pi, rounded"""
    H, _ = cell(prd, tilt)
    n3 = np.rint((np.asarray(k, dtype=np.float64) @ H.astype(np.float64)) / (2 * np.pi)).astype(np.int64)
    return np.hstack([n3, np.zeros((len(n3), 1), np.int64)])
