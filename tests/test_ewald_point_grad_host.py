"""polar_ewald_field_grad_at without a GPU: its NumPy reference pinned on its own, and the plain-C++ arithmetic of the kernels
(csrc/polar_ewald_point_grad.hpp) built by g++ with libm against references.

1. tests/ewald_point_grad_numpy.py on its own, in the charged tilted box of tests/test_ewald_point_host.py (60 atoms, every charge
   raised by 0.05, Q = 3 e, g = 0.6, accuracy 1e-12) and in its neutral twin:
   * central differences (h = 1e-4 A) of ewald_point_numpy.static_at's e_static, at points at least 1.5 A from every atom and
     more than 10 h from the cut_coul shell of every image, and the symmetry of the difference tensor.  Bound 1e-7 of the
     largest component: the differencing's own error is h^2 / 6 times the third derivative of the field -- at most 60 q / r^5
     for a bare charge, 8 at r = 1.5 A and q = 1: 1.3e-8 against components of order 0.1 to 1 -- plus eps |e| / h = 1e-12.
   * the trace: -4 pi e2s Q / V at every point, within 1e-10 of the sum of the absolute terms (the project's figure for whole
     sums against NumPy; the truncation residue of the two sums is 2 g^2 G(rc) = 1e-13 per unit charge).
   * g-independence between g = 0.5 and 0.6: the residue is the erfc(g rc) shell term of the smaller g, as DESIGN section 6e
     records for the field.  Measured 4.7e-9 of the largest component (2 g^2 G(rc) = 4.5e-10 per unit charge at g = 0.5,
     components of order 0.1); asserted at 5e-9, the next 1-2-5 step.
   * a skipped atom on the point: g_static there is the limit of the values 1e-4, 1e-5 and 1e-6 A away, which approach it
     linearly -- what the -(2/3) g^2 (2g/sqrt(pi)) q term is, and the series of the erf form near it.
2. polar_point_grad_pair_ew pair by pair against the 40-digit backend of tests/pair_ref.py (tests/ewald_point_grad_ref.py):
   2,300 pairs by the recipe of test_ewald_point_host.py with r from 0.3 A -- kept and excluded, either side of cut_coul and of
   dd_cutoff, short pairs at 0.3 .. 0.6 A (where the excluded form cancels), atoms on the point kept and excluded -- and a
   hundred excluded atoms from 1e-5 to 0.3 A.  Bound: 2e-15 of scale for all twelve gradient components, the ledger's figure
   for every pair function.  Measured maxima over the four instances (this test prints them): g_static 1.81e-15 (kept atoms
   near cut_coul: the exponent g^2 r^2 = 8.5 carries the rounding of r^2), g_induced 1.53e-15.  For the excluded atoms below
   0.3 A the scale of the closed form (its cancelling terms) grows as 1 / (gr)^2 over the value and says less and less; there
   the error is also taken relative to the VALUE of the pair's largest component, against the series of B1 and B2 at the
   backend's precision.  Bound 1e-7: the closed forms are wrong by up to 8 eps / (2/3 g^2 r^2) = 9e-8 of the value at
   g^2 r^2 = 2^-26, below which the header takes the atom as on the point and leaves 1.8 g^2 r^2 <= 2.7e-8 of the value out
   (measured 3.3e-8).  The six field sums are compared bit for bit with polar_point_pair_ew<..., false> from the same build.
3. ew_point_grad_rows against the NumPy reciprocal gradient: 1e-12 of sum_k c_k |k|^2 |S(k)|, the multiple of eps
   test_ewald_point_host.py asserts for ew_point_rows with the gradient's scale; rows split at arbitrary chunk boundaries; its
   three field sums are those of ew_point_rows<false> bit for bit.
4. The harness as a stand-alone program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import ewald_numpy as ew
import ewald_point_grad_numpy as egn
import ewald_point_grad_ref as egr
import ewald_point_numpy as epn
import pair_ref as pr
import point_ref as ptr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "lammps-induced-dipole-polarization-pair-style_amd")
SRC = os.path.join(ROOT, "tests", "ewald_point_grad", "ewald_point_grad.cpp")
BOUND = 2e-15
N = 2300
RC, DDC, PD, E2S, G = 9.0, 7.5, 2.1304, 18.2226, 0.3243
TILT = (2.1, -1.4, 1.2)
H_FD = 1e-4
COMP = egn.COMP


# ---------------------------------------------------------------------------------------------------------------------
# 1. the reference on its own

def _mini_charged(tilt=TILT, shift=0.05):
    """charges, molecule ids and positions of tests/test_ewald_point_host.py::_mini_charged (seed 620)"""
    n, L = 60, 20.0
    rng = np.random.default_rng(620)
    rng.integers(1, 3, n)
    q = rng.normal(0, 0.4, n)
    q -= q.mean()
    rng.uniform(size=n), rng.uniform(0.3, 1.2, n)
    mol = (np.arange(n) // 3 + 1).astype(np.int32)
    mol[-6:] = 0
    x = rng.uniform(0.5, L - 0.5, (n, 3))
    if tilt is not None:
        x = np.ascontiguousarray(rng.uniform(0, 1, (n, 3)) @ ptr.cell_matrix((L, L, L), tilt).T)
    return x, q + shift, mol, (L, L, L)


def _clear_points(x, prd, tilt, cut, want, seed):
    """The clearance rule of tests/test_gpu_field_grad_at.py::_clear_points, restated for a tilted cell: points at least 1.5 A from
    every atom and further than 10 h from the cut_coul shell of all 27 images."""
    rng = np.random.default_rng(seed)
    Hm = ptr.cell_matrix(prd, tilt)
    sh = np.array([(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)], np.float64) @ Hm.T
    pts = []
    while len(pts) < want:
        p = rng.uniform(0, 1, 3) @ Hm.T
        d0 = ptr.images(p - x, prd, tilt)
        r = np.sqrt(np.sum((d0[:, None, :] + sh[None, :, :]) ** 2, axis=2))
        if np.min(r) >= 1.5 and np.min(np.abs(r - cut)) > 10 * H_FD:
            pts.append(p)
    return np.array(pts)


def test_reference_gradient_is_the_central_difference_of_the_reference_field_and_symmetric():
    x, q, mol, prd = _mini_charged()
    pts = _clear_points(x, prd, TILT, RC, 12, 5)
    pmol = np.where(np.arange(12) % 2 == 0, mol[:12], 0)
    g, _ = egn.static_grad_at(pts, None, pmol, x, q, mol, prd, TILT, RC, 0.6, 1e-12)
    fd = np.zeros((12, 3, 3))
    for b in range(3):
        dp = np.zeros(3)
        dp[b] = H_FD
        step = (pts + dp)[:, b] - (pts - dp)[:, b]
        fd[:, :, b] = (epn.static_at(pts + dp, None, pmol, x, q, mol, prd, TILT, RC, 0.6, 1e-12)[0] -
                       epn.static_at(pts - dp, None, pmol, x, q, mol, prd, TILT, RC, 0.6, 1e-12)[0]) / step[:, None]
    top = np.max(np.abs(g))
    err = max(float(np.max(np.abs(fd[:, a, b] - g[:, k]))) for k, (a, b) in enumerate(COMP)) / top
    asym = float(np.max(np.abs(fd - fd.transpose(0, 2, 1)))) / top
    print("central differences against g_static: %.1e, their asymmetry: %.1e of the largest component %.2e" % (err, asym, top))
    assert err <= 1e-7 and asym <= 1e-7 and top > 0.01


@pytest.mark.parametrize("shift", [0.0, 0.05], ids=["neutral", "charged"])
def test_reference_trace_is_minus_four_pi_q_over_v(shift):
    x, q, mol, prd = _mini_charged(shift=shift)
    assert abs(q.sum() - 60 * shift) < 1e-12
    pts = np.concatenate([_clear_points(x, prd, TILT, RC, 6, 6), x[[4, 9]], x[[7]] + np.array([[0.3, 0.0, 0.0]])])
    skip, pmol = np.array([-1] * 6 + [4, 9, -1]), np.array([0, mol[0], 0, mol[5], 0, 0, mol[4], 0, mol[7]])
    e2s = 18.2226
    g, sc = egn.static_grad_at(pts, skip, pmol, x, q, mol, prd, TILT, RC, 0.6, 1e-12, e2s)
    want = -4 * math.pi * e2s * q.sum() / abs(np.linalg.det(ptr.cell_matrix(prd, TILT)))
    off = np.abs(g[:, :3].sum(axis=1) - want) / sc[:, :3].sum(axis=1)
    print("shift %.2f: trace %.6e wanted %.6e, worst |difference| / sum |terms| %.1e" % (shift, g[0, :3].sum(), want, off.max()))
    assert np.all(off <= 1e-10)
    assert shift == 0.0 or abs(want) > 1e-2


def test_reference_does_not_depend_on_g_in_a_charged_box():
    x, q, mol, prd = _mini_charged()
    pts = np.concatenate([_clear_points(x, prd, TILT, RC, 6, 7), x[[4]], x[[7]] + np.array([[0.3, 0.0, 0.0]])])
    skip, pmol = np.array([-1] * 6 + [4, -1]), np.array([0, mol[0], 0, mol[5], 0, 0, mol[4], mol[7]])
    ga, gb = (egn.static_grad_at(pts, skip, pmol, x, q, mol, prd, TILT, RC, g, 1e-12)[0] for g in (0.5, 0.6))
    res = float(np.max(np.abs(ga - gb)) / np.max(np.abs(gb)))
    print("g 0.5 against 0.6: %.2e of the largest component (erfc(0.5 * 9) = %.1e)" % (res, math.erfc(4.5)))
    assert res <= 5e-9


def test_a_skipped_atom_on_the_point_is_the_limit_of_points_beside_it():
    x, q, mol, prd = _mini_charged()
    atoms = np.array([j for j in range(60) if abs(q[j]) > 0.2][:4])
    u = np.array([0.48, -0.6, 0.64])
    at = lambda p: egn.static_grad_at(p, atoms, mol[atoms], x, q, mol, prd, TILT, RC, 0.6, 1e-12)[0]   # noqa: E731
    g0 = at(x[atoms])
    diff = [float(np.max(np.abs(at(x[atoms] + dl * u) - g0))) for dl in (1e-4, 1e-5, 1e-6)]
    term = (2.0 / 3.0) * 0.36 * (1.2 / math.sqrt(math.pi)) * np.min(np.abs(q[atoms]))
    print("|g(delta) - g(0)| at 1e-4, 1e-5, 1e-6 A: %.2e %.2e %.2e; the limit term is at least %.2e" % (*diff, term))
    assert 9.0 <= diff[0] / diff[1] <= 11.0 and 9.0 <= diff[1] / diff[2] <= 11.0
    assert term > 100 * diff[0]          # without the term, or with another factor, the three values would not approach g(0)


# ---------------------------------------------------------------------------------------------------------------------
# 2. and 3. the C++ header with libm

def _gxx(out, extra):
    return subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", f"-I{PKG}/csrc", "-o", out, SRC] + extra,
                          capture_output=True, text=True)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("ewald_point_grad") / "libewald_point_grad.so")
    r = _gxx(so, ["-fPIC", "-shared"])
    assert r.returncode == 0, r.stderr[-3000:]
    L = C.CDLL(so)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    L.ew_point_grad_pair_eval.restype = None
    L.ew_point_grad_pair_eval.argtypes = [C.c_int, dp, dp, dp, dp, ip, ip, C.c_int, C.c_int] + [C.c_double] * 5 + [dp]
    for f in (L.ew_point_grad_rows_eval, L.ew_point_rows_field_eval):
        f.restype = None
        f.argtypes = [C.c_int, dp, ip, dp, dp, C.c_int, C.c_int, dp]
    return L


_dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))   # noqa: E731
_ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))      # noqa: E731
TINY = slice(2200, N)


@pytest.fixture(scope="module")
def pairs():
    rng = np.random.default_rng(20261022)
    r = rng.uniform(0.3, 12.0, N)
    r[:200] = RC * (1 + rng.uniform(-1e-9, 1e-9, 200))          # either side of cut_coul
    r[200:400] = DDC * (1 + rng.uniform(-1e-9, 1e-9, 200))      # either side of dd_cutoff
    r[400:500] = rng.uniform(0.3, 0.6, 100)                     # short range: the damping terms cancel
    r[2000:2200] = rng.uniform(0.3, 0.6, 200)                   # short intramolecular pairs, excluded below
    r[TINY] = 10.0 ** rng.uniform(-5.0, math.log10(0.3), 100)   # an excluded atom all but on the point
    u = rng.normal(size=(N, 3))
    d = r[:, None] * u / np.linalg.norm(u, axis=1)[:, None]
    d[500:510] = 0.0                                            # atoms on the point
    q = rng.uniform(-1.0, 1.0, N)
    q[rng.random(N) < 0.1] = 0.0
    q[500:510] = rng.uniform(0.2, 1.0, 10)
    q[TINY] = rng.uniform(0.2, 1.0, 100)
    alpha = rng.uniform(0.2, 1.5, N)
    alpha[rng.random(N) < 0.2] = 0.0
    mu = rng.normal(0.0, 0.3, (N, 3))                           # alpha = 0 rows keep theirs: stale dipoles
    kept = (rng.random(N) >= 0.1).astype(np.int32)
    kept[2000:] = 0
    kept[500:505], kept[505:510] = 1, 0                         # on the point: kept and excluded
    induced = np.where(kept == 1, 1, (rng.random(N) < 0.5)).astype(np.int32)   # some excluded atoms are the skip_atom
    induced[TINY] = 0                                           # (the skip_atom: the guest's own site)
    return np.ascontiguousarray(d), q, alpha, np.ascontiguousarray(mu), kept, induced


def _eval(lib, pairs, allpairs, damp):
    d, q, alpha, mu, kept, induced = pairs
    out = np.zeros((N, 24))
    lib.ew_point_grad_pair_eval(N, _dp(d), _dp(q), _dp(mu), _dp(alpha), _ip(kept), _ip(induced), allpairs, damp, RC, DDC, PD, E2S, G, _dp(out))
    return out


@pytest.mark.parametrize("damp", [0, 1])
@pytest.mark.parametrize("allpairs", [1, 0])
def test_point_grad_pair_ew_with_libm_stays_within_the_ledgers_bound(lib, pairs, allpairs, damp):
    d, q, alpha, mu, kept, induced = pairs
    be = pr.backend()
    got = _eval(lib, pairs, allpairs, damp)
    ref = egr.grad_pair_ew(d, q, mu, alpha, kept, induced, RC, None if allpairs else DDC, PD, E2S, G, damp, be)
    rsq = np.sum(d * d, axis=1)
    on = rsq == 0
    st_on = ref["st_on"]
    assert np.any(rsq[:200] <= RC * RC) and np.any(rsq[:200] > RC * RC) and 0 < np.sum(st_on[:200]) < 200
    assert np.sum(st_on & (kept == 0)) > 400 and np.sum(st_on & (kept == 1)) > 500 and np.sum(ref["in_on"]) > 500
    t_tiny = G * G * rsq[TINY]
    assert np.sum(t_tiny < 2.0 ** -26) > 20 and np.sum(t_tiny >= 2.0 ** -26) > 20     # both sides of the on-the-point rule
    worst = {}
    for name, col0, sums in (("g_static", 6, ref["gs"]), ("g_induced", 12, ref["gi"])):
        w = 0.0
        for k, sm in enumerate(sums):
            v, s = sm.unpack()
            off = (s == 0.0) & ~(on & (name == "g_static") & (k < 3))
            assert np.all(got[off, col0 + k] == 0.0), (name, k, "a pair that takes no part added something")
            sel = s != 0.0
            w = max(w, float(np.max(pr.err_over(got[sel, col0 + k], v[sel], s[sel], be))))
        worst[name] = w
    # the excluded atoms below 0.3 A: also relative to the value of the pair's largest component, against the series
    b1, b2 = egr.excluded_b12_series(rsq[TINY], G, be)
    dl = [be.arr(d[TINY, k]) for k in range(3)]
    qe = be.arr(q[TINY]) * be.arr(E2S + np.zeros(100))
    val = [qe * ((b1 if a == b else 0 * b1) - b2 * dl[a] * dl[b]) for a, b in COMP]
    top = np.max(np.abs(np.stack([be.f64(v) for v in val])), axis=0)
    w_tiny = max(float(np.max(pr.err_over(got[TINY, 6 + k], val[k], top, be))) for k in range(6))
    if be.name == "mpmath":      # 40 digits carry the closed form down to 1e-5 A: the series is the same function
        vc = [c.unpack()[0] for c in egr.static_grad_terms(d[TINY], q[TINY], np.zeros(100, bool), E2S, G, be)]
        assert max(float(np.max(np.abs(be.f64(vc[k] - val[k])) / top)) for k in range(6)) <= 1e-17
    print("allpairs %d damp %d  max error / scale: " % (allpairs, damp) + "  ".join("%s %.3e" % kv for kv in worst.items()) +
          "  (excluded atoms at 1e-5 .. 0.3 A, error / value: %.3e)" % w_tiny)
    for name, w in worst.items():
        assert w <= BOUND, (name, w)
    assert w_tiny <= 1e-7, w_tiny
    # atoms on the point, kept or excluded: -q (2/3) g^2 2g/sqrt(pi) on the diagonal, nothing else
    lim = -E2S * q[on] * (2.0 / 3.0) * G * G * (2 * G / math.sqrt(math.pi))
    assert np.sum(on) == 10 and np.all(got[on][:, list(range(0, 6)) + list(range(9, 18))] == 0.0)
    assert np.all(np.abs(got[on, 6:9] - lim[:, None]) <= BOUND * np.abs(lim[:, None])) and np.all(lim != 0)
    # the skip_atom and alpha = 0 with a stale dipole: no induced part
    assert np.all(got[induced == 0][:, [3, 4, 5] + list(range(12, 18))] == 0.0) and np.all(got[alpha == 0.0][:, [3, 4, 5] + list(range(12, 18))] == 0.0)
    # the field sums: the bits of polar_point_pair_ew<..., false> on the same pair, and not all zero
    assert np.array_equal(got[:, 0:6], got[:, 18:24]) and np.sum(got[:, 0:6] != 0) > 3000


def _table(Hm, g, accuracy):
    """the k-vector table of the step (csrc/polar_plan.hpp) from ewald_numpy.kvectors: rows = {h, k, first l, first index}"""
    k, c = ew.kvectors(Hm, g, accuracy)
    n = np.rint(k @ Hm / (2 * math.pi)).astype(np.int64)
    new = np.ones(len(n), bool)
    new[1:] = np.any(n[1:, :2] != n[:-1, :2], axis=1)
    assert np.all(n[1:, 2][~new[1:]] == n[:-1, 2][~new[1:]] + 1)     # consecutive l within a row
    first = np.nonzero(new)[0]
    rows = np.zeros((len(first) + 1, 4), np.int32)
    rows[:-1, :3], rows[:-1, 3] = n[first], first
    rows[-1] = (0, 0, 0, len(k))
    return k, c, rows, np.ascontiguousarray(np.concatenate([k, c[:, None]], axis=1))


@pytest.mark.parametrize("tilt", [None, TILT], ids=["cubic", "tilted"])
@pytest.mark.parametrize("g,accuracy", [(0.32, 1e-6), (0.6, 1e-12)], ids=["hundreds", "ten_thousands"])
def test_point_grad_rows_against_the_numpy_reciprocal_gradient(lib, tilt, g, accuracy):
    x, q, _, prd = _mini_charged(tilt)
    Hm = ptr.cell_matrix(prd, tilt)
    k, c, rows, kv = _table(Hm, g, accuracy)
    nk, nrow = len(k), len(rows) - 1
    assert (300 <= nk <= 999) if accuracy == 1e-6 else (10000 <= nk <= 30000), nk
    S = epn.structure_factors(x, q, k)
    S2 = np.ascontiguousarray(np.stack([S.real, S.imag], axis=1))
    rng = np.random.default_rng(8)
    fr = rng.uniform(0, 1, (40, 3))
    fr[:4] = [[0, 0, 0], [1 - 2.0 ** -53, 0.5, 0.25], [0.5, 1 - 2.0 ** -53, 1 - 2.0 ** -53], [2.0 ** -30, 2.0 ** -30, 0.999]]
    pts = fr @ Hm.T
    g_ref, _, scale = egn.recip_grad_sums(pts, x, q, Hm, g, accuracy)
    s = np.ascontiguousarray(pts @ np.linalg.inv(Hm).T)
    out = np.zeros((len(pts), 9))
    lib.ew_point_grad_rows_eval(len(pts), _dp(s), _ip(rows), _dp(kv), _dp(S2), 0, nrow, _dp(out))
    err = np.max(np.abs(out[:, 3:] - g_ref)) / scale
    print("nk %d rows %d: gradient %.2e of sum c |k|^2 |S|" % (nk, nrow, err))
    assert err <= 1e-12 and np.max(np.abs(g_ref)) > 0
    # rows split at arbitrary boundaries, the pieces folded in order, as the kernels do
    cuts = np.concatenate([[0], np.sort(rng.choice(np.arange(1, nrow), min(9, nrow - 1), replace=False)), [nrow]])
    folded = np.zeros_like(out)
    for r0, r1 in zip(cuts[:-1], cuts[1:]):
        part = np.zeros_like(out)
        lib.ew_point_grad_rows_eval(len(pts), _dp(s), _ip(rows), _dp(kv), _dp(S2), int(r0), int(r1), _dp(part))
        folded += part
    assert np.max(np.abs(folded[:, 3:] - g_ref)) <= 1e-12 * scale
    # the three field sums: ew_point_rows<false>'s, bit for bit, over the whole table and over a piece of it
    for r0, r1 in ((0, nrow), (int(cuts[1]), int(cuts[2]))):
        a, b = np.zeros((len(pts), 9)), np.zeros((len(pts), 4))
        lib.ew_point_grad_rows_eval(len(pts), _dp(s), _ip(rows), _dp(kv), _dp(S2), r0, r1, _dp(a))
        lib.ew_point_rows_field_eval(len(pts), _dp(s), _ip(rows), _dp(kv), _dp(S2), r0, r1, _dp(b))
        assert np.array_equal(a[:, :3], b[:, :3]) and np.max(np.abs(b[:, :3])) > 0 and np.all(b[:, 3] == 0.0)


def test_the_same_code_as_a_program_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    exe = str(tmp_path / "ewald_point_grad_san")
    r = _gxx(exe, ["-DEWALD_POINT_GRAD_MAIN", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe, "2000"], capture_output=True, text=True)
    print(r.stdout.strip())
    assert r.returncode == 0, (r.returncode, r.stdout[-1000:], r.stderr[-3000:])
    m = re.match(r"instances 4 inputs (\d+) pair checks (\d+) row checks (\d+) failures (\d+)", r.stdout)
    assert m and int(m.group(1)) == 2000 and int(m.group(2)) == 16 * 2000 and int(m.group(3)) == 151 and int(m.group(4)) == 0, r.stdout
