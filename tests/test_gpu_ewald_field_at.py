"""polar_ewald_field_at on the MI355X: the Ewald field and potential of the polarized box at arbitrary points.

Systems: `mini` (the 60-atom recipe of tests/test_gpu_field_at.py, seed 620, L = 20 A, cut_coul 9, precision 1e-13, here with
`polar_ewald 1e-6` at g = 0.32: 919 k-vectors, one row chunk; exact mode and list mode with dd_cutoff 9, cubic and tilted,
both damping types), `charged` (the tilted mini with every charge raised by 0.05, accuracy 1e-12 at g = 0.6: 16,926 k-vectors
in 631 rows = 17 row chunks, the last one partial; Q = 3 e, so the neutralising-background term is there) and `mof5_h2`
(tests/golden, exact mode and list mode with dd_cutoff 12.8345).  257 points per case by the recipe of test_gpu_field_at.py:
200 uniform in the box, 20 up to two box lengths outside it, 17 at 0.3 A from an atom, 20 exactly on atoms (that atom
skipped); half of them carry a molecule id of the system.

Tolerances: every output against the NumPy reference (tests/ewald_point_numpy.py) within 1e-10 of its maximum over the points
-- the project's figure for whole-sum field comparisons against NumPy.  At atom sites e_static against ef_static within 1e-10
max|ef_static|, alpha (e_static + e_induced) against mu within 1e-9 max|mu| (the solve stopped at rms dmu <= 1e-13)."""
import copy
import os

import numpy as np
import pytest

import ewald_numpy as ew
import ewald_point_numpy as epn
import point_ref as ptr
from helpers import GOLD

pytestmark = pytest.mark.gpu
TILT = (2.1, -1.4, 1.2)
NPTS = 257
ERR_INPUT, ERR_UNSUPPORTED, ERR_STATE = -1, -4, -5
NAMES = ("e_static", "e_induced", "phi_static", "phi_induced")


def _mini(wl, extra=(), tilt=None, damp="exponential", g=0.32, acc="1e-6", shift=0.0, n=60, seed=620, L=20.0):
    """tests/test_gpu_field_at.py::_mini with the polar_ewald keyword (acc None: without), g_ewald = g and every charge raised
    by `shift`"""
    rng = np.random.default_rng(seed)
    typ = rng.integers(1, 3, n).astype(np.int32)
    q = rng.normal(0, 0.4, n)
    q -= q.mean()
    q += shift
    alpha = np.where(rng.uniform(size=n) < 0.7, rng.uniform(0.3, 1.2, n), 0.0)
    mol = (np.arange(n) // 3 + 1).astype(np.int32)
    mol[-6:] = 0
    x = rng.uniform(0.5, L - 0.5, (n, 3))
    kw = ["polar_ewald", acc] if acc else []
    st = wl.parse_pair_style_args(["8.0", "9.0", "damp_type", damp, "precision", "1e-13", "max_iterations", "200"] + kw + list(extra))
    rows = [["1", "1", "0.10", "3.0"], ["1", "2", "0.08", "3.2"], ["2", "2", "0.06", "3.4"]]
    s = wl.make_system(x, q, alpha, typ, mol, np.zeros(3), np.array([L, L, L]), 2, rows, st, g, name="mini")
    if tilt is not None:   # spread over a tilted cell, no LJ list (the polarization loops are the ones under test)
        s2 = copy.copy(s)
        s2.tilt, s2.triclinic = tilt, 1
        fr = rng.uniform(0, 1, (n, 3))
        s2.x = np.ascontiguousarray(fr @ ptr.cell_matrix((L, L, L), tilt).T)
        s2.nghost = 0
        for k in ("q", "alpha", "type", "molecule"):
            setattr(s2, k, np.ascontiguousarray(getattr(s, k)[:n]))
        s2.owner = np.arange(n)
        s2.ilist = np.zeros(0, np.int32); s2.numneigh = np.zeros(n, np.int32)
        s2.firstneigh = np.zeros(n, np.int64); s2.neigh = np.zeros(0, np.int32)
        s = s2
    return s


def _system(wl, case, mode, tilt, damp):
    lst = ["dd_cutoff", "9.0"] if mode == "list" else []
    if case == "mini":
        return _mini(wl, extra=lst, tilt=tilt, damp=damp), 1e-6
    if case == "charged":
        return _mini(wl, extra=lst, tilt=tilt, damp=damp, g=0.6, acc="1e-12", shift=0.05), 1e-12
    extra = ["precision", "1e-13", "max_iterations", "200", "use_previous", "no", "polar_ewald", "1e-6"] + (["dd_cutoff", "12.8345"] if mode == "list" else [])
    return wl.load_fixture(os.path.join(GOLD, case + ".npz"), extra_args=extra)[0], 1e-6


def _tilt(s):
    return tuple(s.tilt) if getattr(s, "triclinic", 0) else None


def _points(s, seed=3):
    """257 points, their skip_atom and molecule arrays (the recipe of tests/test_gpu_field_at.py::_points)"""
    rng = np.random.default_rng(seed)
    n = s.nlocal
    H = ptr.cell_matrix(s.prd, _tilt(s))
    lo = np.asarray(s.boxlo, np.float64)
    inside = lo + rng.uniform(0, 1, (200, 3)) @ H.T
    outside = lo + rng.uniform(-2, 3, (20, 3)) @ H.T
    near = rng.integers(0, n, 17)
    u = rng.normal(size=(17, 3))
    close = s.x[near] + 0.3 * u / np.linalg.norm(u, axis=1)[:, None]
    on = rng.choice(n, 20, replace=False)
    pts = np.ascontiguousarray(np.concatenate([inside, outside, close, s.x[on]]))
    assert len(pts) == NPTS
    skip = np.full(NPTS, -1, np.int32)
    skip[-20:] = on
    ids = np.unique(s.molecule[:n])
    ids = ids[ids != 0]
    pmol = np.where(rng.random(NPTS) < 0.5, rng.choice(ids, NPTS), 0).astype(np.int32)
    return pts, skip, pmol


_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _close_cached_handles():
    yield
    for v in _CACHE.values():
        v[1].close()
    _CACHE.clear()


def _solved(wl, pkg, case, mode, tilt=None, damp="exponential"):
    """(system, handle after one compute, its outputs, accuracy): one solve per case for the whole module"""
    key = (case, mode, tilt, damp)
    if key not in _CACHE:
        s, acc = _system(wl, case, mode, tilt, damp)
        p = pkg.pair_from_system(s)
        out = p.compute(eflag=1, vflag=2)
        assert out["status"] == 0 and out["rms_dmu"] <= 1e-13 and out["nkvec"] > 0
        _CACHE[key] = (s, p, out, acc)
    return _CACHE[key]


_REF = {}


def _reference(key, s, out, acc, pts, skip, pmol):
    """the NumPy reference of a case's 257 points, computed once"""
    if key not in _REF:
        n, st = s.nlocal, s.settings
        _REF[key] = epn.field_at_numpy(pts, skip, pmol, s.x[:n], s.q[:n], s.alpha[:n], s.molecule[:n], out["mu"], s.prd, _tilt(s), st.cut_coul,
                                       st.dd_cutoff if st.dd_cutoff > 0 else None, st.polar_damp, st.damping_type, np.sqrt(s.qqrd2e),
                                       s.g_ewald, acc)
    return _REF[key]


NUMPY_CASES = [("mini", "exact", None, "exponential"), ("mini", "exact", None, "none"), ("mini", "list", None, "exponential"),
               ("mini", "list", None, "none"), ("mini", "list", TILT, "exponential"), ("mini", "exact", TILT, "exponential"),
               ("charged", "list", TILT, "exponential"), ("mof5_h2", "exact", None, "exponential"), ("mof5_h2", "list", None, "exponential")]


@pytest.mark.parametrize("case,mode,tilt,damp", NUMPY_CASES)
def test_every_output_against_the_numpy_reference(case, mode, tilt, damp, wl, pkg):
    s, p, out, acc = _solved(wl, pkg, case, mode, tilt, damp)
    if case == "charged":   # what this case is about: a charged box, and a k-vector set of several row chunks with a partial last one
        assert abs(s.q[:s.nlocal].sum() - 3.0) < 1e-9
        k, _ = ew.kvectors(ptr.cell_matrix(s.prd, tilt), s.g_ewald, acc)
        hk = np.rint(k @ ptr.cell_matrix(s.prd, tilt) / (2 * np.pi)).astype(int)[:, :2]
        nrow, nk = len(np.unique(hk, axis=0)), len(k)
        assert out["nkvec"] == nk and 15000 <= nk <= 19000
        rpc = -(-nrow * 1024 // nk)
        assert -(-nrow // rpc) >= 3 and nrow % rpc != 0
    pts, skip, pmol = _points(s)
    got = p.ewald_field_at(pts, skip, pmol)
    ref = _reference((case, mode, tilt, damp), s, out, acc, pts, skip, pmol)
    worst = {k: float(np.max(np.abs(got[k] - ref[k])) / np.max(np.abs(ref[k]))) for k in NAMES}
    print(case, mode, tilt, damp, "nkvec %d  max |got - ref| / max |ref|:" % out["nkvec"], "  ".join("%s %.2e" % kv for kv in worst.items()),
          " ms real %.3f recip %.3f" % (got["ms_real"], got["ms_recip"]))
    # (exact mode in a tilted cell: the reference takes Domain::closest_image's image for the uncut induced sums, as the kernel)
    for k in NAMES:
        assert worst[k] <= 1e-10, (k, worst[k])
    assert abs(got["ms"] - got["ms_real"] - got["ms_recip"]) <= 1e-9 * got["ms"] and got["ms_real"] > 0.0 and got["ms_recip"] > 0.0


@pytest.mark.parametrize("case,mode,tilt", [("mof5_h2", "exact", None), ("mof5_h2", "list", None), ("mini", "exact", TILT), ("charged", "list", TILT)])
def test_a_point_on_an_atom_sees_what_the_atom_sees(case, mode, tilt, wl, pkg):
    """every atom: e_static = ef_static[i] of the Ewald step, alpha_i (e_static + e_induced) = mu_i"""
    s, p, out, acc = _solved(wl, pkg, case, mode, tilt)
    n = s.nlocal
    idx = np.arange(n, dtype=np.int32)
    got = p.ewald_field_at(s.x[:n], idx, s.molecule[:n], potential=False)
    ef, mu, alpha = out["ef_static"], out["mu"], s.alpha[:n]
    e_err = np.max(np.abs(got["e_static"] - ef)) / np.max(np.abs(ef))
    pol = alpha != 0
    assert np.sum(pol) > 10
    m_err = np.max(np.abs(alpha[pol, None] * (got["e_static"] + got["e_induced"])[pol] - mu[pol])) / np.max(np.abs(mu))
    print(case, mode, tilt, "e_static vs ef_static %.2e  alpha (e_static + e_induced) vs mu %.2e" % (e_err, m_err))
    assert e_err <= 1e-10 and m_err <= 1e-9


@pytest.mark.parametrize("case,mode,tilt", [("mini", "list", None), ("mini", "exact", None), ("charged", "list", TILT)])
def test_passes_and_order_do_not_change_a_bit(case, mode, tilt, wl, pkg, monkeypatch):
    s, p, out, acc = _solved(wl, pkg, case, mode, tilt)
    rng = np.random.default_rng(17)
    H, lo = ptr.cell_matrix(s.prd, tilt), np.asarray(s.boxlo, np.float64)
    for m in (0, 1, 63, 64, 65, 300):
        pts = np.ascontiguousarray(lo + rng.uniform(-0.5, 1.5, (m, 3)) @ H.T)
        skip = rng.integers(-1, s.nlocal, m).astype(np.int32)
        pmol = rng.integers(0, 4, m).astype(np.int32)
        monkeypatch.delenv("POLAR_FIELD_AT_CHUNK", raising=False)
        one = p.ewald_field_at(pts, skip, pmol)
        assert all(one[k].shape == ((m, 3) if k.startswith("e_") else (m,)) for k in NAMES)
        again = p.ewald_field_at(pts, skip, pmol)
        monkeypatch.setenv("POLAR_FIELD_AT_CHUNK", "37")
        chunked = p.ewald_field_at(pts, skip, pmol)
        monkeypatch.delenv("POLAR_FIELD_AT_CHUNK")
        perm = rng.permutation(m)
        shuffled = p.ewald_field_at(pts[perm], skip[perm], pmol[perm])
        nophi = p.ewald_field_at(pts, skip, pmol, potential=False)
        assert nophi["phi_static"] is None and nophi["phi_induced"] is None
        for k in NAMES:
            assert np.array_equal(one[k], again[k]), (m, k, "second call")
            assert np.array_equal(one[k], chunked[k]), (m, k, "passes of 37")
            assert np.array_equal(one[k][perm], shuffled[k]), (m, k, "permuted")
            if k.startswith("e_"):
                assert np.array_equal(one[k], nophi[k]), (m, k, "field only")
        if m:
            assert np.all(np.isfinite(one["e_static"])) and np.max(np.abs(one["e_induced"])) > 0.0


@pytest.mark.parametrize("case,mode,tilt", [("mini", "exact", TILT), ("mini", "list", None), ("mof5_h2", "exact", None)])
def test_far_points_agree_with_their_wrapped_images(case, mode, tilt, wl, pkg):
    """A point 10^6 box lengths out is a rounded number: at most 2.6e7 A from the origin, it carries half an ulp of that, 1.9e-9 A,
    per axis.  The points are kept 1 A from every atom, where a real-space pair term at distance r moves by at most 3 * that / r
    of itself and a reciprocal term by |k| * that <= 2e-8 of itself; 1e-7 of an output's maximum over the points bounds the
    difference with a decade to spare (the terms of a sum do not all move the same way).  Beyond 2^30 box lengths, where a
    coordinate no longer says where in the box the point is, the call is refused."""
    s, p, out, acc = _solved(wl, pkg, case, mode, tilt)
    n = s.nlocal
    H = ptr.cell_matrix(s.prd, _tilt(s))
    rng = np.random.default_rng(43)
    pts = np.asarray(s.boxlo) + rng.uniform(0, 1, (400, 3)) @ H.T
    dmin = np.array([np.sqrt(np.min(np.sum(ptr.images(q - s.x[:n], s.prd, _tilt(s)) ** 2, axis=1))) for q in pts])
    pts = np.ascontiguousarray(pts[dmin >= 1.0][:64])
    assert len(pts) == 64
    far = pts + (rng.choice([-1.0, 1.0], (64, 3)) * 1.0e6) @ H.T
    near, got = p.ewald_field_at(pts), p.ewald_field_at(far)
    worst = {k: float(np.max(np.abs(got[k] - near[k])) / np.max(np.abs(near[k]))) for k in NAMES}
    print(case, mode, tilt, "far against near, of the maximum:", "  ".join("%s %.2e" % kv for kv in worst.items()))
    for k in NAMES:
        assert np.all(np.isfinite(got[k])) and worst[k] <= 1e-7, (k, worst[k])
    for bad in (2.0 ** 31 * float(s.prd[2]), -1e20, 1e300):
        x = pts[:3].copy()
        x[1, 2] = bad
        assert _code(pkg, lambda: p.ewald_field_at(x)) == ERR_INPUT
    again = p.ewald_field_at(pts)
    for k in NAMES:
        assert np.array_equal(again[k], near[k]), k


def test_a_call_leaves_the_handle_as_it_was(wl, pkg):
    """`deterministic yes`, `use_previous no`, one handle: compute, compute, ewald_field_at, compute.  Repeated computes of such a
    handle agree bit for bit in the forces, the dipoles and the static field (tests/test_gpu_polar_ewald.py::
    test_deterministic_runs_are_bit_identical); the compute after the probe must be one more of them, and a probe of the same
    dipoles gives the same bits."""
    s, _ = wl.load_fixture(os.path.join(GOLD, "mof5_h2.npz"), extra_args=["use_previous", "no", "dd_cutoff", "9.0", "deterministic", "yes", "polar_ewald", "1e-6"])
    p = pkg.pair_from_system(s)
    try:
        a, b = p.compute(eflag=1, vflag=2), p.compute(eflag=1, vflag=2)
        pts, skip, pmol = _points(s)
        first = p.ewald_field_at(pts, skip, pmol)
        c = p.compute(eflag=1, vflag=2)
        second = p.ewald_field_at(pts, skip, pmol)
    finally:
        p.close()
    for x, y in ((a, b), (b, c)):
        for k in ("f", "mu", "ef_static"):
            assert np.array_equal(x[k], y[k]), k
        for k in ("iterations", "sweeps", "status", "dd_pairs", "nkvec"):
            assert x[k] == y[k], k
        assert x["u_ef"] == y["u_ef"]
    for k in NAMES:
        assert np.array_equal(first[k], second[k]), k


def _code(pkg, fn):
    with pytest.raises(pkg.PolarError) as e:
        fn()
    return e.value.code


def _works(s, p):
    out = p.compute(eflag=1, vflag=2)
    got = p.ewald_field_at(s.x[:5], np.arange(5, dtype=np.int32), s.molecule[:5])
    assert np.max(np.abs(got["e_static"] - out["ef_static"][:5])) <= 1e-10 * np.max(np.abs(out["ef_static"]))


def test_keyword_off_is_refused_and_points_to_field_at(wl, pkg):
    s = _mini(wl, acc=None)
    p = pkg.pair_from_system(s)
    p.compute()
    with pytest.raises(pkg.PolarError) as e:
        p.ewald_field_at(s.x[:3])
    assert e.value.code == ERR_UNSUPPORTED and "polar_field_at" in str(e.value)
    p.field_at(s.x[:3])
    assert p.compute()["status"] == 0
    p.close()


def test_call_window_before_any_compute_and_after_set_positions(wl, pkg):
    s = _mini(wl)
    p = pkg.pair_from_system(s)
    assert _code(pkg, lambda: p.ewald_field_at(s.x[:3])) == ERR_STATE
    _works(s, p)
    p.set_positions(s.x)
    assert _code(pkg, lambda: p.ewald_field_at(s.x[:3])) == ERR_STATE
    _works(s, p)
    p.close()


def test_a_row_sharded_handle_is_refused(wl, pkg):
    s = _mini(wl, extra=["dd_cutoff", "9.0"])
    p = pkg.pair_from_system(s, row_range=(0, 30))
    assert _code(pkg, lambda: p.ewald_field_at(s.x[:3])) == ERR_UNSUPPORTED
    p._ck(p.L.polar_set_row_range(p.h, 0, -1))
    _works(s, p)
    p.close()


def test_field_at_still_refuses_a_polar_ewald_handle(wl, pkg):
    s, p, out, acc = _solved(wl, pkg, "mini", "list")
    assert _code(pkg, lambda: p.field_at(s.x[:3])) == ERR_UNSUPPORTED
    p.ewald_field_at(s.x[:3])


@pytest.mark.parametrize("tilt", [None, TILT])
def test_ewald_field_grid_shapes_and_numbers(tilt, wl, pkg):
    s, p, out, acc = _solved(wl, pkg, "mini", "list", tilt)
    g = p.ewald_field_grid((8, 6, 4))
    assert g["e_static"].shape == g["e_induced"].shape == (4, 6, 8, 3) and g["phi_static"].shape == g["phi_induced"].shape == (4, 6, 8)
    flat = p.ewald_field_at(p.grid_points((8, 6, 4)))
    for k in NAMES:
        assert np.array_equal(g[k].reshape(flat[k].shape), flat[k]), k
    assert np.array_equal(g["phi_static"][2, 1, 3], flat["phi_static"][(2 * 6 + 1) * 8 + 3])
    nophi = p.ewald_field_grid((8, 6, 4), potential=False)
    assert nophi["phi_static"] is None and np.array_equal(nophi["e_static"], g["e_static"])
