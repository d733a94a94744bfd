"""polar_field_at on the MI355X: the field and the potential of the polarized box at arbitrary points.

Systems: `mini` (60 atoms, L = 20 A, cut_coul 9, precision 1e-13; with dd_cutoff 9 a 4 x 4 x 4 list grid, whose 5-cell stencil
wraps onto itself; also tilted), `lattice200` (200 atoms on a jittered 4 A lattice, L = 28 A, cut_coul 6, dd_cutoff 5.5: a
9 x 9 x 9 grid with many empty cells, whose stencil must skip cells), `mof5_h2` (tests/golden, exact mode and list mode with
dd_cutoff 12.8345: rows longer than one trip).  257 points per case from a seeded generator: 200 uniform in the box, 20 up to
two box lengths outside it, 17 at 0.3 A from an atom, 20 exactly on atoms (that atom skipped); half of them carry a molecule
id of the system.

Tolerances: 1e-10 of a point's scale (sum of the absolute terms, tests/point_ref.py) against the NumPy brute force -- the figure
this project uses for whole-sum field comparisons against NumPy (test_gpu_polar_ewald.py); a dropped or doubled in-cutoff pair is
>= 1e-4 of scale.  At atom sites e_static against ef_static within 1e-10 max|ef_static|, alpha (e_static + e_induced) against
mu within 1e-9 max|mu| (the solve stopped at rms dmu <= 1e-13: three decades for the contraction factor and the division)."""
import copy
import os

import numpy as np
import pytest

import point_ref as ptr
from helpers import GOLD

pytestmark = pytest.mark.gpu
TILT = (2.1, -1.4, 1.2)
NPTS = 257
ERR_INPUT, ERR_UNSUPPORTED, ERR_STATE = -1, -4, -5


def _mini(wl, n=60, seed=620, L=20.0, extra=(), tilt=None, damp="exponential"):
    """The recipe of tests/test_gpu_polar_ewald.py::_mini without the polar_ewald keyword.  Its seed is another one: with seed 7
    two atoms sit 0.50 A apart (0.19 A in the tilted form), the dipole equations (I + alpha T) mu = alpha E are indefinite
    without damping (tilted: with it as well) and no iteration converges; with seed 620 the nearest approach is 1.76 A
    (tilted 1.22 A) and the smallest eigenvalue of the symmetrised system is >= 0.6 for both damping types, both box shapes
    and both modes, so that every case below has the converged dipoles the atom-site check needs."""
    rng = np.random.default_rng(seed)
    typ = rng.integers(1, 3, n).astype(np.int32)
    q = rng.normal(0, 0.4, n)
    q -= q.mean()
    alpha = np.where(rng.uniform(size=n) < 0.7, rng.uniform(0.3, 1.2, n), 0.0)
    mol = (np.arange(n) // 3 + 1).astype(np.int32)
    mol[-6:] = 0
    x = rng.uniform(0.5, L - 0.5, (n, 3))
    st = wl.parse_pair_style_args(["8.0", "9.0", "damp_type", damp, "precision", "1e-13", "max_iterations", "200"] + list(extra))
    rows = [["1", "1", "0.10", "3.0"], ["1", "2", "0.08", "3.2"], ["2", "2", "0.06", "3.4"]]
    s = wl.make_system(x, q, alpha, typ, mol, np.zeros(3), np.array([L, L, L]), 2, rows, st, 0.32, name="mini")
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


def _lattice200(wl, seed=11):
    """200 of the 343 sites of a 4 A lattice, jittered by +-0.8 A (nearest approach >= 2.4 A); charges, polarizabilities and
    molecule ids as tests/test_force_pair_host.py::small_system draws them, without its 0.7 A pair."""
    rng = np.random.default_rng(seed)
    n, L = 200, 28.0
    grid = np.stack(np.meshgrid(np.arange(7), np.arange(7), np.arange(7), indexing="ij"), -1).reshape(-1, 3)
    x = (grid[rng.permutation(343)[:n]] + 0.5) * 4.0 + rng.uniform(-0.8, 0.8, (n, 3))
    q = rng.uniform(-0.8, 0.8, n)
    alpha = rng.uniform(0.2, 1.2, n)
    q[rng.random(n) < 0.25] = 0.0
    alpha[rng.random(n) < 0.25] = 0.0
    mol = (1 + np.arange(n) // 4).astype(np.int32)
    mol[rng.random(n) < 0.2] = 0
    st = wl.parse_pair_style_args(["2.5", "6.0", "damp_type", "exponential", "damp", "2.1304", "polar_gs_ranked", "yes", "use_previous", "no",
                                   "precision", "1e-13", "max_iterations", "200", "dd_cutoff", "5.5"])
    return wl.make_system(np.mod(x, L), q, alpha, np.ones(n, np.int32), mol, np.zeros(3), np.array([L, L, L]), 1,
                          [["1", "1", "0.0", "3.0", "2.5"]], st, 0.25, name="lattice200")


def _system(wl, case, mode, tilt, damp):
    if case == "mini":
        return _mini(wl, extra=(["dd_cutoff", "9.0"] if mode == "list" else []), tilt=tilt, damp=damp)
    if case == "lattice200":
        return _lattice200(wl)
    extra = ["precision", "1e-13", "max_iterations", "200", "use_previous", "no"] + (["dd_cutoff", "12.8345"] if mode == "list" else [])
    return wl.load_fixture(os.path.join(GOLD, case + ".npz"), extra_args=extra)[0]


def _tilt(s):
    return tuple(s.tilt) if getattr(s, "triclinic", 0) else None


def _points(s, seed=3):
    """257 points, their skip_atom and molecule arrays, and the atom each of the last 20 sits on"""
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
    for _, p, _ in _CACHE.values():
        p.close()
    _CACHE.clear()


def _solved(wl, pkg, case, mode, tilt=None, damp="exponential"):
    """(system, handle after one compute, its outputs): one solve per case for the whole module"""
    key = (case, mode, tilt, damp)
    if key not in _CACHE:
        s = _system(wl, case, mode, tilt, damp)
        p = pkg.pair_from_system(s)
        out = p.compute(eflag=1, vflag=2)
        assert out["status"] == 0 and out["rms_dmu"] <= 1e-13
        _CACHE[key] = (s, p, out)
    return _CACHE[key]


def _reference(s, out, pts, skip, pmol):
    n, st = s.nlocal, s.settings
    return ptr.field_at_numpy(pts, skip, pmol, s.x[:n], s.q[:n], s.alpha[:n], s.molecule[:n], out["mu"], s.prd, _tilt(s), st.cut_coul,
                              st.dd_cutoff if st.dd_cutoff > 0 else None, st.polar_damp, st.damping_type, np.sqrt(s.qqrd2e))


NUMPY_CASES = [("mini", "exact", None, "exponential"), ("mini", "exact", None, "none"), ("mini", "list", None, "exponential"),
               ("mini", "list", TILT, "exponential"), ("lattice200", "list", None, "exponential"),
               ("mof5_h2", "exact", None, "exponential"), ("mof5_h2", "list", None, "exponential")]
NAMES = ("e_static", "e_induced", "phi_static", "phi_induced")


@pytest.mark.parametrize("case,mode,tilt,damp", NUMPY_CASES)
def test_every_output_against_the_numpy_brute_force(case, mode, tilt, damp, wl, pkg):
    s, p, out = _solved(wl, pkg, case, mode, tilt, damp)
    if case == "lattice200":   # the grid this case is about
        assert int(s.prd[0] / (0.5 * 6.0)) == 9
    pts, skip, pmol = _points(s)
    got = p.field_at(pts, skip, pmol)
    ref = _reference(s, out, pts, skip, pmol)
    worst = {}
    for k in NAMES:
        v, sc = ref[k]
        assert np.max(sc) > 0.0
        err = np.abs(got[k] - v)
        worst[k] = float(np.max(np.where(sc > 0, err / np.where(sc > 0, sc, 1.0), np.where(err > 0, np.inf, 0.0))))
    print(case, mode, tilt, damp, "max |got - ref| / scale:", "  ".join("%s %.2e" % kv for kv in worst.items()), " ms %.3f" % got["ms"])
    for k in NAMES:
        v, sc = ref[k]
        assert np.all(np.abs(got[k] - v) <= 1e-10 * sc), (k, worst[k])


@pytest.mark.parametrize("case,mode,tilt,damp", NUMPY_CASES + [("mini", "exact", TILT, "exponential")])
def test_a_point_on_an_atom_sees_what_the_atom_sees(case, mode, tilt, damp, wl, pkg):
    s, p, out = _solved(wl, pkg, case, mode, tilt, damp)
    n = s.nlocal
    idx = np.arange(n, dtype=np.int32) if n <= 300 else np.random.default_rng(1).choice(n, 300, replace=False).astype(np.int32)
    got = p.field_at(s.x[idx], idx, s.molecule[idx], potential=False)
    ef, mu, alpha = out["ef_static"], out["mu"], s.alpha[:n]
    e_err = np.max(np.abs(got["e_static"] - ef[idx])) / np.max(np.abs(ef))
    pol = alpha[idx] != 0
    assert np.sum(pol) > 10
    m_err = np.max(np.abs(alpha[idx][pol, None] * (got["e_static"] + got["e_induced"])[pol] - mu[idx][pol])) / np.max(np.abs(mu))
    print(case, mode, tilt, damp, "e_static vs ef_static %.2e  alpha (e_static + e_induced) vs mu %.2e" % (e_err, m_err))
    assert e_err <= 1e-10 and m_err <= 1e-9


@pytest.mark.parametrize("case,mode", [("mini", "list"), ("lattice200", "list"), ("mini", "exact")])
def test_passes_and_order_do_not_change_a_bit(case, mode, wl, pkg, monkeypatch):
    s, p, out = _solved(wl, pkg, case, mode)
    rng = np.random.default_rng(17)
    H, lo = ptr.cell_matrix(s.prd), np.asarray(s.boxlo, np.float64)
    for m in (0, 1, 63, 64, 65, 1000):
        pts = np.ascontiguousarray(lo + rng.uniform(-0.5, 1.5, (m, 3)) @ H.T)
        skip = rng.integers(-1, s.nlocal, m).astype(np.int32)
        pmol = rng.integers(0, 4, m).astype(np.int32)
        monkeypatch.delenv("POLAR_FIELD_AT_CHUNK", raising=False)
        one = p.field_at(pts, skip, pmol)
        assert all(one[k].shape == ((m, 3) if k.startswith("e_") else (m,)) for k in NAMES)
        again = p.field_at(pts, skip, pmol)
        monkeypatch.setenv("POLAR_FIELD_AT_CHUNK", "37")
        chunked = p.field_at(pts, skip, pmol)
        monkeypatch.delenv("POLAR_FIELD_AT_CHUNK")
        perm = rng.permutation(m)
        shuffled = p.field_at(pts[perm], skip[perm], pmol[perm])
        nophi = p.field_at(pts, skip, pmol, potential=False)
        assert nophi["phi_static"] is None and nophi["phi_induced"] is None
        for k in NAMES:
            assert np.array_equal(one[k], again[k]), (m, k, "second call")
            assert np.array_equal(one[k], chunked[k]), (m, k, "passes of 37")
            assert np.array_equal(one[k][perm], shuffled[k]), (m, k, "permuted")
            if k.startswith("e_"):
                assert np.array_equal(one[k], nophi[k]), (m, k, "field only")
        if m:
            assert np.all(np.isfinite(one["e_static"])) and np.max(np.abs(one["e_induced"])) > 0.0


@pytest.mark.parametrize("case,tilt", [("mini", None), ("mini", TILT), ("lattice200", None)])
def test_points_outside_a_periodic_box_wrap(case, tilt, wl, pkg):
    s, p, out = _solved(wl, pkg, case, "list", tilt)
    pts, skip, pmol = _points(s, seed=9)
    rng = np.random.default_rng(23)
    shift = rng.integers(-2, 3, (NPTS, 3)).astype(np.float64) @ ptr.cell_matrix(s.prd, _tilt(s)).T
    a, b = p.field_at(pts, skip, pmol), p.field_at(pts + shift, skip, pmol)
    ref = _reference(s, out, pts, skip, pmol)
    for k in NAMES:
        assert np.all(np.abs(a[k] - b[k]) <= 1e-12 * ref[k][1]), k


@pytest.mark.parametrize("damp", ["exponential", "none"])
def test_a_point_a_million_box_lengths_out_in_exact_mode(damp, wl, pkg):
    """Exact mode's image rule is closest_image's add / subtract loop, whose trip count grows with the distance: the kernel takes
    whole lattice vectors off a point first, in closed form.  Points on a 2^-20 A raster, moved by 2^20 box lengths of the 20 A
    box along every axis, are exact FP64 numbers and wrap back exactly: the same bits as the points themselves.  Beyond 2^30 box
    lengths, where a coordinate no longer says where in the box the point is, the call is refused."""
    s, p, out = _solved(wl, pkg, "mini", "exact", None, damp)
    rng = np.random.default_rng(41)
    pts = np.round(rng.uniform(0, 20.0, (64, 3)) * 2.0 ** 20) / 2.0 ** 20
    far = pts + rng.choice([-1.0, 1.0], (64, 3)) * (2.0 ** 20 * 20.0)
    assert np.array_equal(far - np.round((far - pts) / 20.0) * 20.0, pts)       # nothing was rounded on the way out
    near, got = p.field_at(pts), p.field_at(far)
    for k in NAMES:
        assert np.all(np.isfinite(got[k])) and np.array_equal(got[k], near[k]), k
    assert np.max(np.abs(near["e_induced"])) > 0.0
    for bad in (2.0 ** 31 * 20.0, -1e20, 1e300):
        x = pts[:3].copy()
        x[1, 2] = bad
        assert _code(pkg, lambda: p.field_at(x)) == ERR_INPUT
    assert np.array_equal(p.field_at(pts)["e_static"], near["e_static"])


@pytest.mark.parametrize("case,mode,tilt", [("mini", "exact", TILT), ("mini", "list", None), ("mof5_h2", "exact", None)])
def test_far_points_agree_with_their_wrapped_images(case, mode, tilt, wl, pkg):
    """The same in a tilted cell, in list mode and in the 25.669 A cell, where the far point is a rounded number: it carries an
    error of half an ulp of 1e6 box lengths (4e-9 A at most) per axis, a pair at distance r moves by 3 * that / r of its term,
    and the points are kept 1 A from every atom: 1e-7 of scale bounds it with a decade to spare."""
    s, p, out = _solved(wl, pkg, case, mode, tilt)
    n = s.nlocal
    H = ptr.cell_matrix(s.prd, _tilt(s))
    rng = np.random.default_rng(43)
    pts = np.asarray(s.boxlo) + rng.uniform(0, 1, (400, 3)) @ H.T
    dmin = np.array([np.sqrt(np.min(np.sum(ptr.images(q - s.x[:n], s.prd, _tilt(s)) ** 2, axis=1))) for q in pts])
    pts = np.ascontiguousarray(pts[dmin >= 1.0][:64])
    assert len(pts) == 64
    far = pts + (rng.choice([-1.0, 1.0], (64, 3)) * 1.0e6) @ H.T
    near, got = p.field_at(pts), p.field_at(far)
    ref = _reference(s, out, pts, None, None)
    for k in NAMES:
        assert np.all(np.abs(got[k] - near[k]) <= 1e-7 * ref[k][1]), k


def test_a_call_leaves_the_handle_as_it_was(wl, pkg):
    """`deterministic yes`, `use_previous no`, one handle: compute, compute, field_at, compute.  Repeated computes of such a
    handle agree bit for bit in the forces, the dipoles and the static field (tests/test_gpu_polar_ewald.py::
    test_deterministic_runs_are_bit_identical); the compute after the probe must be one more of them.  The energies and the virial
    are folded from per-wave atomic adds whose order varies from run to run with or without a probe in between: equal to
    rounding (1e-13, the figure of that test), and the solve takes the same number of sweeps."""
    s, _ = wl.load_fixture(os.path.join(GOLD, "mof5_h2.npz"), extra_args=["use_previous", "no", "dd_cutoff", "9.0", "deterministic", "yes"])
    p = pkg.pair_from_system(s)
    try:
        a, b = p.compute(eflag=1, vflag=2), p.compute(eflag=1, vflag=2)
        pts, skip, pmol = _points(s)
        first = p.field_at(pts, skip, pmol)
        c = p.compute(eflag=1, vflag=2)
        second = p.field_at(pts, skip, pmol)
    finally:
        p.close()
    for x, y in ((a, b), (b, c)):
        for k in ("f", "mu", "ef_static"):
            assert np.array_equal(x[k], y[k]), k
        for k in ("iterations", "sweeps", "status", "dd_pairs"):
            assert x[k] == y[k], k
        assert np.max(np.abs(x["virial"] - y["virial"])) <= 1e-13 * np.max(np.abs(x["virial"]))
        for k in ("eng_vdwl", "eng_coul", "eng_pol", "u_self", "u_ef", "u_dd"):
            assert abs(x[k] - y[k]) <= 1e-13 * abs(x[k]), k
    for k in NAMES:   # and the probe of the same dipoles gives the same bits
        assert np.array_equal(first[k], second[k]), k


def _code(pkg, fn):
    with pytest.raises(pkg.PolarError) as e:
        fn()
    return e.value.code


def _handle(wl, pkg, **kw):
    s = _mini(wl, **kw)
    return s, pkg.pair_from_system(s)


def _works(s, p):
    out = p.compute(eflag=1, vflag=2)
    got = p.field_at(s.x[:5], np.arange(5, dtype=np.int32), s.molecule[:5])
    assert np.max(np.abs(got["e_static"] - out["ef_static"][:5])) <= 1e-10 * np.max(np.abs(out["ef_static"]))


def test_call_window_before_any_compute(wl, pkg):
    s, p = _handle(wl, pkg)
    assert _code(pkg, lambda: p.field_at(s.x[:3])) == ERR_STATE
    _works(s, p)
    p.close()


def test_call_window_after_set_positions(wl, pkg):
    s, p = _handle(wl, pkg)
    p.compute()
    p.field_at(s.x[:3])
    p.set_positions(s.x)
    assert _code(pkg, lambda: p.field_at(s.x[:3])) == ERR_STATE
    _works(s, p)
    p.close()


def test_call_window_after_set_box(wl, pkg):
    s, p = _handle(wl, pkg)
    p.compute()
    p.set_box(s.boxlo, s.prd)
    assert _code(pkg, lambda: p.field_at(s.x[:3])) == ERR_STATE
    _works(s, p)
    p.close()


def test_polar_ewald_is_refused(wl, pkg):
    s, p = _handle(wl, pkg, extra=["polar_ewald", "1e-6"])
    p.compute()
    assert _code(pkg, lambda: p.field_at(s.x[:3])) == ERR_UNSUPPORTED
    p.compute()
    p.close()


def test_a_row_sharded_handle_is_refused(wl, pkg):
    s = _mini(wl, extra=["dd_cutoff", "9.0"])
    p = pkg.pair_from_system(s, row_range=(0, 30))
    assert _code(pkg, lambda: p.field_at(s.x[:3])) == ERR_UNSUPPORTED
    p._ck(p.L.polar_set_row_range(p.h, 0, -1))
    _works(s, p)
    p.close()


def test_a_nan_coordinate_is_refused(wl, pkg):
    s, p = _handle(wl, pkg)
    p.compute()
    x = s.x[:4].copy()
    x[2, 1] = np.nan
    assert _code(pkg, lambda: p.field_at(x)) == ERR_INPUT
    _works(s, p)
    p.close()


def test_a_skip_atom_past_the_end_is_refused(wl, pkg):
    s, p = _handle(wl, pkg)
    p.compute()
    assert _code(pkg, lambda: p.field_at(s.x[:2], np.array([0, s.nlocal], np.int32))) == ERR_INPUT
    assert _code(pkg, lambda: p.field_at(s.x[:2], np.array([-2, 0], np.int32))) == ERR_INPUT
    _works(s, p)
    p.close()


@pytest.mark.parametrize("tilt", [None, TILT])
def test_field_grid_shapes_and_numbers(tilt, wl, pkg):
    s, p, out = _solved(wl, pkg, "mini", "list", tilt)
    g = p.field_grid((5, 4, 3))
    assert g["e_static"].shape == g["e_induced"].shape == (3, 4, 5, 3) and g["phi_static"].shape == g["phi_induced"].shape == (3, 4, 5)
    H, lo = ptr.cell_matrix(s.prd, _tilt(s)), np.asarray(s.boxlo, np.float64)
    pts = np.array([lo + H @ np.array([(i + 0.5) / 5, (j + 0.5) / 4, (k + 0.5) / 3]) for k in range(3) for j in range(4) for i in range(5)])
    assert np.allclose(p.grid_points((5, 4, 3)), pts, rtol=0, atol=1e-12)
    flat = p.field_at(p.grid_points((5, 4, 3)))
    for k in NAMES:
        assert np.array_equal(g[k].reshape(flat[k].shape), flat[k]), k
    assert np.array_equal(g["phi_static"][2, 1, 3], flat["phi_static"][(2 * 4 + 1) * 5 + 3])
