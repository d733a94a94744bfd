"""polar_ewald_field_grad_grid on the MI355X: the Ewald field of the polarized box and its gradient on a regular grid of the cell,
the reciprocal sums as three 1-D transforms with nine coefficient sets (PolarPair.ewald_field_grad_grid(..., recip="grid")), and
the two maps composed of the grid paths, PolarPair.ewald_probe_grid and PolarPair.ewald_probe_force_grid.

Systems, restated from tests/test_gpu_ewald_field_grid.py: `mini` (60 atoms, seed 620, L = 20 A, cut_coul 9, precision 1e-13,
`polar_ewald 1e-6` at g = 0.32: 919 k-vectors) in list mode in the cubic box and in exact mode in the tilted one, `charged` (the
tilted mini with every charge raised by 0.05, accuracy 1e-12 at g = 0.6: 16,926 k-vectors in 631 rows, Q = 3 e) in list mode,
and `mof5_h2` (tests/golden) in list mode with dd_cutoff 12.8345.  One solve per case for the module.
Grids: (8, 6, 4), (5, 7, 3), (67, 3, 2) -- a line of x longer than a wave --, (1, 1, 1) and (3, 1, 130) -- a second block of z --;
offsets (.5, .5, .5) and (0, 0.25, 0.9).  With passes of 37 points these reach every seam: more than one 64-lane block per axis,
an h loop deeper than the unroll (h_max is 3 and more), passes and runs of lines cut mid-line.

Exact (np.array_equal): x against polar_ewald_field_grid's x; e_induced and g_induced against polar_ewald_field_grad_at at x (the
same kernel on the same points); e_static against polar_ewald_field_grid's e_static asked without its potentials; every output
after a second call, with passes of 37 points, and the gradients with field=False.
Tolerance: g_static against polar_ewald_field_grad_at at x, and every output against the NumPy references
(tests/ewald_point_grad_numpy.py::field_grad_numpy, tests/ewald_point_numpy.py::field_at_numpy) at x: the largest
|got - ref| over points and components within 1e-10 of the largest |component of ref| -- the project's figure for whole-sum
comparisons against NumPy, which tests/test_gpu_ewald_field_grad_at.py and tests/test_gpu_ewald_field_grid.py assert; the
per-point path sits at 1e-15 to 7e-14 against that reference.  The compositions: e_lj and f_lj bit for bit
against probe_at at x, the other parts within 1e-10 of their maxima against probe_at / ewald_probe_force_at at x."""
import copy
import os

import numpy as np
import pytest

import ewald_point_grad_numpy as egn
import ewald_point_numpy as epn
import point_ref as ptr
from helpers import GOLD

pytestmark = pytest.mark.gpu
TILT = (2.1, -1.4, 1.2)
ERR_INPUT, ERR_UNSUPPORTED, ERR_STATE = -1, -4, -5
NAMES = ("g_static", "g_induced", "e_static", "e_induced")
CASES = [("mini", "list", None), ("mini", "exact", TILT), ("charged", "list", TILT), ("mof5_h2", "list", None)]
CASE_IDS = ["mini_list_cubic", "mini_exact_tilted", "charged_list_tilted", "mof5_h2_list"]
GRIDS = [(8, 6, 4), (5, 7, 3), (67, 3, 2), (1, 1, 1), (3, 1, 130)]
OFFSETS = [(0.5, 0.5, 0.5), (0.0, 0.25, 0.9)]


def _mini(wl, extra=(), tilt=None, damp="exponential", g=0.32, acc="1e-6", shift=0.0, n=60, seed=620, L=20.0):
    """the recipe of tests/test_gpu_ewald_field_grid.py::_mini: 60 atoms, the polar_ewald keyword (acc None: without),
    g_ewald = g, every charge raised by `shift`"""
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


def _system(wl, case, mode, tilt):
    lst = ["dd_cutoff", "9.0"] if mode == "list" else []
    if case == "mini":
        return _mini(wl, extra=lst, tilt=tilt), 1e-6
    if case == "charged":
        return _mini(wl, extra=lst, tilt=tilt, g=0.6, acc="1e-12", shift=0.05), 1e-12
    extra = ["precision", "1e-13", "max_iterations", "200", "use_previous", "no", "polar_ewald", "1e-6"] + (["dd_cutoff", "12.8345"] if mode == "list" else [])
    return wl.load_fixture(os.path.join(GOLD, case + ".npz"), extra_args=extra)[0], 1e-6


def _tilt(s):
    return tuple(s.tilt) if getattr(s, "triclinic", 0) else None


_CACHE, _GRID = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _close_cached_handles():
    yield
    for v in _CACHE.values():
        v[1].close()
    _CACHE.clear()
    _GRID.clear()


def _solved(wl, pkg, case, mode, tilt):
    """(system, handle after one compute, its outputs, accuracy): one solve per case for the whole module"""
    key = (case, mode, tilt)
    if key not in _CACHE:
        s, acc = _system(wl, case, mode, tilt)
        p = pkg.pair_from_system(s)
        out = p.compute(eflag=1, vflag=2)
        assert out["status"] == 0 and out["rms_dmu"] <= 1e-13 and out["nkvec"] > 0
        _CACHE[key] = (s, p, out, acc)
    return _CACHE[key]


def _grid(wl, pkg, case, mode, tilt, shape, offset):
    """the grid call of a (case, grid, offset), once for the tests that look at it"""
    key = (case, mode, tilt, shape, offset)
    if key not in _GRID:
        s, p, out, acc = _solved(wl, pkg, case, mode, tilt)
        _GRID[key] = p.ewald_field_grad_grid(shape, recip="grid", offset=offset)
    return _GRID[key]


def _flat(got, k):
    return got[k].reshape(-1, got[k].shape[-1])


def _worst(got, ref):
    """max over the components of max_p |got - ref|, of the largest |component of ref| over the points"""
    return float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))


@pytest.mark.parametrize("offset", OFFSETS, ids=["centred", "offset"])
@pytest.mark.parametrize("shape", GRIDS, ids=lambda v: "x".join(str(n) for n in v))
@pytest.mark.parametrize("case,mode,tilt", CASES, ids=CASE_IDS)
def test_every_output_against_the_numpy_reference_at_the_librarys_points(case, mode, tilt, shape, offset, wl, pkg):
    s, p, out, acc = _solved(wl, pkg, case, mode, tilt)
    if case == "charged":
        assert abs(s.q[:s.nlocal].sum() - 3.0) < 1e-9 and 15000 <= out["nkvec"] <= 19000
    got = _grid(wl, pkg, case, mode, tilt, shape, offset)
    nx, ny, nz = shape
    m = nx * ny * nz
    assert got["x"].shape == got["e_static"].shape == got["e_induced"].shape == (nz, ny, nx, 3)
    assert got["g_static"].shape == got["g_induced"].shape == (nz, ny, nx, 6)
    x = np.ascontiguousarray(_flat(got, "x"))
    n, st = s.nlocal, s.settings
    args = (s.x[:n], s.q[:n], s.alpha[:n], s.molecule[:n], out["mu"], s.prd, _tilt(s), st.cut_coul, st.dd_cutoff if st.dd_cutoff > 0 else None,
            st.polar_damp, st.damping_type, np.sqrt(s.qqrd2e), s.g_ewald, acc)
    gref = egn.field_grad_numpy(x, None, None, *args)
    fref = epn.field_at_numpy(x, np.full(m, -1), np.zeros(m, int), *args)
    ref = dict(g_static=gref["g_static"][0], g_induced=gref["g_induced"][0], e_static=fref["e_static"], e_induced=fref["e_induced"])
    worst = {k: _worst(_flat(got, k), ref[k]) for k in NAMES}
    print(case, mode, tilt, shape, offset, "nkvec %d  max |got - ref| / max |ref|:" % out["nkvec"], "  ".join("%s %.2e" % kv for kv in worst.items()),
          " ms real %.3f recip %.3f" % (got["ms_real"], got["ms_recip"]))
    for k in NAMES:
        assert worst[k] <= 1e-10, (k, worst[k])
    assert abs(got["ms"] - got["ms_real"] - got["ms_recip"]) <= 1e-9 * got["ms"] and got["ms_real"] > 0.0 and got["ms_recip"] > 0.0


@pytest.mark.parametrize("offset", OFFSETS, ids=["centred", "offset"])
@pytest.mark.parametrize("shape", GRIDS, ids=lambda v: "x".join(str(n) for n in v))
@pytest.mark.parametrize("case,mode,tilt", CASES, ids=CASE_IDS)
def test_against_the_per_point_call_and_ewald_field_grid(case, mode, tilt, shape, offset, wl, pkg):
    s, p, out, acc = _solved(wl, pkg, case, mode, tilt)
    got = _grid(wl, pkg, case, mode, tilt, shape, offset)
    fg = p.ewald_field_grid(shape, recip="grid", offset=offset, potential=False)
    assert np.array_equal(got["x"], fg["x"])
    assert np.array_equal(got["e_static"], fg["e_static"]) and np.array_equal(got["e_induced"], fg["e_induced"])
    x = np.ascontiguousarray(_flat(got, "x"))
    flat = p.ewald_field_grad_at(x)
    for k in ("e_induced", "g_induced"):
        assert np.array_equal(_flat(got, k), flat[k]), k
    worst = {k: _worst(_flat(got, k), flat[k]) for k in ("g_static", "e_static")}
    print(case, mode, tilt, shape, offset, "grid against points, of the maximum:", "  ".join("%s %.2e" % kv for kv in worst.items()))
    for k, w in worst.items():
        assert w <= 1e-10, (k, w)


@pytest.mark.parametrize("shape", GRIDS, ids=lambda v: "x".join(str(n) for n in v))
@pytest.mark.parametrize("case,mode,tilt", [CASES[0], CASES[2]], ids=["mini_list_cubic", "charged_list_tilted"])
def test_calls_passes_and_the_field_switch_do_not_change_a_bit(case, mode, tilt, shape, wl, pkg, monkeypatch):
    s, p, out, acc = _solved(wl, pkg, case, mode, tilt)
    offset = (0.0, 0.25, 0.9)
    monkeypatch.delenv("POLAR_FIELD_AT_CHUNK", raising=False)
    one = p.ewald_field_grad_grid(shape, recip="grid", offset=offset)
    again = p.ewald_field_grad_grid(shape, recip="grid", offset=offset)
    monkeypatch.setenv("POLAR_FIELD_AT_CHUNK", "37")     # passes of 37 points end inside a line: their runs of lines start and end mid-line
    chunked = p.ewald_field_grad_grid(shape, recip="grid", offset=offset)
    monkeypatch.delenv("POLAR_FIELD_AT_CHUNK")
    nofield = p.ewald_field_grad_grid(shape, recip="grid", offset=offset, field=False)
    assert nofield["e_static"] is None and nofield["e_induced"] is None
    for k in NAMES + ("x",):
        assert np.array_equal(one[k], again[k]), (k, "second call")
        assert np.array_equal(one[k], chunked[k]), (k, "passes of 37")
        if k.startswith("g_") or k == "x":
            assert np.array_equal(one[k], nofield[k]), (k, "field=False")
    assert np.all(np.isfinite(one["g_static"])) and np.max(np.abs(one["g_induced"])) > 0.0


def test_a_call_leaves_the_handle_as_it_was(wl, pkg):
    """`deterministic yes`, `use_previous no`, one handle: compute, compute, grid call, compute.  The compute after the call is
    one more of the bit-identical computes before it, and a second grid call of the same dipoles gives the same bits."""
    s, _ = wl.load_fixture(os.path.join(GOLD, "mof5_h2.npz"), extra_args=["use_previous", "no", "dd_cutoff", "9.0", "deterministic", "yes", "polar_ewald", "1e-6"])
    p = pkg.pair_from_system(s)
    try:
        a, b = p.compute(eflag=1, vflag=2), p.compute(eflag=1, vflag=2)
        first = p.ewald_field_grad_grid((8, 6, 4), recip="grid")
        c = p.compute(eflag=1, vflag=2)
        second = p.ewald_field_grad_grid((8, 6, 4), recip="grid")
    finally:
        p.close()
    for x, y in ((a, b), (b, c)):
        for k in ("f", "mu", "ef_static"):
            assert np.array_equal(x[k], y[k]), k
        for k in ("iterations", "sweeps", "status", "dd_pairs", "nkvec"):
            assert x[k] == y[k], k
        assert x["u_ef"] == y["u_ef"]
    for k in NAMES + ("x",):
        assert np.array_equal(first[k], second[k]), k


def _code(pkg, fn):
    with pytest.raises(pkg.PolarError) as e:
        fn()
    return e.value.code


def _works(s, p):
    out = p.compute(eflag=1, vflag=2)
    got = p.ewald_field_grad_grid((3, 2, 2), recip="grid")
    flat = p.ewald_field_grad_at(got["x"].reshape(-1, 3))
    assert out["status"] == 0 and _worst(got["g_static"].reshape(-1, 6), flat["g_static"]) <= 1e-10


def test_keyword_off_is_refused_and_points_to_field_grad_at(wl, pkg):
    s = _mini(wl, acc=None)
    p = pkg.pair_from_system(s)
    p.compute()
    with pytest.raises(pkg.PolarError) as e:
        p.ewald_field_grad_grid((4, 4, 4), recip="grid")
    assert e.value.code == ERR_UNSUPPORTED and "polar_field_grad_at" in str(e.value)
    p.field_grad_grid((4, 4, 4))
    assert p.compute()["status"] == 0
    p.close()


def test_call_window_before_any_compute_and_after_set_positions(wl, pkg):
    s = _mini(wl)
    p = pkg.pair_from_system(s)
    assert _code(pkg, lambda: p.ewald_field_grad_grid((4, 4, 4), recip="grid")) == ERR_STATE
    _works(s, p)
    p.set_positions(s.x)
    assert _code(pkg, lambda: p.ewald_field_grad_grid((4, 4, 4), recip="grid")) == ERR_STATE
    _works(s, p)
    p.close()


def test_a_row_sharded_handle_is_refused(wl, pkg):
    s = _mini(wl, extra=["dd_cutoff", "9.0"])
    p = pkg.pair_from_system(s, row_range=(0, 30))
    assert _code(pkg, lambda: p.ewald_field_grad_grid((4, 4, 4), recip="grid")) == ERR_UNSUPPORTED
    p._ck(p.L.polar_set_row_range(p.h, 0, -1))
    _works(s, p)
    p.close()


def test_bad_counts_and_offsets_are_refused(wl, pkg):
    s, p, out, acc = _solved(wl, pkg, "mini", "list", None)
    for shape in ((0, 4, 4), (4, -1, 4), (4, 4, 0), (2048, 1024, 1024), (65536, 65536, 1)):
        assert _code(pkg, lambda: p.ewald_field_grad_grid(shape, recip="grid")) == ERR_INPUT, shape
    for offset in ((1.0, 0.5, 0.5), (0.5, -0.25, 0.5), (0.5, 0.5, float("nan")), (float("inf"), 0.5, 0.5)):
        assert _code(pkg, lambda: p.ewald_field_grad_grid((4, 4, 4), recip="grid", offset=offset)) == ERR_INPUT, offset
    with pytest.raises(ValueError):
        p.ewald_field_grad_grid((4, 4, 4), recip="mesh")
    p.ewald_field_grad_grid((4, 4, 4), recip="grid")       # (and the handle still answers)


@pytest.mark.parametrize("tilt", [None, TILT])
def test_the_default_path_is_still_the_flat_call(tilt, wl, pkg):
    s, p, out, acc = _solved(wl, pkg, "mini", "list" if tilt is None else "exact", tilt)
    g = p.ewald_field_grad_grid((8, 6, 4))
    assert "x" not in g and g["g_static"].shape == (4, 6, 8, 6) and g["e_static"].shape == (4, 6, 8, 3)
    flat = p.ewald_field_grad_at(p.grid_points((8, 6, 4)))
    for k in NAMES:
        assert np.array_equal(g[k].reshape(flat[k].shape), flat[k]), k
    moved = p.ewald_field_grad_grid((8, 6, 4), offset=(0.0, 0.25, 0.9), recip="points")
    flat = p.ewald_field_grad_at(p.grid_points((8, 6, 4), (0.0, 0.25, 0.9)))
    for k in NAMES:
        assert np.array_equal(moved[k].reshape(flat[k].shape), flat[k]), k


@pytest.mark.parametrize("case,mode,tilt", [CASES[0], CASES[2]], ids=["mini_list_cubic", "charged_list_tilted"])
def test_the_probe_energy_and_force_maps_of_the_grid_paths(case, mode, tilt, wl, pkg):
    s, p, out, acc = _solved(wl, pkg, case, mode, tilt)
    shape, offset = (5, 7, 3), (0.0, 0.25, 0.9)
    typ, q, al = 2, 0.35, 0.9
    en = p.ewald_probe_grid(shape, typ, q, al, offset=offset)
    fo = p.ewald_probe_force_grid(shape, typ, q, al, offset=offset)
    assert en["x"].shape == fo["x"].shape == (3, 7, 5, 3) and np.array_equal(en["x"], fo["x"])
    assert en["energy"].shape == en["e_lj"].shape == (3, 7, 5) and fo["force"].shape == fo["f_pol"].shape == (3, 7, 5, 3)
    x = np.ascontiguousarray(en["x"].reshape(-1, 3))
    pa = p.probe_at(x, typ, q, al, force=True)
    pf = p.ewald_probe_force_at(x, typ, q, al)
    assert np.array_equal(en["e_lj"].reshape(-1), pa["e_lj"]) and np.array_equal(fo["f_lj"].reshape(-1, 3), pa["f_lj"])
    assert np.array_equal(fo["f_lj"].reshape(-1, 3), pf["f_lj"]) and np.max(np.abs(pa["e_lj"])) > 0 and np.max(np.abs(pa["f_lj"])) > 0
    worst = {k: _worst(en[k].reshape(-1), pa[k]) for k in ("e_coul", "e_pol", "energy")}
    worst.update({k: _worst(fo[k].reshape(-1, 3), pf[k]) for k in ("f_coul", "f_pol", "force")})
    print(case, mode, "maps against the per-point calls, of the maximum:", "  ".join("%s %.2e" % kv for kv in worst.items()))
    for k, w in worst.items():
        assert w <= 1e-10, (k, w)
    assert np.max(np.abs(pa["e_coul"])) > 0 and np.max(np.abs(pa["e_pol"])) > 0 and np.max(np.abs(pf["f_pol"])) > 0
