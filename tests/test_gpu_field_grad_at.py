"""polar_field_grad_at and polar_probe_force_at on the MI355X: the gradient of the field at points and the full force on a test
site.

Systems and points are those of tests/probe_systems.py (`mini` exact / list / tilted, both damping types; `lattice_lj`; `mof5_h2`
in list mode), 257 points per case: in the box, up to two box lengths out, 0.3 A from an atom, on atoms with that atom skipped;
half of them with a molecule id.

Tolerances.  Every component of g_static and g_induced against the NumPy brute force (tests/point_grad_ref.py): 1e-10 of its scale,
the project's figure for whole-point sums against NumPy (a dropped or doubled in-cutoff pair is >= 1e-4).  The field outputs, f_coul
and f_lj are checked bit for bit against the handle's own calls; f_pol against the NumPy expression of the call's own outputs
within 8 eps of the sum of the absolute terms (three products and two adds per component, one more product by alpha; NumPy has no
fma, the library fuses two of them: each of the at most six roundings is below one eps of that sum).  The force against central
differences of probe_at's energy: ten times the mismatch the NumPy reference shows against central differences of the NumPy energy
at the same points and step.  Measured worst cases per case: DESIGN section 6h."""
import numpy as np
import pytest

import point_grad_ref as pgr
import point_ref as ptr
import probe_ref as prb
import probe_systems as ps

pytestmark = pytest.mark.gpu
TILT = ps.TILT
NPTS = ps.NPTS
EPS = 2.0 ** -52
ERR_INPUT, ERR_UNSUPPORTED, ERR_STATE = -1, -4, -5
GKEYS = ("g_static", "g_induced")

_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _close_cached_handles():
    yield
    for v in _CACHE.values():
        v[1].close()
    _CACHE.clear()


def _system(wl, case, mode, tilt, damp):
    if case == "mini":
        extra = (["dd_cutoff", "9.0"] if mode == "list" else []) + (["damp_type", "none"] if damp == "none" else [])
        s = ps.mini(wl, extra=extra, tilt=tilt)
        assert s.settings.damping_type == (1 if damp == "none" else 0)
        return s
    return ps.system(wl, case, mode, tilt)


def _solved(wl, pkg, case, mode="list", tilt=None, damp="exponential"):
    """(system, handle after one compute, its outputs, points): one solve per case for the whole module"""
    key = (case, mode, tilt, damp)
    if key not in _CACHE:
        s = _system(wl, case, mode, tilt, damp)
        p = pkg.pair_from_system(s)
        out = p.compute(eflag=1, vflag=2)
        assert out["status"] == 0
        _CACHE[key] = (s, p, out, ps.draw_points(s, 3))
    return _CACHE[key]


def _ref_args(s, out):
    n, st = s.nlocal, s.settings
    return (s.x[:n], s.q[:n], s.alpha[:n], s.molecule[:n], out["mu"], s.prd, ps.tilt_of(s), st.cut_coul,
            st.dd_cutoff if st.dd_cutoff > 0 else None, st.polar_damp, st.damping_type, np.sqrt(s.qqrd2e))


CASES = [("mini", "exact", None, "exponential"), ("mini", "exact", None, "none"), ("mini", "list", None, "exponential"),
         ("mini", "list", None, "none"), ("mini", "exact", TILT, "exponential"), ("mini", "exact", TILT, "none"),
         ("mini", "list", TILT, "exponential"), ("mini", "list", TILT, "none"), ("lattice_lj", "list", None, "exponential"),
         ("mof5_h2", "list", None, "exponential")]


@pytest.mark.parametrize("case,mode,tilt,damp", CASES)
def test_both_gradients_against_the_numpy_brute_force(case, mode, tilt, damp, wl, pkg):
    s, p, out, pt = _solved(wl, pkg, case, mode, tilt, damp)
    got = p.field_grad_at(pt["x"], pt["skip"], pt["mol"])
    ref = pgr.field_grad_numpy(pt["x"], pt["skip"], pt["mol"], *_ref_args(s, out))
    worst = {}
    for k in GKEYS:
        v, sc = ref[k]
        assert np.max(sc) > 0.0 and got[k].shape == (NPTS, 6)
        err = np.abs(got[k] - v)
        worst[k] = float(np.max(np.where(sc > 0, err / np.where(sc > 0, sc, 1.0), np.where(err > 0, np.inf, 0.0))))
    print(case, mode, tilt, damp, "max |got - ref| / scale:", "  ".join("%s %.2e" % kv for kv in worst.items()), " ms %.3f" % got["ms"])
    for k in GKEYS:
        v, sc = ref[k]
        assert np.all(np.abs(got[k] - v) <= 1e-10 * sc), (k, worst[k])          # no point is left out
    if damp == "none":   # the undamped induced gradient is traceless
        tr = got["g_induced"][:, 0] + got["g_induced"][:, 1] + got["g_induced"][:, 2]
        assert np.all(np.abs(tr) <= 1e-10 * ref["g_induced"][1][:, :3].sum(axis=1))


@pytest.mark.parametrize("case,mode,tilt,damp", [("mini", "exact", None, "exponential"), ("mini", "exact", None, "none"),
                                                 ("mini", "list", None, "exponential"), ("mini", "list", None, "none"),
                                                 ("mini", "list", TILT, "exponential"), ("lattice_lj", "list", None, "exponential")])
def test_fields_forces_passes_and_order_bit_for_bit(case, mode, tilt, damp, wl, pkg, monkeypatch):
    s, p, out, pt = _solved(wl, pkg, case, mode, tilt, damp)
    monkeypatch.delenv("POLAR_FIELD_AT_CHUNK", raising=False)
    one = p.field_grad_at(pt["x"], pt["skip"], pt["mol"])
    fa = p.field_at(pt["x"], pt["skip"], pt["mol"])
    # the field outputs are field_at's, bit for bit
    assert np.array_equal(one["e_static"], fa["e_static"]) and np.array_equal(one["e_induced"], fa["e_induced"])
    assert np.max(np.abs(fa["e_static"])) > 0 and np.max(np.abs(fa["e_induced"])) > 0
    # passes, order, a second call, field=False: no bit of any gradient component changes
    again = p.field_grad_at(pt["x"], pt["skip"], pt["mol"])
    monkeypatch.setenv("POLAR_FIELD_AT_CHUNK", "37")
    chunked = p.field_grad_at(pt["x"], pt["skip"], pt["mol"])
    monkeypatch.delenv("POLAR_FIELD_AT_CHUNK")
    perm = np.random.default_rng(17).permutation(NPTS)
    shuffled = p.field_grad_at(pt["x"][perm], pt["skip"][perm], pt["mol"][perm])
    nofield = p.field_grad_at(pt["x"], pt["skip"], pt["mol"], field=False)
    assert nofield["e_static"] is None and nofield["e_induced"] is None
    for k in GKEYS:
        assert np.array_equal(one[k], again[k]), (k, "second call")
        assert np.array_equal(one[k], chunked[k]), (k, "passes of 37")
        assert np.array_equal(one[k][perm], shuffled[k]), (k, "permuted")
        assert np.array_equal(one[k], nofield[k]), (k, "field=False")
    # the forces on a site
    pf = p.probe_force_at(pt["x"], pt["type"], pt["q"], pt["alpha"], pt["skip"], pt["mol"])
    e2s = np.sqrt(s.qqrd2e)
    et = fa["e_static"] + fa["e_induced"]
    assert np.array_equal(pf["f_coul"], (pt["q"] * e2s)[:, None] * et)
    pa = p.probe_at(pt["x"], pt["type"], pt["q"], pt["alpha"], pt["skip"], pt["mol"], force=True)
    assert np.array_equal(pf["f_lj"], pa["f_lj"]) and np.max(np.abs(pf["f_lj"])) > 0
    assert np.array_equal(pf["force"], pf["f_lj"] + pf["f_coul"] + pf["f_pol"])
    G = one["g_static"] + one["g_induced"]
    full = np.stack([G[:, [0, 3, 4]], G[:, [3, 1, 5]], G[:, [4, 5, 2]]], axis=1)           # [m, a, b]
    want = pt["alpha"][:, None] * np.einsum("ma,mab->mb", et, full)
    mag = pt["alpha"][:, None] * np.einsum("ma,mab->mb", np.abs(et), np.abs(full))
    assert np.all(np.abs(pf["f_pol"] - want) <= 8 * EPS * mag)
    assert np.max(np.abs(pf["f_pol"])) > 0 and np.all(pf["f_pol"][pt["alpha"] == 0] == 0)
    monkeypatch.setenv("POLAR_FIELD_AT_CHUNK", "37")
    pf2 = p.probe_force_at(pt["x"][perm], pt["type"][perm], pt["q"][perm], pt["alpha"][perm], pt["skip"][perm], pt["mol"][perm])
    monkeypatch.delenv("POLAR_FIELD_AT_CHUNK")
    for k in ("f_lj", "f_coul", "f_pol"):
        assert np.array_equal(pf[k][perm], pf2[k]), k


H = 1e-4


def _clear_points(wl, s, mode, want=64, seed=41):
    """Of 64 drawn points, those at least 1.5 A from every atom and further than 10 h from every cut_coul, dd_cutoff and per-pair LJ
    cutoff shell (all 27 images) and, in exact mode, from every half-box image flip."""
    rng = np.random.default_rng(seed)
    n, st = s.nlocal, s.settings
    prd = np.asarray(s.prd, np.float64)
    tb = ps.tables_of(wl, s, False)
    cuts = [st.cut_coul] + ([st.dd_cutoff] if st.dd_cutoff > 0 else [])
    ljc = np.sqrt(np.asarray(tb["cut_ljsq"], np.float64))
    pts, types = rng.uniform(0, prd[0], (want, 3)), rng.integers(1, s.ntypes + 1, want).astype(np.int32)
    keep = []
    for k in range(want):
        raw = pts[k] - s.x[:n]
        d0 = raw - prd * np.round(raw / prd)
        sh = np.array([(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)], np.float64) * prd
        r = np.sqrt(np.sum((d0[:, None, :] + sh[None, :, :]) ** 2, axis=2))             # [n, 27]
        ok = np.min(r) >= 1.5 and all(np.min(np.abs(r - c)) > 10 * H for c in cuts)
        ok = ok and np.min(np.abs(r - ljc[types[k], s.type[:n]][:, None])) > 10 * H
        if mode == "exact":
            ok = ok and np.min(np.abs(np.abs(d0) - 0.5 * prd)) > 10 * H
        if ok:
            keep.append(k)
    return pts[keep], types[keep]


def _numpy_energy_and_force(wl, s, out, x, typ, q, al):
    tb = ps.tables_of(wl, s, False)
    n = s.nlocal
    args = _ref_args(s, out)
    fa = ptr.field_at_numpy(x, None, None, *args)
    lj = prb.probe_lj_numpy(x, typ, None, None, s.x[:n], s.type[:n], s.molecule[:n], tb, s.prd, ps.tilt_of(s))
    et = fa["e_static"][0] + fa["e_induced"][0]
    energy = lj["e_lj"] + q * np.sqrt(s.qqrd2e) * (fa["phi_static"][0] + fa["phi_induced"][0]) - 0.5 * al * np.sum(et * et, axis=1)
    return energy, et, lj["f_lj"]


@pytest.mark.parametrize("mode", ["list", "exact"])
def test_the_force_is_minus_the_gradient_of_probe_ats_energy(mode, wl, pkg):
    s, p, out, _ = _solved(wl, pkg, "mini", mode)
    x, typ = _clear_points(wl, s, mode)
    m = len(x)
    assert m >= 24, m
    q, al = np.full(m, 0.35), np.full(m, 0.9)
    e2s = np.sqrt(s.qqrd2e)
    pf = p.probe_force_at(x, typ, q, al)
    # the reference's own mismatch against central differences of the NumPy energy, same points, same step
    g = pgr.field_grad_numpy(x, None, None, *_ref_args(s, out))
    G = g["g_static"][0] + g["g_induced"][0]
    full = np.stack([G[:, [0, 3, 4]], G[:, [3, 1, 5]], G[:, [4, 5, 2]]], axis=1)
    _, et, flj = _numpy_energy_and_force(wl, s, out, x, typ, q, al)
    f_ref = flj + (q * e2s)[:, None] * et + al[:, None] * np.einsum("ma,mab->mb", et, full)
    fd_ref, fd_got = np.zeros((m, 3)), np.zeros((m, 3))
    for b in range(3):
        e = np.zeros(3)
        e[b] = H
        step = (x + e)[:, b] - (x - e)[:, b]
        ep, em = _numpy_energy_and_force(wl, s, out, x + e, typ, q, al)[0], _numpy_energy_and_force(wl, s, out, x - e, typ, q, al)[0]
        fd_ref[:, b] = -(ep - em) / step
        fd_got[:, b] = -(p.probe_at(x + e, typ, q, al)["energy"] - p.probe_at(x - e, typ, q, al)["energy"]) / step
    scale = np.max(np.abs(f_ref))
    mis_ref = float(np.max(np.abs(f_ref - fd_ref)) / scale)
    mis_got = float(np.max(np.abs(pf["force"] - fd_got)) / scale)
    print(mode, "points %d  |F - fd| / max|F|:  reference %.2e  library %.2e" % (m, mis_ref, mis_got))
    assert mis_ref < 1e-5          # (the reference force IS the gradient of the reference energy, to the differencing's error)
    assert mis_got <= 10 * mis_ref


def test_a_call_leaves_the_handle_as_it_was(wl, pkg):
    """`deterministic yes`: compute, compute, the two calls, compute -- forces, dipoles and the static field keep their bits."""
    s, _ = wl.load_fixture(ps.GOLD + "/mof5_h2.npz", extra_args=["use_previous", "no", "dd_cutoff", "9.0", "deterministic", "yes"])
    p = pkg.pair_from_system(s)
    try:
        a, b = p.compute(eflag=1, vflag=2), p.compute(eflag=1, vflag=2)
        pt = ps.draw_points(s, 3)
        g1 = p.field_grad_at(pt["x"], pt["skip"], pt["mol"])
        f1 = p.probe_force_at(pt["x"], pt["type"], pt["q"], pt["alpha"], pt["skip"], pt["mol"])
        c = p.compute(eflag=1, vflag=2)
        g2 = p.field_grad_at(pt["x"], pt["skip"], pt["mol"])
    finally:
        p.close()
    for k in ("f", "mu", "ef_static"):
        assert np.array_equal(a[k], b[k]) and np.array_equal(b[k], c[k]), k
    for k in GKEYS:
        assert np.array_equal(g1[k], g2[k]), k
    assert np.all(np.isfinite(f1["force"]))


def _code(pkg, fn):
    with pytest.raises(pkg.PolarError) as e:
        fn()
    assert len(str(e.value)) > 10 and "polar_" in str(e.value)
    return e.value.code


def test_call_window_refusals_and_bad_input(wl, pkg):
    s = ps.mini(wl, extra=["dd_cutoff", "9.0"])
    p = pkg.pair_from_system(s)
    calls = (lambda x=s.x[:3], **kw: p.field_grad_at(x, **kw), lambda x=s.x[:3], **kw: p.probe_force_at(x, 1, 0.1, 0.1, **kw))
    try:
        for f in calls:
            assert _code(pkg, f) == ERR_STATE                                   # before any compute
        p.compute()
        for f in calls:
            f()
        p.set_positions(s.x)
        for f in calls:
            assert _code(pkg, f) == ERR_STATE                                   # after polar_set_positions
        p.compute()
        for f in calls:
            f()
        p.set_box(s.boxlo, s.prd)
        for f in calls:
            assert _code(pkg, f) == ERR_STATE                                   # after polar_set_box
        p.compute()
        bad = s.x[:4].copy()
        bad[2, 1] = np.nan
        for f in calls:
            assert _code(pkg, lambda: f(bad)) == ERR_INPUT
            assert _code(pkg, lambda: f(s.x[:4], skip_atom=np.array([0, 1, s.nlocal, 2], np.int32))) == ERR_INPUT
        assert _code(pkg, lambda: p.probe_force_at(s.x[:4], [1, 0, 1, 2], 0.1, 0.1)) == ERR_INPUT
        assert _code(pkg, lambda: p.probe_force_at(s.x[:4], [1, 2, s.ntypes + 1, 2], 0.1, 0.1)) == ERR_INPUT
        empty = p.field_grad_at(np.zeros((0, 3)))                               # npoints == 0 is a no-op
        assert empty["g_static"].shape == (0, 6) and empty["e_static"].shape == (0, 3)
        assert p.probe_force_at(np.zeros((0, 3)), 1, 0.1, 0.1)["force"].shape == (0, 3)
    finally:
        p.close()
    for kw, syskw in ((dict(row_range=(0, 30)), dict(extra=["dd_cutoff", "9.0"])), (dict(), None)):
        s2 = ps.mini(wl, **syskw) if syskw else ps.system(wl, "mini_ew", "list")
        p2 = pkg.pair_from_system(s2, **kw)
        try:
            if not kw:
                p2.compute()
            assert _code(pkg, lambda: p2.field_grad_at(s2.x[:3])) == ERR_UNSUPPORTED   # a row-sharded handle; polar_ewald
            assert _code(pkg, lambda: p2.probe_force_at(s2.x[:3], 1, 0.1, 0.1)) == ERR_UNSUPPORTED
        finally:
            p2.close()


def test_grid_shapes_and_insertion_force(wl, pkg):
    s, p, out, pt = _solved(wl, pkg, "mini", "list")
    g = p.field_grad_grid((4, 3, 2))
    assert g["g_static"].shape == g["g_induced"].shape == (2, 3, 4, 6) and g["e_static"].shape == g["e_induced"].shape == (2, 3, 4, 3)
    fl = p.field_grad_at(p.grid_points((4, 3, 2)))
    for k in GKEYS + ("e_static", "e_induced"):
        assert np.array_equal(g[k].reshape(fl[k].shape), fl[k]), k
    rng = np.random.default_rng(29)
    centre = rng.uniform(0, 20.0, (8, 1, 3))
    u = rng.normal(size=(8, 1, 3))
    u /= np.linalg.norm(u, axis=2)[:, :, None]
    sites = centre + np.array([-1.16, 0.0, 1.16])[None, :, None] * u
    typ, q, al = np.array([1, 2, 1]), np.array([-0.35, 0.7, -0.35]), np.array([0.85, 1.2, 0.85])
    mol = np.where(np.arange(8) % 2 == 1, rng.integers(1, 19, 8), 0).astype(np.int32)
    ins = p.insertion_force(sites, typ, q, al, molecule=mol)
    flat = p.probe_force_at(sites.reshape(-1, 3), np.tile(typ, 8), np.tile(q, 8), np.tile(al, 8), None, np.repeat(mol, 3))
    f = flat["force"].reshape(8, 3, 3)
    assert ins["force"].shape == ins["torque"].shape == (8, 3) and np.array_equal(ins["force"], f.sum(axis=1))
    assert np.array_equal(ins["torque"], np.cross(sites - sites.mean(axis=1)[:, None, :], f).sum(axis=1)) and np.max(np.abs(ins["torque"])) > 0
    about = p.insertion_force(sites, typ, q, al, centre=sites[:, 1, :], molecule=mol)
    assert np.array_equal(about["torque"], np.cross(sites - sites[:, 1:2, :], f).sum(axis=1))
