"""polar_ewald_field_grad_at and polar_ewald_probe_force_at on the MI355X: the gradient of the Ewald field at points and the
full force on a test site, for handles with `polar_ewald`.

Systems are the small ones of tests/test_gpu_ewald_field_at.py, restated: `mini` (60 atoms, L = 20 A, cut_coul 9, `polar_ewald
1e-6` at g = 0.32: 919 k-vectors, one row chunk; exact mode and list mode with dd_cutoff 9, cubic and tilted, both damping
types), `charged` (the tilted mini in list mode with every charge raised by 0.05, accuracy 1e-12 at g = 0.6: 16,926 k-vectors in
17 row chunks, the last one partial, Q = 3 e: the chunked fold) and `mof5_h2` (tests/golden, list mode with dd_cutoff 12.8345:
five cells or more per axis, the stencil crosses the seam).  257 points per case from probe_systems.draw_points: in the box, up
to two box lengths out, 0.3 A from an atom, on atoms with that atom skipped; half of them with a molecule id.  One solve per
case, cached for the module, and one NumPy reference per case.

Tolerances.  Every component of both gradients against the NumPy reference (tests/ewald_point_grad_numpy.py) within 1e-10 of
its maximum over the points, the figure tests/test_gpu_ewald_field_at.py asserts (a dropped or doubled in-cutoff pair is >= 1e-4).
The field outputs, f_lj, f_coul and the sum of the three forces are checked bit for bit against the handle's own calls; f_pol
against the NumPy expression of the call's own outputs within 8 eps of the sum of the absolute terms (the rule of
tests/test_gpu_field_grad_at.py).  g_induced against polar_field_grad_at's bits is NOT checked: that call needs a finished step
of a handle without the keyword, whose records then hold that handle's own dipoles (polar_upload_mu writes the next step's
initial guess, not the records the point kernels read) -- g_induced is compared with the NumPy induced gradient at 1e-10 instead.
The force against central differences (H = 1e-4 A) of probe_at's energy on the same handle: ten times the mismatch the NumPy
reference shows against central differences of the NumPy energy at the same points.  Measured worst cases: DESIGN section 6i."""
import copy
import os

import numpy as np
import pytest

import ewald_point_grad_numpy as egn
import ewald_point_numpy as epn
import point_ref as ptr
import probe_ref as prb
import probe_systems as ps

pytestmark = pytest.mark.gpu
TILT = ps.TILT
NPTS = ps.NPTS
EPS = 2.0 ** -52
ERR_INPUT, ERR_UNSUPPORTED, ERR_STATE = -1, -4, -5
GKEYS = ("g_static", "g_induced")
H = 1e-4


def _mini(wl, extra=(), tilt=None, damp="exponential", g=0.32, acc="1e-6", shift=0.0, n=60, seed=620, L=20.0):
    """tests/test_gpu_ewald_field_at.py::_mini: the 60-atom recipe with the polar_ewald keyword (acc None: without), g_ewald = g
    and every charge raised by `shift`"""
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
    s = wl.make_system(x, q, alpha, typ, mol, np.zeros(3), np.array([L, L, L]), 2, ps.MINI_ROWS, st, g, name="mini")
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
    return wl.load_fixture(os.path.join(ps.GOLD, case + ".npz"), extra_args=extra)[0], 1e-6


_CACHE, _REF = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _close_cached_handles():
    yield
    for v in _CACHE.values():
        v[1].close()
    _CACHE.clear()
    _REF.clear()


def _solved(wl, pkg, case, mode="list", tilt=None, damp="exponential"):
    """(system, handle after one compute, its outputs, accuracy, points): one solve per case for the whole module"""
    key = (case, mode, tilt, damp)
    if key not in _CACHE:
        s, acc = _system(wl, case, mode, tilt, damp)
        p = pkg.pair_from_system(s)
        out = p.compute(eflag=1, vflag=2)
        assert out["status"] == 0 and out["rms_dmu"] <= 1e-13 and out["nkvec"] > 0
        _CACHE[key] = (s, p, out, acc, ps.draw_points(s, 3))
    return _CACHE[key]


def _ref_args(s, out, acc):
    n, st = s.nlocal, s.settings
    return (s.x[:n], s.q[:n], s.alpha[:n], s.molecule[:n], out["mu"], s.prd, ps.tilt_of(s), st.cut_coul,
            st.dd_cutoff if st.dd_cutoff > 0 else None, st.polar_damp, st.damping_type, np.sqrt(s.qqrd2e), s.g_ewald, acc)


def _reference(key, s, out, acc, pt):
    """the NumPy gradients of a case's 257 points, computed once"""
    if key not in _REF:
        _REF[key] = egn.field_grad_numpy(pt["x"], pt["skip"], pt["mol"], *_ref_args(s, out, acc))
    return _REF[key]


CASES = [("mini", "exact", None, "exponential"), ("mini", "exact", None, "none"), ("mini", "list", None, "exponential"),
         ("mini", "list", None, "none"), ("mini", "exact", TILT, "exponential"), ("mini", "list", TILT, "exponential"),
         ("charged", "list", TILT, "exponential"), ("mof5_h2", "list", None, "exponential")]


@pytest.mark.parametrize("case,mode,tilt,damp", CASES)
def test_both_gradients_against_the_numpy_reference(case, mode, tilt, damp, wl, pkg):
    s, p, out, acc, pt = _solved(wl, pkg, case, mode, tilt, damp)
    if case == "charged":   # what this case is about: a charged box and a k-vector set of several row chunks with a partial last one
        assert abs(s.q[:s.nlocal].sum() - 3.0) < 1e-9 and 15000 <= out["nkvec"] <= 19000
    got = p.ewald_field_grad_at(pt["x"], pt["skip"], pt["mol"])
    ref = _reference((case, mode, tilt, damp), s, out, acc, pt)
    worst = {}
    for k in GKEYS:
        v = ref[k][0]
        top = np.max(np.abs(v), axis=0)
        assert got[k].shape == (NPTS, 6) and np.all(top > 0.0)
        worst[k] = float(np.max(np.max(np.abs(got[k] - v), axis=0) / top))
    print(case, mode, tilt, damp, "nkvec %d  max |got - ref| / max |ref| per component:" % out["nkvec"],
          "  ".join("%s %.2e" % kv for kv in worst.items()), " ms real %.3f recip %.3f" % (got["ms_real"], got["ms_recip"]))
    for k in GKEYS:
        assert worst[k] <= 1e-10, (k, worst[k])
    assert abs(got["ms"] - got["ms_real"] - got["ms_recip"]) <= 1e-9 * got["ms"] and got["ms_real"] > 0.0 and got["ms_recip"] > 0.0
    if damp == "none":   # the undamped induced gradient is traceless
        tr = got["g_induced"][:, 0] + got["g_induced"][:, 1] + got["g_induced"][:, 2]
        assert np.all(np.abs(tr) <= 1e-10 * ref["g_induced"][1][:, :3].sum(axis=1))


@pytest.mark.parametrize("case,mode,tilt,damp", [("mini", "exact", None, "none"), ("mini", "list", None, "exponential"),
                                                 ("mini", "list", TILT, "exponential"), ("charged", "list", TILT, "exponential")])
def test_fields_forces_passes_and_order_bit_for_bit(case, mode, tilt, damp, wl, pkg, monkeypatch):
    s, p, out, acc, pt = _solved(wl, pkg, case, mode, tilt, damp)
    monkeypatch.delenv("POLAR_FIELD_AT_CHUNK", raising=False)
    one = p.ewald_field_grad_at(pt["x"], pt["skip"], pt["mol"])
    fa = p.ewald_field_at(pt["x"], pt["skip"], pt["mol"])
    # the field outputs are ewald_field_at's, bit for bit
    assert np.array_equal(one["e_static"], fa["e_static"]) and np.array_equal(one["e_induced"], fa["e_induced"])
    assert np.max(np.abs(fa["e_static"])) > 0 and np.max(np.abs(fa["e_induced"])) > 0
    # passes, order, a second call, field=False: no bit of any gradient component changes
    again = p.ewald_field_grad_at(pt["x"], pt["skip"], pt["mol"])
    monkeypatch.setenv("POLAR_FIELD_AT_CHUNK", "37")
    chunked = p.ewald_field_grad_at(pt["x"], pt["skip"], pt["mol"])
    monkeypatch.delenv("POLAR_FIELD_AT_CHUNK")
    perm = np.random.default_rng(17).permutation(NPTS)
    shuffled = p.ewald_field_grad_at(pt["x"][perm], pt["skip"][perm], pt["mol"][perm])
    nofield = p.ewald_field_grad_at(pt["x"], pt["skip"], pt["mol"], field=False)
    assert nofield["e_static"] is None and nofield["e_induced"] is None
    for k in GKEYS:
        assert np.array_equal(one[k], again[k]), (k, "second call")
        assert np.array_equal(one[k], chunked[k]), (k, "passes of 37")
        assert np.array_equal(one[k][perm], shuffled[k]), (k, "permuted")
        assert np.array_equal(one[k], nofield[k]), (k, "field=False")
    assert np.array_equal(chunked["e_static"], fa["e_static"]) and np.array_equal(shuffled["e_static"], fa["e_static"][perm])
    # the forces on a site
    pf = p.ewald_probe_force_at(pt["x"], pt["type"], pt["q"], pt["alpha"], pt["skip"], pt["mol"])
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
    pf2 = p.ewald_probe_force_at(pt["x"][perm], pt["type"][perm], pt["q"][perm], pt["alpha"][perm], pt["skip"][perm], pt["mol"][perm])
    monkeypatch.delenv("POLAR_FIELD_AT_CHUNK")
    for k in ("f_lj", "f_coul", "f_pol"):
        assert np.array_equal(pf[k][perm], pf2[k]), k


def clear_points(wl, s, mode, want=64, seed=41):
    """The rule of tests/test_gpu_field_grad_at.py::_clear_points, restated: of 64 drawn points, those at least 1.5 A from every
    atom and further than 10 H from every cut_coul, dd_cutoff and per-pair LJ cutoff shell (all 27 images) and, in exact mode, from
    every half-box image flip."""
    rng = np.random.default_rng(seed)
    n, st = s.nlocal, s.settings
    prd = np.asarray(s.prd, np.float64)
    tb = ps.tables_of(wl, s, False)
    cuts = [st.cut_coul] + ([st.dd_cutoff] if st.dd_cutoff > 0 else [])
    ljc = np.sqrt(np.asarray(tb["cut_ljsq"], np.float64))
    pts, types = rng.uniform(0, prd[0], (want, 3)), rng.integers(1, s.ntypes + 1, want).astype(np.int32)
    sh = np.array([(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)], np.float64) * prd
    keep = []
    for k in range(want):
        raw = pts[k] - s.x[:n]
        d0 = raw - prd * np.round(raw / prd)
        r = np.sqrt(np.sum((d0[:, None, :] + sh[None, :, :]) ** 2, axis=2))             # [n, 27]
        ok = np.min(r) >= 1.5 and all(np.min(np.abs(r - c)) > 10 * H for c in cuts)
        ok = ok and np.min(np.abs(r - ljc[types[k], s.type[:n]][:, None])) > 10 * H
        if mode == "exact":
            ok = ok and np.min(np.abs(np.abs(d0) - 0.5 * prd)) > 10 * H
        if ok:
            keep.append(k)
    return pts[keep], types[keep]


def _numpy_energy_and_force(wl, s, out, acc, x, typ, q, al):
    tb = ps.tables_of(wl, s, False)
    n = s.nlocal
    fa = epn.field_at_numpy(x, None, None, *_ref_args(s, out, acc))
    lj = prb.probe_lj_numpy(x, typ, None, None, s.x[:n], s.type[:n], s.molecule[:n], tb, s.prd, ps.tilt_of(s))
    et = fa["e_static"] + fa["e_induced"]
    energy = lj["e_lj"] + q * np.sqrt(s.qqrd2e) * (fa["phi_static"] + fa["phi_induced"]) - 0.5 * al * np.sum(et * et, axis=1)
    return energy, et, lj["f_lj"]


@pytest.mark.parametrize("mode", ["list", "exact"])
def test_the_force_is_minus_the_gradient_of_probe_ats_energy(mode, wl, pkg):
    s, p, out, acc, _ = _solved(wl, pkg, "mini", mode)
    x, typ = clear_points(wl, s, mode)
    m = len(x)
    assert m >= 24, m
    q, al = np.full(m, 0.35), np.full(m, 0.9)
    e2s = np.sqrt(s.qqrd2e)
    pf = p.ewald_probe_force_at(x, typ, q, al)
    # the reference's own mismatch against central differences of the NumPy energy, same points, same step
    g = egn.field_grad_numpy(x, None, None, *_ref_args(s, out, acc))
    G = g["g_static"][0] + g["g_induced"][0]
    full = np.stack([G[:, [0, 3, 4]], G[:, [3, 1, 5]], G[:, [4, 5, 2]]], axis=1)
    _, et, flj = _numpy_energy_and_force(wl, s, out, acc, x, typ, q, al)
    f_ref = flj + (q * e2s)[:, None] * et + al[:, None] * np.einsum("ma,mab->mb", et, full)
    fd_ref, fd_got = np.zeros((m, 3)), np.zeros((m, 3))
    for b in range(3):
        e = np.zeros(3)
        e[b] = H
        step = (x + e)[:, b] - (x - e)[:, b]
        ep, em = (_numpy_energy_and_force(wl, s, out, acc, x + sg * e, typ, q, al)[0] for sg in (1, -1))
        fd_ref[:, b] = -(ep - em) / step
        fd_got[:, b] = -(p.probe_at(x + e, typ, q, al)["energy"] - p.probe_at(x - e, typ, q, al)["energy"]) / step
    scale = np.max(np.abs(f_ref))
    mis_ref = float(np.max(np.abs(f_ref - fd_ref)) / scale)
    mis_got = float(np.max(np.abs(pf["force"] - fd_got)) / scale)
    print(mode, "points %d  |F - fd| / max|F|:  reference %.2e  library %.2e" % (m, mis_ref, mis_got))
    assert mis_ref < 1e-5          # (the reference force IS the gradient of the reference energy, to the differencing's error)
    assert mis_got <= 10 * mis_ref


def test_a_call_leaves_the_handle_as_it_was(wl, pkg):
    """`deterministic yes`, mof5_h2 with polar_ewald: compute, compute, both calls, compute -- forces, dipoles and the static
    field keep their bits, and a second call on the same dipoles gives the same gradients."""
    s, _ = wl.load_fixture(os.path.join(ps.GOLD, "mof5_h2.npz"),
                           extra_args=["use_previous", "no", "dd_cutoff", "9.0", "deterministic", "yes", "polar_ewald", "1e-6"])
    p = pkg.pair_from_system(s)
    try:
        a, b = p.compute(eflag=1, vflag=2), p.compute(eflag=1, vflag=2)
        pt = ps.draw_points(s, 3)
        g1 = p.ewald_field_grad_at(pt["x"], pt["skip"], pt["mol"])
        f1 = p.ewald_probe_force_at(pt["x"], pt["type"], pt["q"], pt["alpha"], pt["skip"], pt["mol"])
        c = p.compute(eflag=1, vflag=2)
        g2 = p.ewald_field_grad_at(pt["x"], pt["skip"], pt["mol"])
    finally:
        p.close()
    for k in ("f", "mu", "ef_static"):
        assert np.array_equal(a[k], b[k]) and np.array_equal(b[k], c[k]), k
    for k in GKEYS:
        assert np.array_equal(g1[k], g2[k]), k
    assert np.all(np.isfinite(f1["force"])) and np.max(np.abs(f1["f_pol"])) > 0


def _code(pkg, fn, names=()):
    with pytest.raises(pkg.PolarError) as e:
        fn()
    assert len(str(e.value)) > 10 and all(nm in str(e.value) for nm in names), str(e.value)
    return e.value.code


def test_call_window_refusals_and_bad_input(wl, pkg):
    s = _mini(wl, extra=["dd_cutoff", "9.0"])
    p = pkg.pair_from_system(s)
    calls = (lambda x=s.x[:3], **kw: p.ewald_field_grad_at(x, **kw), lambda x=s.x[:3], **kw: p.ewald_probe_force_at(x, 1, 0.1, 0.1, **kw))
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
        assert _code(pkg, lambda: p.ewald_probe_force_at(s.x[:4], [1, 0, 1, 2], 0.1, 0.1)) == ERR_INPUT
        assert _code(pkg, lambda: p.ewald_probe_force_at(s.x[:4], [1, 2, s.ntypes + 1, 2], 0.1, 0.1)) == ERR_INPUT
        empty = p.ewald_field_grad_at(np.zeros((0, 3)))                         # npoints == 0 is a no-op
        assert empty["g_static"].shape == (0, 6) and empty["e_static"].shape == (0, 3)
        assert p.ewald_probe_force_at(np.zeros((0, 3)), 1, 0.1, 0.1)["force"].shape == (0, 3)
        # the calls without the keyword in their name still refuse this handle, and say where to go
        assert _code(pkg, lambda: p.field_grad_at(s.x[:3]), ["polar_ewald_field_grad_at"]) == ERR_UNSUPPORTED
        assert _code(pkg, lambda: p.probe_force_at(s.x[:3], 1, 0.1, 0.1), ["polar_ewald_probe_force_at"]) == ERR_UNSUPPORTED
    finally:
        p.close()
    # a row-sharded handle
    p2 = pkg.pair_from_system(_mini(wl, extra=["dd_cutoff", "9.0"]), row_range=(0, 30))
    try:
        assert _code(pkg, lambda: p2.ewald_field_grad_at(s.x[:3])) == ERR_UNSUPPORTED
        assert _code(pkg, lambda: p2.ewald_probe_force_at(s.x[:3], 1, 0.1, 0.1)) == ERR_UNSUPPORTED
    finally:
        p2.close()
    # the keyword off: refused, and the message names the call for such a handle
    s3 = _mini(wl, acc=None)
    p3 = pkg.pair_from_system(s3)
    try:
        p3.compute()
        assert _code(pkg, lambda: p3.ewald_field_grad_at(s3.x[:3]), ["polar_field_grad_at"]) == ERR_UNSUPPORTED
        assert _code(pkg, lambda: p3.ewald_probe_force_at(s3.x[:3], 1, 0.1, 0.1), ["polar_probe_force_at"]) == ERR_UNSUPPORTED
        p3.field_grad_at(s3.x[:3])
    finally:
        p3.close()


def test_grid_shapes_and_insertion_force(wl, pkg):
    s, p, out, acc, pt = _solved(wl, pkg, "mini", "list")
    g = p.ewald_field_grad_grid((4, 3, 2))
    assert g["g_static"].shape == g["g_induced"].shape == (2, 3, 4, 6) and g["e_static"].shape == g["e_induced"].shape == (2, 3, 4, 3)
    fl = p.ewald_field_grad_at(p.grid_points((4, 3, 2)))
    for k in GKEYS + ("e_static", "e_induced"):
        assert np.array_equal(g[k].reshape(fl[k].shape), fl[k]), k
    rng = np.random.default_rng(29)
    centre = rng.uniform(0, 20.0, (8, 1, 3))
    u = rng.normal(size=(8, 1, 3))
    u /= np.linalg.norm(u, axis=2)[:, :, None]
    sites = centre + np.array([-1.16, 0.0, 1.16])[None, :, None] * u
    typ, q, al = np.array([1, 2, 1]), np.array([-0.35, 0.7, -0.35]), np.array([0.85, 1.2, 0.85])
    mol = np.where(np.arange(8) % 2 == 1, rng.integers(1, 19, 8), 0).astype(np.int32)
    ins = p.ewald_insertion_force(sites, typ, q, al, molecule=mol)
    flat = p.ewald_probe_force_at(sites.reshape(-1, 3), np.tile(typ, 8), np.tile(q, 8), np.tile(al, 8), None, np.repeat(mol, 3))
    f = flat["force"].reshape(8, 3, 3)
    assert ins["force"].shape == ins["torque"].shape == (8, 3) and np.array_equal(ins["force"], f.sum(axis=1))
    assert np.array_equal(ins["torque"], np.cross(sites - sites.mean(axis=1)[:, None, :], f).sum(axis=1)) and np.max(np.abs(ins["torque"])) > 0
    about = p.ewald_insertion_force(sites, typ, q, al, centre=sites[:, 1, :], molecule=mol)
    assert np.array_equal(about["torque"], np.cross(sites - sites[:, 1:2, :], f).sum(axis=1))
