"""polar_probe_at on the MI355X: LJ, Coulomb and first-order induction energy of test sites.

Systems (tests/probe_systems.py): `mini` (exact mode and dd_cutoff 9, orthogonal and tilted; `mini_ew` with polar_ewald),
`lattice_lj` (9 x 9 x 9 cells, trimmed stencils of two to five cells, reach = cutall for type 2, inert sites that live only in
the second copy of the grid; once with `pair_modify shift yes`), `mof5_h2` (ten types, cut_lj far below cutall).  257 points per
case, which leaves the last workgroup partial.

Tolerances.  e_lj and every component of f_lj against the NumPy brute force (tests/probe_ref.py): 1e-10 of the point's scale --
the project's figure for whole sums against NumPy; a dropped or doubled in-reach pair is orders above it.  The composition of the
field half is checked bit for bit against the handle's own field call (e_pol: 4 eps relative).  Measured worst cases per case:
DESIGN section 6g."""
import os
import subprocess
import sys

import numpy as np
import pytest

import probe_ref as prb
import probe_systems as ps

pytestmark = pytest.mark.gpu
TILT = ps.TILT
NPTS = ps.NPTS
EPS = 2.0 ** -52
ERR_INPUT, ERR_UNSUPPORTED, ERR_STATE = -1, -4, -5
HERE = os.path.dirname(os.path.abspath(__file__))

_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _close_cached_handles():
    yield
    for v in _CACHE.values():
        v[1].close()
    _CACHE.clear()


def _solved(wl, pkg, case, mode="list", tilt=None, shift=False):
    """(system, handle after one compute, its outputs, points, NumPy reference): one solve and one reference per case"""
    key = (case, mode, tilt, shift)
    if key not in _CACHE:
        s = ps.system(wl, case, mode, tilt)
        p = pkg.pair_from_system(s, modify_args=("shift", "yes") if shift else ())
        out = p.compute(eflag=1, vflag=2)
        assert out["status"] == 0
        pt, ref = ps.points_and_reference(wl, s, shift)
        _CACHE[key] = (s, p, out, pt, ref)
    return _CACHE[key]


def _probe(p, pt, force=True, sl=slice(None), **kw):
    a = dict(x=pt["x"][sl], type=pt["type"][sl], q=pt["q"][sl], alpha=pt["alpha"][sl], skip_atom=pt["skip"][sl], molecule=pt["mol"][sl])
    a.update(kw)
    return p.probe_at(a["x"], a["type"], a["q"], a["alpha"], a["skip_atom"], a["molecule"], force=force)


def _lj_errors(got, ref):
    e = np.abs(got["e_lj"] - ref["e_lj"])
    f = np.max(np.abs(got["f_lj"] - ref["f_lj"]), axis=1)
    assert np.all(e[ref["e_scale"] == 0] == 0) and np.all(f[ref["f_scale"] == 0] == 0)
    we = float(np.max(e / np.where(ref["e_scale"] > 0, ref["e_scale"], 1.0)))
    wf = float(np.max(f / np.where(ref["f_scale"] > 0, ref["f_scale"], 1.0)))
    return we, wf


CASES = [("mini", "exact", None, False), ("mini", "list", None, False), ("mini", "exact", TILT, False), ("mini", "list", TILT, False),
         ("mini_ew", "exact", None, False), ("mini_ew", "list", None, False), ("lattice_lj", "list", None, False),
         ("lattice_lj", "list", None, True), ("mof5_h2", "list", None, False)]


@pytest.mark.parametrize("case,mode,tilt,shift", CASES)
def test_e_lj_and_f_lj_against_the_numpy_brute_force(case, mode, tilt, shift, wl, pkg):
    s, p, out, pt, ref = _solved(wl, pkg, case, mode, tilt, shift)
    if case == "lattice_lj":   # the grid and the sites this case is about
        n = s.nlocal
        assert int(s.prd[0] / (0.5 * 6.0)) == 9
        inert = (s.q[:n] == 0) & (s.alpha[:n] == 0)
        assert 5 <= np.sum(inert) <= 25
        assert p.extract("cell_active") == n - np.sum(inert)            # they live only in the second copy of the grid
        if shift:
            assert np.any(ps.tables_of(wl, s, True)["offset"][1:, 1:] != 0)
    assert np.sum(ref["e_scale"] > 0) > 100 and np.all(np.isfinite(ref["e_lj"]))
    got = _probe(p, pt)
    we, wf = _lj_errors(got, ref)
    print(case, mode, tilt, "shift" if shift else "", "max |got - ref| / scale:  e_lj %.2e  f_lj %.2e   ms %.3f" % (we, wf, got["ms"]))
    assert np.all(np.abs(got["e_lj"] - ref["e_lj"]) <= 1e-10 * ref["e_scale"]), we               # no point is left out
    assert np.all(np.abs(got["f_lj"] - ref["f_lj"]) <= 1e-10 * ref["f_scale"][:, None]), wf
    assert np.array_equal(got["energy"], got["e_lj"] + got["e_coul"] + got["e_pol"])


@pytest.mark.parametrize("case,mode,tilt", [("mini", "exact", None), ("mini", "list", None), ("mini", "list", TILT), ("lattice_lj", "list", None),
                                            ("mof5_h2", "list", None), ("mini_ew", "exact", None), ("mini_ew", "list", None)])
def test_the_field_half_is_the_handles_field_call_bit_for_bit(case, mode, tilt, wl, pkg):
    s, p, out, pt, ref = _solved(wl, pkg, case, mode, tilt)
    got = _probe(p, pt)
    fa = (p.ewald_field_at if case == "mini_ew" else p.field_at)(pt["x"], pt["skip"], pt["mol"])
    e2s = np.sqrt(s.qqrd2e)
    et = fa["e_static"] + fa["e_induced"]
    assert np.array_equal(got["e_total"], et)
    assert np.array_equal(got["e_coul"], (pt["q"] * e2s) * (fa["phi_static"] + fa["phi_induced"]))
    want = -0.5 * pt["alpha"] * (et[:, 0] * et[:, 0] + et[:, 1] * et[:, 1] + et[:, 2] * et[:, 2])
    assert np.all(np.abs(got["e_pol"] - want) <= 4 * EPS * np.abs(want))
    assert np.max(np.abs(got["e_coul"])) > 0 and np.max(np.abs(got["e_pol"])) > 0 and np.all(got["e_pol"][pt["alpha"] == 0] == 0)


@pytest.mark.parametrize("shift", [False, True], ids=["noshift", "shift"])
def test_half_the_sum_over_the_atoms_is_the_steps_eng_vdwl(shift, wl, pkg):
    """The step itself as the yardstick: `mini` in list mode, built with exclude_intra and every atom in a molecule (atoms with id 0
    would be excluded from each other by the list but not by the probe's rule); points on every atom i with its type, skip_atom =
    i, molecule = mol_i.  1e-10 of the summed scales."""
    s = ps.mini(wl, extra=["dd_cutoff", "9.0"], all_in_molecules=True, exclude_intra=True)
    n = s.nlocal
    assert np.all(s.molecule[:n] != 0)
    p = pkg.pair_from_system(s, modify_args=("shift", "yes") if shift else ())
    try:
        out = p.compute(eflag=1, vflag=2)
        idx = np.arange(n, dtype=np.int32)
        got = p.probe_at(s.x[:n], s.type[:n], None, None, idx, s.molecule[:n])
    finally:
        p.close()
    ref = prb.probe_lj_numpy(s.x[:n], s.type[:n], idx, s.molecule[:n], s.x[:n], s.type[:n], s.molecule[:n], ps.tables_of(wl, s, shift), s.prd)
    scale = float(np.sum(ref["e_scale"]))
    half = 0.5 * float(np.sum(got["e_lj"]))
    print("shift %d  eng_vdwl %.15g  half the probe sum %.15g  difference / scale %.2e" % (shift, out["eng_vdwl"], half, abs(half - out["eng_vdwl"]) / scale))
    assert scale > 0 and out["eng_vdwl"] != 0.0
    assert abs(half - out["eng_vdwl"]) <= 1e-10 * scale


def test_the_inert_copy_of_the_grid(wl, pkg, tmp_path):
    """`lattice_lj` under POLAR_CELL_INERT=0 and under POLAR_NL_INERT=0, each in a fresh handle in a child process: no second
    copy of the grid there, the inert sites sit in the front one.  e_lj agrees with the default run within 1e-12 of scale, and
    every inert site's term is present: the reference check passes in all three."""
    s, p, out, pt, ref = _solved(wl, pkg, "lattice_lj")
    n = s.nlocal
    default = _probe(p, pt)
    assert max(_lj_errors(default, ref)) <= 1e-10
    # the reference without the inert sites differs: the check would notice their absence
    act = ~((s.q[:n] == 0) & (s.alpha[:n] == 0))
    keep = np.where(act)[0]
    remap = np.full(n, -1)
    remap[keep] = np.arange(len(keep))
    without = prb.probe_lj_numpy(pt["x"], pt["type"], np.where(pt["skip"] >= 0, remap[pt["skip"]], -1), pt["mol"], s.x[:n][act], s.type[:n][act],
                                 s.molecule[:n][act], ps.tables_of(wl, s, False), s.prd)
    assert np.sum(np.abs(without["e_lj"] - ref["e_lj"]) > 1e-6 * ref["e_scale"]) > 10
    pts = str(tmp_path / "points.npz")
    np.savez(pts, **pt)
    for var in ("POLAR_CELL_INERT", "POLAR_NL_INERT"):
        env = {k: v for k, v in os.environ.items() if k not in ("POLAR_CELL_INERT", "POLAR_NL_INERT")}
        env[var] = "0"
        outp = str(tmp_path / (var + ".npz"))
        r = subprocess.run([sys.executable, os.path.join(HERE, "probe_child.py"), "0", pts, outp], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        z = np.load(outp)
        assert z["cell_active"] == n, var                                  # no second copy: every site in the front one
        child = dict(e_lj=z["e_lj"], f_lj=z["f_lj"])
        we, wf = _lj_errors(child, ref)
        d = float(np.max(np.abs(child["e_lj"] - default["e_lj"]) / np.where(ref["e_scale"] > 0, ref["e_scale"], 1.0)))
        print(var + "=0: against the reference e_lj %.2e f_lj %.2e; against the default run %.2e" % (we, wf, d))
        assert we <= 1e-10 and wf <= 1e-10
        assert np.all(np.abs(child["e_lj"] - default["e_lj"]) <= 1e-12 * ref["e_scale"])


@pytest.mark.parametrize("case,mode", [("mini", "exact"), ("mini", "list"), ("lattice_lj", "list"), ("mini_ew", "list")])
def test_passes_order_and_halves_do_not_change_a_bit(case, mode, wl, pkg, monkeypatch):
    s, p, out, pt, ref = _solved(wl, pkg, case, mode)
    keys = ("e_lj", "f_lj", "e_coul", "e_pol", "e_total", "energy")
    monkeypatch.delenv("POLAR_FIELD_AT_CHUNK", raising=False)
    one = _probe(p, pt)
    again = _probe(p, pt)
    monkeypatch.setenv("POLAR_FIELD_AT_CHUNK", "64")
    chunked = _probe(p, pt)
    monkeypatch.delenv("POLAR_FIELD_AT_CHUNK")
    perm = np.random.default_rng(17).permutation(NPTS)
    shuffled = _probe(p, {k: v[perm] for k, v in pt.items()})
    for k in keys:
        assert np.array_equal(one[k], again[k]), (k, "second call")
        assert np.array_equal(one[k], chunked[k]), (k, "passes of 64")
        assert np.array_equal(one[k][perm], shuffled[k]), (k, "permuted")
    noforce = _probe(p, pt, force=False)
    assert noforce["f_lj"] is None and np.array_equal(noforce["e_lj"], one["e_lj"])
    lj_only = _probe(p, pt, q=None, alpha=None)
    assert lj_only["e_total"] is None and np.array_equal(lj_only["e_lj"], one["e_lj"]) and np.array_equal(lj_only["f_lj"], one["f_lj"])
    field_only = _probe(p, pt, force=False, type=None)
    for k in ("e_coul", "e_pol", "e_total"):
        assert np.array_equal(field_only[k], one[k]), (k, "field only")
    assert np.all(field_only["e_lj"] == 0)
    empty = p.probe_at(np.zeros((0, 3)), 1, 0.0, 0.0, force=True)
    assert empty["e_lj"].shape == (0,) and empty["f_lj"].shape == (0, 3)


def test_a_call_leaves_the_handle_as_it_was(wl, pkg):
    """`deterministic yes`, `use_previous no`, one handle: compute, compute, probe_at, compute.  The forces, the dipoles, the
    static field and the sweep counts of the compute after the probe have the bits of the one before it, as two computes in a
    row have.  The energies and the virial are NOT bit-reproducible between two computes of one handle with or without a probe
    in between -- they are folded from per-wave atomic adds whose order varies from run to run (tests/test_gpu_field_at.py::
    test_a_call_leaves_the_handle_as_it_was; seen here as well: eng_pol -4.893276190256672 / -4.89327619025667 in a run whose
    first two computes agreed) -- so they are held to the figure of that test, 1e-13 relative, before and after the probe."""
    s, _ = wl.load_fixture(os.path.join(ps.GOLD, "mof5_h2.npz"), extra_args=["use_previous", "no", "dd_cutoff", "9.0", "deterministic", "yes"])
    p = pkg.pair_from_system(s)
    try:
        a, b = p.compute(eflag=1, vflag=2), p.compute(eflag=1, vflag=2)
        pt = ps.draw_points(s, 3)
        first = _probe(p, pt)
        c = p.compute(eflag=1, vflag=2)
        second = _probe(p, pt)
    finally:
        p.close()
    for k in ("f", "mu", "ef_static"):
        assert np.array_equal(a[k], b[k]) and np.array_equal(b[k], c[k]), k
    for k in ("iterations", "sweeps", "status", "dd_pairs"):
        assert a[k] == b[k] == c[k], k
    for x, y in ((a, b), (b, c)):
        for k in ("eng_vdwl", "eng_coul", "eng_pol", "u_self", "u_ef", "u_dd"):
            assert abs(x[k] - y[k]) <= 1e-13 * abs(x[k]), k
        assert np.max(np.abs(x["virial"] - y["virial"])) <= 1e-13 * np.max(np.abs(x["virial"]))
    for k in ("e_lj", "f_lj", "e_coul", "e_pol", "e_total"):   # and the probe of the same dipoles gives the same bits
        assert np.array_equal(first[k], second[k]), k


def _code(pkg, fn):
    with pytest.raises(pkg.PolarError) as e:
        fn()
    assert len(str(e.value)) > 10 and "polar_" in str(e.value)
    return e.value.code


def _works(s, p):
    p.compute(eflag=1, vflag=2)
    got = p.probe_at(s.x[:5], s.type[:5], 0.3, 0.5, np.arange(5, dtype=np.int32), s.molecule[:5])
    assert np.all(np.isfinite(got["energy"])) and np.max(np.abs(got["e_lj"])) > 0


def test_the_call_window(wl, pkg):
    s = ps.mini(wl)
    p = pkg.pair_from_system(s)
    try:
        assert _code(pkg, lambda: p.probe_at(s.x[:3], 1, 0.1, 0.1)) == ERR_STATE      # before the first compute
        _works(s, p)
        p.set_positions(s.x)
        assert _code(pkg, lambda: p.probe_at(s.x[:3], 1, 0.1, 0.1)) == ERR_STATE      # after polar_set_positions
        _works(s, p)
    finally:
        p.close()


def test_bad_sites_are_refused(wl, pkg):
    s = ps.mini(wl, extra=["dd_cutoff", "9.0"])
    p = pkg.pair_from_system(s)
    try:
        p.compute()
        x = s.x[:4]
        assert _code(pkg, lambda: p.probe_at(x, [1, 0, 1, 2], 0.1, 0.1)) == ERR_INPUT
        assert _code(pkg, lambda: p.probe_at(x, [1, 2, s.ntypes + 1, 2], 0.1, 0.1)) == ERR_INPUT
        assert _code(pkg, lambda: p.probe_at(x, 1, [0.1, np.nan, 0.0, 0.0], 0.1)) == ERR_INPUT
        assert _code(pkg, lambda: p.probe_at(x, 1, 0.1, [0.1, 0.2, -0.5, 0.0])) == ERR_INPUT
        assert _code(pkg, lambda: p.probe_at(x, 1, 0.1, np.inf)) == ERR_INPUT
        bad = x.copy()
        bad[2, 1] = np.nan
        assert _code(pkg, lambda: p.probe_at(bad, 1, 0.1, 0.1)) == ERR_INPUT              # what polar_field_at refuses
        assert _code(pkg, lambda: p.probe_at(x, 1, 0.1, 0.1, skip_atom=[0, 1, s.nlocal, 2])) == ERR_INPUT
        # e_lj asked for without types (the C entry point; the Python wrapper does not let one ask)
        import ctypes as C
        xx, e = np.ascontiguousarray(x), np.zeros(4)
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        assert p.L.polar_probe_at(p.h, 4, dp(xx), None, None, None, None, None, dp(e), None, None, None, None, None) == ERR_INPUT
        _works(s, p)
    finally:
        p.close()


def test_a_row_sharded_handle_is_refused(wl, pkg):
    s = ps.mini(wl, extra=["dd_cutoff", "9.0"])
    p = pkg.pair_from_system(s, row_range=(0, 30))
    try:
        assert _code(pkg, lambda: p.probe_at(s.x[:3], 1, 0.1, 0.1)) == ERR_UNSUPPORTED
        p._ck(p.L.polar_set_row_range(p.h, 0, -1))
        _works(s, p)
    finally:
        p.close()


@pytest.mark.parametrize("mode,cut_lj", [("list", "10.0"), ("exact", "10.5")])
def test_an_lj_reach_the_walk_does_not_cover(mode, cut_lj, wl, pkg):
    """List mode: an LJ cutoff beyond cutall = 9.  Exact mode: the 20 A box narrower than two LJ cutoffs.  UNSUPPORTED with an LJ
    output asked for; the field-only call is still served and is the handle's field call."""
    s = ps.mini(wl, extra=(["dd_cutoff", "9.0"] if mode == "list" else []), cut_lj=cut_lj)
    p = pkg.pair_from_system(s)
    try:
        p.compute()
        assert _code(pkg, lambda: p.probe_at(s.x[:3], 1, 0.1, 0.1)) == ERR_UNSUPPORTED
        assert _code(pkg, lambda: p.probe_at(s.x[:3], 1, None, None, force=True)) == ERR_UNSUPPORTED
        x = s.x[:7] + 0.4
        got = p.probe_at(x, None, 0.3, 0.7)
        fa = p.field_at(x)
        assert np.array_equal(got["e_total"], fa["e_static"] + fa["e_induced"]) and np.max(np.abs(got["e_coul"])) > 0
    finally:
        p.close()


def test_insertion_energy_and_probe_grid(wl, pkg):
    s, p, out, pt, ref = _solved(wl, pkg, "mini", "list")
    rng = np.random.default_rng(29)
    # 16 trials of a three-site guest (a CO2-like rod of types 1-2-1), the odd trials re-insertions of a molecule of the box
    centre = rng.uniform(0, 20.0, (16, 1, 3))
    u = rng.normal(size=(16, 1, 3))
    u /= np.linalg.norm(u, axis=2)[:, :, None]
    sites = centre + np.array([-1.16, 0.0, 1.16])[None, :, None] * u
    typ, q, al = np.array([1, 2, 1]), np.array([-0.35, 0.7, -0.35]), np.array([0.85, 1.2, 0.85])
    mol = np.where(np.arange(16) % 2 == 1, rng.integers(1, 19, 16), 0).astype(np.int32)
    ins = p.insertion_energy(sites, typ, q, al, molecule=mol)
    flat = p.probe_at(sites.reshape(-1, 3), np.tile(typ, 16), np.tile(q, 16), np.tile(al, 16), None, np.repeat(mol, 3))
    for k in ("e_lj", "e_coul", "e_pol"):
        assert ins[k].shape == (16,) and np.array_equal(ins[k], flat[k].reshape(16, 3).sum(axis=1)), k
    assert np.array_equal(ins["energy"], ins["e_lj"] + ins["e_coul"] + ins["e_pol"]) and np.max(np.abs(ins["e_lj"])) > 0
    one = p.insertion_energy(sites[:2], 1, 0.0, 0.0, skip_atom=[3, -1])
    assert one["e_lj"].shape == (2,)
    g = p.probe_grid((5, 4, 3), 2, q=0.2, alpha=0.5)
    assert g["e_lj"].shape == g["e_coul"].shape == g["e_pol"].shape == g["energy"].shape == (3, 4, 5) and g["e_total"].shape == (3, 4, 5, 3)
    gp = p.grid_points((5, 4, 3))
    fl = p.probe_at(gp, 2, 0.2, 0.5)
    for k in ("e_lj", "e_coul", "e_pol", "energy", "e_total"):
        assert np.array_equal(g[k].reshape(fl[k].shape), fl[k]), k
    first, last = p.probe_at(gp[:1], 2, 0.2, 0.5), p.probe_at(gp[-1:], 2, 0.2, 0.5)
    assert g["energy"][0, 0, 0] == first["energy"][0] and g["energy"][2, 3, 4] == last["energy"][0]
    assert np.allclose(gp[0], np.asarray(s.boxlo) + np.asarray(s.prd) * [0.1, 0.125, 1 / 6], rtol=0, atol=1e-12)
