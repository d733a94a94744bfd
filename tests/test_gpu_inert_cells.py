"""The cell order with the inert sites behind the grid (build_cells, csrc/polar_step.hip) against the order that keeps them
between the others (`POLAR_CELL_INERT=0`, read when a handle is created), on the same inputs in the product library.

With the split on, an inert site (q == 0 and alpha == 0) is binned to a second copy of the list grid that no candidate walk
visits.  The sequence of the other atoms in cell order is unchanged -- the inert ones only vanish from between them -- so every
full-list and dipole-list row holds the same atoms in the same order, the colour phases hold the same rows in the same order,
and with `deterministic yes`, `fixed_iteration yes`, `use_previous no` the dipoles, the static field and every count come out
in the same bits: np.array_equal / ==, the groups of tests/test_gpu_nl_dense_trips.py (_assert_same_bits).  Forces, the virial
and the energies are accumulated with floating-point atomics and do not repeat bit for bit even between two runs of one
handle: they are held to that file's run-to-run bound (1e-12 of the largest entry).  eng_vdwl belongs to them here: it is the
one of that file's "exact" scalars that is known to differ in its last bit between two handles.

polar_pair_extract("cell_active") -- the atoms the last cell build filed in the grid's own bins -- shows that each handle
really took its order: all atoms with the split off, the atoms that are not inert with it on.

Every case is also run to convergence with the split on and compared with the CPU oracle at the tolerances of
tests/test_gpu_inert_sites.py (1e-7 on dipoles, forces, energies and virial, 1e-9 on the static field); for the 10,792-atom
replica the oracle's recorded result holds forces, dipoles and eng_pol only, and polar_field_at is compared with the NumPy
brute force of tests/test_gpu_field_at.py at that file's 1e-10 of a point's scale."""
import contextlib
import copy
import importlib
import os

import numpy as np
import pytest

import test_gpu_field_at as tfa
import test_gpu_inert_sites as tis
import test_gpu_nl_dense_trips as tdt
from helpers import force_rel_err, rel

pytestmark = pytest.mark.gpu

TOL = tis.TOL                     # against the oracle
RUN_TO_RUN = tdt.RUN_TO_RUN       # between two handles, for what is summed with atomics
FIXED, CUT, MOF = tdt.FIXED, tdt.CUT, tdt.MOF
EXACT_ARRAYS = ("mu", "ef_static")
EXACT_SCALARS = ("sweeps", "ncolors", "status", "dd_pairs", "nl_entries", "force_rows")
ATOMIC_ARRAYS = ("f", "virial")
ATOMIC_SCALARS = ("eng_pol", "eng_coul", "eng_vdwl")


# ---- handles ----------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _env(pairs):
    old = {k: os.environ.get(k) for k, _ in pairs}
    try:
        for k, v in pairs:
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _plain(p):
    return p.compute(eflag=1, vflag=2)


def _counters(p, out):
    for k in ("nl_entries", "force_rows", "cell_active", "nl_dense"):
        out[k] = p.extract(k)
    return out


def _run(pkg, s, split, scenario=_plain, setup=None, env=(), lab=False, row_range=None):
    """One handle with the inert sites behind the grid (the default) or created under POLAR_CELL_INERT=0.  The environment
    spans the whole scenario: POLAR_INIT_PITCH is read by the first list build, not by polar_create."""
    pairs = [("POLAR_CELL_INERT", None if split else "0"), ("POLAR_NL_INERT", None), ("POLAR_NL_DENSE", None)] + list(env)
    with _env(pairs):
        p = pkg.pair_from_system(s, lab=lab, row_range=row_range)
        try:
            if setup is not None:
                setup(p)
            return _counters(p, scenario(p))
        finally:
            p.close()


def _inert(s):
    n = s.nlocal
    return (s.q[:n] == 0.0) & (s.alpha[:n] == 0.0)


def _assert_orders(s, on, off):
    """each handle took its order: the grid's own bins hold every atom, or the ones that are not inert"""
    n, nin = s.nlocal, int(_inert(s).sum())
    print("    cell_active: split on %d, off %d of %d atoms (%d inert)" % (on["cell_active"], off["cell_active"], n, nin))
    assert off["cell_active"] == n and on["cell_active"] == n - nin


def _assert_same_bits(name, on, off):
    for k in EXACT_ARRAYS + ATOMIC_ARRAYS:
        a, b = np.asarray(on[k]), np.asarray(off[k])
        print("%s: %-9s max |split - no split| %.3e of %.3e" % (name, k, np.max(np.abs(a - b)), np.max(np.abs(b))))
    for k in EXACT_SCALARS + ATOMIC_SCALARS:
        print("%s: %-10s split %r  no split %r" % (name, k, on[k], off[k]))
    assert on["dd_pairs"] > 0 and on["nl_entries"] > 0                       # the comparison is not empty
    for k in EXACT_ARRAYS:
        assert np.array_equal(np.asarray(on[k]), np.asarray(off[k])), k
    for k in EXACT_SCALARS:
        assert on[k] == off[k], k
    for k in ATOMIC_ARRAYS:
        assert np.max(np.abs(np.asarray(on[k]) - np.asarray(off[k]))) <= RUN_TO_RUN * np.max(np.abs(np.asarray(off[k]))), k
    for k in ATOMIC_SCALARS:
        assert abs(on[k] - off[k]) <= RUN_TO_RUN * abs(off[k]), k


def _ab(name, pkg, s, **kw):
    on, off = _run(pkg, s, True, **kw), _run(pkg, s, False, **kw)
    _assert_same_bits(name, on, off)
    return on, off


def _assert_oracle(name, out, ref, s):
    """tests/test_gpu_inert_sites.py::_oracle_ok, with its figures printed first"""
    from oracle import oracle
    f = oracle.fold_ghost_forces(out["f"], s.owner, s.nlocal)
    fr = oracle.fold_ghost_forces(ref["f"], s.owner, s.nlocal)
    print("%s: against the oracle: forces %.2e  dipoles %.2e  static field %.2e  eng_pol %.2e" % (
        name, force_rel_err(f, fr), np.max(np.abs(out["mu"] - ref["mu"])) / max(np.max(np.abs(ref["mu"])), 1e-30),
        np.max(np.abs(out["ef_static"] - ref["ef_static"])) / max(np.max(np.abs(ref["ef_static"])), 1e-30), rel(out["eng_pol"], ref["eng_pol"], 1e-9)))
    assert ref["status"] == 0
    tis._oracle_ok(out, ref, s)


# ---- the systems ------------------------------------------------------------------------------------------------------
def _retyped(s, inert=(), charged=()):
    """the system with the sites `inert` stripped of charge and polarizability and the sites `charged` of their
    polarizability alone (no ghosts in these systems)"""
    assert s.nghost == 0
    s2 = copy.copy(s)
    q, a = s.q.copy(), s.alpha.copy()
    q[list(inert)] = 0.0
    a[list(inert)] = 0.0
    a[list(charged)] = 0.0
    assert not np.any(q[list(charged)] == 0.0)
    s2.q, s2.alpha = np.ascontiguousarray(q), np.ascontiguousarray(a)
    return s2


def _cells_320(x):
    """cell of every atom in the list grid of the 24 x 24 x 30 box at cutoff 9 (list_grid: floor(width / 4.5) = 5 x 5 x 6)"""
    nc = np.array([5, 5, 6])
    c = np.minimum((x / np.array([24.0, 24.0, 30.0]) * nc).astype(np.int64), nc - 1)
    return (c[:, 2] * nc[1] + c[:, 1]) * nc[0] + c[:, 0]


def _slab_kinds(s):
    """The 320-atom system of tests/test_gpu_nl_dense_trips.py with three kinds of site: every atom of its fullest cell inert,
    the next fullest cell without an inert atom, a quarter of the others inert and a tenth of the polarizable ones charged only."""
    rng = np.random.default_rng(320)
    n = s.nlocal
    cell = _cells_320(s.x[:n])
    order = np.argsort(-np.bincount(cell, minlength=150), kind="stable")
    c_inert, c_none = int(order[0]), int(order[1])
    rest = np.flatnonzero((cell != c_inert) & (cell != c_none))
    pick = rng.permutation(rest)
    inert = np.concatenate([np.flatnonzero(cell == c_inert), pick[:len(rest) // 4]])
    pol = [i for i in pick[len(rest) // 4:] if s.alpha[i] != 0.0]
    s2 = _retyped(s, inert=inert, charged=pol[:len(pol) // 10])
    ine = _inert(s2)
    assert (cell == c_inert).sum() >= 3 and ine[cell == c_inert].all()
    assert (cell == c_none).sum() >= 3 and not ine[cell == c_none].any()
    assert 60 < ine.sum() < 120 and np.sum((s2.q[:n] != 0.0) & (s2.alpha[:n] == 0.0)) > 60 and np.sum(s2.alpha[:n] != 0.0) > 100
    return s2


def _slab_pair(wl):
    s, s_orc = tdt._slab(wl)
    s2 = _slab_kinds(s)
    s_orc2 = copy.copy(s_orc)
    s_orc2.q, s_orc2.alpha = s2.q, s2.alpha
    return s2, s_orc2


@pytest.fixture(scope="module")
def mof(wl, pkg, oracle):
    """the 1,349-atom cell in list mode, its oracle result and the converged product result: computed once, read below"""
    s = tdt._mof(wl, (1, 1, 1))
    sc = tdt._converging(s)
    return dict(s=s, sc=sc, ref=oracle.compute(sc, eflag=1, vflag=2), on=_run(pkg, s, True), conv=_run(pkg, sc, True))


# ---- the cases --------------------------------------------------------------------------------------------------------
def test_mof_cell_with_four_cells_per_dimension(mof, pkg):
    """dd_cutoff 12.8345 in the 25.669 A cell: 4 x 4 x 4 cells, every stencil row a whole row of cells, no second piece"""
    s = mof["s"]
    assert _inert(s).sum() == 370 and s.nlocal == 1349
    off = _run(pkg, s, False)
    _assert_orders(s, mof["on"], off)
    _assert_same_bits("mof5_1x1x1", mof["on"], off)
    _assert_oracle("mof5_1x1x1", mof["conv"], mof["ref"], mof["sc"])


def test_mof_replica_with_eight_cells_per_dimension(wl, pkg, oracle):
    """replicate 2 2 2: 10,792 atoms, +-2 stencil, trimmed rows, runs that wrap around the box"""
    s = tdt._mof(wl, (2, 2, 2))
    on, off = _ab("mof5_2x2x2", pkg, s)
    _assert_orders(s, on, off)
    sc = tdt._converging(s)
    tdt._assert_oracle("mof5_2x2x2", oracle, sc, _run(pkg, sc, True), ref=tdt._stored_oracle(sc, "2x2x2"))


def test_constructed_system_with_an_all_inert_cell_and_a_cell_without(wl, pkg, oracle):
    s = _slab_kinds(tdt._slab(wl)[0])                                        # (all three directions periodic here)
    on, off = _ab("320 atoms", pkg, s)
    _assert_orders(s, on, off)
    sc = tdt._converging(s)
    _assert_oracle("320 atoms", _run(pkg, sc, True), oracle.compute(sc, eflag=1, vflag=2), sc)


def test_system_without_an_inert_atom(wl, pkg, oracle):
    s = tdt._slab(wl)[0]
    assert not _inert(s).any()
    on, off = _ab("no inert atom", pkg, s)
    _assert_orders(s, on, off)
    sc = tdt._converging(s)
    _assert_oracle("no inert atom", _run(pkg, sc, True), oracle.compute(sc, eflag=1, vflag=2), sc)


def test_triclinic_box(wl, pkg, oracle):
    s = tdt._tilted(wl)
    rng = np.random.default_rng(90)
    pick = rng.permutation(s.nlocal)
    s = _retyped(s, inert=pick[:27], charged=[i for i in pick[27:] if s.alpha[i] != 0.0][:6])
    assert s.triclinic and _inert(s).sum() == 27
    on, off = _ab("tilted", pkg, s)
    _assert_orders(s, on, off)
    sc = tdt._converging(s)
    _assert_oracle("tilted", _run(pkg, sc, True), oracle.compute(sc, eflag=1, vflag=2), sc)


def test_box_with_a_non_periodic_direction(wl, pkg, oracle):
    s, s_orc = _slab_pair(wl)
    on, off = _ab("slab", pkg, s, setup=tdt._open_z)
    _assert_orders(s, on, off)
    per = _run(pkg, s, True)                                                 # the same atoms with z periodic: other lists
    assert per["dd_pairs"] > on["dd_pairs"]
    sc = tdt._converging(s)
    ref = oracle.compute(tdt._converging(s_orc), eflag=1, vflag=2)           # (a box 45 high: no pair reaches across z)
    _assert_oracle("slab", _run(pkg, sc, True, setup=tdt._open_z), ref, sc)


def test_pitch_overflow_retry(mof, pkg):
    """POLAR_INIT_PITCH=64: the first build overflows every row and the step is redone with a larger pitch"""
    s = mof["s"]
    forced = (("POLAR_INIT_PITCH", "64"),)
    on, off = _ab("pitch 64", pkg, s, env=forced)
    _assert_orders(s, on, off)
    _assert_same_bits("pitch 64 against an un-forced run", on, mof["on"])
    _assert_oracle("pitch 64", _run(pkg, mof["sc"], True, env=forced), mof["ref"], mof["sc"])


def test_reneighbor_step_with_the_colours_revalidated(mof, wl, pkg, oracle):
    """A second compute after set_atoms with positions moved by 0.01 A: cells are rebuilt, the list build re-validates the
    colouring in force (the RECHECK instance) and keeps it."""
    s = mof["s"]
    dx = np.random.default_rng(23).uniform(-0.01, 0.01, (s.nlocal, 3))
    s2 = copy.copy(s)
    s2.x = s.x + dx[s.owner]

    def scenario(p):
        p.compute(eflag=1, vflag=2)
        p.set_atoms(s2.nlocal, s2.nghost, s2.x, s2.q, s2.alpha, s2.type, s2.molecule)
        return p.compute(eflag=1, vflag=2)

    on, off = _ab("reneighbor", pkg, s, scenario=scenario)
    _assert_orders(s, on, off)
    assert on["ms_color_host"] == 0.0 and off["ms_color_host"] == 0.0        # colours kept in both
    assert not np.array_equal(mof["on"]["mu"], on["mu"])                     # the second step did see the moved atoms
    sc2 = tdt._converging(s2)
    _assert_oracle("reneighbor", _run(pkg, mof["sc"], True, scenario=scenario), oracle.compute(sc2, eflag=1, vflag=2), sc2)


def test_set_atoms_that_makes_inert_sites_charged_and_back(wl, pkg, oracle):
    """Three computes on one handle; polar_set_atoms gives forty inert sites a charge before the second and takes it away
    again before the third.  The bins are worked out from the resident q and alpha every step."""
    s = _slab_kinds(tdt._slab(wl)[0])
    n = s.nlocal
    flip = np.flatnonzero(_inert(s))[::2][:40]
    s2 = copy.copy(s)
    q = s.q.copy()
    q[flip] = np.where(np.arange(len(flip)) % 2 == 0, 0.2, -0.2)
    s2.q = np.ascontiguousarray(q)
    assert len(flip) == 40 and _inert(s2).sum() == _inert(s).sum() - 40

    def scenario(p):
        steps = []
        for t in (s, s2, s):
            p.set_atoms(t.nlocal, t.nghost, t.x, t.q, t.alpha, t.type, t.molecule)
            steps.append(_counters(p, p.compute(eflag=1, vflag=2)))
        return {"steps": steps, **steps[-1]}

    on, off = _run(pkg, s, True, scenario=scenario), _run(pkg, s, False, scenario=scenario)
    for k, t in enumerate((s, s2, s)):
        _assert_same_bits("set_atoms, step %d" % (k + 1), on["steps"][k], off["steps"][k])
        _assert_orders(t, on["steps"][k], off["steps"][k])
    a, b, c = on["steps"]
    assert b["nl_entries"] > a["nl_entries"] == c["nl_entries"] and b["force_rows"] == a["force_rows"] + 40 == c["force_rows"] + 40
    assert np.array_equal(a["ef_static"], c["ef_static"]) and not np.array_equal(a["ef_static"], b["ef_static"])
    sc, sc2 = tdt._converging(s), tdt._converging(s2)

    def conv(p):
        p.compute(eflag=1, vflag=2)
        p.set_atoms(sc2.nlocal, sc2.nghost, sc2.x, sc2.q, sc2.alpha, sc2.type, sc2.molecule)
        return p.compute(eflag=1, vflag=2)

    _assert_oracle("set_atoms", _run(pkg, sc, True, scenario=conv), oracle.compute(sc2, eflag=1, vflag=2), sc2)


def test_lab_library_per_run_walk_with_the_split_on(mof, pkg):
    """k_nl_build<.., DENSE = false> (the lab library under POLAR_NL_DENSE=0) reads the same cell_first: the same lists"""
    s = mof["s"]
    lab = _run(pkg, s, True, lab=True, env=(("POLAR_NL_DENSE", "0"),))
    assert lab["nl_dense"] == 0.0 and mof["on"]["nl_dense"] == 1.0
    assert lab["cell_active"] == mof["on"]["cell_active"] == s.nlocal - 370
    _assert_same_bits("lab per-run walk against the product", lab, mof["on"])
    _assert_oracle("lab per-run walk", _run(pkg, mof["sc"], True, lab=True, env=(("POLAR_NL_DENSE", "0"),)), mof["ref"], mof["sc"])


def test_row_sharded_handle(mof, wl, pkg, oracle):
    """A handle that owns half the rows (675 of 1,349), stepped through the stepwise interface, in both orders; then both
    halves in lock-step with the split on against the oracle (tests/test_gpu_nl_dense_trips.py::test_row_sharded_handle)."""
    import test_gpu_parity as tgp
    par = importlib.import_module(pkg.__name__ + ".parallel")
    own = np.arange(0, 675)
    sg = wl.replicate_fixture(MOF, 1, 1, 1, extra_args=FIXED + ["dd_cutoff", CUT], rows=own, full=True)
    nall = sg.nlocal + sg.nghost

    def scenario(p):
        be = par.HipShardBackend(p, int(own[0]), int(own[-1]) + 1, 0)
        be.begin(1, 2)
        for _ in range(be.max_it + 1):
            be.sweep()
            be.sweep_end(None)
        out = be.finish()
        out["f"] = p.download("f", 3 * nall).reshape(-1, 3)
        out["mu"] = p.download("mu", 3 * sg.nlocal).reshape(-1, 3)
        out["ef_static"] = p.download("ef_static", 3 * sg.nlocal).reshape(-1, 3)[own]   # (rows of other shards are never computed here)
        return out

    on, off = _ab("half the rows", pkg, sg, scenario=scenario)
    _assert_orders(sg, on, off)
    assert np.any(on["mu"][:675]) and not np.any(on["f"][675:sg.nlocal])     # the shard worked on its rows and on no others
    assert on["force_rows"] == 675 - _inert(sg)[:675].sum()
    ef_ref = mof["ref"]["ef_static"]                                         # the static field needs no dipole of the other half
    assert np.max(np.abs(on["ef_static"] - ef_ref[own])) < 1e-9 * np.max(np.abs(ef_ref))
    conv = ["use_previous", "no", "precision", "1e-12", "max_iterations", "200", "deterministic", "yes", "dd_cutoff", CUT]
    sf = tgp._full_list_system(wl, "mof5_h2", conv)
    offs = [0, 675, sf.nlocal]
    bes = []
    with _env([("POLAR_CELL_INERT", None), ("POLAR_NL_INERT", None)]):
        for r in range(2):
            p = pkg.pair_from_system(sf)
            p.set_neighbors_csr(np.arange(offs[r], offs[r + 1]).astype(np.int32), sf.extra["full_numneigh"], sf.extra["full_first"], sf.extra["full_neigh"])
            bes.append(par.HipShardBackend(p, offs[r], offs[r + 1], 0))
    try:
        def exchange():                                                      # every shard receives the other one's own dipoles
            mine = [be.own_mu().clone() for be in bes]
            bes[0].set_mu(offs[1], offs[2], mine[1])
            bes[1].set_mu(offs[0], offs[1], mine[0])

        for be in bes:
            be.begin(1, 2)
        exchange()
        for sw in range(bes[0].max_it + 1):
            for be in bes:
                be.sweep()
            total = sum(be.local_change().clone() for be in bes)
            for be in bes:
                be.sweep_end(total)
            exchange()
            if sw % 4 == 3 and all(be.state()[0] for be in bes):
                break
        outs = [be.finish() for be in bes]
        f, mu = np.zeros((sf.nlocal, 3)), np.zeros((sf.nlocal, 3))
        for r, be in enumerate(bes):
            assert be.pair.extract("cell_active") == sf.nlocal - 370
            f[offs[r]:offs[r + 1]] = be.pair.download("f", 3 * (sf.nlocal + sf.nghost)).reshape(-1, 3)[offs[r]:offs[r + 1]]
            mu[offs[r]:offs[r + 1]] = be.pair.download("mu", 3 * sf.nlocal).reshape(-1, 3)[offs[r]:offs[r + 1]]
    finally:
        for be in bes:
            be.pair.close()
    sh = wl.load_fixture(MOF, extra_args=conv)[0]
    ref = oracle.compute(sh, eflag=1, vflag=2)
    e_f = force_rel_err(f, oracle.fold_ghost_forces(ref["f"], sh.owner, sh.nlocal))
    e_mu = np.max(np.abs(mu - ref["mu"])) / np.max(np.abs(ref["mu"]))
    print("two half shards against the oracle: forces %.2e  dipoles %.2e  (bound %.0e)" % (e_f, e_mu, TOL))
    assert e_f < TOL and e_mu < TOL
    assert rel(sum(o["eng_pol"] for o in outs), ref["eng_pol"]) < TOL


def test_field_at_on_64_points_in_both_orders(wl, pkg):
    """polar_field_at walks the records of a point's stencil through cell_first: with the split on it meets no inert record
    (each would add an exact zero) and its lanes take the others in other places, so the sums differ in their rounding --
    held to the bound of tests/test_gpu_field_at.py, 1e-10 of a point's scale, between the orders and against NumPy."""
    s = tfa._system(wl, "mof5_h2", "list", None, "exponential")
    pts, skip, pmol = tfa._points(s)
    sel = np.r_[0:40, 200:208, 220:228, 249:257]                             # inside the box, outside it, 0.3 A from an atom, on atoms
    pts, skip, pmol = np.ascontiguousarray(pts[sel]), np.ascontiguousarray(skip[sel]), np.ascontiguousarray(pmol[sel])
    assert len(pts) == 64
    got = {}

    def scenario(p):
        out = p.compute(eflag=1, vflag=2)
        assert out["status"] == 0 and out["rms_dmu"] <= 1e-13
        out["field"] = p.field_at(pts, skip, pmol)
        return out

    for split in (True, False):
        got[split] = _run(pkg, s, split, scenario=scenario)
    _assert_orders(s, got[True], got[False])
    ref = tfa._reference(s, got[True], pts, skip, pmol)
    for k in tfa.NAMES:
        v, sc = ref[k]
        a, b = got[True]["field"][k], got[False]["field"][k]
        safe = np.where(sc > 0, sc, 1.0)
        print("field_at %-11s max |split - no split| / scale %.2e   max |split - numpy| / scale %.2e" % (
            k, np.max(np.abs(a - b) / safe), np.max(np.abs(a - v) / safe)))
        assert np.max(sc) > 0.0
        assert np.all(np.abs(a - b) <= 1e-10 * sc), k
        assert np.all(np.abs(a - v) <= 1e-10 * sc), k
