"""Dense candidate trips of the list build (k_nl_build<.., DENSE = true>, the product library) against the per-run walk they
replaced (DENSE = false: the lab library with POLAR_NL_DENSE=0), on the same inputs.

Only the enumeration of the candidates differs: the same candidates in the same order go through the same per-candidate code,
so every list comes out entry for entry the same.  With `deterministic yes`, `fixed_iteration yes`, `use_previous no` two runs
on identical lists agree bit for bit in the dipoles, the static field and every count, which are compared with np.array_equal
/ ==, not with a tolerance: a reordered, lost or duplicated candidate changes a rounding or a count.  (Forces, virial, eng_pol
and eng_coul do not repeat bit for bit even within one library: see ATOMIC below.)  Every case is also run to convergence in
the product library and compared with the CPU oracle under the suite's parity bound (1e-7 on dipoles and forces), so that the
two paths cannot agree by being wrong in the same way."""
import copy
import dataclasses
import importlib
import os

import numpy as np
import pytest

import closest_image_ref as cir
from helpers import GOLD, force_rel_err, rel

pytestmark = pytest.mark.gpu

TOL = 1e-7                    # the suite's parity bound against the oracle (tests/test_gpu_parity.py, tests/test_gpu_edges.py)
CUT = "12.8345"
FIXED = ["use_previous", "no", "fixed_iteration", "yes", "max_iterations", "10", "deterministic", "yes"]
MOF = os.path.join(GOLD, "mof5_h2.npz")
ARRAYS = ("f", "mu", "ef_static", "virial")
SCALARS = ("eng_pol", "eng_coul", "eng_vdwl", "dd_pairs", "sweeps", "ncolors")
# Forces, virial and the two energies below are accumulated with floating-point atomics whose order changes from run to
# run: two runs of ONE library on the same input differ in them (measured on the MI355X, product against product and lab
# against lab alike: f 7e-15 of 1.4 on bulk_h2, 2e-14 of 6.9 on mof5_h2, 1.2e-10 of 5.4e5 on the 2 x 1 x 1 replica; virial
# 4e-13 of 16 and 9e-13 of 109; eng_coul 6e-14 of 1e4; eng_pol 3e-17 of 0.11), while mu, ef_static, eng_vdwl, dd_pairs,
# sweeps and ncolors repeat in every bit.  The bit-for-bit comparison therefore covers the second group -- every dipole
# after eleven sweeps over the dd lists, every static field summed over the nl lists in list order, every count -- and
# the first group is held to the run-to-run bound the suite already uses for these settings
# (tests/test_gpu_parity.py::test_deterministic_keyword_gives_bit_identical_runs: 1e-12 of the largest entry).
ATOMIC = ("f", "virial", "eng_pol", "eng_coul")
RUN_TO_RUN = 1e-12


def _converging(s):
    """the same system under the reference's stop rule at 1e-12 (for the comparison with the oracle)"""
    s2 = copy.copy(s)
    s2.settings = dataclasses.replace(s.settings, fixed_iteration=0, polar_precision=1e-12, iterations_max=200)
    return s2


def _stored_oracle(s, tag):
    """The oracle's result for the replicated boxes, recorded by tests/golden/make_nl_dense_ref.py (5 s and 20 s of CPU time)."""
    z = np.load(os.path.join(GOLD, "oracle_list_mof5_replicas.npz"))
    assert np.array_equal(z["x_" + tag], s.x[:s.nlocal].astype(np.float32))      # the same atoms in the same order
    f = np.zeros((s.nlocal + s.nghost, 3))
    f[:s.nlocal] = z["f_" + tag]
    return {"f": f, "mu": z["mu_" + tag], "eng_pol": float(z["eng_pol_" + tag]), "status": 0}


def _plain(p):
    return p.compute(eflag=1, vflag=2)


def _run(pkg, s, lab, monkeypatch, scenario=_plain, setup=None, env=()):
    """One handle of the product library (dense trips) or of the lab library with POLAR_NL_DENSE=0 (per-run walk)."""
    for k, v in env:
        monkeypatch.setenv(k, v)
    if lab:
        monkeypatch.setenv("POLAR_NL_DENSE", "0")
    try:
        p = pkg.pair_from_system(s, lab=lab)
        try:
            if setup is not None:
                setup(p)
            out = scenario(p)
            out["nl_dense"] = p.extract("nl_dense")
            return out
        finally:
            p.close()
    finally:
        monkeypatch.delenv("POLAR_NL_DENSE", raising=False)
        for k, _ in env:
            monkeypatch.delenv(k, raising=False)


def _assert_same_bits(name, new, old):
    for k in ARRAYS:
        a, b = np.asarray(new[k]), np.asarray(old[k])
        print("%s: %-9s max |dense - per-run| %.3e of %.3e" % (name, k, np.max(np.abs(a - b)) if a.size else 0.0, np.max(np.abs(b)) if b.size else 0.0))
    for k in SCALARS:
        print("%s: %-9s dense %r  per-run %r" % (name, k, new[k], old[k]))
    assert new["status"] == old["status"]
    assert new["dd_pairs"] > 0                                   # the comparison is not empty
    for k in ARRAYS:
        if k in ATOMIC:
            assert np.max(np.abs(np.asarray(new[k]) - np.asarray(old[k]))) <= RUN_TO_RUN * np.max(np.abs(np.asarray(old[k]))), k
        else:
            assert np.array_equal(np.asarray(new[k]), np.asarray(old[k])), k
    for k in SCALARS:
        if k in ATOMIC:
            assert abs(new[k] - old[k]) <= RUN_TO_RUN * abs(old[k]), k
        else:
            assert new[k] == old[k], k


def _assert_paths(new, old):
    """the product run walked dense trips, the lab run really took the per-run walk (the flag is set by the launch itself)"""
    assert new["nl_dense"] == 1.0 and old["nl_dense"] == 0.0


def _assert_oracle(name, oracle, s, out, ref=None):
    ref = oracle.compute(s, eflag=1, vflag=2) if ref is None else ref
    f = oracle.fold_ghost_forces(out["f"], s.owner, s.nlocal)
    fr = oracle.fold_ghost_forces(ref["f"], s.owner, s.nlocal)
    e_f = force_rel_err(f, fr)
    e_mu = np.max(np.abs(out["mu"] - ref["mu"])) / np.max(np.abs(ref["mu"]))
    print("%s: against the oracle: forces %.2e  dipoles %.2e  eng_pol %.2e  (bound %.0e)" % (name, e_f, e_mu, rel(out["eng_pol"], ref["eng_pol"]), TOL))
    assert out["status"] == ref["status"] == 0
    assert e_f < TOL and e_mu < TOL
    assert rel(out["eng_pol"], ref["eng_pol"]) < TOL


# ---- the systems -----------------------------------------------------------------------------------------------------

def _mof(wl, reps):
    if reps == (1, 1, 1):
        return wl.load_fixture(MOF, extra_args=FIXED + ["dd_cutoff", CUT])[0]
    return wl.replicate_fixture(MOF, *reps, extra_args=FIXED + ["dd_cutoff", CUT])


def _bulk(wl):
    return wl.load_fixture(os.path.join(GOLD, "bulk_h2.npz"), extra_args=FIXED + ["dd_cutoff", "9.0"])[0]


def _tilted(wl):
    """the recorded 90-atom system in the 16 A cell with tilt (tests/test_gpu_closest_image.py), cutoffs just below half its
    smallest perpendicular width: the TRI instance, trimming off"""
    sd = cir.system("t8")
    cut = 0.999 * 0.5 * cir.widths(sd["prd"], sd["tilt"]).min()
    return cir.mini_system(wl, sd["x"], sd["prd"], sd["tilt"], 1, cut, extra=FIXED + ["dd_cutoff", repr(float(cut))])


def _slab(wl):
    """320 atoms on a jittered 3 A lattice filling a 24 x 24 x 30 box that is not periodic in z (6 cells along z: the stencil
    rows beyond the two faces are dropped; image arithmetic with inverse length 0 along z).  The oracle knows periodic
    boxes only: it gets the same atoms in a box 45 high, where no pair within the 9 A cutoff reaches across z."""
    rng = np.random.default_rng(17)
    g = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(10), indexing="ij"), -1).reshape(-1, 3)
    x = (g[rng.permutation(len(g))[:320]] + 0.5) * 3.0 + rng.uniform(-0.45, 0.45, (320, 3))    # nearest approach >= 2.1 A
    extra = FIXED + ["dd_cutoff", "9.0"]
    s = cir.mini_system(wl, x, (24.0, 24.0, 30.0), (0.0, 0.0, 0.0), 0, 9.0, extra=extra)
    s_orc = cir.mini_system(wl, x, (24.0, 24.0, 45.0), (0.0, 0.0, 0.0), 0, 9.0, extra=extra)
    assert np.array_equal(s.q, s_orc.q) and np.array_equal(s.alpha, s_orc.alpha)
    return s, s_orc


def _open_z(p):
    p.set_box((0.0, 0.0, 0.0), (24.0, 24.0, 30.0), periodic=(1, 1, 0))


CASES = {
    "mof5_1x1x1": lambda wl: _mof(wl, (1, 1, 1)),      # 4 cells per dimension: whole rows of cells, no second piece
    "bulk_h2": _bulk,                                  # box = 2 x cutoff exactly
    "mof5_2x1x1": lambda wl: _mof(wl, (2, 1, 1)),      # cells 8 x 4 x 4: +-2 stencil with wrapped second pieces in x only
    "mof5_2x2x2": lambda wl: _mof(wl, (2, 2, 2)),      # 8 cells each way: trimmed rows, two-piece runs, runs shorter and longer than 64
    "tilted": _tilted,
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_dense_trips_give_the_bits_of_the_per_run_walk(case, wl, pkg, oracle, monkeypatch):
    s = CASES[case](wl)
    new = _run(pkg, s, False, monkeypatch)
    old = _run(pkg, s, True, monkeypatch)
    _assert_paths(new, old)
    _assert_same_bits(case, new, old)
    sc = _converging(s)
    ref = _stored_oracle(sc, case[5:]) if case in ("mof5_2x1x1", "mof5_2x2x2") else None
    _assert_oracle(case, oracle, sc, _run(pkg, sc, False, monkeypatch), ref=ref)


def test_box_with_a_non_periodic_direction(wl, pkg, oracle, monkeypatch):
    s, s_orc = _slab(wl)
    new = _run(pkg, s, False, monkeypatch, setup=_open_z)
    old = _run(pkg, s, True, monkeypatch, setup=_open_z)
    _assert_paths(new, old)
    _assert_same_bits("slab", new, old)
    per = _run(pkg, s, False, monkeypatch)                        # the same atoms with z periodic: other lists, other numbers
    assert per["dd_pairs"] > new["dd_pairs"]
    sc = _converging(s)
    ref = oracle.compute(_converging(s_orc), eflag=1, vflag=2)
    _assert_oracle("slab", oracle, sc, _run(pkg, sc, False, monkeypatch, setup=_open_z), ref=ref)


def test_pitch_overflow_retry_gives_the_bits_of_an_unforced_run(wl, pkg, oracle, monkeypatch):
    """POLAR_INIT_PITCH=64: the first build overflows every row (true counts returned, writes stopped at the pitch) and the
    step is redone with a larger pitch."""
    s = _mof(wl, (1, 1, 1))
    free = _run(pkg, s, False, monkeypatch)
    forced = (("POLAR_INIT_PITCH", "64"),)
    new = _run(pkg, s, False, monkeypatch, env=forced)
    old = _run(pkg, s, True, monkeypatch, env=forced)
    _assert_paths(new, old)
    _assert_same_bits("pitch 64, dense against per-run", new, old)
    _assert_same_bits("pitch 64 against an un-forced run", new, free)
    sc = _converging(s)
    _assert_oracle("pitch 64", oracle, sc, _run(pkg, sc, False, monkeypatch, env=forced))


def test_reneighbor_step_keeps_the_colours_and_the_bits(wl, pkg, oracle, monkeypatch):
    """A second compute after set_atoms with positions moved by 0.01 A: the list build re-validates the colouring in force
    (the RECHECK instance) and keeps it."""
    s = _mof(wl, (1, 1, 1))
    dx = np.random.default_rng(23).uniform(-0.01, 0.01, (s.nlocal, 3))
    s2 = copy.copy(s)
    s2.x = s.x + dx[s.owner]                                     # ghosts move with their owners

    def scenario(p):
        p.compute(eflag=1, vflag=2)
        p.set_atoms(s2.nlocal, s2.nghost, s2.x, s2.q, s2.alpha, s2.type, s2.molecule)    # no new LJ / Coulomb list: inside its skin
        return p.compute(eflag=1, vflag=2)

    new = _run(pkg, s, False, monkeypatch, scenario=scenario)
    old = _run(pkg, s, True, monkeypatch, scenario=scenario)
    _assert_paths(new, old)
    _assert_same_bits("reneighbor", new, old)
    assert new["ms_color_host"] == 0.0 and old["ms_color_host"] == 0.0       # colours kept in both
    first = _run(pkg, s, False, monkeypatch)
    assert not np.array_equal(first["mu"], new["mu"])                        # the second step did see the moved atoms
    sc = _converging(s)
    sc2 = _converging(s2)
    conv = _run(pkg, sc, False, monkeypatch, scenario=scenario)
    _assert_oracle("reneighbor", oracle, sc2, conv)


def test_row_sharded_handle(wl, pkg, oracle, monkeypatch):
    """A handle that owns half the rows (675 of 1,349: not a multiple of the four rows of a workgroup), stepped through the
    stepwise interface; then both halves in lock-step against the oracle."""
    import test_gpu_parity as tgp
    par = importlib.import_module(pkg.__name__ + ".parallel")
    args = FIXED + ["dd_cutoff", CUT]
    own = np.arange(0, 675)
    sg = wl.replicate_fixture(MOF, 1, 1, 1, extra_args=args, rows=own, full=True)
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
        # (the static field of the own rows only: the rows of other shards are never computed on this handle and their
        # slots hold whatever the allocation held)
        out["ef_static"] = p.download("ef_static", 3 * sg.nlocal).reshape(-1, 3)[own]
        return out

    new = _run(pkg, sg, False, monkeypatch, scenario=scenario)
    old = _run(pkg, sg, True, monkeypatch, scenario=scenario)
    _assert_paths(new, old)
    _assert_same_bits("half the rows", new, old)
    assert np.any(new["mu"][:675]) and not np.any(new["f"][675:sg.nlocal])   # the shard worked on its rows and on no others
    conv = ["use_previous", "no", "precision", "1e-12", "max_iterations", "200", "deterministic", "yes", "dd_cutoff", CUT]
    sf = tgp._full_list_system(wl, "mof5_h2", conv)                          # full (newton-off) LJ / Coulomb rows for every atom
    offs = [0, 675, sf.nlocal]
    bes = []
    for r in range(2):
        p = pkg.pair_from_system(sf)
        p.set_neighbors_csr(np.arange(offs[r], offs[r + 1]).astype(np.int32), sf.extra["full_numneigh"], sf.extra["full_first"], sf.extra["full_neigh"])
        bes.append(par.HipShardBackend(p, offs[r], offs[r + 1], 0))

    def exchange():                                                          # every shard receives the other one's own dipoles
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
        f[offs[r]:offs[r + 1]] = be.pair.download("f", 3 * (sf.nlocal + sf.nghost)).reshape(-1, 3)[offs[r]:offs[r + 1]]
        mu[offs[r]:offs[r + 1]] = be.pair.download("mu", 3 * sf.nlocal).reshape(-1, 3)[offs[r]:offs[r + 1]]
        be.pair.close()
    tot = {"eng_pol": sum(o["eng_pol"] for o in outs)}
    sh = wl.load_fixture(MOF, extra_args=conv)[0]
    ref = oracle.compute(sh, eflag=1, vflag=2)
    e_f = force_rel_err(f, oracle.fold_ghost_forces(ref["f"], sh.owner, sh.nlocal))
    e_mu = np.max(np.abs(mu - ref["mu"])) / np.max(np.abs(ref["mu"]))
    print("two half shards against the oracle: forces %.2e  dipoles %.2e  (bound %.0e)" % (e_f, e_mu, TOL))
    assert e_f < TOL and e_mu < TOL
    assert rel(tot["eng_pol"], ref["eng_pol"]) < TOL
