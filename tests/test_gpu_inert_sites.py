"""Inert sites (q == 0 and alpha == 0: LJ-only sites) are left out of the library's full list and their force rows are skipped.

Such a site adds an exact zero to the static field, the polarization force and the rank metric (tests/test_inert_host.py pins
that on the pair function), so k_nl_build writes no entry for it and k_polar_force leaves a row whose atom is inert before
its first list access.  `POLAR_NL_INERT=0` (read when a handle is created) keeps every partner and every row: the A/B
partner.  Checked here through the C-ABI:

  * a mixed random system (30 % inert, 10 % charged only, 10 % polarizable without charge, the rest both; rows of one to three
    64-entry trips, some of which lose a trip to the drop) against the oracle at the tolerances of tests/test_gpu_fuzz.py, and against a
    handle created under POLAR_NL_INERT=0 at the bound tests/test_gpu_lj_skin.py uses between two handles that add the same
    pairs in another order (1e-12 of the largest magnitude);
  * polar_pair_extract("nl_entries" / "force_rows") against NumPy brute force under the minimum image: integers, compared exactly;
  * constructed rows of exactly 63, 64, 65 and 0 listed partners, each with inert partners inside the cutoff as well;
  * one case each: no damping, pairwise plus per-atom virial, the lab library's literal pair form, polar_ewald, a triclinic box, `debug yes` with an inert atom 0,
    a system without an inert site; and polar_set_atoms that makes an inert atom charged and a charged atom inert.
The oracle knows neither polar_ewald nor the switch: that variant is compared with the switch-off handle alone."""
import copy
import os

import numpy as np
import pytest

from helpers import force_rel_err, rel

pytestmark = pytest.mark.gpu

TOL = 1e-7     # against the oracle: tests/test_gpu_fuzz.py
AB = 1e-12     # between the two handles: tests/test_gpu_lj_skin.py
CUT, DDCUT = 7.0, 6.0
GS = ["polar_gs_ranked", "yes", "precision", "1e-12", "max_iterations", "200"]


def _kinds(rng, q, alpha, inert=0.30, charged=0.10, polar_q0=0.10):
    """q and alpha with the given fractions of inert / charged-only / polarizable-without-charge sites.  Polarizabilities are
    only ever taken away (the generator's polarizable sites are where a solve converges), charges are kept or cleared."""
    n = len(q)
    q, alpha = q.copy(), alpha.copy()
    pol = np.flatnonzero(alpha != 0.0)
    have_inert = int(np.sum((q == 0.0) & (alpha == 0.0)))
    pick = rng.permutation(pol)
    n_in = max(int(round(inert * n)) - have_inert, 0)
    n_ch, n_pq = int(round(charged * n)), int(round(polar_q0 * n))
    a, b, c = pick[:n_in], pick[n_in:n_in + n_ch], pick[n_in + n_ch:n_in + n_ch + n_pq]
    q[a] = 0.0; alpha[a] = 0.0
    alpha[b] = 0.0
    q[b] = np.where(q[b] == 0.0, 0.3, q[b])
    q[c] = 0.0
    ch = q != 0.0
    q[ch] -= q[ch].mean()
    assert not np.any(q[ch] == 0.0)
    return q, alpha


def _mixed(wl, extra=(), seed=5, inert=0.30, inert_first=False):
    """~600 atoms of the synthetic generator in its 19.6 A periodic box, with ghosts and the LJ / Coulomb half list.
    inert_first: atom 0 changes places with the first inert atom."""
    rng = np.random.default_rng(4000 + seed)
    d = wl.synth(600, seed=seed)
    if inert > 0:
        q, alpha = _kinds(rng, d["q"], d["alpha"], inert=inert)
    else:   # no inert site at all: the generator's LJ-only sites get a charge
        q, alpha = d["q"].copy(), d["alpha"].copy()
        z = (q == 0.0) & (alpha == 0.0)
        q[z] = rng.uniform(0.05, 0.3, int(z.sum())) * rng.choice([-1.0, 1.0], int(z.sum()))
        q -= q.mean()
        assert not np.any((q == 0.0) & (alpha == 0.0))
    assert 0.49 * d["prd"].min() - 1.0 > CUT
    perm = np.arange(len(q))
    if inert_first:
        k = int(np.flatnonzero((q == 0.0) & (alpha == 0.0))[0])
        perm[0], perm[k] = k, 0
    args = ["2.5", repr(CUT), "use_previous", "no", "damp_type", "exponential", "damp", "2.1304", "dd_cutoff", repr(DDCUT)] + GS + list(extra)
    st = wl.parse_pair_style_args(args)
    g = wl.ewald_g(1.0e-4, q, st.cut_coul, d["prd"])
    return wl.make_system(d["x"][perm], q[perm], alpha[perm], d["type"][perm], d["molecule"][perm], np.zeros(3), d["prd"], d["ntypes"],
                          wl.synth_coeff_rows(), st, g, bonds=None, exclude_intra=True, skin=1.0, name="inert%d" % seed)


def _polar_only(wl, x, q, alpha, mol, prd, cut, ddcut, extra=(), tilt=None):
    """No ghosts and no LJ / Coulomb list: f, the energies and the virial hold the polarization part alone."""
    n = len(x)
    rng = np.random.default_rng(1)
    x0 = rng.uniform(1.0, float(min(prd)) - 1.0, (n, 3))   # make_system lays its (unused) lists out on these
    st = wl.parse_pair_style_args(["2.5", repr(float(cut)), "use_previous", "no", "damp_type", "exponential", "damp", "2.1304",
                                   "dd_cutoff", repr(float(ddcut))] + GS + list(extra))
    s = wl.make_system(x0, q, alpha, np.ones(n, np.int32), mol, np.zeros(3), np.array(prd, float), 1, [["1", "1", "0.0", "3.0"]], st,
                       0.25, name="inert_polar_only", build_list=False)
    s = copy.copy(s)
    if tilt is not None:
        s.tilt, s.triclinic = tuple(float(t) for t in tilt), 1
    s.x, s.nghost, s.owner = np.ascontiguousarray(x, dtype=np.float64), 0, np.arange(n)
    for k in ("q", "alpha", "type", "molecule"):
        setattr(s, k, np.ascontiguousarray(getattr(s, k)[:n]))
    s.ilist = np.zeros(0, np.int32); s.numneigh = np.zeros(n, np.int32)
    s.firstneigh = np.zeros(n, np.int64); s.neigh = np.zeros(0, np.int32)
    return s


def _handle(pkg, s, inert_on, lab_literal=False):
    """A handle created with the switch on (the default) or under POLAR_NL_INERT=0 (read by polar_create).
    lab_literal: the lab library with POLAR_FORCE_LITERAL=1, the term-by-term pair arithmetic (csrc/lab/force_pair_literal.hpp)."""
    env = {"POLAR_NL_INERT": None if inert_on else "0", "POLAR_FORCE_LITERAL": "1" if lab_literal else None}
    old = {k: os.environ.pop(k, None) for k in env}
    try:
        for k, v in env.items():
            if v is not None:
                os.environ[k] = v
        return pkg.pair_from_system(s, lab=lab_literal)
    finally:
        for k in env:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


def _run(pkg, s, inert_on, eflag=1, vflag=2, lab_literal=False):
    p = _handle(pkg, s, inert_on, lab_literal)
    try:
        out = p.compute(eflag=eflag, vflag=vflag)
        out["nl_entries"], out["force_rows"] = p.extract("nl_entries"), p.extract("force_rows")
        if s.settings.debug:
            out["dbg"] = np.concatenate(p.debug_forces())
        return out
    finally:
        p.close()


def _brute(s, cutall):
    """(partners within cutall per local atom, non-inert partners per local atom) under the orthogonal minimum image."""
    n = s.nlocal
    x = np.asarray(s.x[:n], dtype=float)
    prd = np.asarray(s.prd, dtype=float)
    d = x[:, None, :] - x[None, :, :]
    d -= prd * np.rint(d / prd)
    r2 = np.einsum("ijk,ijk->ij", d, d)
    np.fill_diagonal(r2, np.inf)
    assert np.min(np.abs(r2 / cutall ** 2 - 1.0)) > 1e-9            # no comparison with the cutoff can go either way
    inside = r2 <= cutall ** 2
    live = ~((s.q[:n] == 0.0) & (s.alpha[:n] == 0.0))
    return inside.sum(axis=1), (inside & live[None, :]).sum(axis=1), live


def _same(on, off, s, what=""):
    """the two handles agree to AB of the largest magnitude (the same pairs, added in another order)"""
    assert on["status"] == off["status"] and on["iterations"] == off["iterations"] and on["dd_pairs"] == off["dd_pairs"], what
    worst = {}
    for k in ("f", "mu", "ef_static", "eatom", "vatom"):
        if on.get(k) is None:
            continue
        scale = max(np.max(np.abs(off[k])), 1e-300)
        worst[k] = float(np.max(np.abs(on[k] - off[k])) / scale)
    for k in ("eng_vdwl", "eng_coul", "eng_pol", "u_ef", "u_dd", "u_self"):
        worst[k] = rel(on[k], off[k]) if off[k] != 0.0 else abs(on[k])
    x = np.asarray(s.x, dtype=float)
    fx = np.abs(off["f"][:, [0, 1, 2, 1, 2, 2]] * x[:, [0, 1, 2, 0, 0, 1]]).sum(axis=0)   # the terms of the six virial sums
    vscale = max(float(fx.max()), float(np.max(np.abs(off["virial"]))), 1e-300)
    worst["virial"] = float(np.max(np.abs(on["virial"] - off["virial"])) / (3.0 * vscale))
    print("   ", what, "on/off:", " ".join("%s %.1e" % kv for kv in worst.items()))
    for k, v in worst.items():
        assert v < AB, (what, k, v)


def _oracle_ok(out, ref, s, peratom=False):
    from oracle import oracle
    assert out["status"] == ref["status"], (out["status"], ref["status"])
    scale = max(np.max(np.abs(ref["mu"])), 1e-30)
    assert np.max(np.abs(out["mu"] - ref["mu"])) / scale < TOL
    assert np.max(np.abs(out["ef_static"] - ref["ef_static"])) < 1e-9 * max(np.max(np.abs(ref["ef_static"])), 1e-30)
    f = oracle.fold_ghost_forces(out["f"], s.owner, s.nlocal)
    fr = oracle.fold_ghost_forces(ref["f"], s.owner, s.nlocal)
    assert force_rel_err(f, fr) < TOL
    for k in ("eng_vdwl", "eng_coul", "eng_pol"):
        assert rel(out[k], ref[k], 1e-9) < TOL, k
    assert np.max(np.abs(out["virial"] - ref["virial"])) < TOL * max(np.max(np.abs(ref["virial"])), 1e-30)
    if peratom:
        for k in ("eatom", "vatom"):
            a = oracle.fold_ghost_forces(out[k], s.owner, s.nlocal)
            b = oracle.fold_ghost_forces(ref[k], s.owner, s.nlocal)
            assert np.max(np.abs(a - b)) < TOL * max(np.max(np.abs(b)), 1e-30), k


def _counts_ok(on, off, s):
    """nl_entries is what the list build counted while it wrote.  force_rows is NOT counted inside the force launch (the issue
    allows no per-row atomic there): the library applies the kernel's own test to the records when asked, so this comparison
    pins the predicate and the bookkeeping (rows, switch), not the early return itself -- that shows in the kernel's time
     and, for its results, in the comparisons with the oracle and the switch-off handle."""
    every, listed, live = _brute(s, max(CUT, DDCUT))
    for o in (on, off):
        assert o["nl_entries"] == int(o["nl_entries"]) and o["force_rows"] == int(o["force_rows"])
    print("    nl_entries on %d off %d (brute force %d / %d), force_rows on %d off %d of %d atoms" % (
        on["nl_entries"], off["nl_entries"], listed.sum(), every.sum(), on["force_rows"], off["force_rows"], s.nlocal))
    assert int(on["nl_entries"]) == int(listed.sum()) and int(off["nl_entries"]) == int(every.sum())
    assert int(on["force_rows"]) == int(live.sum()) and int(off["force_rows"]) == s.nlocal
    return every, listed, live


@pytest.fixture(scope="module")
def mixed(wl, pkg, oracle):
    """the mixed system, its oracle result and the results of both handles: computed once, read by the tests below"""
    s = _mixed(wl)
    return dict(s=s, ref=oracle.compute(s, eflag=1, vflag=2), on=_run(pkg, s, True), off=_run(pkg, s, False))


def test_mixed_system_has_the_kinds_and_rows_the_drop_shortens(mixed):
    s = mixed["s"]
    n = s.nlocal
    q, a = s.q[:n], s.alpha[:n]
    fr = [np.mean((q == 0) & (a == 0)), np.mean((q != 0) & (a == 0)), np.mean((q == 0) & (a != 0)), np.mean((q != 0) & (a != 0))]
    print("    %d atoms: inert %.3f, charged only %.3f, polarizable without charge %.3f, both %.3f" % (n, *fr))
    assert abs(fr[0] - 0.30) < 0.02 and abs(fr[1] - 0.10) < 0.02 and abs(fr[2] - 0.10) < 0.02 and fr[3] > 0.4
    every, listed, _ = _brute(s, max(CUT, DDCUT))
    trips = lambda c: -(-c // 64)
    print("    partners per row %d ... %d, listed %d ... %d; rows that lose a trip: %d" % (
        every.min(), every.max(), listed.min(), listed.max(), np.sum(trips(listed) < trips(every))))
    assert every.max() <= 3 * 64 and len(set(trips(every))) >= 2 and len(set(trips(listed))) >= 2
    assert np.sum(trips(listed) < trips(every)) >= 20


def test_mixed_system_matches_the_oracle_and_the_switch_off_handle(mixed):
    s = mixed["s"]
    assert mixed["ref"]["status"] == 0
    for o in (mixed["on"], mixed["off"]):
        _oracle_ok(o, mixed["ref"], s)
    _same(mixed["on"], mixed["off"], s, "mixed")


def test_counters_equal_the_brute_force_counts(mixed):
    _counts_ok(mixed["on"], mixed["off"], mixed["s"])


def _shell(k, radius, rng):
    """k points spread over a sphere (Fibonacci spiral, randomly rotated)"""
    i = np.arange(k) + 0.5
    z = 1.0 - 2.0 * i / max(k, 1)
    ph = i * np.pi * (3.0 - np.sqrt(5.0))
    p = np.stack([np.sqrt(1.0 - z * z) * np.cos(ph), np.sqrt(1.0 - z * z) * np.sin(ph), z], axis=1)
    rot, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return radius * p @ rot.T


def test_constructed_rows_of_63_64_65_and_0_listed_partners(wl, pkg):
    """Four row atoms 30 A apart in a 60 A box (cutoff 9): 63, 64, 65 and 0 charged or polarizable partners on a 6.5 A shell,
    and three inert partners each on a 4 A shell -- with them the rows hold 66, 67, 68 and 3 entries, so the trip count of the
    first two changes by the drop and the last row becomes empty."""
    rng = np.random.default_rng(63)
    L, cut = 60.0, 9.0
    centres = np.array([[15.0, 15.0, 15.0], [45.0, 15.0, 15.0], [15.0, 45.0, 15.0], [45.0, 45.0, 45.0]])
    want = [63, 64, 65, 0]
    x, q, al = [], [], []
    for c, k in zip(centres, want):
        x.append(c[None, :]); q.append([0.5]); al.append([0.8])
        sh = _shell(k, 6.5, rng)
        x.append(c + sh)
        kq = rng.uniform(0.1, 0.4, k) * rng.choice([-1.0, 1.0], k)
        ka = np.zeros(k)
        ka[::8] = 0.5                      # every eighth partner polarizable, half of those without charge
        kq[::16] = 0.0
        q.append(kq); al.append(ka)
        x.append(c + _shell(3, 4.0, rng)); q.append(np.zeros(3)); al.append(np.zeros(3))
    x = np.vstack(x) + rng.uniform(-0.05, 0.05, (sum(want) + 4 * 4, 3))
    q, al = np.concatenate(q), np.concatenate(al)
    n = len(x)
    rows = np.cumsum([0] + [k + 4 for k in want])[:4]          # the indices of the four row atoms
    s = _polar_only(wl, x, q, al, np.zeros(n, np.int32), (L, L, L), cut, cut)
    every, listed, live = _brute(s, cut)
    assert [int(listed[r]) for r in rows] == want and all(every[r] - listed[r] == 3 for r in rows)
    on, off = _run(pkg, s, True), _run(pkg, s, False)
    assert on["status"] == 0 and off["status"] == 0
    assert int(on["nl_entries"]) == listed.sum() and int(off["nl_entries"]) == every.sum()
    assert int(on["force_rows"]) == live.sum() == n - 12 and int(off["force_rows"]) == n
    _same(on, off, s, "constructed")
    for r, k in zip(rows, want):
        for key in ("ef_static", "f"):
            assert np.max(np.abs(on[key][r] - off[key][r])) <= AB * np.max(np.abs(off[key])), (k, key)
        assert np.any(on["ef_static"][r] != 0.0) == (k > 0)
    last = rows[3]
    assert np.all(on["ef_static"][last] == 0.0) and np.all(on["f"][last] == 0.0) and np.all(on["mu"][last] == 0.0)
    inert = np.flatnonzero(~live)
    assert np.all(on["f"][inert] == 0.0) and np.all(on["mu"][inert] == 0.0)      # no LJ here: an inert site feels nothing
    assert np.any(on["ef_static"][inert[:9]] != 0.0)                             # ... but its static field is still computed


def test_variant_without_damping(wl, pkg, oracle):
    s = _mixed(wl, extra=["damp_type", "none"], seed=6)
    ref = oracle.compute(s, eflag=1, vflag=2)
    on, off = _run(pkg, s, True), _run(pkg, s, False)
    _oracle_ok(on, ref, s)
    _same(on, off, s, "damping none")
    _counts_ok(on, off, s)


def test_variant_pairwise_and_per_atom_virial(wl, pkg, oracle):
    s = _mixed(wl, seed=7)
    ref = oracle.compute(s, eflag=3, vflag=5)
    on, off = _run(pkg, s, True, eflag=3, vflag=5), _run(pkg, s, False, eflag=3, vflag=5)
    _oracle_ok(on, ref, s, peratom=True)
    _same(on, off, s, "pairwise + per-atom virial")
    n = s.nlocal
    inert = (s.q[:n] == 0.0) & (s.alpha[:n] == 0.0)
    assert np.any(on["vatom"][:n][inert] != 0.0)          # (their LJ part: inert sites do have LJ)


def test_variant_lab_library_with_the_literal_pair_form(mixed, pkg):
    """The lab library's term-by-term pair arithmetic (POLAR_FORCE_LITERAL=1) is device code only, so the host program cannot
    pin its zeros: every part of it sits behind `alpha != 0 && q != 0` guards of the two sides and its outputs start at +0.
    Here: the same rows dropped, the same results as with every row walked, and as the product library's."""
    s = mixed["s"]
    on, off = _run(pkg, s, True, lab_literal=True), _run(pkg, s, False, lab_literal=True)
    _oracle_ok(on, mixed["ref"], s)
    _same(on, off, s, "lab, literal pair form")
    _counts_ok(on, off, s)
    assert np.max(np.abs(on["f"] - mixed["on"]["f"])) <= 1e-10 * np.max(np.abs(mixed["on"]["f"]))   # (two forms of one arithmetic: the bound of tests/test_force_pair_host.py)


def test_variant_polar_ewald(wl, pkg):
    s = _mixed(wl, extra=["polar_ewald", "1e-6"], seed=8)
    on, off = _run(pkg, s, True), _run(pkg, s, False)
    assert on["status"] == 0 and on["nkvec"] > 0
    _same(on, off, s, "polar_ewald")
    _counts_ok(on, off, s)


def test_variant_triclinic_box(wl, pkg, oracle):
    rng = np.random.default_rng(9)
    d = wl.synth(600, seed=9)
    q, alpha = _kinds(rng, d["q"], d["alpha"])
    L = float(d["prd"][0])
    tilt = (0.21 * L, -0.13 * L, 0.17 * L)
    fr = d["x"] / L                                        # the generator's geometry, sheared with the cell
    x = np.stack([fr[:, 0] * L + fr[:, 1] * tilt[0] + fr[:, 2] * tilt[1], fr[:, 1] * L + fr[:, 2] * tilt[2], fr[:, 2] * L], axis=1)
    s = _polar_only(wl, x, q, alpha, d["molecule"], (L, L, L), 6.0, 5.0, tilt=tilt)
    ref = oracle.compute(s, eflag=1, vflag=2)
    on, off = _run(pkg, s, True), _run(pkg, s, False)
    _oracle_ok(on, ref, s)
    _same(on, off, s, "triclinic")
    live = ~((q == 0.0) & (alpha == 0.0))
    assert int(on["force_rows"]) == live.sum() and int(off["force_rows"]) == len(q)
    assert 0 < on["nl_entries"] < off["nl_entries"]


def test_variant_debug_with_an_inert_atom_0(wl, pkg, oracle):
    s = _mixed(wl, extra=["debug", "yes"], seed=10, inert_first=True)
    assert s.q[0] == 0.0 and s.alpha[0] == 0.0
    ref = oracle.compute(s, eflag=1, vflag=2)
    on, off = _run(pkg, s, True), _run(pkg, s, False)
    _oracle_ok(on, ref, s)
    _same(on, off, s, "debug")
    assert np.all(on["dbg"] == 0.0) and np.all(off["dbg"] == 0.0)                # its six zeros, written or left
    assert np.all(ref["force_atom0"] == 0.0) and np.all(ref["dipole_force_atom0"] == 0.0)


def test_variant_without_an_inert_site_changes_nothing(wl, pkg, oracle):
    s = _mixed(wl, seed=11, inert=0.0)
    ref = oracle.compute(s, eflag=1, vflag=2)
    on, off = _run(pkg, s, True), _run(pkg, s, False)
    _oracle_ok(on, ref, s)
    _same(on, off, s, "no inert site")
    every, listed, live = _brute(s, max(CUT, DDCUT))
    assert np.all(live) and np.array_equal(every, listed)
    assert int(on["nl_entries"]) == int(off["nl_entries"]) == every.sum()
    assert int(on["force_rows"]) == int(off["force_rows"]) == s.nlocal


def test_set_atoms_that_changes_the_kind_of_two_atoms_is_followed(mixed, wl, pkg):
    """One handle, two computes: between them polar_set_atoms gives an inert atom a charge and makes a charged atom inert.
    The kinds are worked out from the resident arrays every step, so the second result is that of a fresh handle."""
    s = mixed["s"]
    n = s.nlocal
    q, a = s.q.copy(), s.alpha.copy()
    owner = np.asarray(s.owner)
    i_in = int(np.flatnonzero((q[:n] == 0.0) & (a[:n] == 0.0))[3])
    i_ch = int(np.flatnonzero((q[:n] != 0.0) & (a[:n] == 0.0))[2])
    q[owner == i_in] = q[i_ch]                               # (ghosts carry their owners' values; the total charge stays)
    q[owner == i_ch] = 0.0
    s2 = copy.copy(s)
    s2.q = np.ascontiguousarray(q)
    p = _handle(pkg, s, True)
    try:
        first = p.compute(eflag=1, vflag=2)
        assert np.max(np.abs(first["f"] - mixed["on"]["f"])) <= AB * np.max(np.abs(mixed["on"]["f"]))
        p.set_atoms(s2.nlocal, s2.nghost, s2.x, s2.q, s2.alpha, s2.type, s2.molecule)
        assert p.extract("nl_entries") == 0.0 and p.extract("force_rows") == 0.0   # counters of a compute call: none on these atoms yet
        second = p.compute(eflag=1, vflag=2)
        second["nl_entries"], second["force_rows"] = p.extract("nl_entries"), p.extract("force_rows")
    finally:
        p.close()
    fresh = _run(pkg, s2, True)
    _same(second, fresh, s2, "set_atoms")
    assert second["nl_entries"] == fresh["nl_entries"] and second["force_rows"] == fresh["force_rows"] == mixed["on"]["force_rows"]
    assert second["nl_entries"] != mixed["on"]["nl_entries"] or np.any(second["ef_static"] != first["ef_static"])
    assert np.max(np.abs(second["ef_static"] - first["ef_static"])) > 1e-6 * np.max(np.abs(first["ef_static"]))
