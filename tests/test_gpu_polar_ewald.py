"""`polar_ewald <accuracy>` on the MI355X: the Ewald static field against the NumPy implementation (tests/ewald_numpy.py),
energies / forces / virial against the oracle's LJ/Coulomb and dipole-dipole stages plus the NumPy charge-dipole terms,
g-independence, keyword off = unchanged, determinism, refusals, and configs[2] at full size."""
import ctypes as C
import copy
import os

import numpy as np
import pytest

import ewald_numpy as ew
from helpers import GOLD

pytestmark = pytest.mark.gpu
ACC = "1e-8"


def _mini(wl, n=60, seed=7, L=20.0, extra=(), tilt=None):
    rng = np.random.default_rng(seed)
    typ = rng.integers(1, 3, n).astype(np.int32)
    q = rng.normal(0, 0.4, n)
    q -= q.mean()
    alpha = np.where(rng.uniform(size=n) < 0.7, rng.uniform(0.3, 1.2, n), 0.0)
    mol = (np.arange(n) // 3 + 1).astype(np.int32)
    mol[-6:] = 0
    x = rng.uniform(0.5, L - 0.5, (n, 3))
    st = wl.parse_pair_style_args(["8.0", "9.0", "damp_type", "exponential", "precision", "1e-13", "max_iterations", "200",
                                   "polar_ewald", ACC] + list(extra))
    rows = [["1", "1", "0.10", "3.0"], ["1", "2", "0.08", "3.2"], ["2", "2", "0.06", "3.4"]]
    s = wl.make_system(x, q, alpha, typ, mol, np.zeros(3), np.array([L, L, L]), 2, rows, st, 0.32, name="mini")
    if tilt is not None:   # spread over a tilted cell, no LJ list (the polarization loops are the ones under test)
        s2 = copy.copy(s)
        s2.tilt, s2.triclinic = tilt, 1
        fr = rng.uniform(0, 1, (n, 3))
        s2.x = np.ascontiguousarray(fr @ ew.cell((L, L, L), tilt).T)
        s2.nghost = 0
        for k in ("q", "alpha", "type", "molecule"):
            setattr(s2, k, np.ascontiguousarray(getattr(s, k)[:n]))
        s2.owner = np.arange(n)
        s2.ilist = np.zeros(0, np.int32); s2.numneigh = np.zeros(n, np.int32)
        s2.firstneigh = np.zeros(n, np.int64); s2.neigh = np.zeros(0, np.int32)
        s = s2
    return s


def _H(s):
    return ew.cell(s.prd, getattr(s, "tilt", (0.0, 0.0, 0.0)) if getattr(s, "triclinic", 0) else (0.0, 0.0, 0.0))


def _np_field(s, acc=float(ACC)):
    n = s.nlocal
    return ew.field(s.x[:n], s.q[:n], s.molecule[:n], _H(s), s.settings.cut_coul, s.g_ewald, acc, np.sqrt(s.qqrd2e))


def _run(pkg, s, **kw):
    p = pkg.pair_from_system(s)
    try:
        return p.compute(**kw)
    finally:
        p.close()


CASES = [("mini", "exact", None), ("mini", "list", None), ("mini", "exact", (2.1, -1.4, 1.2)), ("mini", "list", (2.1, -1.4, 1.2)),
         ("mof5_h2", "exact", None), ("mof5_h2", "list", None), ("bulk_h2", "exact", None)]
# (Bulk H2's box is shorter than 2 cut_coul: list mode refuses it, with or without the keyword)


@pytest.mark.parametrize("case,mode,tilt", CASES)
def test_static_field_against_numpy(case, mode, tilt, wl, pkg):
    extra = ["dd_cutoff", "9.0"] if mode == "list" else []
    if case == "mini":
        s = _mini(wl, extra=extra, tilt=tilt)
    else:
        extra = ["dd_cutoff", "12.8345"] if mode == "list" else []
        s, _ = wl.load_fixture(os.path.join(GOLD, case + ".npz"), extra_args=["polar_ewald", ACC, "use_previous", "no"] + extra)
    out = _run(pkg, s, eflag=1, vflag=2)
    ref = _np_field(s)
    assert np.max(np.abs(out["ef_static"] - ref)) < 1e-10 * np.max(np.abs(ref))
    assert out["nkvec"] > 0 and out["ms_kspace"] > 0.0


def _oracle_parts(oracle, s, mu):
    """LJ/Coulomb (orc_ljcoul) and dipole-dipole (orc_polar_forces with the charges off) at the dipoles mu."""
    L = oracle.lib()
    nall = s.nlocal + s.nghost
    st, keep = oracle.make_struct(s)
    f_lj = np.zeros((nall, 3)); ev, ec = C.c_double(0), C.c_double(0); v_lj = np.zeros(6)
    dp = C.POINTER(C.c_double)
    L.orc_ljcoul(C.byref(st), 1, 1, f_lj.ctypes.data_as(dp), C.byref(ev), C.byref(ec), v_lj.ctypes.data_as(dp), None, None)
    s0 = copy.copy(s)
    s0.q = np.zeros_like(s.q)
    st0, keep0 = oracle.make_struct(s0)
    f_dd = np.zeros((nall, 3)); res = oracle.OrcResult()
    m = np.ascontiguousarray(mu, dtype=np.float64)
    L.orc_polar_forces(C.byref(st0), 1, 1, m.ctypes.data_as(dp), f_dd.ctypes.data_as(dp), C.byref(res), None)
    return f_lj, v_lj, ev.value, ec.value, f_dd, res


@pytest.mark.parametrize("mode", ["exact", "list"])
def test_energy_forces_virial_against_numpy_and_oracle(mode, wl, pkg, oracle):
    s = _mini(wl, extra=(["dd_cutoff", "9.0"] if mode == "list" else []))   # (the oracle truncates at dd_cutoff too)
    out = _run(pkg, s, eflag=1, vflag=1)
    n = s.nlocal
    mu = out["mu"]
    f_lj, v_lj, evdwl, ecoul, f_dd, res = _oracle_parts(oracle, s, mu)
    e2s = np.sqrt(s.qqrd2e)
    H = _H(s)
    f_q, v_q = ew.forces_virial(s.x[:n], s.q[:n], s.molecule[:n], mu, H, s.settings.cut_coul, s.g_ewald, float(ACC), e2s)
    E = _np_field(s)
    u_ef = -float(np.sum(mu * E))
    eng_pol = res.u_self + res.u_dd + u_ef
    assert abs(out["eng_pol"] - eng_pol) < 1e-9 * abs(eng_pol)
    assert abs(out["u_ef"] - u_ef) < 1e-9 * abs(u_ef)
    f_ref = oracle.fold_ghost_forces(f_lj + f_dd, s.owner, n)
    f_ref += f_q
    f_dev = oracle.fold_ghost_forces(out["f"], s.owner, n)
    assert np.max(np.abs(f_dev - f_ref)) < 1e-9 * np.max(np.abs(f_ref))
    v_ref = v_lj + np.array(res.virial) + v_q
    assert np.max(np.abs(out["virial"] - v_ref)) < 1e-9 * np.max(np.abs(v_ref))
    if mode == "list":
        return   # (the oracle's dense solve below is exact mode's: list mode's dipole tensor stops at dd_cutoff)
    # the solver is unchanged: the oracle's solve fed the NumPy field takes as many sweeps and lands on the same dipoles
    L = oracle.lib()
    st, keep = oracle.make_struct(s)
    dp = C.POINTER(C.c_double)
    mat = np.zeros((3 * n, 3 * n)); rank = np.zeros(n); rmin = np.zeros(1)
    L.orc_build_dipole_field_matrix(C.byref(st), mat.ctypes.data_as(dp))
    L.orc_rank_metric(C.byref(st), rank.ctypes.data_as(dp), rmin.ctypes.data_as(dp))
    E = np.ascontiguousarray(E)
    mu0 = np.ascontiguousarray(s.settings.polar_gamma * s.alpha[:n, None] * E)
    r2 = oracle.OrcResult()
    L.orc_dipole_solver.restype = C.c_int
    it = L.orc_dipole_solver(C.byref(st), mat.ctypes.data_as(dp), E.ctypes.data_as(dp), rank.ctypes.data_as(dp),
                             mu0.ctypes.data_as(dp), C.byref(r2), None)
    assert np.max(np.abs(mu0 - mu)) < 1e-9 * np.max(np.abs(mu))
    assert out["iterations"] == it


def test_two_tiles_per_chunk_against_numpy_and_oracle(wl, pkg, oracle, tmp_path):
    """The handle's own k-space launches where a chunk of k_ew_sfac takes two tiles: MOF-5 + H2 (1,349 atoms), list mode,
    g_ewald 0.6, polar_ewald 1e-12.  The plan (through the probe's host entry, tests/ewald_kspace_load.py) gives 35,855
    k-vectors, nm = 25, tiles of 32 atoms and chunks of 45: a tile of 32 and one of 13 per chunk, the second trip of the tile
    loop that the 60-atom systems above never take; k_ew_force runs 6 workgroups and writes f through d_perm.  (The kernels
    alone, at every tiling, against long double: tests/test_gpu_ewald_kspace.py.)

    ef_static against the NumPy field, f / u_ef / eng_pol / the vflag = 1 virial against oracle + NumPy as in
    test_energy_forces_virial_against_numpy_and_oracle, with this file's tolerances (1e-10, 1e-9).  The NumPy sums run in
    blocks of 2,048 k-vectors (kblock: the dense [n, nk] arrays would take several GB) and cost about 6 s of CPU."""
    import ewald_kspace_load as kl
    acc = "1e-12"
    s, _ = wl.load_fixture(os.path.join(GOLD, "mof5_h2.npz"), g_ewald=0.6,
                           extra_args=["dd_cutoff", "12.8345", "polar_ewald", acc, "use_previous", "no", "precision", "1e-13",
                                       "max_iterations", "200"])
    n = s.nlocal
    pl = kl.load(pkg, tmp_path).plan(s.prd, (0.0, 0.0, 0.0), s.g_ewald, float(acc), n)
    assert (pl["nk"], pl["nm"], pl["tile"], pl["chunk"]) == (35855, 25, 32, 45)
    assert pl["tile"] < pl["chunk"] <= 2 * pl["tile"] and (n + 255) // 256 == 6
    out = _run(pkg, s, eflag=1, vflag=1)
    assert out["status"] == 0 and out["nkvec"] == pl["nk"]
    e2s, H, kb = np.sqrt(s.qqrd2e), _H(s), 2048
    E = ew.field(s.x[:n], s.q[:n], s.molecule[:n], H, s.settings.cut_coul, s.g_ewald, float(acc), e2s, kblock=kb)
    assert np.max(np.abs(out["ef_static"] - E)) < 1e-10 * np.max(np.abs(E))
    mu = out["mu"]
    f_lj, v_lj, _, _, f_dd, res = _oracle_parts(oracle, s, mu)
    f_q, v_q = ew.forces_virial(s.x[:n], s.q[:n], s.molecule[:n], mu, H, s.settings.cut_coul, s.g_ewald, float(acc), e2s, kblock=kb)
    u_ef = -float(np.sum(mu * E))
    eng_pol = res.u_self + res.u_dd + u_ef
    assert abs(out["eng_pol"] - eng_pol) < 1e-9 * abs(eng_pol)
    assert abs(out["u_ef"] - u_ef) < 1e-9 * abs(u_ef)
    f_ref = oracle.fold_ghost_forces(f_lj + f_dd, s.owner, n)
    f_ref += f_q
    f_dev = oracle.fold_ghost_forces(out["f"], s.owner, n)
    assert np.max(np.abs(f_dev - f_ref)) < 1e-9 * np.max(np.abs(f_ref))
    v_ref = v_lj + np.array(res.virial) + v_q
    assert np.max(np.abs(out["virial"] - v_ref)) < 1e-9 * np.max(np.abs(v_ref))


@pytest.mark.parametrize("route", ["fdotr_half_list", "fdotr_full_list"])
def test_fdotr_virial_with_the_reciprocal_terms(route, wl, pkg, oracle):
    """vflag = 2: the fdotr virial over the pair forces (locals and ghosts with LAMMPS' half list; with the device-built full
    list the LJ/Coulomb part is tallied pairwise and f.x covers the polarization forces only), taken BEFORE the reciprocal
    forces go into f, plus the k-space formula."""
    full = route == "fdotr_full_list"
    s = _mini(wl, extra=["dd_cutoff", "9.0"] if full else [])
    p = pkg.pair_from_system(s, device_neigh=full)
    try:
        out = p.compute(eflag=1, vflag=2)
    finally:
        p.close()
    n, nall = s.nlocal, s.nlocal + s.nghost
    f_lj, v_lj, _, _, f_dd, res = _oracle_parts(oracle, s, out["mu"])
    f_real, f_rec, _, v_rec = ew.forces_virial(s.x[:n], s.q[:n], s.molecule[:n], out["mu"], _H(s), s.settings.cut_coul, s.g_ewald,
                                               float(ACC), np.sqrt(s.qqrd2e), parts=True)
    f_pol = f_dd[:n] + f_real
    if full:
        v_ref = v_lj + ew.fdotr(s.x[:n], f_pol) + v_rec
    else:
        fp = f_lj.copy()
        fp[:n] += f_pol
        v_ref = ew.fdotr(s.x[:nall], fp) + v_rec
    assert np.max(np.abs(out["virial"] - v_ref)) < 1e-9 * np.max(np.abs(v_ref))
    f_ref = f_lj.copy()
    f_ref[:n] += f_pol + f_rec
    assert np.max(np.abs(out["f"] - f_ref)) < 1e-9 * np.max(np.abs(f_ref))


def test_field_and_energy_do_not_depend_on_g(wl, pkg):
    outs = []
    for g in (0.36, 0.40):                   # erfc(g cut_coul) <= 3e-11 for both
        s, _ = wl.load_fixture(os.path.join(GOLD, "mof5_h2.npz"), extra_args=["polar_ewald", "1e-10", "use_previous", "no"], g_ewald=g)
        outs.append(_run(pkg, s, eflag=1, vflag=2))
    a, b = outs
    rms = np.sqrt(np.mean(a["ef_static"] ** 2))
    assert np.sqrt(np.mean((a["ef_static"] - b["ef_static"]) ** 2)) < 1e-6 * rms
    assert abs(a["eng_pol"] - b["eng_pol"]) < 1e-6 * abs(a["eng_pol"])


DET = ["use_previous", "no", "dd_cutoff", "9.0", "deterministic", "yes"]


def _set(p, **kw):
    st = p.get_settings()
    for k, v in kw.items():
        setattr(st, k, v)
    p._ck(p.L.polar_set_settings(p.h, C.byref(st)))


def _same(a, b, ewald):
    for k in ("f", "mu", "ef_static"):
        assert np.array_equal(a[k], b[k]), k
    if ewald:
        assert a["u_ef"] == b["u_ef"]      # the Ewald u_ef: a fixed-order reduction (k_ew_force, k_ew_finish)
    # (the virial and the other energies are folded from per-wave atomic adds into the accumulator slots -- k_virial_fdotr,
    #  k_polar_force, the LJ/Coulomb kernel -- whose order varies, with or without the keyword: equal to rounding)
    assert np.max(np.abs(a["virial"] - b["virial"])) <= 1e-13 * np.max(np.abs(a["virial"]))
    for k in ("eng_vdwl", "eng_coul", "eng_pol", "u_self", "u_ef", "u_dd"):
        assert abs(a[k] - b[k]) <= 1e-13 * abs(a[k]), k


def test_keyword_off_is_bit_identical(wl, pkg):
    """polar_ewald 0 (explicitly set on the same handle) against the keyword not given: the same bits everywhere; on, the
    field differs from the reference model's."""
    s, _ = wl.load_fixture(os.path.join(GOLD, "mof5_h2.npz"), extra_args=DET)
    p = pkg.pair_from_system(s)
    try:
        a = p.compute(eflag=1, vflag=2)
        _set(p, polar_ewald=0.0)
        b = p.compute(eflag=1, vflag=2)
        _set(p, polar_ewald=1e-6)
        e = p.compute(eflag=1, vflag=2)
    finally:
        p.close()
    _same(a, b, False)
    assert a["nkvec"] == 0 and a["ms_kspace"] == 0.0 and e["nkvec"] > 0
    assert not np.allclose(a["ef_static"], e["ef_static"], rtol=1e-6, atol=0)


def test_deterministic_runs_are_bit_identical(wl, pkg):
    s, _ = wl.load_fixture(os.path.join(GOLD, "mof5_h2.npz"), extra_args=DET + ["polar_ewald", "1e-6"])
    p = pkg.pair_from_system(s)
    try:
        a, b = p.compute(eflag=1, vflag=2), p.compute(eflag=1, vflag=2)
        c, d = p.compute(eflag=1, vflag=1), p.compute(eflag=1, vflag=1)
    finally:
        p.close()
    _same(a, b, True)
    _same(c, d, True)


def test_refusals_leave_the_handle_usable(wl, pkg):
    s = _mini(wl, extra=["dd_cutoff", "9.0", "deterministic", "yes"])   # (bit-identical repeats: the handle is as before)
    p = pkg.pair_from_system(s)

    try:
        ok = p.compute(eflag=1, vflag=2)
        assert ok["status"] == 0
        with pytest.raises(pkg.PolarError) as e:
            p.compute(eflag=1, vflag=4)
        assert e.value.code == -4 and "per-atom virial" in str(e.value)
        assert np.array_equal(p.compute(eflag=1, vflag=2)["f"], ok["f"])
        p._ck(p.L.polar_set_row_range(p.h, 0, s.nlocal // 2))
        with pytest.raises(pkg.PolarError) as e:
            p.compute(eflag=1, vflag=2)
        assert e.value.code == -4 and "row-sharded" in str(e.value)
        p._ck(p.L.polar_set_row_range(p.h, 0, -1))
        assert np.array_equal(p.compute(eflag=1, vflag=2)["f"], ok["f"])
        _set(p, rccl_halo=1)
        with pytest.raises(pkg.PolarError) as e:
            p.compute(eflag=1, vflag=2)
        assert e.value.code == -4 and "rccl_halo" in str(e.value)
        _set(p, rccl_halo=0)
        assert np.array_equal(p.compute(eflag=1, vflag=2)["f"], ok["f"])
        p.set_box(s.boxlo, s.prd, periodic=(1, 1, 0))
        with pytest.raises(pkg.PolarError) as e:
            p.compute(eflag=1, vflag=2)
        assert e.value.code == -4 and "periodic" in str(e.value)
        p.set_box(s.boxlo, s.prd, periodic=(1, 1, 1))
        assert np.array_equal(p.compute(eflag=1, vflag=2)["f"], ok["f"])
        # the in-library multi-GPU driver (RCCL, a communicator of one) refuses the keyword before its first collective
        p._ck(p.L.polar_set_list_style(p.h, 0))
        d = pkg.PolarDist(pkg.PolarDist.unique_id(), 0, 1, device=0)
        try:
            rows = np.arange(0, s.nlocal, 3, dtype=np.int32)
            d.set_halo(p, [0], [rows], [rows])
            with pytest.raises(pkg.PolarError) as e:
                d.step(p, eflag=1, vflag=2)
            assert e.value.code == -4 and "multi-GPU driver" in str(e.value)
        finally:
            d.close()
        assert p.compute(eflag=1, vflag=2)["status"] == 0
    finally:
        p.close()


def test_full_size_configs2(wl, pkg):
    extra = ["use_previous", "no", "polar_gs_ranked", "yes", "dd_cutoff", "12.8345", "fixed_iteration", "no",
             "precision", "1e-11", "max_iterations", "100", "polar_ewald", "1e-6"]
    s = wl.replicate_fixture(os.path.join(GOLD, "mof5_h2.npz"), 5, 5, 4, extra_args=extra, build_list=True)
    out = _run(pkg, s, eflag=1, vflag=2)
    assert out["status"] == 0
    lhs = out["u_self"] + out["u_ef"] + out["u_dd"]
    rhs = -0.5 * float(np.sum(out["ef_static"] * out["mu"]))
    assert abs(lhs - rhs) < 1e-8 * abs(rhs)
    assert np.max(np.abs(out["f"].sum(axis=0))) < 1e-9 * np.abs(out["f"]).sum()
    assert out["ms_kspace"] > 0.0 and out["nkvec"] > 1000
    print(f"\nconfigs[2] polar_ewald 1e-6: nkvec={out['nkvec']} ms_kspace={out['ms_kspace']:.3f} ms_total={out['ms_total']:.3f} "
          f"iterations={out['iterations']} E_pol={out['eng_pol']:.6f}")
