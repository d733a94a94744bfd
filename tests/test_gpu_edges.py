"""Edge cases of the HIP path against the oracle: empty and tiny systems, no polarizable atoms,
no charges, no ghosts, free (non-periodic) boundaries in list mode, unwrapped coordinates, and the
pitched-list overflow retry."""
import copy
import os

import numpy as np
import pytest

from helpers import GOLD, force_rel_err, rel

pytestmark = pytest.mark.gpu
TOL = 1e-7


def _mini(wl, n=40, seed=3, L=24.0, cut=9.0, extra=(), alpha_scale=1.0, q_scale=1.0, periodic=(1, 1, 1)):
    rng = np.random.default_rng(seed)
    x = rng.uniform(2.0, L - 2.0, (n, 3))
    typ = rng.integers(1, 3, n).astype(np.int32)
    q = rng.normal(0, 0.4, n) * q_scale
    q -= q.mean()
    alpha = np.where(rng.uniform(size=n) < 0.7, rng.uniform(0.3, 1.2, n), 0.0) * alpha_scale
    mol = (np.arange(n) // 2 + 1).astype(np.int32)
    st = wl.parse_pair_style_args(["8.0", repr(cut), "damp_type", "exponential", "precision", "1e-13",
                                   "max_iterations", "200"] + list(extra))
    rows = [["1", "1", "0.10", "3.0"], ["1", "2", "0.08", "3.2"], ["2", "2", "0.06", "3.4"]]
    s = wl.make_system(x, q, alpha, typ, mol, np.zeros(3), np.array([L, L, L]), 2, rows, st, 0.25, name="mini")
    return s


def _check(pkg, oracle, s, tol=TOL, periodic=(1, 1, 1)):
    ref = oracle.compute(s, eflag=1, vflag=2)
    p = pkg.pair_from_system(s)
    out = p.compute()
    if s.nlocal:
        f = oracle.fold_ghost_forces(out["f"], s.owner, s.nlocal)
        fr = oracle.fold_ghost_forces(ref["f"], s.owner, s.nlocal)
        if np.any(fr):
            assert force_rel_err(f, fr) < tol
        if np.any(ref["mu"]):
            assert np.max(np.abs(out["mu"] - ref["mu"])) / np.max(np.abs(ref["mu"])) < tol
    for k in ("eng_vdwl", "eng_coul", "eng_pol"):
        assert abs(out[k] - ref[k]) <= tol * max(abs(ref[k]), 1e-9)
    assert out["status"] == ref["status"]
    return out, ref


@pytest.mark.parametrize("mode", ["exact", "list"])
def test_small_random_system(mode, wl, pkg, oracle):
    s = _mini(wl, extra=(["dd_cutoff", "9.0"] if mode == "list" else []))
    out, ref = _check(pkg, oracle, s)
    if mode == "exact":
        assert out["iterations"] == ref["iterations"]


@pytest.mark.parametrize("mode", ["exact", "list"])
def test_no_polarizable_atoms(mode, wl, pkg, oracle):
    s = _mini(wl, alpha_scale=0.0, extra=(["dd_cutoff", "9.0"] if mode == "list" else []))
    out, ref = _check(pkg, oracle, s)
    assert out["eng_pol"] == 0.0 and not np.any(out["mu"])
    assert out["iterations"] == ref["iterations"] == 1


def test_no_charges_gives_no_field(wl, pkg, oracle):
    s = _mini(wl, q_scale=0.0)
    out, ref = _check(pkg, oracle, s)
    assert not np.any(out["ef_static"]) and out["eng_pol"] == 0.0


@pytest.mark.parametrize("n", [1, 2, 3])
def test_tiny_systems(n, wl, pkg, oracle):
    s = _mini(wl, n=n, seed=n)
    _check(pkg, oracle, s)


def test_empty_system(wl, pkg):
    s = _mini(wl, n=2)
    p = pkg.pair_from_system(s)
    p.set_atoms(0, 0, np.zeros((0, 3)), np.zeros(0), np.zeros(0), np.zeros(0, np.int32), np.zeros(0, np.int32))
    p.set_neighbors_csr(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int64), np.zeros(0, np.int32))
    out = p.compute()
    assert out["eng_pol"] == 0.0 and out["eng_vdwl"] == 0.0 and out["f"].shape == (0, 3)


def test_unwrapped_coordinates_list_mode(wl, pkg, oracle):
    """LAMMPS atoms drift out of the box between reneighborings: shift some atoms by whole box lengths."""
    s = _mini(wl, extra=["dd_cutoff", "9.0"])
    ref = oracle.compute(s, eflag=1, vflag=2)
    s2 = copy.copy(s)
    x = s.x.copy()
    n = s.nlocal
    x[:n:3, 0] += s.prd[0]
    x[1:n:4, 2] -= s.prd[2]
    s2.x = x
    out = pkg.pair_from_system(s2).compute()
    # polarization part is image-invariant; the LJ/coul half list refers to explicit ghosts, so compare
    # dipoles and E_pol only
    assert np.max(np.abs(out["mu"] - ref["mu"])) / np.max(np.abs(ref["mu"])) < TOL
    assert rel(out["eng_pol"], ref["eng_pol"]) < TOL


def test_pitch_overflow_retry(wl, pkg, oracle, monkeypatch):
    """A deliberately tiny list pitch must be detected and the step redone with a larger one."""
    monkeypatch.setenv("POLAR_INIT_PITCH", "64")
    s, _ = wl.load_fixture(os.path.join(GOLD, "bulk_h2.npz"), extra_args=["use_previous", "no", "dd_cutoff", "9.0",
                                                                            "precision", "1e-13", "max_iterations", "200"])
    out, ref = _check(pkg, oracle, s)


def test_two_consecutive_steps_reuse_lists_and_colours(wl, pkg, oracle):
    """Second compute on moved coordinates without a new neighbor list (neighbor->ago > 0)."""
    s = _mini(wl, n=60, extra=["dd_cutoff", "9.0"])
    p = pkg.pair_from_system(s)
    p.compute()
    rng = np.random.default_rng(9)
    s2 = copy.copy(s)
    dx = rng.normal(0, 0.03, (s.nlocal, 3))
    x2 = s.x.copy()
    x2 += dx[s.owner]                      # ghosts move with their owners
    s2.x = x2
    p.set_atoms(s2.nlocal, s2.nghost, s2.x, s2.q, s2.alpha, s2.type, s2.molecule)   # no set_neighbors
    out = p.compute()
    ref = oracle.compute(s2, eflag=1, vflag=2)
    f = oracle.fold_ghost_forces(out["f"], s.owner, s.nlocal)
    fr = oracle.fold_ghost_forces(ref["f"], s.owner, s.nlocal)
    assert force_rel_err(f, fr) < TOL
    assert rel(out["eng_pol"], ref["eng_pol"]) < TOL


def test_triclinic_box_exact_mode(wl, pkg, oracle):
    """Triclinic branch of Domain::closest_image (domain.cpp:1258-1305) in the all-pairs kernels.
    No LJ/coul list here (inum = 0, no ghosts): the polarization loops are the ones that use the
    minimum image.  Checker = the oracle, whose orc_closest_image is pinned bit for bit, triclinic branch included, by the
    reference's compiled domain.cpp (tests/test_closest_image.py, tests/golden/ref_closest_image.npz)."""
    rng = np.random.default_rng(11)
    n, L = 90, 16.0
    s = _mini(wl, n=n, seed=11, L=L, cut=7.5)
    s2 = copy.copy(s)
    s2.tilt, s2.triclinic = (3.1, -2.2, 1.7), 1
    # spread the atoms over the tilted cell: x = frac . (a, b, c)
    fr = rng.uniform(0, 1, (n, 3))
    xy, xz, yz = s2.tilt
    x = np.stack([fr[:, 0] * L + fr[:, 1] * xy + fr[:, 2] * xz, fr[:, 1] * L + fr[:, 2] * yz, fr[:, 2] * L], axis=1)
    s2.x = np.ascontiguousarray(x)
    s2.nghost = 0
    for k in ("q", "alpha", "type", "molecule"):
        setattr(s2, k, np.ascontiguousarray(getattr(s, k)[:n]))
    s2.owner = np.arange(n)
    s2.ilist = np.zeros(0, np.int32); s2.numneigh = np.zeros(n, np.int32)
    s2.firstneigh = np.zeros(n, np.int64); s2.neigh = np.zeros(0, np.int32)
    for extra in ([], ["polar_gs_ranked", "no", "polar_gs", "yes"]):
        s2.settings = wl.parse_pair_style_args(["8.0", "7.5", "damp_type", "exponential", "precision", "1e-13",
                                                "max_iterations", "200"] + extra)
        out, ref = _check(pkg, oracle, s2)
        assert out["iterations"] == ref["iterations"]
    # list mode in the tilted cell (cell grid in fractional coordinates, whole lattice vectors taken off c, b, a):
    # against the oracle's list mode, whose pair list comes from closest_image's triclinic branch.  That branch is pinned
    # by the reference's compiled domain.cpp (tests/test_closest_image.py); the device functions are compared with the
    # recorded images directly, and this cell's pair count with brute force, in tests/test_gpu_closest_image.py.  (With
    # cut 7.5 in a 16 A cell no pair here reaches an image that is not the nearest one; the exact-mode tensor above does.)
    for extra in (["precision", "1e-13", "max_iterations", "200"],
                  ["polar_gs_ranked", "no", "fixed_iteration", "yes", "max_iterations", "5"]):
        s2.settings = wl.parse_pair_style_args(["8.0", "7.5", "damp_type", "exponential", "dd_cutoff", "7.5"] + extra)
        out, ref = _check(pkg, oracle, s2)
        assert out["dd_pairs"] > 0
    # the colour phases of the list-mode GS in the tilted cell (Jones-Plassmann path: the cell pass needs cells twice the
    # colour distance wide there): no two atoms of a phase within 2.4 A of each other, over all 27 images
    s2_gs = copy.copy(s2)
    s2_gs.settings = wl.parse_pair_style_args(["8.0", "7.5", "damp_type", "exponential", "dd_cutoff", "7.5", "precision", "1e-13", "max_iterations", "200"])
    p = pkg.pair_from_system(s2_gs)
    p.compute()
    nc, col = p.colors(n)
    p.close()
    assert nc >= 1 and np.all(col[s2.alpha[:n] != 0] >= 0)
    a, b, c = np.array([L, 0, 0]), np.array([xy, L, 0]), np.array([xz, yz, L])
    shifts = np.array([i * a + j * b + k * c for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1)])
    for q in range(nc):
        xq = s2.x[col == q]
        d = xq[:, None, None, :] - xq[None, :, None, :] + shifts[None, None, :, :]
        r2 = np.einsum("ijkl,ijkl->ijk", d, d).min(axis=2)
        r2[np.arange(len(xq)), np.arange(len(xq))] = np.inf
        assert r2.min() > 2.4 ** 2, (q, np.sqrt(r2.min()))
    # a box too thin for the cutoff between two opposite faces is refused (widths, not edge lengths, count)
    s3 = copy.copy(s2)
    s3.tilt = (7.9, 0.0, 0.0)
    s3.settings = wl.parse_pair_style_args(["8.0", "7.5", "dd_cutoff", "7.5"])
    with pytest.raises(pkg.PolarError, match="box lengths"):
        pkg.pair_from_system(s3).compute()


def _filter_csr(s, wl, keep_fn):
    """Rebuild the uploaded half list keeping entries for which keep_fn(i, j_owner, code) -> new code or None."""
    first = np.zeros_like(s.firstneigh)
    nn = np.zeros_like(s.numneigh)
    out = []
    pos = 0
    for i in s.ilist:
        row = s.neigh[s.firstneigh[i]:s.firstneigh[i] + s.numneigh[i]].view(np.uint32)
        new = []
        for e in row:
            j, code = int(e & 0x3FFFFFFF), int(e >> 30)
            c = keep_fn(int(i), int(s.owner[j]), code)
            if c is not None:
                new.append(j | (c << 30))
        first[i], nn[i] = pos, len(new)
        pos += len(new)
        out.extend(new)
    return nn, first, np.asarray(out, dtype=np.uint32).view(np.int32)


@pytest.mark.parametrize("flag", [0, 1])
def test_device_neighbor_build_special_flag_drop_and_plain(flag, wl, pkg, oracle, monkeypatch):
    """neighbor->special_flag 0 (special partners are not listed at all) and 1 (listed as ordinary
    pairs) in polar_build_neighbors, each against an uploaded list edited the same way; plus a
    per-type-pair cutneighsq and a forced row-pitch overflow inside the build."""
    if flag == 1:
        monkeypatch.setenv("POLAR_INIT_PITCH", "64")  # first build overflows its rows and is redone
    s, _ = wl.load_fixture(os.path.join(GOLD, "bulk_h2.npz"), extra_args=["use_previous", "no"])
    assert s.extra["special"], "fixture is expected to carry bonds"
    nn, first, neigh = _filter_csr(s, wl, (lambda i, j, c: (None if c else 0)) if flag == 0 else (lambda i, j, c: 0))
    # reference for the edited list: the CPU oracle on the same edited half list
    import copy
    s_edit = copy.copy(s)
    s_edit.numneigh, s_edit.firstneigh, s_edit.neigh = nn, first, neigh
    ref = oracle.compute(s_edit, eflag=1, vflag=2)
    fref = oracle.fold_ghost_forces(ref["f"], s.owner, s.nlocal)
    p = pkg.pair_from_system(s)
    nsp, sp = wl.lammps_special_arrays(s.nlocal, s.extra["special"])
    w = s.ntypes + 1
    # per-type-pair neighbor cutoffs: (cut_ij + skin)^2 exactly as neighbor->cutneighsq holds them
    cn = (np.sqrt(s.tables["cutsq"]) + 2.0) ** 2
    cn[0, :] = cn[:, 0] = 0.0
    p.build_neighbors(cn, (np.asarray(s.owner) + 1).astype(np.int32), nsp, sp, special_flag=(1, flag, flag, flag),
                      exclude_molecule_intra=s.extra["exclude_intra"])
    out = p.compute()
    assert force_rel_err(out["f"][:s.nlocal], fref) < 1e-7
    for k in ("eng_vdwl", "eng_coul", "eng_pol"):
        assert rel(out[k], ref[k], 1e-9) < 1e-7
    # the uploaded edited list gives the same numbers as the device build (two routes, one oracle)
    p.set_neighbors_csr(s.ilist, nn, first, neigh)
    up = p.compute()
    assert force_rel_err(oracle.fold_ghost_forces(up["f"], s.owner, s.nlocal), fref) < 1e-7
    p.close()


_SOLVERS = {
    "ranked": [],
    "gs": ["polar_gs_ranked", "no", "polar_gs", "yes"],
    "jacobi5": ["polar_gs_ranked", "no", "fixed_iteration", "yes", "max_iterations", "5"],
    "zodid": ["polar_gs_ranked", "no", "zodid", "yes"],
    "undamped": ["damp_type", "none", "max_iterations", "400"],
}


@pytest.mark.parametrize("seed", [11, 12, 13, 14])
@pytest.mark.parametrize("solver", sorted(_SOLVERS))
def test_random_systems_against_the_oracle(seed, solver, wl, pkg, oracle):
    """Random boxes of different size, density, shape and cutoffs, every solver flavour, exact and list
    mode: GPU vs oracle (forces, dipoles, energies, status).  The box shapes include sides with fewer than
    five list cells (the stencil then visits every cell once) and a long thin box."""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(30, 260))
    cut = float(rng.uniform(6.0, 9.0))
    shape = [(2.05, 2.05, 2.05), (2.6, 3.4, 5.2), (2.1, 2.1, 9.0), (4.3, 2.2, 2.9)][seed % 4]
    Lx, Ly, Lz = (cut * f for f in shape)
    x = rng.uniform(0.0, 1.0, (n, 3)) * np.array([Lx, Ly, Lz])
    # keep atoms apart (no polarization catastrophe): reject points closer than 1.9 A
    keep = []
    for a in range(n):
        d = x[keep] - x[a] if keep else np.zeros((0, 3))
        d -= np.array([Lx, Ly, Lz]) * np.round(d / np.array([Lx, Ly, Lz]))
        if not len(d) or np.min(np.sum(d * d, axis=1)) > 1.9 ** 2:
            keep.append(a)
    x = x[keep]
    n = len(x)
    typ = rng.integers(1, 3, n).astype(np.int32)
    q = rng.normal(0, 0.4, n)
    q -= q.mean()
    alpha = np.where(rng.uniform(size=n) < 0.7, rng.uniform(0.3, 1.2, n), 0.0)
    mol = rng.integers(0, max(2, n // 3), n).astype(np.int32)   # molecule 0 is never excluded
    rows = [["1", "1", "0.10", "3.0"], ["1", "2", "0.08", "3.2"], ["2", "2", "0.06", "3.4"]]
    for mode in ("exact", "list"):
        extra = ["damp_type", "exponential", "precision", "1e-13", "max_iterations", "300"] + _SOLVERS[solver]
        if mode == "list":
            extra += ["dd_cutoff", repr(cut)]
        st = wl.parse_pair_style_args(["7.0", repr(cut)] + extra)
        s = wl.make_system(x, q, alpha, typ, mol, np.zeros(3), np.array([Lx, Ly, Lz]), 2, rows, st, 0.25,
                           name=f"rand{seed}")
        out, ref = _check(pkg, oracle, s)
        if mode == "exact" and solver in ("ranked", "gs", "jacobi5"):
            assert out["iterations"] == ref["iterations"]


def test_results_come_back_the_same_with_and_without_the_static_field(wl, pkg):
    """polar_compute with ef_static == NULL (the caller does not want E_static): forces and dipoles are those of the full call;
    two calls in a row give the same numbers (the dipoles and the field travel on their own stream beside the force kernel,
    the forces in four pieces: nothing of one call may leak into the next)."""
    s, _ = wl.load_fixture(os.path.join(GOLD, "mof5_h2.npz"), extra_args=["use_previous", "no", "dd_cutoff", "9.0", "deterministic", "yes"])
    p = pkg.pair_from_system(s)
    a = p.compute(eflag=1, vflag=2)
    b = p.compute(eflag=1, vflag=2, want_ef=False)
    c = p.compute(eflag=1, vflag=2)
    for o in (b, c):
        assert np.array_equal(o["f"], a["f"]) and np.array_equal(o["mu"], a["mu"])
    assert np.array_equal(c["ef_static"], a["ef_static"]) and not np.any(b["ef_static"])
    assert np.any(a["ef_static"])
    p.close()


def test_neighbor_arrays_may_change_once_polar_set_neighbors_has_returned(wl, pkg):
    """polar_set_neighbors* copies the rows into pinned memory before it returns and lets the transfer to the device finish under
    the calls that follow (include/polar_mi355x.h): a caller -- LAMMPS re-uses its neighbor pages -- may overwrite its arrays at
    once.  36,423 atoms: 18 M list entries = three 32-MB chunks on the upload stream.  The same list handed over twice, the
    caller's copy destroyed right after the second hand-over: same forces and energies as the run that kept it."""
    extra = ["use_previous", "no", "polar_gs_ranked", "yes", "dd_cutoff", "12.8345", "fixed_iteration", "yes", "max_iterations", "3",
             "deterministic", "yes"]       # (four sweeps are far from the fixed point: only the deterministic sweep repeats itself there)
    s = wl.replicate_fixture(os.path.join(GOLD, "mof5_h2.npz"), 3, 3, 3, extra_args=extra)
    p = pkg.pair_from_system(s)
    ref = p.compute(eflag=1, vflag=2)
    ilist, numneigh = np.array(s.ilist, dtype=np.int32), np.array(s.numneigh, dtype=np.int32)
    firstneigh, neigh = np.array(s.firstneigh, dtype=np.int64), np.array(s.neigh, dtype=np.int32)
    assert neigh.size > 2 * (8 << 20)
    p.set_neighbors_csr(ilist, numneigh, firstneigh, neigh)
    neigh[:] = 0; numneigh[:] = 0; firstneigh[:] = 0; ilist[:] = 0          # (the transfer may still be under way)
    out = p.compute(eflag=1, vflag=2)
    p.close()
    assert out["status"] == ref["status"] == 0 and out["sweeps"] == ref["sweeps"]
    assert np.max(np.abs(out["f"] - ref["f"])) < 1e-7 * np.max(np.abs(ref["f"]))
    for k in ("eng_vdwl", "eng_coul", "eng_pol"):
        assert abs(out[k] - ref[k]) < 1e-9 * abs(ref[k]), k
