"""Systems and points of tests/test_gpu_probe_at.py, shared with the child process it starts (tests/probe_child.py).  Not a
test module.  The recipes are copies: `mini` and `lattice200` of tests/test_gpu_field_at.py, the latter with two types and
per-pair LJ cutoffs.

  mini        60 atoms, L = 20 A, two types with epsilon > 0, cut_lj 8, cut_coul 9; exact mode and dd_cutoff 9 (a 4 x 4 x 4 list
              grid: the stencil covers the whole axis); orthogonal and TILT; with polar_ewald 1e-6 as `mini_ew`
  lattice_lj  200 atoms on a jittered 4 A lattice, L = 28 A, pair cutoffs 5.0 / 4.0 / 6.0, cut_coul 6, dd_cutoff 5.5: 9 x 9 x 9 cells
              with empty ones, a trimmed stencil of two to five cells per axis, reach = cutall for type 2, about 6 % inert sites
  mof5_h2     tests/golden, list mode with dd_cutoff 12.8345: ten types, cut_lj far below cutall"""
import copy
import os

import numpy as np

import point_ref as ptr
import probe_ref as prb

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TILT = (2.1, -1.4, 1.2)
NPTS = 257
MINI_ROWS = [["1", "1", "0.10", "3.0"], ["1", "2", "0.08", "3.2"], ["2", "2", "0.06", "3.4"]]
LATTICE_ROWS = [["1", "1", "0.10", "3.0", "5.0"], ["1", "2", "0.08", "3.2", "4.0"], ["2", "2", "0.06", "3.4", "6.0"]]


def mini(wl, n=60, seed=620, L=20.0, extra=(), tilt=None, cut_lj="8.0", all_in_molecules=False, exclude_intra=False):
    """The recipe of tests/test_gpu_field_at.py::_mini (seed 620: nearest approach 1.76 A, tilted 1.22 A)."""
    rng = np.random.default_rng(seed)
    typ = rng.integers(1, 3, n).astype(np.int32)
    q = rng.normal(0, 0.4, n)
    q -= q.mean()
    alpha = np.where(rng.uniform(size=n) < 0.7, rng.uniform(0.3, 1.2, n), 0.0)
    mol = (np.arange(n) // 3 + 1).astype(np.int32)
    if not all_in_molecules:
        mol[-6:] = 0
    x = rng.uniform(0.5, L - 0.5, (n, 3))
    st = wl.parse_pair_style_args([cut_lj, "9.0", "damp_type", "exponential", "precision", "1e-13", "max_iterations", "200"] + list(extra))
    s = wl.make_system(x, q, alpha, typ, mol, np.zeros(3), np.array([L, L, L]), 2, MINI_ROWS, st, 0.32, name="mini", exclude_intra=exclude_intra)
    if tilt is not None:   # spread over a tilted cell, no LJ list (the step's LJ loop is not under test there)
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


def lattice_lj(wl, seed=11):
    """The lattice200 recipe of tests/test_gpu_field_at.py with two types (drawn from a generator of their own, so that the
    recipe's other draws stay what they were) and the pair cutoffs 5.0 / 4.0 / 6.0."""
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
    typ = np.random.default_rng(seed + 1000).integers(1, 3, n).astype(np.int32)
    st = wl.parse_pair_style_args(["2.5", "6.0", "damp_type", "exponential", "damp", "2.1304", "polar_gs_ranked", "yes", "use_previous", "no",
                                   "precision", "1e-13", "max_iterations", "200", "dd_cutoff", "5.5"])
    return wl.make_system(np.mod(x, L), q, alpha, typ, mol, np.zeros(3), np.array([L, L, L]), 2, LATTICE_ROWS, st, 0.25, name="lattice_lj")


def system(wl, case, mode="list", tilt=None):
    if case == "mini":
        return mini(wl, extra=(["dd_cutoff", "9.0"] if mode == "list" else []), tilt=tilt)
    if case == "mini_ew":
        return mini(wl, extra=["polar_ewald", "1e-6"] + (["dd_cutoff", "9.0"] if mode == "list" else []), tilt=tilt)
    if case == "lattice_lj":
        return lattice_lj(wl)
    extra = ["precision", "1e-13", "max_iterations", "200", "use_previous", "no"] + (["dd_cutoff", "12.8345"] if mode == "list" else [])
    return wl.load_fixture(os.path.join(GOLD, case + ".npz"), extra_args=extra)[0]


def tilt_of(s):
    return tuple(s.tilt) if getattr(s, "triclinic", 0) else None


def tables_of(wl, s, shift):
    """lj1 .. lj4, offset, cut_ljsq as the handle has them: those of the system, with the offsets of `pair_modify shift yes`"""
    st = s.settings
    return wl.init_one_all(s.ntypes, s.extra["coeff_rows"], st.cut_lj_global, st.cut_coul, offset_flag=1 if shift else 0)


def draw_points(s, seed):
    """257 points: 200 in the box, 20 up to two box lengths outside, 17 at 0.3 A from an atom, 20 on atoms with that atom
    skipped.  Types over all of 1 .. ntypes, half the points with a molecule id of the system, q and alpha per point."""
    rng = np.random.default_rng(seed)
    n = s.nlocal
    H = ptr.cell_matrix(s.prd, tilt_of(s))
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
    ptype = rng.integers(1, s.ntypes + 1, NPTS).astype(np.int32)
    ptype[:s.ntypes] = np.arange(1, s.ntypes + 1)            # every type at least once
    pq = rng.normal(0, 0.4, NPTS)
    pa = np.where(rng.random(NPTS) < 0.8, rng.uniform(0.2, 1.5, NPTS), 0.0)
    return dict(x=pts, skip=skip, mol=pmol, type=ptype, q=pq, alpha=pa)


def points_and_reference(wl, s, shift=False, seed=3):
    """The points of a case and their NumPy reference.  A point within 1e-9 A of a cutoff shell of some pair, where `<` could
    fall either way, makes the reference itself ambiguous: the seed is redrawn (here, on the CPU) until there is none."""
    n = s.nlocal
    tb = tables_of(wl, s, shift)
    for attempt in range(20):
        pt = draw_points(s, seed + 1000 * attempt)
        ref = prb.probe_lj_numpy(pt["x"], pt["type"], pt["skip"], pt["mol"], s.x[:n], s.type[:n], s.molecule[:n], tb, s.prd, tilt_of(s))
        if np.min(ref["shell"]) > 1e-9:
            return pt, ref
    raise AssertionError("no seed without a point on a cutoff shell")
