"""The cell order with the inert sites behind the grid (csrc/polar_plan.hpp: cell_bin, cell_bins, cell_bins_fit) on the host.

The header is plain C++: g++ builds tests/cell_order/cell_order_host.cpp around it, a stand-alone program (with the address
and undefined-behaviour sanitizers where the toolchain has them) that answers for the bin rule and the sizes, and plays the
counting sort of build_cells -- count, scan, fill, sort -- through tables of exactly those sizes.  Nothing is loaded into
Python and no GPU is needed.  Everything is an integer: exact comparison.

What the order must satisfy, checked here against a NumPy construction that knows nothing of bins:
  * split off: the parent's order -- cells ascending; inside a cell the polarizable atoms, then all the others, each group in
    ascending atom index (one ascending group without "polarizable first");
  * split on: the atoms that are not inert, in exactly the sequence they have in the parent's order, followed by the inert
    ones cell by cell in ascending atom index; cell_first[0 .. ncell] spans the former alone, and every active cell is
    polarizable first, then charged, each ascending."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "lammps-induced-dipole-polarization-pair-style_amd")
SRC = os.path.join(ROOT, "tests", "cell_order", "cell_order_host.cpp")

POLAR, POLAR_NEUTRAL, CHARGED, INERT = (0.7, 1.3), (0.0, 0.9), (-0.4, 0.0), (0.0, 0.0)    # (q, alpha)
KINDS = (POLAR, POLAR_NEUTRAL, CHARGED, INERT)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("cell_order") / "cell_order_host")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", f"-I{PKG}/csrc", "-o", exe, SRC]
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr:      # a toolchain without the sanitizer runtimes: the plain program
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(text):
        p = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert p.returncode == 0, (p.returncode, p.stderr[-3000:])
        return [[int(v) for v in ln.split()] for ln in p.stdout.splitlines()]
    return run


def _is_inert(q, a):
    return q == 0.0 and a == 0.0


def _order(host, ncell, split, pol_first, cell, q, alpha):
    n = len(cell)
    text = "order %d %d %d %d\n" % (ncell, split, pol_first, n) + "".join("%d %r %r\n" % (cell[i], float(q[i]), float(alpha[i])) for i in range(n))
    out = host(text)
    # (an empty table prints an empty line, which splitlines keeps)
    perm, first, npol = out[0], out[1], out[2]
    return np.array(perm, dtype=np.int64), np.array(first, dtype=np.int64), np.array(npol, dtype=np.int64)


def _parent_order(ncell, pol_first, cell, alpha):
    """Cells ascending; inside a cell polarizable first, then the others, each ascending (all ascending without pol_first)."""
    idx = np.arange(len(cell))
    group = (np.asarray(alpha) == 0.0).astype(np.int64) if pol_first else np.zeros(len(cell), dtype=np.int64)
    return idx[np.lexsort((idx, group, np.asarray(cell)))]


# ---- the bin rule and the sizes -----------------------------------------------------------------------------------------
def test_bin_rule_over_the_site_kinds(host):
    for ncell in (1, 2, 64, 6400):
        cells = sorted({0, ncell // 2, ncell - 1})
        text, want = "", []
        for c in cells:
            for q, a in KINDS:
                for split in (0, 1):
                    inert = _is_inert(q, a)
                    text += "bin %d %d %d %d\n" % (c, ncell, inert, split)
                    # only a site with neither a charge nor a polarizability leaves the grid, and only with the split on
                    want.append(ncell + c if (split and (q, a) == INERT) else c)
        got = [ln[0] for ln in host(text)]
        assert got == want, ncell


def test_sizes_handed_to_scan_and_sort(host):
    for ncell in (1, 2, 5, 64, 6400, 25000):
        off, on = host("sizes %d 0\nsizes %d 1\n" % (ncell, ncell))
        # nbins, entries of the count table, of the fill counters, where the back counters start, entries of cell_first, fits
        assert off == [ncell, ncell + 1, 2 * (ncell + 1), ncell + 1, ncell + 2, 1]        # the parent's sizes
        assert on == [2 * ncell, 2 * ncell + 1, 2 * (2 * ncell + 1), 2 * ncell + 1, 2 * ncell + 2, 1]
    # the scan writes nbins + 1 entries, the fill reads cell_first[bin + 1], the front and the back counters do not overlap
    for ncell, split in ((1, 1), (7, 0), (7, 1)):
        nbins, cnt, fill, back, first, _ = host("sizes %d %d\n" % (ncell, split))[0]
        assert first >= nbins + 1 and cnt >= nbins and back >= nbins and fill >= back + nbins
    # bin indices are 32-bit on the device
    assert host("sizes %d 0\n" % (2**31 - 2))[0][5] == 1
    assert host("sizes %d 0\n" % (2**31 - 1))[0][5] == 0
    assert host("sizes %d 1\n" % (2**30 - 1))[0][5] == 1
    assert host("sizes %d 1\n" % 2**30)[0][5] == 0


# ---- the order itself ---------------------------------------------------------------------------------------------------
def _check_system(host, ncell, cell, q, alpha, pol_first=1):
    cell, q, alpha = np.asarray(cell, dtype=np.int64), np.asarray(q, dtype=np.float64), np.asarray(alpha, dtype=np.float64)
    n = len(cell)
    inert = (q == 0.0) & (alpha == 0.0)
    parent = _parent_order(ncell, pol_first, cell, alpha)
    p0, f0, np0 = _order(host, ncell, 0, pol_first, cell, q, alpha)
    p1, f1, np1 = _order(host, ncell, 1, pol_first, cell, q, alpha)
    # split off: the parent's order, and the scan spans every atom
    assert np.array_equal(p0, parent)
    assert len(f0) == ncell + 1 and f0[0] == 0 and f0[ncell] == n
    assert np.array_equal(np.diff(f0), np.bincount(cell, minlength=ncell))
    # split on: a permutation; the atoms that are not inert in the parent's sequence, then the inert ones
    assert np.array_equal(np.sort(p1), np.arange(n))
    nact = int((~inert).sum())
    assert len(f1) == 2 * ncell + 1 and f1[0] == 0 and f1[ncell] == nact and f1[2 * ncell] == n
    assert np.array_equal(p1[:nact], parent[~inert[parent]])
    assert not inert[p1[:nact]].any() and inert[p1[nact:]].all()
    assert np.array_equal(np.diff(f1)[:ncell], np.bincount(cell[~inert], minlength=ncell))
    assert np.array_equal(np.diff(f1)[ncell:], np.bincount(cell[inert], minlength=ncell))
    for c in range(ncell):
        act = p1[f1[c]:f1[c + 1]]
        assert (cell[act] == c).all()
        if pol_first:
            npc = int(np1[c])
            assert npc == int((alpha[act] != 0.0).sum())
            assert (alpha[act[:npc]] != 0.0).all() and (alpha[act[npc:]] == 0.0).all() and (q[act[npc:]] != 0.0).all()
            assert (np.diff(act[:npc]) > 0).all() and (np.diff(act[npc:]) > 0).all()
            assert np0[c] == npc                                           # the polarizable counts the colouring reads do not move
        else:
            assert (np.diff(act) > 0).all()
        ine = p1[f1[ncell + c]:f1[ncell + c + 1]]
        assert (cell[ine] == c).all() and (np.diff(ine) > 0).all()
        assert np1[ncell + c] == 0                                         # an inert bin has no polarizable front
    return inert


def test_named_cells(host):
    P, N, C, I = KINDS
    # cell 0 empty, cell 1 only inert atoms, cell 2 without an inert atom, cell 3 mixed, cell 4 empty, cell 5 mixed, atoms interleaved
    kinds = {1: [I, I, I], 2: [C, P, N, C, P], 3: [I, P, C, I, N, I], 5: [C, I, P]}
    atoms = [(c, k) for c, ks in kinds.items() for k in ks]
    rng = np.random.default_rng(5)
    rng.shuffle(atoms)
    cell = [a[0] for a in atoms]
    q = [a[1][0] for a in atoms]
    alpha = [a[1][1] for a in atoms]
    for pol_first in (1, 0):
        _check_system(host, 6, cell, q, alpha, pol_first)
    p1, f1, _ = _order(host, 6, 1, 1, cell, q, alpha)
    assert list(np.diff(f1)) == [0, 0, 5, 3, 0, 2, 0, 3, 0, 3, 0, 1]


def test_one_cell_and_no_atoms(host):
    P, N, C, I = KINDS
    ks = [I, P, C, I, N, C, I]
    _check_system(host, 1, [0] * len(ks), [k[0] for k in ks], [k[1] for k in ks])
    p1, f1, _ = _order(host, 1, 1, 1, [0] * len(ks), [k[0] for k in ks], [k[1] for k in ks])
    assert list(p1) == [1, 4, 2, 5, 0, 3, 6] and list(f1) == [0, 4, 7]
    # no inert atom at all: the two orders are one
    ks = [P, C, N, C]
    a = _order(host, 1, 0, 1, [0] * 4, [k[0] for k in ks], [k[1] for k in ks])
    b = _order(host, 1, 1, 1, [0] * 4, [k[0] for k in ks], [k[1] for k in ks])
    assert np.array_equal(a[0], b[0]) and list(b[1]) == [0, 4, 4]
    # only inert atoms; no atoms
    _check_system(host, 3, [2, 0, 2], [0.0] * 3, [0.0] * 3)
    p, f, _ = _order(host, 4, 1, 1, [], [], [])
    assert len(p) == 0 and list(f) == [0] * 9


def test_random_small_systems(host):
    rng = np.random.default_rng(20250131)
    seen_inert_only = seen_none = seen_empty = 0
    for trial in range(120):
        ncell = int(rng.choice([1, 2, 3, 8, 27, 64]))
        n = int(rng.integers(0, 6 * ncell + 3))
        share = rng.choice([0.0, 0.1, 0.27, 0.6, 1.0])
        kind = np.where(rng.random(n) < share, 3, rng.integers(0, 3, n))
        q = np.array([KINDS[k][0] for k in kind], dtype=np.float64)
        alpha = np.array([KINDS[k][1] for k in kind], dtype=np.float64)
        cell = rng.integers(0, ncell, n) if trial % 3 else np.minimum(rng.integers(0, 2 * ncell, n), ncell - 1)   # (a crowded last cell)
        pol_first = 0 if trial % 5 == 4 else 1
        inert = _check_system(host, ncell, cell, q, alpha, pol_first)
        for c in range(ncell):
            m = cell == c
            seen_empty += not m.any()
            seen_inert_only += bool(m.any() and inert[m].all())
            seen_none += bool(m.any() and not inert[m].any())
    assert seen_empty > 20 and seen_inert_only > 20 and seen_none > 20
