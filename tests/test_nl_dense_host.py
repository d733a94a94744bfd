"""The dense-trip enumeration of the list build (csrc/polar_nl_dense.hpp: run table, stream position -> atom index) on the
host.

The header is plain C++: g++ builds tests/nl_dense/nl_dense_walk.cpp around it, a stand-alone program (with the address and
undefined-behaviour sanitizers where the toolchain has them) that emulates k_nl_build's wave -- exclusive scan of the row
lengths, mask of the rows with atoms, one nl_dense_shift call per lane and trip -- and prints the atom index of every
(trip, lane).  For every run table that sequence must be the plain concatenation of the runs (stencil rows in order, piece 0
before piece 1, ascending index: the visiting order of the per-run walk), every position at or beyond the total must be idle,
and the number of trips must be ceil(total / 64).  Exact comparison: these are integers."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "lammps-induced-dipole-polarization-pair-style_amd")
SRC = os.path.join(ROOT, "tests", "nl_dense", "nl_dense_walk.cpp")


@pytest.fixture(scope="module")
def walker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("nl_dense") / "nl_dense_walk")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", f"-I{PKG}/csrc", "-o", exe, SRC]
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr:      # a toolchain without the sanitizer runtimes: the plain program
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def _expected(table):
    out = []
    for ra0, rb0, ra1, rb1 in table:
        out += list(range(ra0, rb0)) + list(range(ra1, rb1))
    return out


def _named_tables():
    run = lambda a, n: (a, a + n)
    T = {}
    T["total 0, no rows"] = []
    T["total 0, 25 empty rows"] = [(7, 7, 0, 0)] * 25
    T["skipped rows (rb < ra) between runs"] = [(10, 40, 0, 0), (0, 0, 0, 0), (90, 80, 5, 3), (200, 230, 0, 0)]
    T["exactly 64"] = [(100, 164, 0, 0)]
    T["exactly 128"] = [(100, 228, 0, 0)]
    T["64 then 64: a row ends on a trip boundary"] = [(0, 64, 0, 0), (500, 564, 0, 0), (900, 903, 0, 0)]
    T["64 + 64 as the two pieces of one row"] = [(1000, 1064, 0, 64)]
    T["one run longer than 3 x 64"] = [(31, 31 + 3 * 64 + 17, 0, 0)]
    T["one run of 5 x 64 between short ones"] = [(0, 3, 0, 0), (1000, 1320, 0, 0), (5, 9, 0, 0)]
    T["50 runs of length 1"] = [(*run(10 * k, 1), *run(5000 + 10 * k, 1)) for k in range(25)]
    T["both pieces in every row"] = [(*run(300 * k + 200, 37 + k), *run(300 * k, 11 + 2 * k)) for k in range(25)]
    T["piece 0 empty, piece 1 not"] = [(50, 50, 400, 470), (600, 610, 0, 0), (70, 70, 0, 90)]
    T["empty rows first and last"] = [(0, 0, 0, 0)] * 3 + [(64, 200, 0, 0)] + [(9, 9, 0, 0)] * 3
    T["first run crosses several trips, then singles"] = [(0, 190, 0, 0)] + [(*run(1000 + 3 * k, 1), 0, 0) for k in range(20)]
    return T


def _random_tables(n, seed):
    rng = np.random.default_rng(seed)
    tabs = []
    for _ in range(n):
        nsr = int(rng.integers(0, 26))
        kind = rng.integers(0, 4)
        t = []
        for _ in range(nsr):
            if kind == 0:      # the headline shape: runs of ~70 atoms, some rows skipped, a few wrapped
                l0 = 0 if rng.random() < 0.1 else int(rng.integers(20, 120))
                l1 = int(rng.integers(1, 60)) if rng.random() < 0.2 else 0
            elif kind == 1:    # short runs, many empty
                l0 = int(rng.integers(0, 4)); l1 = int(rng.integers(0, 3))
            elif kind == 2:    # lengths around the trip size
                l0 = int(rng.choice([0, 1, 63, 64, 65, 127, 128, 129])); l1 = int(rng.choice([0, 0, 1, 63, 64, 65]))
            else:              # whole rows of a small box, no second piece
                l0 = int(rng.integers(0, 400)); l1 = 0
            a0, a1 = int(rng.integers(0, 100000)), int(rng.integers(0, 100000))
            b0 = a0 + l0 if (l0 or rng.random() < 0.5) else a0 - int(rng.integers(1, 5))   # an empty run may be stored as rb < ra
            t.append((a0, b0, a1, a1 + l1))
        tabs.append(t)
    return tabs


def _run(walker, tables):
    text = "%d\n" % len(tables) + "".join("%d\n" % len(t) + "".join("%d %d %d %d\n" % r for r in t) for t in tables)
    r = subprocess.run([walker], input=text, capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    tok = r.stdout.split()
    pos, out = 0, []
    for _ in tables:
        total, trips = int(tok[pos]), int(tok[pos + 1])
        pos += 2
        out.append((total, trips, [int(v) for v in tok[pos:pos + 64 * trips]]))
        pos += 64 * trips
    assert pos == len(tok)
    return out


def _check(name, table, got):
    total, trips, seq = got
    want = _expected(table)
    assert total == len(want), name
    assert trips == -(-total // 64), name
    assert len(seq) == 64 * trips, name
    assert seq[:total] == want, name                       # every candidate once, in the visiting order of the per-run walk
    assert all(v == -1 for v in seq[total:]), name         # positions at or beyond the total are idle


def test_named_run_tables_come_out_as_the_concatenation_of_their_runs(walker):
    T = _named_tables()
    assert sum(len(_expected(t)) for t in T.values()) > 0
    for (name, table), got in zip(T.items(), _run(walker, list(T.values()))):
        _check(name, table, got)
    assert _run(walker, [T["total 0, no rows"]])[0] == (0, 0, [])


def test_random_run_tables_come_out_as_the_concatenation_of_their_runs(walker):
    tabs = _random_tables(4000, 20240607)
    got = _run(walker, tabs)
    both = sum(1 for t in tabs for r in t if r[1] > r[0] and r[3] > r[2])
    assert both > 1000                                     # rows with both pieces are well represented
    for k, (t, g) in enumerate(zip(tabs, got)):
        _check("random table %d" % k, t, g)
