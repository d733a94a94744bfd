"""The minimum-image rule against the reference's OWN compiled Domain::closest_image.

tests/golden/ref_closest_image.npz records what oracle/_ref/ref_closest_image -- the reference's src/domain.cpp, compiled
from where it lies behind oracle/ref_seam/domain_harness.cpp -- returns for ~630 pairs in each of eleven boxes (orthogonal,
tilted up to and beyond |tilt| = L/2, partly periodic) and for all ordered pairs of two 90-atom systems.  Here, on the CPU:

  1. the fixture is what the compiled reference gives today (where the reference is present);
  2. the oracle's orc_closest_image returns the same bits for every pair;
  3. what the rule IS, stated independently by brute force over the 125 nearest lattice images: always a lattice translate,
     the nearest image in orthogonal boxes, and in tilted boxes the nearest image whenever the nearest image is closer than
     half the smallest perpendicular width -- beyond that often NOT (7 - 33 % of random pairs), which is what exact mode
     (no dipole-dipole cutoff) inherits and list mode never meets;
  4. the NumPy field / tensor builder that tests/test_gpu_closest_image.py feeds with the recorded images agrees with the
     oracle where the oracle is pinned (orthogonal box).
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import closest_image_ref as cir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "oracle", "_ref", "ref_closest_image")
BOXES = cir.box_names()
SYSTEMS = ["t3p1", "t8"]


def _run_reference(prd, tilt, periodic, triclinic, xi, xj):
    head = np.array(list(prd) + list(tilt) + list(periodic) + [triclinic, len(xi)], np.float64)
    body = np.hstack([np.ascontiguousarray(xi, np.float64), np.ascontiguousarray(xj, np.float64)])
    r = subprocess.run([EXE], input=head.tobytes() + body.tobytes(), capture_output=True, check=True, timeout=60)
    return np.frombuffer(r.stdout, np.float64).reshape(len(xi), 3)


def _oracle_images(oracle, prd, tilt, periodic, triclinic, xi, xj):
    L = oracle.lib()
    s = oracle.OrcSystem()
    s.prd[:] = [float(v) for v in prd]
    s.tilt[:] = [float(v) for v in tilt]
    s.periodic[:] = [int(v) for v in periodic]
    s.triclinic = int(triclinic)
    f = L.orc_closest_image
    f.restype = None
    f.argtypes = [C.POINTER(oracle.OrcSystem), oracle.dp, oracle.dp, oracle.dp]
    xi, xj = np.ascontiguousarray(xi, np.float64), np.ascontiguousarray(xj, np.float64)
    out = np.empty_like(xi)
    pi, pj, po = (a.ctypes.data for a in (xi, xj, out))
    ref = C.byref(s)
    for k in range(len(xi)):
        f(ref, C.cast(pi + 24 * k, oracle.dp), C.cast(pj + 24 * k, oracle.dp), C.cast(po + 24 * k, oracle.dp))
    return out


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def _ordered_pairs(sysd):
    n = len(sysd["x"])
    i, j = np.divmod(np.arange(n * n), n)
    return sysd["x"][i], sysd["x"][j], sysd["xjimage"].reshape(-1, 3)


def test_fixture_layout():
    """every box and class of the issue is there, the arrays are float64, and the file is no larger than the largest
    fixture the suite already held (tests/golden/oracle_exact_10792.npz)"""
    z = cir.fixture()
    assert z["xi"].dtype == z["xj"].dtype == z["xjimage"].dtype == z["sys_xjimage"].dtype == np.float64
    assert len(BOXES) == 11 and z["first"][-1] == len(z["xi"]) == len(z["klass"])
    for name in BOXES:
        b = cir.box(name)
        assert 500 <= len(b["xi"]) <= 700
        assert set(np.unique(b["klass"])) == {0, 1, 2, 3}
        assert _same_bits(b["xi"][b["klass"] == 3], b["xj"][b["klass"] == 3])
    assert z["sys_xjimage"].shape == (2, 90, 90, 3)
    assert os.path.getsize(os.path.join(cir.GOLD, "ref_closest_image.npz")) <= os.path.getsize(
        os.path.join(cir.GOLD, "oracle_exact_10792.npz"))


@pytest.mark.parametrize("name", BOXES + ["system:" + s for s in SYSTEMS])
def test_fixture_is_current(name):
    """1. the compiled reference reproduces the recorded images bit for bit"""
    if not os.path.exists(EXE):
        pytest.skip("oracle/_ref/ref_closest_image is not built (the reference tree is not on this machine)")
    if name.startswith("system:"):
        sd = cir.system(name[7:])
        xi, xj, want = _ordered_pairs(sd)
        got = _run_reference(sd["prd"], sd["tilt"], (1, 1, 1), 1, xi, xj)
    else:
        b = cir.box(name)
        got, want = _run_reference(b["prd"], b["tilt"], b["periodic"], b["triclinic"], b["xi"], b["xj"]), b["xjimage"]
    assert _same_bits(got, want)


@pytest.mark.parametrize("name", BOXES + ["system:" + s for s in SYSTEMS])
def test_oracle_closest_image_equals_the_reference_bit_for_bit(name, oracle):
    """2. orc_closest_image (oracle/polar_oracle.c) against the recorded reference: additions and subtractions only, so
    every class -- ties, coincident points, points several cells away -- has to come out with the same bits"""
    if name.startswith("system:"):
        sd = cir.system(name[7:])
        xi, xj, want = _ordered_pairs(sd)
        got = _oracle_images(oracle, sd["prd"], sd["tilt"], (1, 1, 1), 1, xi, xj)
        assert _same_bits(got, want)
        return
    b = cir.box(name)
    got = _oracle_images(oracle, b["prd"], b["tilt"], b["periodic"], b["triclinic"], b["xi"], b["xj"])
    for k in range(4):
        m = b["klass"] == k
        bad = np.flatnonzero((got[m].view(np.uint64) != b["xjimage"][m].view(np.uint64)).any(1))
        assert len(bad) == 0, ("class", "abcd"[k], "first mismatch", b["xi"][m][bad[0]], b["xj"][m][bad[0]],
                               got[m][bad[0]], b["xjimage"][m][bad[0]])


@pytest.mark.parametrize("name", BOXES)
def test_what_the_rule_is(name):
    """3. brute force over the 125 images i a + j b + k c, |i|, |j|, |k| <= 2, around the reference's image.

    Shares of class (a) / (b) pairs whose reference image is NOT the nearest image (the fixture as committed):
    tri_16_3p1 7.6 %, tri_16_half_pmp 12.2 %, tri_16_half_mpm 12.5 %, tri_20_14_12_half 23.0 %, tri_16_large_tilt 8.7 %,
    tri_ppf 8.0 %, tri_fpp 33.3 %; 0 in every box without tilt.  Such a pair always has a nearest-image distance of at
    least half the shortest periodic box edge (if every component of the nearest image were inside its half edge, the
    z, y, x sequence would find exactly it), and never one below half the smallest perpendicular width."""
    b = cir.box(name)
    prd, tilt, per = b["prd"], b["tilt"], b["periodic"]
    h = cir.cell(prd, tilt)
    # a lattice translate of xj, whole lattice vectors, none along a non-periodic dimension
    nlat = (b["xjimage"] - b["xj"]) @ np.linalg.inv(h)
    assert np.max(np.abs(nlat - np.rint(nlat))) < 1e-9
    assert not np.any(np.rint(nlat)[:, np.asarray(per) == 0])
    d = b["xjimage"] - b["xi"]
    r = np.sqrt((d ** 2).sum(-1))
    _, rmin = cir.nearest(prd, tilt, per, d)
    far = r > rmin * (1 + 1e-12) + 1e-12
    ab = b["klass"] < 2
    print("%-20s class a/b pairs whose reference image is not the nearest: %d of %d = %.1f %%; closest such pair %.3f A"
          % (name, far[ab].sum(), ab.sum(), 100.0 * far[ab].mean(), rmin[far].min() if far.any() else np.nan))
    tilted = bool(b["triclinic"]) and bool(np.any(tilt != 0.0))
    if not tilted:
        assert not far.any()          # orthogonal (or zero tilt): the nearest image, ties aside (compared by distance)
        return
    w = cir.widths(prd, tilt, per)
    assert not far[rmin < 0.5 * w.min() * (1 - 1e-12)].any()
    edge = min(prd[k] for k in range(3) if per[k])
    assert far[ab].sum() >= 20        # the fixture holds enough of what only the reference's own sequence decides
    assert rmin[far].min() >= 0.5 * edge * (1 - 1e-12)


@pytest.mark.parametrize("name", SYSTEMS)
def test_recorded_systems(name):
    """the two 90-atom systems: no two atoms closer than 1.9 A, the recorded image of (j, i) is the mirror of (i, j) to
    rounding, and hundreds of pairs whose image is not the nearest"""
    sd = cir.system(name)
    x, n = sd["x"], len(sd["x"])
    d = (x[:, None, :] - sd["xjimage"])
    assert _same_bits(sd["xjimage"][np.arange(n), np.arange(n)], x)
    assert np.max(np.abs(d + d.transpose(1, 0, 2))) <= 8 * np.spacing(np.abs(x).max())
    off = ~np.eye(n, dtype=bool)
    _, rmin = cir.nearest(sd["prd"], sd["tilt"], (1, 1, 1), d[off])
    assert rmin.min() >= 1.9
    far = np.sqrt((d[off] ** 2).sum(-1)) > rmin * (1 + 1e-12)
    print("system %s: %d of %d ordered pairs not at the nearest image" % (name, far.sum(), far.size))
    assert far.sum() >= 400


def test_numpy_builder_against_the_oracle_in_the_orthogonal_twin(wl, oracle):
    """4. closest_image_ref.static_field / dipole_matrix on the ORTHOGONAL twin of the 90-atom system (same positions,
    tilt removed; the orthogonal branch of the oracle is pinned by the reference's goldens), displacements from
    orc_closest_image: ef_static and every tensor block to 1e-13 relative."""
    sd = cir.system("t3p1")
    x, n = sd["x"], len(sd["x"])
    s = cir.mini_system(wl, x, sd["prd"], (0.0, 0.0, 0.0), 0, 7.5, extra=["precision", "1e-13", "max_iterations", "200"])
    i, j = np.divmod(np.arange(n * n), n)
    img = _oracle_images(oracle, sd["prd"], (0, 0, 0), (1, 1, 1), 0, x[i], x[j]).reshape(n, n, 3)
    D = cir.pair_del(x, img)
    ref = oracle.compute(s, eflag=1, vflag=2)
    ef = cir.static_field(D, s.q, s.molecule, s.settings.cut_coul, s.qqrd2e)
    assert np.any(ref["ef_static"])
    assert np.max(np.abs(ef - ref["ef_static"])) <= 1e-13 * np.max(np.abs(ref["ef_static"]))
    st, keep = oracle.make_struct(s)
    Mo = np.zeros((3 * n, 3 * n))
    f = oracle.lib().orc_build_dipole_field_matrix
    f.restype = None
    f.argtypes = [C.POINTER(oracle.OrcSystem), oracle.dp]
    f(C.byref(st), Mo.ctypes.data_as(oracle.dp))
    M = cir.dipole_matrix(D, s.alpha, s.settings.polar_damp)
    pol = np.repeat(s.alpha != 0.0, 3)
    assert np.array_equal(np.diag(M)[pol], np.diag(Mo)[pol])             # 1 / alpha
    Mb, Mob = (a.reshape(n, 3, n, 3).transpose(0, 2, 1, 3) for a in (M, Mo))
    offd = ~np.eye(n, dtype=bool)
    scale = np.abs(Mob).max(axis=(2, 3))
    assert np.all(np.abs(Mb - Mob).max(axis=(2, 3))[offd] <= 1e-13 * scale[offd])
    # and the solve: the oracle's ranked Gauss-Seidel at precision 1e-13 against the direct solve
    mu, epol = cir.solve_dipoles(M, ef, s.alpha)
    assert np.max(np.abs(mu - ref["mu"])) <= 1e-9 * np.max(np.abs(mu))
    assert abs(epol - ref["eng_pol"]) <= 1e-9 * abs(epol)
