"""The device minimum-image functions, and the kernels built on them, against the reference's compiled
Domain::closest_image as recorded in tests/golden/ref_closest_image.npz (see tests/test_closest_image.py for what the
fixture holds and why the triclinic sequence is worth pinning: it often does not return the nearest image).

  * tests/image_probe/image_probe.hip calls min_image_del, min_image_rint and min_image_rint_w<false / true> of
    csrc/polar_common.hpp once per recorded pair;
  * exact mode (no dipole-dipole cutoff: 7 - 12 % of the tensor blocks of these cells sit on a non-nearest image) against a
    NumPy float64 solve whose tensor is built from the RECORDED images;
  * list mode in tilted and thin boxes against brute force over the 27 nearest cells.

Nothing here reads the reference tree: only the fixture."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import closest_image_ref as cir

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
BOXES = cir.box_names()
SYSTEMS = ["t3p1", "t8"]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def probe(pkg, tmp_path_factory):
    """image_probe.hip compiled for gfx950 with the library's own flags, loaded after the library (and with it torch's HIP
    runtime, see pkg.lib)"""
    if not os.path.exists(pkg.HIPCC):
        pytest.skip("hipcc not available")
    pkg.lib()
    so = str(tmp_path_factory.mktemp("image_probe") / "libimage_probe.so")
    subprocess.check_call([pkg.HIPCC] + pkg.HIP_FLAGS + ["-Wno-unused-function", "-I", os.path.join(os.path.dirname(pkg.__file__), "csrc"),
                           "-o", so, os.path.join(HERE, "image_probe", "image_probe.hip")])
    lib = C.CDLL(so)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    lib.image_probe_run.restype = C.c_int
    lib.image_probe_run.argtypes = [dp, dp, ip, C.c_int, C.c_longlong, dp, dp, ip]

    def run(prd, tilt, periodic, triclinic, xi, xj):
        n = len(xi)
        prd, tilt = np.ascontiguousarray(prd, np.float64), np.ascontiguousarray(tilt, np.float64)
        per = np.ascontiguousarray(periodic, np.int32)
        pairs = np.ascontiguousarray(np.hstack([xi, xj]), np.float64)
        out, flag = np.zeros((n, 12)), np.zeros((n, 2), np.int32)
        rc = lib.image_probe_run(prd.ctypes.data_as(dp), tilt.ctypes.data_as(dp), per.ctypes.data_as(ip), int(triclinic), n,
                                 pairs.ctypes.data_as(dp), out.ctypes.data_as(dp), flag.ctypes.data_as(ip))
        assert rc == 0, "HIP error %d in image_probe_run" % rc
        return dict(del_ci=out[:, 0:3], del_rint=out[:, 3:6], del_w0=out[:, 6:9], del_w1=out[:, 9:12],
                    flag_w0=flag[:, 0], flag_w1=flag[:, 1])
    return run


@pytest.fixture(scope="module")
def probed(probe):
    """every box of the fixture through the probe, one launch per box, once for all the tests below"""
    out = {}
    for name in BOXES:
        b = cir.box(name)
        out[name] = probe(b["prd"], b["tilt"], b["periodic"], b["triclinic"], b["xi"], b["xj"])
    return out


@pytest.mark.parametrize("name", BOXES)
def test_min_image_del_is_the_reference_image_bit_for_bit(name, probed):
    """min_image_del, every class (ties, coincident points, points several cells out): x_i + (-del) has the bits of the
    reference's xjimage -- the promise of the comment above wrap_ci, "pairs at exactly L/2 pick the same image"."""
    b, o = cir.box(name), probed[name]
    got = b["xi"] + (-o["del_ci"])
    for k in range(4):
        m = b["klass"] == k
        bad = np.flatnonzero((_bits(got[m]) != _bits(b["xjimage"][m])).any(1))
        assert len(bad) == 0, ("class", "abcd"[k], len(bad), "first", b["xi"][m][bad[0]], b["xj"][m][bad[0]], got[m][bad[0]],
                               b["xjimage"][m][bad[0]])


def test_min_image_del_on_the_recorded_systems(probe):
    """the same for all ordered pairs of the two 90-atom systems the exact-mode test below runs"""
    for name in SYSTEMS:
        sd = cir.system(name)
        n = len(sd["x"])
        i, j = np.divmod(np.arange(n * n), n)
        o = probe(sd["prd"], sd["tilt"], (1, 1, 1), 1, sd["x"][i], sd["x"][j])
        assert np.array_equal(_bits(sd["x"][i] + (-o["del_ci"])), _bits(sd["xjimage"].reshape(-1, 3)))


@pytest.mark.parametrize("name", BOXES)
def test_min_image_rint_random_and_unwrapped_pairs(name, probed):
    """min_image_rint, classes (a) and (b): every component within 8 ulp of the largest coordinate of the pair from
    x_i - xjimage of the reference.  (One FMA per lattice vector against the reference's repeated additions for a point
    up to four cells out; the two can choose different images only at exact ties, which these classes do not hold.)
    Measured on the MI355X: 6 ulp at worst, in the 16 A cell with the non-dyadic tilt (3.1, -2.2, 1.7), where every tilt factor
    carried into x rounds; 1 - 2.75 ulp in the other ten boxes."""
    b, o = cir.box(name), probed[name]
    m = b["klass"] < 2
    want = b["xi"][m] - b["xjimage"][m]
    ulp = np.spacing(np.maximum(np.abs(b["xi"][m]).max(1), np.abs(b["xj"][m]).max(1)))
    err = np.abs(o["del_rint"][m] - want).max(1) / ulp
    print("%-20s min_image_rint against the reference, classes a/b: worst %.2f ulp of the largest coordinate" % (name, err.max()))
    assert err.max() <= 8.0


@pytest.mark.parametrize("name", BOXES)
def test_min_image_rint_ties_and_coincident_points(name, probed):
    """min_image_rint, classes (c) and (d), where rint() and the reference's comparisons may legitimately choose different
    images: the result is x_i - x_j plus whole lattice vectors (none along a non-periodic dimension), |del_k| <= L_k / 2
    in every periodic dimension to one ulp of the largest coordinate of the pair, and a non-periodic component that no tilt
    factor feeds (z always; any in a box without tilt) keeps the bits of x_i - x_j."""
    b, o = cir.box(name), probed[name]
    m = b["klass"] >= 2
    xi, xj, got = b["xi"][m], b["xj"][m], o["del_rint"][m]
    per = np.asarray(b["periodic"]) != 0
    raw = xi - xj
    nlat = (got - raw) @ np.linalg.inv(cir.cell(b["prd"], b["tilt"]))
    assert np.max(np.abs(nlat - np.rint(nlat))) < 1e-9
    assert not np.any(np.rint(nlat)[:, ~per])
    ulp = np.spacing(np.maximum(np.abs(xi).max(1), np.abs(xj).max(1)))
    for k in range(3):
        if per[k]:
            assert np.all(np.abs(got[:, k]) <= 0.5 * b["prd"][k] + ulp)
        elif k == 2 or not np.any(b["tilt"] != 0.0) or not b["triclinic"]:
            assert np.array_equal(_bits(got[:, k]), _bits(raw[:, k]))
    d = b["klass"][m] == 3
    assert not np.any(got[d])         # coincident points: no displacement at all


@pytest.mark.parametrize("name", BOXES)
def test_min_image_rint_w(name, probed):
    """min_image_rint_w<TRI> (the list build): TRI = true returns the bits of min_image_rint, TRI = false the same in a box
    without tilt; the returned flag ("a lattice vector was taken off") is false exactly where the result has the bits of
    x_i - x_j."""
    b, o = cir.box(name), probed[name]
    assert np.array_equal(_bits(o["del_w1"]), _bits(o["del_rint"]))
    if not (b["triclinic"] and np.any(b["tilt"] != 0.0)):
        assert np.array_equal(_bits(o["del_w0"]), _bits(o["del_rint"]))
    raw = _bits(b["xi"] - b["xj"])
    for res, flag in ((o["del_w0"], o["flag_w0"]), (o["del_w1"], o["flag_w1"])):
        unshifted = (_bits(res) == raw).all(1)
        assert set(np.unique(flag)) <= {0, 1}
        assert np.array_equal(flag == 0, unshifted)
    assert o["flag_w1"].min() == 0 and o["flag_w1"].max() == 1     # both outcomes occur in every box


# ---------------------------------------------------------------------------------------------------------------------
# exact mode

# Largest difference between the ORACLE's solve (precision 1e-13, ranked and plain Gauss-Seidel) and the NumPy direct solve
# on the two recorded systems, measured on the CPU: mu 1.6e-14 of max|mu| (t8, ranked; 9.9e-15 on t3p1), eng_pol 5.8e-15
# relative.  The GPU gets ten times the larger figure for both (a different sweep order stops at a different distance from
# the fixed point under the same 1e-13 stop rule), capped at 1e-8.
ORACLE_VS_NUMPY = 1.6e-14
SOLVE_TOL = min(10 * ORACLE_VS_NUMPY, 1e-8)


def _numpy_reference(s, D, cut_coul):
    ef = cir.static_field(D, s.q, s.molecule, cut_coul, s.qqrd2e)
    mu, epol = cir.solve_dipoles(cir.dipole_matrix(D, s.alpha, s.settings.polar_damp), ef, s.alpha)
    return ef, mu, epol


@pytest.mark.parametrize("name", SYSTEMS)
def test_exact_mode_follows_the_reference_images(name, wl, pkg):
    """Exact mode (cut_coul 7.5, precision 1e-13, ranked and plain Gauss-Seidel) on the two recorded 90-atom systems in
    tilted 16 A cells, against NumPy float64: static field and dipole tensor from the RECORDED reference images (532 and
    934 of the 8010 ordered pairs are not at the nearest image), a direct solve of (1 / alpha + T) mu = E over the
    polarizable atoms, eng_pol = -1/2 sum mu . E.

    Tolerance for mu (of max|mu|) and eng_pol (relative): SOLVE_TOL = 1.6e-13, ten times what separates the oracle's own
    solve from the NumPy solve on these systems (1.6e-14, measured on the CPU).  ef_static: 1e-10 of its maximum.
    The test bites: with the tensor rebuilt from NEAREST images the NumPy dipoles move by 2.9e-3 (t3p1) and 3.1e-3 (t8) of
    max|mu| (asserted: at least 100 x SOLVE_TOL), while the static field, whose cutoff lies below half the box edge, does
    not change at all."""
    sd = cir.system(name)
    x, n = sd["x"], len(sd["x"])
    D = cir.pair_del(x, sd["xjimage"])
    ef = mu = epol = None
    for extra in ([], ["polar_gs_ranked", "no", "polar_gs", "yes"]):
        s = cir.mini_system(wl, x, sd["prd"], sd["tilt"], 1, 7.5, extra=["precision", "1e-13", "max_iterations", "200"] + extra)
        if ef is None:
            ef, mu, epol = _numpy_reference(s, D, 7.5)
        p = pkg.pair_from_system(s)
        out = p.compute()
        p.close()
        assert out["status"] == 0
        e_ef = np.max(np.abs(out["ef_static"] - ef)) / np.max(np.abs(ef))
        e_mu = np.max(np.abs(out["mu"] - mu)) / np.max(np.abs(mu))
        e_ep = abs(out["eng_pol"] - epol) / abs(epol)
        print("%s %-6s iterations %d  ef_static %.2e  mu %.2e  eng_pol %.2e  (tolerance %.1e)"
              % (name, "plain" if extra else "ranked", out["iterations"], e_ef, e_mu, e_ep, SOLVE_TOL))
        assert e_ef <= 1e-10
        assert e_mu <= SOLVE_TOL
        assert e_ep <= SOLVE_TOL
    # the companion: nearest images instead of the reference's
    best, _ = cir.nearest(sd["prd"], sd["tilt"], (1, 1, 1), (x[:, None, :] - sd["xjimage"]).reshape(-1, 3))
    Dn = cir.upper_antisymmetric(best.reshape(n, n, 3))
    efn, mun, _ = _numpy_reference(s, Dn, 7.5)
    moved = np.max(np.abs(mun - mu)) / np.max(np.abs(mu))
    print("%s: dipoles from nearest images differ from the pinned ones by %.2e of max|mu|" % (name, moved))
    assert moved >= 100 * SOLVE_TOL
    assert np.array_equal(efn, ef)


# ---------------------------------------------------------------------------------------------------------------------
# list mode

def _thin_box_system():
    """90 atoms in the orthogonal 20 x 14 x 12 box, no two (over all images) closer than 1.9 A"""
    prd, tilt = np.array([20.0, 14.0, 12.0]), np.zeros(3)
    rng = np.random.default_rng(5)
    sh = cir.image_shifts(prd, tilt, reach=1)
    x = np.zeros((0, 3))
    while len(x) < 90:
        p = rng.uniform(0, 1, 3) * prd
        if len(x) == 0 or np.sqrt((((x - p)[:, None, :] + sh[None]) ** 2).sum(-1)).min() >= 1.9:
            x = np.vstack([x, p])
    return dict(name="ortho_20_14_12", prd=prd, tilt=tilt, x=x)


def _list_case(name):
    return _thin_box_system() if name == "ortho_20_14_12" else cir.system(name)


@pytest.mark.parametrize("name", SYSTEMS + ["ortho_20_14_12"])
def test_list_mode_pair_count_against_brute_force(name, wl, pkg):
    """List mode with cut_coul = dd_cutoff = 0.999 x half the smallest perpendicular width (computed here from the cell
    vectors), in the two tilted cells and in a thin orthogonal box.

    What k_nl_build admits to the dipole-dipole list (csrc/polar_lists.hpp): the directed pairs (i, j), j != i, BOTH
    polarizable (alpha != 0), with minimum-image rsq < dd_cutoff^2 -- strictly.  dd_pairs is their number; the NumPy count
    runs over the 27 images of every directed pair (at most one can be inside below half the width).  No pair of these
    inputs lies within 1e-9 A of the cutoff (asserted), so the strict comparison cannot go either way.  ef_static is
    compared as in exact mode (<=, molecule rule, nearest image: inside half the width that IS the reference's image)."""
    sd = _list_case(name)
    x, n = sd["x"], len(sd["x"])
    tri = int(np.any(sd["tilt"] != 0.0))
    w = cir.widths(sd["prd"], sd["tilt"])
    cut = 0.999 * 0.5 * w.min()
    s = cir.mini_system(wl, x, sd["prd"], sd["tilt"], tri, cut,
                        extra=["dd_cutoff", repr(float(cut)), "precision", "1e-13", "max_iterations", "200"])
    sh = cir.image_shifts(sd["prd"], sd["tilt"], reach=1)
    r = np.sqrt(((x[:, None, None, :] - x[None, :, None, :] + sh[None, None]) ** 2).sum(-1))     # [i, j, image]
    off = ~np.eye(n, dtype=bool)
    assert np.abs(r[off] - cut).min() > 1e-9
    pol = s.alpha != 0.0
    inside = (r < cut) & off[:, :, None] & pol[:, None, None] & pol[None, :, None]
    assert inside.sum(-1).max() <= 1
    p = pkg.pair_from_system(s)
    out = p.compute()
    p.close()
    assert out["status"] == 0
    print("%s: cutoff %.4f, dd_pairs %d, brute force %d" % (name, cut, out["dd_pairs"], inside.sum()))
    assert out["dd_pairs"] == inside.sum() > 0
    k = r.argmin(-1)
    D = x[:, None, :] - x[None, :, :] + sh[k]
    D[~off] = 0.0
    ef = cir.static_field(D, s.q, s.molecule, cut, s.qqrd2e)
    assert np.max(np.abs(out["ef_static"] - ef)) <= 1e-10 * np.max(np.abs(ef))


@pytest.mark.parametrize("name", SYSTEMS + ["ortho_20_14_12"])
def test_list_mode_cutoff_against_the_perpendicular_width(name, wl, pkg):
    """A cutoff 0.1 % above half the smallest perpendicular width is refused ("box lengths"), one 0.1 % below is accepted;
    the widths come from the cell vectors (NumPy), not from the library."""
    sd = _list_case(name)
    tri = int(np.any(sd["tilt"] != 0.0))
    half = 0.5 * cir.widths(sd["prd"], sd["tilt"]).min()
    if tri:
        assert half < 0.5 * sd["prd"].min() - 0.05      # the width, not the edge, is what decides here
    for factor, ok in ((1.001, False), (0.999, True)):
        cut = factor * half
        s = cir.mini_system(wl, sd["x"], sd["prd"], sd["tilt"], tri, cut, extra=["dd_cutoff", repr(float(cut))])
        p = pkg.pair_from_system(s)
        try:
            if ok:
                assert p.compute()["status"] == 0
            else:
                with pytest.raises(pkg.PolarError, match="box lengths"):
                    p.compute()
        finally:
            p.close()
