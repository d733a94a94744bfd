"""tests/ewald_kspace_ref.py (long double, phases from the integer (h, k, l) reduced modulo 1) against tests/ewald_numpy.py
(FP64, phases x @ k.T), which the finite-difference and brute-force tests of tests/test_polar_ewald_host.py pin.

Two cases: 60 atoms as the `_mini` of tests/test_gpu_polar_ewald.py, cubic L = 20 and tilted by (2.1, -1.4, 1.2), g = 0.32,
accuracy 1e-8.  Bound: 1e-12 of scale (the FP64 side carries |k.x| eps, about 1e-14, in every phase).  And the one thing
the reduction modulo 1 promises on its own: S(k) does not move when every atom is shifted by a lattice vector."""
import os

import numpy as np
import pytest

import ewald_kspace_ref as kr
import ewald_numpy as ew

pytestmark = pytest.mark.skipif(not kr.available(), reason="np.longdouble has no 64-bit mantissa here")

G, ACC, L, E2S = 0.32, 1e-8, 20.0, float(np.sqrt(332.06371))
CASES = {"cubic": (0.0, 0.0, 0.0), "tilted": (2.1, -1.4, 1.2)}
TOL = 1e-12


def _system(tilt, n=60, seed=7):
    rng = np.random.default_rng(seed)
    q = rng.normal(0, 0.4, n)
    q -= q.mean()
    mu = rng.normal(0, 0.3, (n, 3)) * (rng.uniform(size=n) < 0.7)[:, None]
    H = ew.cell((L, L, L), tilt)
    x = rng.uniform(0, 1, (n, 3)) @ H.T
    ef_s = rng.normal(0, 1.0, (n, 3))
    mol = np.zeros(n, np.int32)
    return H, x, q, mu, ef_s, mol


@pytest.fixture(scope="module", params=sorted(CASES))
def both(request):
    tilt = CASES[request.param]
    H, x, q, mu, ef_s, mol = _system(tilt)
    k, c = ew.kvectors(H, G, ACC)
    hkl = kr.hkl_of(k, (L, L, L), tilt)
    assert np.abs(2 * np.pi * hkl[:, :3] @ np.linalg.inv(H) - k).max() < 1e-12          # the integers are the right ones
    ref = kr.reference((L, L, L), tilt, G, E2S, x, q, mu, ef_s, hkl, np.hstack([k, c[:, None]]))
    erec = ew.field(x, q, mol, H, 8.0, G, ACC, E2S, parts=True)[1]
    _, f_rec, _, w_rec = ew.forces_virial(x, q, mol, mu, H, 8.0, G, ACC, E2S, parts=True)
    return dict(name=request.param, tilt=tilt, x=x, q=q, hkl=hkl, ref=ref, erec=erec, f_rec=f_rec, w_rec=w_rec, nk=len(k))


def test_field_forces_and_virial_against_ewald_numpy(both):
    r = both["ref"]
    assert both["nk"] > 1000
    e_e = float(np.max(np.abs(r["erec"] - both["erec"])) / r["erec_scale"])
    e_f = float(np.max(np.abs(r["f"] - both["f_rec"]) / r["f_scale"][:, None]))
    e_w = float(np.max(np.abs(r["w_atom"] + r["w_k"] - both["w_rec"]) / (r["w_atom_scale"] + r["w_k_scale"])))
    print("%s: %d k-vectors; of scale: E_rec %.2e  F_rec %.2e  reciprocal virial %.2e" % (both["name"], both["nk"], e_e, e_f, e_w))
    assert e_e <= TOL and e_f <= TOL and e_w <= TOL
    # the scales are what they are called: no value exceeds the sum of its terms' absolute values
    assert np.all(np.abs(r["erec"]) <= r["erec_scale"]) and np.all(np.abs(r["f"]) <= r["f_scale"][:, None])
    assert np.all(np.hypot(r["S"][:, 0], r["S"][:, 1]) <= r["S_scale"]) and np.all(np.hypot(r["M"][:, 0], r["M"][:, 1]) <= r["M_scale"])
    assert np.all(np.abs(r["w_k"]) <= r["w_k_scale"]) and np.all(np.abs(r["w_atom"]) <= r["w_atom_scale"])


def test_probe_compiles_and_plans_the_cases(pkg, tmp_path):
    """tests/ewald_kspace_probe/ewald_kspace_probe.hip builds for gfx950 with the library's flags, and its host-only plan entry
    gives every box of tests/test_gpu_ewald_kspace.py the nm, nk and tile it was chosen for -- and MOF-5 at g = 0.6, accuracy
    1e-12 (tests/test_gpu_polar_ewald.py) chunks longer than a tile.  No GPU is touched."""
    import ewald_kspace_load as kl
    if not os.path.exists(pkg.HIPCC):
        pytest.skip("hipcc not available")
    probe = kl.load(pkg, tmp_path)
    for name, (prd, tilt, g, acc, nm, nk, tile) in kl.CASES.items():
        pl = probe.plan(prd, tilt, g, acc, 70)
        assert (pl["nm"], pl["nk"]) == (nm, nk), name
        assert tile is None or pl["tile"] == tile, name
        assert pl["nchunk"] * pl["chunk"] >= 70 > (pl["nchunk"] - 1) * pl["chunk"], name
    pl = probe.plan((25.669,) * 3, kl.NOTILT, 0.6, 1e-12, 1349)
    assert (pl["nk"], pl["nm"], pl["tile"], pl["chunk"]) == (35855, 25, 32, 45)


def test_structure_factors_do_not_see_a_lattice_shift(both):
    prd = (L, L, L)
    H, _ = kr.cell(prd, both["tilt"])
    S0, scale = kr.structure_factors(prd, both["tilt"], both["x"], both["q"], both["hkl"])
    assert np.array_equal(S0, both["ref"]["S"])
    for nvec in ((1, 0, 0), (0, -1, 0), (1, -1, 1)):
        shift = H[:, 0] * nvec[0] + H[:, 1] * nvec[1] + H[:, 2] * nvec[2]
        S1, _ = kr.structure_factors(prd, both["tilt"], both["x"], both["q"], both["hkl"], shift=shift)
        err = float(np.max(np.abs(S1 - S0)) / scale)
        print("%s: shift %s moves S(k) by %.2e of scale" % (both["name"], nvec, err))
        assert err <= 1e-17
