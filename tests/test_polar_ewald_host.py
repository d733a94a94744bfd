"""CPU tests of `polar_ewald <accuracy>`: the keyword through the pair_style grammar (library and Python mirror), and the
NumPy implementation of the Ewald static field, forces and virial (tests/ewald_numpy.py) checked against itself and
against a brute-force lattice sum."""
import math

import numpy as np
import pytest

import ewald_numpy as ew


def test_keyword_default_accept_and_errors(pkg, wl):
    p = pkg.PolarPair(0)
    p.settings(["9.0", "9.0"])
    assert p.get_settings().polar_ewald == 0.0
    assert wl.parse_pair_style_args(["9.0", "9.0"]).polar_ewald == 0.0
    args = ["9.0", "9.0", "dd_cutoff", "8.5", "polar_ewald", "1e-6"]
    p.settings(args)
    s = p.get_settings()
    assert s.polar_ewald == 1e-6 and wl.parse_pair_style_args(args).polar_ewald == 1e-6
    assert s.dd_cutoff == 8.5 and s.polar_gs_ranked == 1   # the other keywords are unaffected
    for bad in ("-1", "1", "2.5"):
        with pytest.raises(pkg.PolarError) as e:
            pkg.PolarPair(0).settings(["9.0", "9.0", "polar_ewald", bad])
        assert "Illegal pair_style command" in str(e.value)
        with pytest.raises(ValueError, match="Illegal pair_style command"):
            wl.parse_pair_style_args(["9.0", "9.0", "polar_ewald", bad])
    p.settings(["9.0", "9.0", "polar_ewald", "0"])
    assert p.get_settings().polar_ewald == 0.0


def test_load_system_carries_the_keyword(pkg, wl):
    from helpers import GOLD
    import os
    s, _ = wl.load_fixture(os.path.join(GOLD, "bulk_h2.npz"), extra_args=["polar_ewald", "1e-5"])
    assert s.settings.polar_ewald == 1e-5
    p = pkg.PolarPair(0)
    p.load_system(s)
    assert p.get_settings().polar_ewald == 1e-5


def _box(n=12, L=11.0, seed=5, tilt=(0.0, 0.0, 0.0)):
    rng = np.random.default_rng(seed)
    H = ew.cell((L, L * 1.1, L * 0.95), tilt)
    s = rng.uniform(0, 1, (n, 3))
    x = s @ H.T
    q = rng.normal(0, 0.7, n)
    q -= q.mean()
    mol = np.array([1, 1, 1, 2, 2, 0, 0, 3, 3, 0, 0, 0][:n])
    mu = rng.normal(0, 0.3, (n, 3))
    return x, q, mol, mu, H


def test_field_does_not_depend_on_g():
    x, q, mol, _, H = _box()
    cut = 5.2
    g1, g2 = 1.0, 1.15                       # erfc(g cut) <= 1e-7 for both
    assert math.erfc(g1 * cut) <= 1e-7
    e1 = ew.field(x, q, mol, H, cut, g1, 1e-16)
    e2 = ew.field(x, q, mol, H, cut, g2, 1e-16)
    rms = np.sqrt(np.mean(e1 ** 2))
    assert np.sqrt(np.mean((e1 - e2) ** 2)) / rms < 1e-7


def test_field_equals_brute_force_lattice_sum():
    x, q, mol, _, _ = _box(n=8, L=9.0)
    H = ew.cell((9.0, 9.0, 9.0))              # cubic: the image shells are spheres, the surface term is 4 pi P / 3V
    x = np.mod(x, 9.0)
    e = ew.field(x, q, mol, H, 4.2, 1.0, 1e-16)
    b = ew.brute_field(x, q, mol, H, 4.2, 20)
    assert np.max(np.abs(e - b)) / np.max(np.abs(e)) < 1e-5


def test_forces_are_the_gradient_of_the_energy():
    x, q, mol, mu, H = _box()
    cut, g, acc = 5.2, 0.7, 1e-10
    f, _ = ew.forces_virial(x, q, mol, mu, H, cut, g, acc)
    h = 1e-5
    for i in (0, 3, 7, 10):
        for a in range(3):
            xp, xm = x.copy(), x.copy()
            xp[i, a] += h
            xm[i, a] -= h
            fd = -(ew.energy(xp, q, mol, mu, H, cut, g, acc) - ew.energy(xm, q, mol, mu, H, cut, g, acc)) / (2 * h)
            assert abs(fd - f[i, a]) < 1e-6 * max(1.0, np.max(np.abs(f)))
    assert np.max(np.abs(f.sum(0))) < 1e-10 * np.max(np.abs(f))


@pytest.mark.parametrize("tilt", [(0.0, 0.0, 0.0), (1.3, -0.8, 0.6)])
def test_virial_matches_an_affine_strain(tilt):
    x, q, mol, mu, H = _box(tilt=tilt)
    cut, g, acc = 5.2, 0.7, 1e-10
    _, v = ew.forces_virial(x, q, mol, mu, H, cut, g, acc)
    h = 1e-6
    comps = [(0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)]
    for c, (a, b) in enumerate(comps):
        # LAMMPS' v_ab = sum r_a F_b = -dU/d eps_ba for the strain r_b -> r_b + eps_ba r_a (dipoles held fixed)
        def u(t):
            e = np.eye(3)
            e[b, a] += t
            return ew.energy(x @ e.T, q, mol, mu, e @ H, cut, g, acc)
        fd = -(u(h) - u(-h)) / (2 * h)
        assert abs(fd - v[c]) < 1e-6 * max(1.0, np.max(np.abs(v))), (c, fd, v[c])


def test_triclinic_with_zero_tilt_is_the_orthogonal_box():
    x, q, mol, mu, H = _box()
    a = ew.field(x, q, mol, H, 5.2, 0.7, 1e-10)
    b = ew.field(x, q, mol, ew.cell(np.diag(H), (0.0, 0.0, 0.0)), 5.2, 0.7, 1e-10)
    assert np.array_equal(a, b)
    fa, va = ew.forces_virial(x, q, mol, mu, H, 5.2, 0.7, 1e-10)
    fb, vb = ew.forces_virial(x, q, mol, mu, ew.cell(np.diag(H)), 5.2, 0.7, 1e-10)
    assert np.array_equal(fa, fb) and np.array_equal(va, vb)
