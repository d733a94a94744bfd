"""The row kernels at the tightness of the pair probe: static field, one Jacobi sweep, polarization forces, energies and
virial of a 560-atom system against sums of tests/pair_ref.py over brute-force minimum-image pairs.

tests/test_gpu_math_probe.py shows that the arithmetic of one pair is right; this shows that the kernels add up every pair,
and add it once -- padded trips, the DUMMY record, two-lane record fetches, wave reductions, the list-mode sweep's LDS gather.
Every quantity is compared per atom (or per scalar) with a running error bound

    4 x sum_pairs(eps_pair x |terms|) + 4 x (n_terms + 4) x 2^-53 x sum |terms|

(eps_pair: the per-pair bound of the probe for the functions that kernel uses; the 4 covers the reduction order and FMA
contraction), never with one global tolerance.  A dropped or doubled pair is orders of magnitude above it, which the test
asserts: one in-cutoff pair removed from the reference sum of the longest row makes the comparison fail.

The system: a jittered 2.4 A lattice in one half of a 24 A periodic box and a 4.8 A one in the other, so that the rows of the
dipole-dipole list (dd_cutoff 9) take one, two and three 64-entry trips (asserted from a brute-force count); four-atom
molecules; a quarter of the atoms without charge, a quarter without polarizability; one 0.74 A pair inside a molecule.  The
coordinates are multiples of 2^-20 A, so that every minimum-image displacement is exact in FP64 however it is formed: the
reference sees the displacements the kernels see.  No LJ / Coulomb list (inum = 0): f, the energies and the virial hold the
polarization part alone.  One committed Jacobi sweep from a caller's mu0 (`use_previous yes`, `fixed_iteration yes
max_iterations 1`; the reference returns before its last copy, PS.cpp:1214): mu = alpha (E_static - T mu0).

Forces, energies and virial are summed from the dipoles the device returned (taken as exact inputs), so that their bound is
the force kernel's alone; mu itself is compared with alpha (E - T mu0) of the reference, its bound the static field's plus
the sweep's.  The reference is evaluated in long double (pair_ref: within 1e-17 of scale of 40-digit mpmath,
tests/test_pair_ref_host.py): 157,000 pairs a run.

Measured on the MI355X (every run prints its figures): no quantity above 0.4 % of its bound -- 2.5e-16 of sum|terms| at worst
(f, list mode, no damping), ef_static and mu 1.1e-16, the energies and the virial below 3e-17; with the pair (207, 490) at
8.987 A left out of the reference sums, ef_static misses its bound by a factor 1.9e8, mu by 6.4e7 and f by 2.8e9."""
import copy
import math

import numpy as np
import pytest

import math_probe_cases as mc
import pair_ref as pr

pytestmark = pytest.mark.gpu

EPS = math.ldexp(1.0, -53)
ULP = math.ldexp(1.0, -52)
L, CUT, PD = 24.0, 9.0, 2.1304
GRID = math.ldexp(1.0, -20)

# per-pair bounds, of scale (+ x the part of the scale that carries e^-a), by kernel:
#  static field: rsq (three roundings, entering r^-3 with weight 3/2), the library rsqrt (2 ulp, three times), four more
#                operations and the factor e2s -- the 16 x 2^-53 the probe asserts for the Ewald factors;
#  exact-mode sweep (tensor_scalars, libm): the probe's 8 x 2^-53 for s3, s5, rsq's roundings with weight 5/2, and the
#                eight operations of s3 mu - s5 d (d . mu): 24 x 2^-53;
#  list-mode sweep (tensor_scalars_lp): rsqrt_pos 3e-14, five times in s5; exp_neg_fast<10> 3.1e-13 on the damped part; the same
#                24 x 2^-53 for the rest;
#  force kernel: the probe's bound for polar_force_pair with PairMath.
EPS_STATIC = (16 * EPS, 0.0)
EPS_SWEEP = {"exact": (24 * EPS, 0.0), "list": (5 * 3e-14 + 24 * EPS, 3.1e-13)}
EPS_FORCE = (2e-15 + 5 * ULP, 2.4e-16 + 2 * ULP)


def _system(wl, damp, mode):
    rng = np.random.default_rng(77)
    pts = []
    for lo, hi, a in ((0.0, 12.0, 2.4), (12.0, 24.0, 4.8)):
        g = np.stack(np.meshgrid(np.arange(lo, hi, a), np.arange(0.0, L, a), np.arange(0.0, L, a), indexing="ij"), -1).reshape(-1, 3)
        pts.append(g + 0.5 * a + rng.uniform(-0.3, 0.3, g.shape))
    x = np.vstack(pts)
    n = len(x)
    q = rng.uniform(-0.8, 0.8, n)
    alpha = rng.uniform(0.3, 1.2, n)
    q[rng.random(n) < 0.25] = 0.0
    alpha[rng.random(n) < 0.25] = 0.0
    mol = (1 + np.arange(n) // 4).astype(np.int32)
    x[1] = x[0] + np.array([0.74, 0.0, 0.0])              # inside molecule 1
    q[0], q[1], alpha[0], alpha[1] = 0.4, -0.3, 0.6, 0.5
    x = np.mod(np.round(x / GRID) * GRID, L)
    args = ["8.0", repr(CUT), "damp_type", "exponential" if damp == 0 else "none", "damp", repr(PD), "use_previous", "yes",
            "polar_gs_ranked", "no", "polar_gs", "no", "fixed_iteration", "yes", "max_iterations", "1"]
    if mode == "list":
        args += ["dd_cutoff", "9.0", "deterministic", "yes"]
    st = wl.parse_pair_style_args(args)
    s = wl.make_system(x, q, alpha, np.ones(n, np.int32), mol, np.zeros(3), np.array([L, L, L]), 1, [["1", "1", "0.0", "3.0"]], st,
                       0.25, name="pair_accuracy", build_list=False)
    s = copy.copy(s)
    s.x, s.nghost, s.owner = np.ascontiguousarray(x), 0, np.arange(n)
    for k in ("q", "alpha", "type", "molecule"):
        setattr(s, k, np.ascontiguousarray(getattr(s, k)[:n]))
    mu0 = rng.normal(0.0, 0.05, (n, 3)) * (alpha != 0.0)[:, None]
    return s, mu0


class _Pairs:
    """the unordered minimum-image pairs i < j of the system and what decides their parts"""

    def __init__(self, s, mode):
        n = s.nlocal
        self.n = n
        self.I, self.J = np.triu_indices(n, 1)
        raw = s.x[self.I] - s.x[self.J]
        assert not np.any(np.abs(raw) == 0.5 * L)                       # no pair sits at L / 2
        self.d = raw - L * np.rint(raw / L)                              # exact: the coordinates are multiples of 2^-20
        assert np.array_equal((self.d - raw) / L, np.rint((self.d - raw) / L)) and np.all(np.abs(self.d) < 0.5 * L)
        self.rsq = self.d[:, 0] * self.d[:, 0] + self.d[:, 1] * self.d[:, 1] + self.d[:, 2] * self.d[:, 2]
        assert np.min(np.abs(self.rsq / CUT ** 2 - 1.0)) > 1e-9         # no comparison with a cutoff can go either way
        self.molok = (s.molecule[self.I] != s.molecule[self.J]) | (s.molecule[self.I] == 0)
        pol = s.alpha != 0.0
        self.dd_on = pol[self.I] & pol[self.J] & ((self.rsq < CUT ** 2) if mode == "list" else True)
        self.static_on = (self.rsq <= CUT ** 2) & self.molok


class _Acc:
    """per-atom (or scalar) sums of pair terms: value (long double), sum of |terms|, the pairs' own error bound, term count"""

    def __init__(self, be, shape):
        self.v = np.zeros(shape, dtype=np.longdouble if be.name == "longdouble" else object) + be.arr(0.0)
        self.s, self.b, self.k = np.zeros(shape), np.zeros(shape), np.zeros(shape)

    def add(self, idx, sm, sign, eps, on):
        """scatter the Sum `sm` (one per pair) of the pairs `on` into rows idx (None: one scalar)"""
        v = np.where(on, sm.v, 0 * sm.v) * sign
        pb = np.where(on, eps[0] * sm.s + eps[1] * sm.es, 0.0)
        if idx is None:
            self.v = self.v + v.sum()
            self.s += np.where(on, sm.s, 0.0).sum(); self.b += pb.sum(); self.k += on.sum()
        else:
            np.add.at(self.v, idx, v)
            np.add.at(self.s, idx, np.where(on, sm.s, 0.0)); np.add.at(self.b, idx, pb); np.add.at(self.k, idx, on * 1.0)

    def bound(self):
        return 4.0 * self.b + 4.0 * (self.k + 4.0) * EPS * self.s


def _compare(name, got, acc, be, scale=1.0, extra=0.0, quiet=False):
    """|got - scale x sum| <= scale x bound (+ extra) everywhere; returns the worst ratio"""
    err = np.abs(be.f64(be.arr(got) - acc.v * scale))
    bound = abs(scale) * acc.bound() + extra
    ok = bool(np.all(err <= bound))
    pos = bound > 0
    worst = float(np.max(err[pos] / bound[pos], initial=0.0))
    if not quiet:
        tot = np.abs(scale) * acc.s
        print("    %-10s worst %.3f of the bound, %.2e of sum|terms|" % (name, worst, float(np.max(err[pos] / tot[pos], initial=0.0))))
    return ok, worst


def _reference_fields(s, P, mu0, damp, mode, be, drop=None):
    """E_static / e2s and the induced field -T mu0, per atom.  drop: a pair index left out (the test that the comparison bites)"""
    keep = np.ones(len(P.I), bool)
    if drop is not None:
        keep[drop] = False
    E, F = _Acc(be, (P.n, 3)), _Acc(be, (P.n, 3))
    rsq = pr.rsq_of(P.d, be)                                              # exact; the FP64 P.rsq only decides the cutoffs
    fac = pr._static_field_factor(rsq, -1.0 / CUT ** 2)
    dl = [pr.leaf(be, P.d[:, k]) for k in range(3)]
    qi, qj = pr.leaf(be, s.q[P.I]), pr.leaf(be, s.q[P.J])
    s3, s5 = pr._tensor_scalars(rsq, PD, damp)
    mi, mj = [pr.leaf(be, mu0[P.I, k]) for k in range(3)], [pr.leaf(be, mu0[P.J, k]) for k in range(3)]
    di, dj = pr._dot(mi, dl), pr._dot(mj, dl)
    for k in range(3):
        E.add((P.I, k), fac * qj * dl[k], 1, EPS_STATIC, P.static_on & keep)
        E.add((P.J, k), fac * qi * dl[k], -1, EPS_STATIC, P.static_on & keep)
        # field at i from mu_j: -(s3 mu_j - s5 d (d . mu_j)); the tensor is even in d
        F.add((P.I, k), s5 * dl[k] * dj - s3 * mj[k], 1, EPS_SWEEP[mode], P.dd_on & keep)
        F.add((P.J, k), s5 * dl[k] * di - s3 * mi[k], 1, EPS_SWEEP[mode], P.dd_on & keep)
    return E, F


def _reference_forces(s, P, mu, damp, mode, be, drop=None):
    keep = np.ones(len(P.I), bool)
    if drop is not None:
        keep[drop] = False
    z = np.zeros(len(P.I))
    ref = pr.polar_pair(P.d, mu[P.I], s.q[P.I], s.alpha[P.I], mu[P.J], s.q[P.J], s.alpha[P.J], P.molok, CUT ** 2 + z,
                        (CUT ** 2 + z) if mode == "list" else None, -1.0 / CUT ** 2 + z, PD, math.sqrt(s.qqrd2e), damp,
                        rsq64=P.rsq, be=be)
    f, uef, udd, vir = _Acc(be, (P.n, 3)), _Acc(be, ()), _Acc(be, ()), _Acc(be, (6,))
    on = (ref["cd_on"] | ref["dd_on"]) & keep
    p = [ref["cd"][k] + ref["dd"][k] for k in range(3)]
    dl = [pr.leaf(be, P.d[:, k]) for k in range(3)]
    for k in range(3):
        f.add((P.I, k), p[k], 1, EPS_FORCE, on)
        f.add((P.J, k), p[k], -1, EPS_FORCE, on)
    uef.add(None, ref["uef"], 1, EPS_FORCE, ref["cd_on"] & keep)
    udd.add(None, ref["udd"], 1, EPS_FORCE, ref["dd_on"] & keep)
    for c, (a, b) in enumerate(((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))):
        one = _Acc(be, ())
        one.add(None, dl[a] * p[b], 1, EPS_FORCE, on)
        vir.v[c], vir.s[c], vir.b[c], vir.k[c] = one.v, one.s, one.b, one.k
    return f, uef, udd, vir, on


@pytest.mark.parametrize("damp", [0, 1], ids=["exponential", "none"])
@pytest.mark.parametrize("mode", ["exact", "list"])
def test_row_kernels_add_up_every_pair_once(mode, damp, wl, pkg, oracle):
    be = mc.judge()
    s, mu0 = _system(wl, damp, mode)
    n = s.nlocal
    P = _Pairs(s, mode)
    pol = s.alpha != 0.0
    assert abs(np.mean(s.q == 0.0) - 0.25) < 0.06 and abs(np.mean(~pol) - 0.25) < 0.06
    r01 = math.sqrt(P.rsq[0])
    assert (P.I[0], P.J[0]) == (0, 1) and abs(r01 - 0.74) < 1e-5 and not P.molok[0] and P.dd_on[0]
    # rows of the dipole-dipole list (dd_cutoff 9): one, two and three trips of 64
    inside = pol[P.I] & pol[P.J] & (P.rsq < CUT ** 2)
    rows = np.bincount(P.I[inside], minlength=n) + np.bincount(P.J[inside], minlength=n)
    rows = rows[pol]
    print("%s / damp %d: %d atoms, dipole-dipole rows of %d ... %d entries (%d / %d / %d rows of one / two / three trips)" % (
        mode, damp, n, rows.min(), rows.max(), np.sum(rows <= 64), np.sum((rows > 64) & (rows <= 128)), np.sum(rows > 128)))
    assert rows.min() < 64 and np.any((rows > 64) & (rows <= 128)) and rows.max() > 128

    p = pkg.pair_from_system(s)
    out = p.compute(eflag=1, vflag=1, mu=mu0)
    p.close()
    assert out["status"] == 0 and out["iterations"] == 1
    assert out["eng_vdwl"] == 0.0 and out["eng_coul"] == 0.0           # no LJ / Coulomb list: the polarization part alone
    if mode == "list":
        assert out["dd_pairs"] == 2 * inside.sum()

    # the choice of settings against the oracle: one committed sweep (it returns before the copy of its second)
    orc = oracle.compute(s, eflag=1, vflag=1, mu0=mu0)
    assert orc["iterations"] == 1 and orc["sweeps"] == 2 and orc["status"] == 0

    e2s = math.sqrt(s.qqrd2e)
    E, F = _reference_fields(s, P, mu0, damp, mode, be)
    ok_e, _ = _compare("ef_static", out["ef_static"], E, be, scale=e2s)
    # mu = alpha (e2s E + F): the two bounds add; 4 x 2^-53 of the terms for the last product and sum
    M = _Acc(be, (n, 3))
    a = s.alpha[:, None]
    M.v = be.arr(a) * (E.v * e2s + F.v)
    M.s, M.b, M.k = a * (e2s * E.s + F.s), a * (e2s * E.b + F.b), E.k + F.k
    ok_m, _ = _compare("mu", out["mu"], M, be)
    assert np.max(np.abs(orc["mu"] - be.f64(M.v))) <= 1e-10 * np.max(np.abs(orc["mu"]))
    assert not np.any(out["mu"][~pol])

    mu = out["mu"]
    f, uef, udd, vir, on = _reference_forces(s, P, mu, damp, mode, be)
    ok_f, _ = _compare("f", out["f"][:n], f, be)
    ok_ue, _ = _compare("u_ef", out["u_ef"], uef, be)
    ok_ud, _ = _compare("u_dd", out["u_dd"], udd, be)
    ok_v, _ = _compare("virial", out["virial"], vir, be)
    # eng_pol = u_self + u_ef + u_dd, u_self = sum |mu|^2 / (2 alpha) of the returned dipoles
    us = _Acc(be, ())
    ai = pr._inv(pr.leaf(be, np.repeat(s.alpha[pol], 3)))
    mm = pr.leaf(be, mu[pol].ravel())
    us.add(None, 0.5 * (mm * mm * ai), 1, (4 * EPS, 0.0), np.ones(3 * int(pol.sum()), bool))
    ok_us, _ = _compare("u_self", out["u_self"], us, be)
    tot = _Acc(be, ())
    tot.v, tot.s, tot.b, tot.k = us.v + uef.v + udd.v, us.s + uef.s + udd.s, us.b + uef.b + udd.b, us.k + uef.k + udd.k
    ok_ep, _ = _compare("eng_pol", out["eng_pol"], tot, be)
    assert ok_e and ok_m and ok_f and ok_ue and ok_ud and ok_v and ok_us and ok_ep

    # the comparison bites: one in-cutoff pair less in the reference sum of the longest row, and it fails
    longest = np.flatnonzero(pol)[rows.argmax()]
    of_row = np.flatnonzero(((P.I == longest) | (P.J == longest)) & inside & P.static_on & on)
    drop = of_row[np.argmax(P.rsq[of_row])]                            # the FARTHEST such pair: the smallest terms
    E1, F1 = _reference_fields(s, P, mu0, damp, mode, be, drop=drop)
    M.v = be.arr(a) * (E1.v * e2s + F1.v)
    f1 = _reference_forces(s, P, mu, damp, mode, be, drop=drop)[0]
    missed = [_compare("ef_static", out["ef_static"], E1, be, scale=e2s, quiet=True), _compare("mu", out["mu"], M, be, quiet=True),
              _compare("f", out["f"][:n], f1, be, quiet=True)]
    print("    without the pair (%d, %d) at %.3f A: ef_static %.1e, mu %.1e, f %.1e x the bound" % (
        P.I[drop], P.J[drop], math.sqrt(P.rsq[drop]), missed[0][1], missed[1][1], missed[2][1]))
    assert not missed[0][0] and not missed[1][0] and not missed[2][0]
    assert min(m[1] for m in missed) > 100.0
