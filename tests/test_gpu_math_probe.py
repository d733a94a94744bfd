"""The hand-rolled device arithmetic against a high-precision reference (tests/pair_ref.py), function by function.

tests/math_probe/math_probe.hip calls the project's own device functions once per input -- rsqrt_pos, rsqrt_pos3, exp_neg,
exp_neg_fast<10 / 12>, tensor_scalars_lp / tensor_scalars / tensor_scalars_k, ewald_b1 / ewald_b12, and polar_force_pair
with the device policy PairMath -- and the tests hold every result against the accuracy the source comments promise or a
bound derived from the number format.  Errors are |got - reference| over the SCALE of the reference (the sum of the
absolute values of its terms, see pair_ref.py), or in ulps of the reference value for the primitives.

The primitives are judged by mpmath at 40 digits (when it imports); the tensor scalars, Ewald factors and pairs by
math_probe_cases.judge(): long double, which tests/test_pair_ref_host.py holds within 1e-17 of scale of mpmath.

Measured on the MI355X: see the accuracy ledger in DESIGN.md; every test prints its worst case."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import math_probe_cases as mc
import pair_ref as pr

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
EPS = math.ldexp(1.0, -53)
ULP = math.ldexp(1.0, -52)

RSQRT_POS = 3e-14                                   # "2^-45 = 3e-14 relative", csrc/polar_common.hpp
RSQRT_POS3_ULP = 1.0                                # "correct to an ulp"
SEED = math.ldexp(1.0, -22)                         # what both comments take v_rsq_f64 to deliver
EXP10 = 3.1e-13                                     # (ln2/2)^11 / 11! = 2.2e-13 absolute, over e^r >= 2^-1/2
EXP12 = 2.4e-16                                     # (ln2/2)^13 / 13! = 1.7e-16 absolute, over 2^-1/2; plus 2 ulp
assert (math.log(2) / 2) ** 11 / math.factorial(11) * math.sqrt(2) <= EXP10 <= 3.2e-13
assert (math.log(2) / 2) ** 13 / math.factorial(13) * math.sqrt(2) <= EXP12 <= 2.5e-16


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def probe(pkg, tmp_path_factory):
    """math_probe.hip compiled for gfx950 with the library's own flags, loaded after the library (and with it torch's HIP
    runtime, see pkg.lib)"""
    if not os.path.exists(pkg.HIPCC):
        pytest.skip("hipcc not available")
    pkg.lib()
    so = str(tmp_path_factory.mktemp("math_probe") / "libmath_probe.so")
    subprocess.check_call([pkg.HIPCC] + pkg.HIP_FLAGS + ["-Wno-unused-function", "-I", os.path.join(os.path.dirname(pkg.__file__), "csrc"),
                           "-o", so, os.path.join(HERE, "math_probe", "math_probe.hip")])
    lib = C.CDLL(so)
    dp, ip, ll, d = C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_longlong, C.c_double
    for name, args in (("math_probe_rsqrt", [ll, dp, dp]), ("math_probe_exp", [ll, dp, dp]), ("math_probe_tensor", [ll, dp, d, dp]),
                       ("math_probe_ewald", [ll, dp, d, ip, dp]),
                       ("math_probe_pair", [C.c_int, C.c_int, C.c_int, ll, dp, d, d, d, dp, dp])):
        getattr(lib, name).restype, getattr(lib, name).argtypes = C.c_int, args

    class Probe:
        @staticmethod
        def _run(fn, n, ncol, *args):
            out = np.zeros((n, ncol))
            rc = fn(*[a.ctypes.data_as(dp if a.dtype == np.float64 else ip) if isinstance(a, np.ndarray) else a for a in args],
                    out.ctypes.data_as(dp))
            assert rc == 0, "HIP error %d in %s" % (rc, fn.__name__)
            return out

        def rsqrt(self, x):
            x = np.ascontiguousarray(x, np.float64)
            return self._run(lib.math_probe_rsqrt, len(x), 3, len(x), x)

        def exp(self, x):
            x = np.ascontiguousarray(x, np.float64)
            return self._run(lib.math_probe_exp, len(x), 3, len(x), x)

        def tensor(self, r2, pd):
            r2 = np.ascontiguousarray(r2, np.float64)
            return self._run(lib.math_probe_tensor, len(r2), 12, len(r2), r2, float(pd))

        def ewald(self, rsq, g, kept):
            rsq, kept = np.ascontiguousarray(rsq, np.float64), np.ascontiguousarray(kept, np.int32)
            return self._run(lib.math_probe_ewald, len(rsq), 3, len(rsq), rsq, float(g), kept)

        def pair(self, allpairs, damp, ew, inp):
            inp = np.ascontiguousarray(inp, np.float64)
            return self._run(lib.math_probe_pair, len(inp), 12, int(allpairs), int(damp), int(ew), len(inp), inp, mc.PD, mc.E2S,
                             mc.G_EWALD, mc.SENTINEL)
    return Probe()


# ---------------------------------------------------------------------------------------------------------------------
# the primitives

def test_rsqrt(probe):
    """rsqrt_pos3 within 1 ulp of 1/sqrt(x) and rsqrt_pos within 3e-14 of it, on every input: the r^2 range of real pairs, every
    power of two from 2^-60 to 2^200 with its neighbours, and the padding distance 1e60.  The seed is reported, and compared
    with the 2^-22 both comments assume.
    Measured on the MI355X: seed 5.1e-8 = 2^-24.2; rsqrt_pos 3.9e-15; rsqrt_pos3 0.98 ulp."""
    be = pr.backend()
    x = mc.rsqrt_inputs()
    out = probe.rsqrt(x)
    ref, _ = pr.rsqrt(x, be)
    ref64 = pr.to_f64(ref, be)
    assert np.all(np.isfinite(out)) and np.all(out > 0)
    seed = pr.err_over(out[:, 0], ref, ref64, be)
    e2 = pr.err_over(out[:, 1], ref, ref64, be)
    e3 = pr.err_over(out[:, 2], ref, np.spacing(ref64), be)
    print("v_rsq_f64 seed: worst %.3e relative = 2^%.2f (the comments take 2^-22)" % (seed.max(), math.log2(seed.max())))
    print("rsqrt_pos : worst %.3e relative (promise 3e-14)" % e2.max())
    print("rsqrt_pos3: worst %.3f ulp (promise 1 ulp), %.3e relative" % (e3.max(), (e3 * np.spacing(ref64) / ref64).max()))
    assert e3.max() <= RSQRT_POS3_ULP, x[e3.argmax()]
    assert e2.max() <= RSQRT_POS, x[e2.argmax()]
    if seed.max() > SEED:           # (reported, not asserted: the two bounds above are what the kernels rely on)
        print("NOTE: the seed is worse than the 2^-22 the comments of rsqrt_pos / rsqrt_pos3 start from")


@pytest.fixture(scope="module")
def exps(probe):
    """inputs, what the probe returns for them, and e^max(x, -745) of the reference (evaluated once)"""
    be = pr.backend()
    x = mc.exp_inputs()
    ref, _ = pr.exp(np.maximum(x, -745.0), be)
    return x, probe.exp(x), be, ref


def test_exp_neg(exps):
    """exp_neg (degree 13, ldexp): within 2 ulp of e^max(x, -745) -- an ulp of the reference value, 2^-1074 where it is subnormal
    (x < -708.4) -- and below the clamp exactly the value at the clamp.
    Measured on the MI355X: 0.84 ulp where the result is normal, 0 ulp where it is subnormal."""
    x, out, be, ref = exps
    got = out[:, 0]
    ref64 = pr.to_f64(ref, be)
    err = pr.err_over(got, ref, np.spacing(ref64), be)
    normal = ref64 >= np.finfo(np.float64).tiny
    print("exp_neg: worst %.3f ulp where the result is normal, %.3f ulp (of 2^-1074) where it is subnormal"
          % (err[normal].max(), err[~normal].max()))
    assert err.max() <= 2.0, x[err.argmax()]
    at_clamp = got[np.flatnonzero(x == -745.0)[0]]
    assert np.all(_bits(got[x < -745.0]) == _bits(at_clamp)) and np.sum(x < -745.0) >= 4


@pytest.mark.parametrize("deg", [10, 12])
def test_exp_neg_fast(deg, exps):
    """exp_neg_fast<DEG>, every input: within the truncation bound of its polynomial (3.1e-13 relative at degree 10; 2.4e-16
    relative plus 2 ulp at degree 12) of e^max(x, -700); exactly 1 at +0 and -0; finite, positive and normal everywhere --
    the rounding ties of the reduction, where |r| is largest, the clamp, and the arguments the padding pairs produce
    (-2.1304e30, -inf), which return the bits of the value at -700; and monotone over the sorted inputs to within twice the
    error bound (two neighbouring results may err in opposite directions).
    Measured on the MI355X: degree 10, 2.99e-13 relative at x = -640.12 (0.96 of the bound; the source comment's 2.2e-13 was
    the dropped term, not a relative error); degree 12, 3.6e-16 relative = 2.3 ulp at x = -303.25 (0.65 of the bound)."""
    x, out, be, ref = exps
    got = out[:, 1 if deg == 10 else 2]
    ref = np.where(x < -700.0, ref[np.flatnonzero(x == -700.0)[0]], ref)           # e^max(x, -700)
    ref64 = pr.to_f64(ref, be)
    assert np.all(np.isfinite(got)) and np.all(got >= np.finfo(np.float64).tiny)
    assert np.all(got[x == 0.0] == 1.0) and np.sum(x == 0.0) == 2
    at_clamp = got[np.flatnonzero(x == -700.0)[0]]
    below = x < -700.0
    assert np.all(_bits(got[below]) == _bits(at_clamp)) and below.sum() >= 6 + 4
    rel = EXP10 if deg == 10 else EXP12
    ulps = 0.0 if deg == 10 else 2.0
    err = pr.err_over(got, ref, 1.0, be)
    bound = rel * ref64 + ulps * np.spacing(ref64)
    w = (err / ref64).argmax()
    print("exp_neg_fast<%d>: worst %.3e relative (at x = %r), %.2f of the bound; %.2f ulp" % (
        deg, (err / ref64).max(), x[w], (err / bound).max(), (err / np.spacing(ref64)).max()))
    assert np.all(err <= bound), x[(err / bound).argmax()]
    order = np.argsort(x, kind="stable")
    g = got[order]
    slack = 2.0 * (rel + ulps * ULP)
    assert np.all(g[1:] >= g[:-1] * (1.0 - slack))


# ---------------------------------------------------------------------------------------------------------------------
# tensor scalars

@pytest.mark.parametrize("pd", mc.TENSOR_PD)
def test_tensor_scalars(pd, probe):
    """s3 against r^-3 and s5 against 3 r^-5 (the scales), r from 0.5 to 30 A and 0.70, 0.74, 0.9572, with and without damping.
    tensor_scalars_lp (the sweep's: rsqrt_pos, exp_neg_fast<10>): 3 x 3e-14 + 3.1e-13 x e^-a p(a) + 4 x 2^-53, the bound
    evaluated per point from the reference.  tensor_scalars and tensor_scalars_k (library rsqrt; exp and exp_neg): 8 x 2^-53.
    At r^2 = 1e60 (the sweep's padding pairs) all of them are finite and their product with a zero dipole is exactly 0.
    Measured on the MI355X: tensor_scalars_lp<0> s3 2.9e-13, s5 3.0e-13 (0.74 of the bound, pd 0.5); <1> s3 1.2e-14, s5 2.0e-14;
    tensor_scalars = tensor_scalars_k: s3 3.7 x 2^-53, s5 5.5 x 2^-53.  (With r^-5 formed as rinv (rinv rinv)^2 the last stood at
    8.9 x 2^-53: the finding behind rinv2_newton in csrc/polar_common.hpp.)"""
    be = mc.judge()
    r2 = np.concatenate([mc.tensor_inputs(), [mc.PADDING_RSQ]])
    out = probe.tensor(r2, pd)
    assert np.all(np.isfinite(out)) and np.all(out * 0.0 == 0.0)
    assert np.all(_bits(out[-1] * 0.0) == 0) and np.all(out[-1] > 0.0)          # the DUMMY-record contract
    plain = pr.tensor_scalars(r2, pd, 1, be)
    scale0 = [pr.to_f64(plain[0].v, be), pr.to_f64(plain[1].v, be)]
    for damp in (0, 1):
        ref = pr.tensor_scalars(r2, pd, damp, be)
        for k, nm in enumerate(("s3", "s5")):
            damped = ref[k].es / scale0[k]                                      # e^-a p(a)
            for form, col, bound in (("tensor_scalars_lp", 0, 3 * RSQRT_POS + EXP10 * damped + 4 * EPS),
                                     ("tensor_scalars", 4, 8 * EPS + 0 * damped), ("tensor_scalars_k", 8, 8 * EPS + 0 * damped)):
                err = pr.err_over(out[:, col + 2 * damp + k], ref[k].v, scale0[k], be)
                w = (err / bound).argmax()
                print("pd %.4f %-17s<%d> %s: worst %.3e of scale (%.2f of the bound, at r = %.4f)" % (
                    pd, form, damp, nm, err.max(), (err / bound).max(), math.sqrt(r2[w])))
                assert np.all(err <= bound), (form, damp, nm, math.sqrt(r2[w]))


# ---------------------------------------------------------------------------------------------------------------------
# Ewald factors

@pytest.mark.parametrize("g", mc.EWALD_G)
def test_ewald_factors(g, probe):
    """B1 of ewald_b1 and B1, B2 of ewald_b12 within 16 x 2^-53 of scale, kept pairs (erfc form) from 0.5 to 12 A and excluded
    ones (erf form) from 0.05 to 12 A; the two B1 bit for bit the same.
    Measured on the MI355X: B1 4.6 x 2^-53 kept, 2.8 excluded; B2 4.4 kept, 4.3 excluded.  (The exponent g*g*rsq formed with two
    plain products reaches 30 x 2^-53 at g r = 4.7 in NumPy FP64: a relative error of the exponent is multiplied by g^2 r^2.
    ewald_gauss in csrc/polar_common.hpp carries the rounding errors along.)"""
    be = mc.judge()
    rsq, kept = mc.ewald_inputs()
    out = probe.ewald(rsq, g, kept)
    assert np.array_equal(_bits(out[:, 0]), _bits(out[:, 1]))
    b1, b2 = pr.ewald_b12(rsq, g, kept, be)
    for nm, got, sm in (("B1", out[:, 1], b1), ("B2", out[:, 2], b2)):
        err = pr.err_over(got, sm.v, sm.s, be)
        for tag, m in (("kept", kept), ("excluded", ~kept)):
            w = np.flatnonzero(m)[err[m].argmax()]
            print("g %.4f %s %-8s: worst %.2f x 2^-53 of scale (at r = %.4f)" % (g, nm, tag, err[m].max() / EPS, math.sqrt(rsq[w])))
        assert err.max() <= 16 * EPS, (nm, math.sqrt(rsq[err.argmax()]))


# ---------------------------------------------------------------------------------------------------------------------
# the pair function with the device policy

@pytest.fixture(scope="module")
def pairs(probe):
    return mc.pair_inputs(lambda a: probe.pair(True, 1, False, a)[:, 11])


@pytest.mark.parametrize("allpairs,damp,ew", mc.COMBOS)
def test_pair_function_with_the_device_policy(allpairs, damp, ew, probe, pairs):
    """polar_force_pair<ALLPAIRS, DAMP, true, EW, true, PairMath> on 20,000 random pairs and the edge cases of
    math_probe_cases.pair_inputs: cd, dd, uef, udd and p each within 2e-15 of scale + 5 ulp (r^-5 from rsqrt_pos3) + the
    degree-12 exponential's bound x the part of the scale that carries e^-a; a part the reference leaves out leaves its
    accumulator untouched (bits of the sentinel); p == cd + dd to 2 ulp of scale.
    Measured on the MI355X, of scale: cd 1.2e-15 (1.7e-15 under polar_ewald), dd 1.0e-15, uef 7.7e-16, udd 8.7e-16, p 1.7e-15
    (0.56 of the bound at worst); p - (cd + dd) exactly 0."""
    inp, labels = pairs
    out = probe.pair(allpairs, damp, ew, inp)
    worst = mc.check_pairs(out, inp, labels, allpairs, damp, ew, rsqrt_ulps=5.0, exp_bound=EXP12 + 2 * ULP, be=mc.judge())
    print("device ALLPAIRS %d DAMP %d EW %d: " % (allpairs, damp, ew) +
          "  ".join("%s %.2e of scale (%.2f of the bound)" % ((k,) + v) for k, v in worst.items()))
