"""Inputs, and the comparison with tests/pair_ref.py, that the host build of polar_force_pair() (tests/test_pair_ref_host.py) and
the device probe (tests/test_gpu_math_probe.py) share: the same pairs, the same edge cases, the same checks; only the
bounds differ (libm behind the host policy, the Newton / polynomial forms behind the device's)."""
import math

import numpy as np

import pair_ref as pr

EPS = math.ldexp(1.0, -53)
ULP = math.ldexp(1.0, -52)          # an ulp of a value is at most this much of it

PD = 2.1304
E2S = math.sqrt(332.06371)
CUT_COUL, DD_CUTOFF = 9.0, 7.5
G_EWALD = 0.3243
NPAIRS = 20000
COMBOS = [(ap, damp, ew) for damp in (0, 1) for ew in (False, True) for ap in (True, False)]

# The accumulators start from these.  Tiny, so that an added pair term of ordinary size comes back exactly (the probe's output
# IS the term: no subtraction of a sentinel, no rounding of its own), distinct and of both signs, so that an untouched
# accumulator is recognised by its bits.  [8]: what p starts from (WANT_P: polar_force_pair overwrites it).
SENTINEL = np.array([1e-300, -2e-300, 3e-300, -4e-300, 5e-300, -6e-300, 7e-300, -8e-300, 9e-300])



def judge():
    """The backend the large comparisons take: long double (vectorised; tests/test_pair_ref_host.py shows it within 1e-17 of
    scale of the 40-digit one) where numpy has a real one, mpmath otherwise."""
    return pr.backend("longdouble" if np.finfo(np.longdouble).nmant >= 63 else "mpmath")


# columns of the pair input
D, MUI, QI, AI, MUJ, QJ, AJ, MOLOK, CUTSQ, DDSQ, FSHIFT = slice(0, 3), slice(3, 6), 6, 7, slice(8, 11), 11, 12, 13, 14, 15, 16


def _unit(rng, n):
    u = rng.normal(size=(n, 3))
    return u / np.linalg.norm(u, axis=1)[:, None]


def _random_pairs(rng, n, rlo=0.6, rhi=12.0):
    a = np.zeros((n, 17))
    a[:, D] = _unit(rng, n) * rng.uniform(rlo, rhi, n)[:, None]
    a[:, MUI] = _unit(rng, n) * rng.uniform(0.0, 0.5, n)[:, None]
    a[:, MUJ] = _unit(rng, n) * rng.uniform(0.0, 0.5, n)[:, None]
    a[:, QI], a[:, QJ] = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    a[:, AI], a[:, AJ] = rng.uniform(0.2, 1.2, n), rng.uniform(0.2, 1.2, n)
    a[:, MOLOK] = rng.random(n) >= 0.15
    a[:, CUTSQ], a[:, DDSQ], a[:, FSHIFT] = CUT_COUL ** 2, DD_CUTOFF ** 2, -1.0 / CUT_COUL ** 2
    return a


def pair_inputs(rsq_of):
    """NPAIRS random pairs (|d| 0.6 - 12 A, dipoles up to 0.5, charges up to 1, cut_coul 9, dd_cutoff 7.5, 15 % of them inside
    one molecule) and the edge cases; `rsq_of(inputs)` returns the FP64 rsq the implementation under test forms for them
    (the cutoff cases are placed on it).  Returns (inputs [n, 17], labels: name -> index array)."""
    rng = np.random.default_rng(20240611)
    blocks, labels, at = [_random_pairs(rng, NPAIRS)], {"random": np.arange(NPAIRS)}, NPAIRS

    def add(name, a):
        nonlocal at
        blocks.append(a)
        labels[name] = np.arange(at, at + len(a))
        at += len(a)

    k = 16
    for name, col, r in (("cut_coulsq", CUTSQ, CUT_COUL), ("ddcutsq", DDSQ, DD_CUTOFF)):
        a = _random_pairs(rng, k, r, r)
        a[:, MOLOK] = 1.0
        rsq = rsq_of(a)
        for tag, v in (("at", rsq), ("above", np.nextafter(rsq, np.inf)), ("below", np.nextafter(rsq, -np.inf))):
            b = a.copy()
            b[:, col] = v                       # rsq == cutoff^2, one ulp below it, one ulp above it
            if col == CUTSQ:
                b[:, FSHIFT] = -1.0 / v
            add("rsq_%s_%s" % (tag, name), b)
    for name, cols in (("alpha_i_0_stale_mu", [AI]), ("alpha_j_0_stale_mu", [AJ]), ("q_i_0", [QI]), ("q_j_0", [QJ]),
                       ("alpha_i_alpha_j_0", [AI, AJ]), ("q_i_q_j_0", [QI, QJ])):
        a = _random_pairs(rng, k, 1.0, 7.0)
        for c in cols:
            a[:, c] = 0.0
        add(name, a)
    a = _random_pairs(rng, k, 0.6, 8.9)
    a[:, MOLOK] = 0.0
    add("molok_false", a)
    a = _random_pairs(rng, k, 0.7, 0.7)
    a[:, MOLOK] = np.arange(k) % 2
    add("r_0.7", a)
    return np.ascontiguousarray(np.vstack(blocks)), labels


_TERMS = {}


def pair_reference(inp, damp, ew, be):
    """pair_ref.pair_terms of the inputs, evaluated once per (damping, Ewald, backend) and shared by the instances"""
    key = (damp, ew, be.name, hash(inp.tobytes()))
    if key not in _TERMS:
        _TERMS[key] = pr.pair_terms(inp[:, D], inp[:, MUI], inp[:, QI], inp[:, AI], inp[:, MUJ], inp[:, QJ], inp[:, AJ],
                                    inp[:, MOLOK] != 0, inp[:, FSHIFT], PD, E2S, damp, G_EWALD if ew else None, be)
    return _TERMS[key]


def check_pairs(out, inp, labels, allpairs, damp, ew, rsqrt_ulps, exp_bound, be=None):
    """out [n, 12] of a pair probe against pair_ref.polar_pair.  Bound per output: (2e-15 + rsqrt_ulps ulp) of scale +
    exp_bound x the part of the scale that carries e^-a.  Returns the worst figures, asserts everything."""
    be = be or pr.backend()
    n = len(inp)
    rsq = out[:, 11]
    ref = pr.polar_pair(inp[:, D], inp[:, MUI], inp[:, QI], inp[:, AI], inp[:, MUJ], inp[:, QJ], inp[:, AJ], inp[:, MOLOK] != 0,
                        inp[:, CUTSQ], None if allpairs else inp[:, DDSQ], inp[:, FSHIFT], PD, E2S, damp,
                        g_ewald=G_EWALD if ew else None, rsq64=rsq, be=be, terms=pair_reference(inp, damp, ew, be))
    cd_on, dd_on = ref["cd_on"], ref["dd_on"]
    # every listed case is decided the way its name says
    for tag, want in (("at", ew), ("above", True), ("below", False)):
        assert np.all(cd_on[labels["rsq_%s_cut_coulsq" % tag]] == want), tag
    for tag, want in (("at", allpairs), ("above", True), ("below", allpairs)):
        assert np.all(dd_on[labels["rsq_%s_ddcutsq" % tag]] == want), tag
    assert not dd_on[labels["alpha_i_0_stale_mu"]].any() and not dd_on[labels["alpha_j_0_stale_mu"]].any()
    assert ew or not cd_on[labels["molok_false"]].any()
    bits = lambda a: np.ascontiguousarray(a, np.float64).view(np.uint64)
    rel = 2e-15 + rsqrt_ulps * ULP
    worst = {}
    names = [("cd", 0, ref["cd"], cd_on), ("dd", 3, ref["dd"], dd_on), ("uef", 6, [ref["uef"]], cd_on & (not ew)),
             ("udd", 7, [ref["udd"]], dd_on)]
    psum = [ref["cd"][k] + ref["dd"][k] for k in range(3)]
    parts = np.zeros((n, 3))
    for name, col, sums, on in names:
        on = on & np.ones(n, bool)
        w_err, w_ratio = 0.0, 0.0
        for k, sm in enumerate(sums):
            got = out[:, col + k]
            # a part the reference leaves out leaves its accumulator untouched
            assert np.array_equal(bits(got[~on]), bits(np.full(int((~on).sum()), SENTINEL[col + k]))), (name, k, "touched")
            g = np.where(on, got, 0.0)
            g = np.where(np.abs(g) <= 1e-280, 0.0, g)      # (an exact zero was added to the sentinel)
            err = pr.err_over(g, sm.v, 1.0, be)
            bound = rel * sm.s + exp_bound * sm.es
            bad = np.flatnonzero(err > bound)
            assert len(bad) == 0, (name, k, len(bad), "first", bad[0], inp[bad[0]], got[bad[0]], float(sm.v[bad[0]]), err[bad[0]], bound[bad[0]])
            pos = sm.s > 0
            w_err = max(w_err, float(np.max(err[pos] / sm.s[pos], initial=0.0)))
            w_ratio = max(w_ratio, float(np.max(err[pos] / bound[pos], initial=0.0)))
            if name in ("cd", "dd"):
                parts[:, k] += g
        worst[name] = (w_err, w_ratio)
    # p: the pair's whole force, assigned (never the sentinel), the reference's cd + dd, and cd + dd of the outputs to 2 ulp of scale
    w_err = w_ratio = w_sum = 0.0
    for k in range(3):
        got = out[:, 8 + k]
        assert not np.any(bits(got) == bits(SENTINEL[8:9])[0])
        sm = psum[k]
        err = pr.err_over(got, sm.v, 1.0, be)
        bound = rel * sm.s + exp_bound * sm.es
        bad = np.flatnonzero(err > bound)
        assert len(bad) == 0, ("p", k, len(bad), bad[0], err[bad[0]], bound[bad[0]])
        assert np.all(got[~cd_on & ~dd_on] == 0.0)
        d = np.abs(got - parts[:, k])
        assert np.all(d <= 2 * ULP * sm.s), ("p != cd + dd", k)
        pos = sm.s > 0
        w_err = max(w_err, float(np.max(err[pos] / sm.s[pos], initial=0.0)))
        w_ratio = max(w_ratio, float(np.max(err[pos] / bound[pos], initial=0.0)))
        w_sum = max(w_sum, float(np.max(d[pos] / sm.s[pos], initial=0.0)))
    worst["p"] = (w_err, w_ratio)
    worst["p-(cd+dd)"] = (w_sum, w_sum / (2 * ULP))
    return worst


# ---------------------------------------------------------------------------------------------------------------------
# inputs of the primitive, tensor-scalar and Ewald probes

TENSOR_PD = (2.1304, 0.5, 6.0)
EWALD_G = (0.25, 0.3243, 0.40)
PADDING_RSQ = 1e60                  # the r^2 of the sweep's padding pairs (DUMMY record)


def _neighbours(x, k):
    out = [x]
    lo = hi = x
    for _ in range(k):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        out += [lo, hi]
    return np.concatenate(out)


def rsqrt_inputs():
    """x > 0: 100,000 values with log10(x) uniform in [-2, 4] (the r^2 of real pairs), every power of two from 2^-60 to 2^200
    with its two FP64 neighbours, and 1e60"""
    rng = np.random.default_rng(101)
    return np.concatenate([10.0 ** rng.uniform(-2.0, 4.0, 100000), _neighbours(np.ldexp(1.0, np.arange(-60, 201)), 1), [PADDING_RSQ]])


EXP_SPECIAL = np.array([-700.0, -700.0000001, -745.0, -746.0, -1e30, -2.1304e30, -np.inf])


def exp_inputs():
    """x <= 0: 100,000 uniform in [-60, 0], 20,000 uniform in [-700, 0], +0 and -0, the FP64 values nearest -(n + 1/2) ln 2 for
    n = 0 ... 1010 with two neighbours on each side (the rounding ties of the reduction), and EXP_SPECIAL"""
    rng = np.random.default_rng(102)
    ties = np.asarray(-(np.arange(1011) + np.longdouble(0.5)) * np.log(np.longdouble(2)), dtype=np.float64)
    return np.concatenate([rng.uniform(-60.0, 0.0, 100000), rng.uniform(-700.0, 0.0, 20000), [0.0, -0.0], _neighbours(ties, 2),
                           EXP_SPECIAL])


def tensor_inputs():
    """r^2 (what the kernels see) for 50,000 r uniform in [0.5, 30] A, then 0.70, 0.74 and 0.9572"""
    r = np.concatenate([np.random.default_rng(103).uniform(0.5, 30.0, 50000), [0.70, 0.74, 0.9572]])
    return r * r


def ewald_inputs():
    """(rsq, kept): kept pairs with r uniform in [0.5, 12] A, excluded ones in [0.05, 12] A (a quarter of them below 0.5)"""
    rng = np.random.default_rng(104)
    r = np.concatenate([rng.uniform(0.5, 12.0, 1500), rng.uniform(0.5, 12.0, 1500), rng.uniform(0.05, 0.5, 500)])
    kept = np.arange(len(r)) < 1500
    return r * r, kept
