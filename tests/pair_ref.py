"""A high-precision reference of the arithmetic the kernels do per pair, written term by term as the reference pair style
writes it (oracle/polar_oracle.c, the PS.cpp lines it cites) -- none of the library's closed forms.

Two backends evaluate the same definitions:
  * "mpmath": 40 significant digits (a private context; the global mpmath precision is left alone) -- the default
    when mpmath imports;
  * "longdouble": numpy.longdouble with at least a 64-bit significand (asserted), erf / erfc from a positive-term series
    and a continued fraction written here.  tests/test_pair_ref_host.py checks that the two agree to 1e-17 of scale, so
    either is adequate to judge FP64 code; the whole-system sums of tests/test_gpu_pair_accuracy.py (10^5 pairs) take the
    vectorised long-double one.

Every quantity comes back as a `Sum`: its value and its SCALE, the sum of the absolute values of the terms that were
added to form it (products of sums are expanded: the scale of a product is the product of the scales).  Errors are
measured as |got - value| / scale, so that a result that cancels legitimately -- (1 + f_shift r^2) near the cutoff,
1 - e^-a (...) at short range, pre4 / pre5 of the reference -- does not produce a meaningless relative error.  `es` is
the part of the scale whose terms carry the factor e^-a (the bound of a polynomial exponential is propagated with it).
`unpack()` returns (value, scale).  Inputs are FP64 arrays and enter exactly."""
import math

import numpy as np

try:
    import mpmath
except ImportError:          # pragma: no cover
    mpmath = None

DIGITS = 40


class _MP:
    name = "mpmath"

    def __init__(self):
        self.ctx = mpmath.mp.clone()
        self.ctx.dps = DIGITS
        c = self.ctx
        self._new = np.frompyfunc(lambda v: c.mpf(float(v)), 1, 1)
        self.sqrt, self.exp = np.frompyfunc(c.sqrt, 1, 1), np.frompyfunc(c.exp, 1, 1)
        self.erf, self.erfc = np.frompyfunc(c.erf, 1, 1), np.frompyfunc(c.erfc, 1, 1)
        self.two_over_sqrtpi = 2 / c.sqrt(c.pi)

    def arr(self, a):
        a = np.asarray(a)
        return a if a.dtype == object else np.asarray(self._new(np.asarray(a, np.float64)), dtype=object)

    def f64(self, a):
        return np.asarray(a, dtype=object).astype(np.float64)


class _LD:
    name = "longdouble"

    def __init__(self):
        assert np.finfo(np.longdouble).nmant >= 63, "numpy.longdouble is no wider than FP64 here"
        self.sqrt, self.exp = np.sqrt, np.exp
        self.pi = 4 * np.arctan(np.longdouble(1))
        self.two_over_sqrtpi = 2 / np.sqrt(self.pi)

    def arr(self, a):
        return np.asarray(a, dtype=np.longdouble)

    def f64(self, a):
        return np.asarray(a, dtype=np.float64)

    def erf(self, x):
        """2/sqrt(pi) e^(-x^2) sum_n 2^n x^(2n+1) / (2n+1)!!, x >= 0: all terms positive, nothing cancels"""
        x = self.arr(x)
        t = x.copy()
        s = x.copy()
        for n in range(1, 400):
            t = t * (2 * x * x) / (2 * n + 1)
            s = s + t
            if not np.any(t > s * np.longdouble(1e-22)):
                break
        return 2 / np.sqrt(self.pi) * np.exp(-x * x) * s

    def erfc(self, x):
        """1 - erf below 1 (erfc >= 0.157 there); above it the continued fraction
        e^(-x^2)/sqrt(pi) / (x + (1/2)/(x + 1/(x + (3/2)/(x + ...)))), evaluated from a fixed depth"""
        x = self.arr(x)
        big = x >= 1
        xb = np.where(big, x, np.longdouble(1))
        f = xb.copy()
        for k in range(600, 0, -1):
            f = xb + (np.longdouble(k) / 2) / f
        cf = np.exp(-xb * xb) / np.sqrt(self.pi) / f
        return np.where(big, cf, 1 - self.erf(np.where(big, np.longdouble(0), x)))


_BACKENDS = {}


def backend(name=None):
    """"mpmath", "longdouble", or None: mpmath when it imports, long double otherwise"""
    if name is None:
        name = "mpmath" if mpmath is not None else "longdouble"
    if name not in _BACKENDS:
        _BACKENDS[name] = _MP() if name == "mpmath" else _LD()
    return _BACKENDS[name]


class Sum:
    """value (backend precision), scale and escale (FP64: they only normalise errors)"""
    __slots__ = ("be", "v", "s", "es")

    def __init__(self, be, v, s=None, es=None):
        self.be, self.v = be, v
        self.s = np.abs(be.f64(v)) if s is None else s
        self.es = np.zeros_like(self.s) if es is None else es

    def __add__(self, o):
        if not isinstance(o, Sum):          # an exact constant: one more term
            return Sum(self.be, self.v + o, self.s + abs(float(o)), self.es)
        return Sum(self.be, self.v + o.v, self.s + o.s, self.es + o.es)

    __radd__ = __add__

    def __neg__(self):
        return Sum(self.be, -self.v, self.s, self.es)

    def __sub__(self, o):
        return self + (-o)

    def __rsub__(self, o):
        return (-self) + o

    def __mul__(self, o):
        if not isinstance(o, Sum):          # an exact constant
            return Sum(self.be, self.v * o, self.s * abs(float(o)), self.es * abs(float(o)))
        return Sum(self.be, self.v * o.v, self.s * o.s, self.s * o.s - (self.s - self.es) * (o.s - o.es))

    __rmul__ = __mul__

    def where(self, mask):
        """the sum where mask holds, an empty sum (0, scale 0) elsewhere"""
        return Sum(self.be, np.where(mask, self.v, 0 * self.v), np.where(mask, self.s, 0.0), np.where(mask, self.es, 0.0))

    def unpack(self):
        return self.v, self.s

    def __iter__(self):
        return iter((self.v, self.s))


def leaf(be, a):
    return Sum(be, be.arr(a))


def _inv(x):
    """1 / x for a sum of one-signed terms (a single term of the result)"""
    return Sum(x.be, 1 / x.v)


def _sqrt(x):
    return Sum(x.be, x.be.sqrt(x.v))


def _exp(x, damp=False):
    r = Sum(x.be, x.be.exp(x.v))
    if damp:
        r.es = r.s.copy()
    return r


# ---------------------------------------------------------------------------------------------------------------------
# the primitives

def rsqrt(x, be=None):
    be = be or backend()
    return _inv(_sqrt(leaf(be, x)))


def exp(x, be=None):
    be = be or backend()
    return _exp(leaf(be, x))


# ---------------------------------------------------------------------------------------------------------------------
# dipole tensor scalars, PS.cpp:1284-1306:  T_pq = delta_pq s3 - d_p d_q s5,  s3 = damping_term1 / r^3, s5 = 3 damping_term2 / r^5

def tensor_scalars(r2, pd, damp, be=None):
    """damp 0: exponential, 1: none.  r2 is the FP64 squared distance the kernels see.  Returns (s3, s5)."""
    be = be or backend()
    return _tensor_scalars(leaf(be, r2), pd, damp)


def _tensor_scalars(r2, pd, damp):
    be = r2.be
    r = _sqrt(r2)
    r3, r5 = _inv(r * r * r), _inv(r * r * r * r * r)
    if damp == 0:
        pd = leaf(be, pd + np.zeros_like(r2.s))
        e = _exp(-(pd * r), damp=True)
        d1 = 1 - e * (pd * pd * r2 * 0.5 + pd * r + 1)
        d2 = 1 - e * (pd * pd * pd * r2 * r * _sixth(be) + pd * pd * r2 * 0.5 + pd * r + 1)
        return d1 * r3, 3 * (d2 * r5)
    return r3, 3 * r5


def _sixth(be):
    return Sum(be, be.arr(1.0) / 6)


# ---------------------------------------------------------------------------------------------------------------------
# `polar_ewald` radial factors: E = q B1 d, dE_a/dd_b = q (B1 delta_ab - B2 d_a d_b)

def ewald_b12(rsq, g, kept, be=None):
    """B1 = (erfc(g r)/r + 2g/sqrt(pi) e^(-g^2 r^2)) / r^2 for a kept pair; an excluded pair takes the bare 1/r^3 off, which
    leaves -(erf(g r)/r - 2g/sqrt(pi) e^(-g^2 r^2)) / r^2.  B2 = (3 B1 + 2g/sqrt(pi) 2 g^2 e^(-g^2 r^2)) / r^2.
    `kept` is a boolean array.  Returns (B1, B2)."""
    be = be or backend()
    return _ewald_b12(leaf(be, rsq), g, kept)


def _ewald_b12(rsq, g, kept):
    be = rsq.be
    kept = np.asarray(kept, bool) & np.ones(rsq.s.shape, bool)
    g = leaf(be, g + np.zeros_like(rsq.s))
    r = _sqrt(rsq)
    rinv, r2inv = _inv(r), _inv(rsq)
    gr = g * r
    e = g * be.two_over_sqrtpi * _exp(-(g * g * rsq))
    ec = Sum(be, np.where(kept, be.erfc(np.where(kept, gr.v, 0 * gr.v)), 0 * gr.v))
    ef = Sum(be, np.where(kept, 0 * gr.v, be.erf(np.where(kept, 0 * gr.v, gr.v))))
    b1k = (ec * rinv + e) * r2inv
    b1x = -((ef * rinv - e) * r2inv)
    b1 = b1k.where(kept) + b1x.where(~kept)
    b2 = (3 * b1 + 2 * (g * g * e)) * r2inv
    return b1, b2


# ---------------------------------------------------------------------------------------------------------------------
# the shifted-force static field factor, PS.cpp:324-361: E_i += ef_temp q_j d, ef_temp = (1/rsq + f_shift) / r

def static_field_factor(rsq, f_shift, be=None):
    be = be or backend()
    return _static_field_factor(leaf(be, rsq), f_shift)


def _static_field_factor(rsq, f_shift):
    return (_inv(rsq) + leaf(rsq.be, f_shift + np.zeros_like(rsq.s))) * _inv(_sqrt(rsq))


def rsq_of(d, be=None):
    """|d|^2 of exact FP64 displacements d [n, 3], in the backend's precision (what the kernels round to FP64)"""
    be = be or backend()
    dl = [leaf(be, np.asarray(d)[:, k]) for k in range(3)]
    return dl[0] * dl[0] + dl[1] * dl[1] + dl[2] * dl[2]


# ---------------------------------------------------------------------------------------------------------------------
# the polarization pair, PS.cpp:406-641 (oracle/polar_oracle.c polar_pair)

def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def polar_pair(d, mui, qi, ai, muj, qj, aj, molok, cut_coulsq, ddcutsq, f_shift, pd, e2s, damp, g_ewald=None, rsq64=None,
               be=None, terms=None):
    """The force on i from j and the pair's energies, n pairs at once.

    d [n, 3] = x_i - x_j(image); mui, muj [n, 3]; qi, ai, qj, aj, cut_coulsq, f_shift [n]; molok [n] bool; ddcutsq [n] or
    None (no dipole-dipole cutoff: the all-pairs form); pd, e2s, g_ewald scalars; damp 0 exponential, 1 none.
    g_ewald None: the shifted-force charge-dipole tensor of PS.cpp:454-510, rsq < cut_coulsq (strict) outside the molecule;
    else the gradient of the real-space Ewald field, rsq <= cut_coulsq, excluded pairs included with the erf form, and
    u_ef left alone (it is -sum mu . E there).  rsq64: the FP64 rsq that decides the cutoffs (default: computed here in
    FP64).  A dipole whose alpha is zero takes no part, whatever the array holds.  terms: what pair_terms() returned for
    the same pairs (the cutoffs only select).

    Returns a dict: cd, dd (lists of three Sums), uef, udd (Sums), cd_on, dd_on (which parts the reference evaluates)."""
    d = np.asarray(d, np.float64)
    if rsq64 is None:
        rsq64 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
    molok = np.asarray(molok, bool)
    ew = g_ewald is not None
    cd_on = (rsq64 <= cut_coulsq) if ew else ((rsq64 < cut_coulsq) & molok)
    dd_on = (np.asarray(ai) != 0) & (np.asarray(aj) != 0)
    if ddcutsq is not None:
        dd_on = dd_on & (rsq64 < ddcutsq)
    t = terms or pair_terms(d, mui, qi, ai, muj, qj, aj, molok, f_shift, pd, e2s, damp, g_ewald, be)
    return dict(cd_on=cd_on, dd_on=dd_on, cd=[c.where(cd_on) for c in t["cd"]], uef=t["uef"].where(cd_on),
                dd=[c.where(dd_on) for c in t["dd"]], udd=t["udd"].where(dd_on))


def pair_terms(d, mui, qi, ai, muj, qj, aj, molok, f_shift, pd, e2s, damp, g_ewald=None, be=None):
    """the parts of polar_pair() before the cutoffs select them"""
    be = be or backend()
    d = np.asarray(d, np.float64)
    z = np.zeros(len(d))
    molok = np.asarray(molok, bool)
    ew = g_ewald is not None
    out = {}
    dl = [leaf(be, d[:, k]) for k in range(3)]
    mi = [leaf(be, np.where(np.asarray(ai) != 0, np.asarray(mui)[:, k], 0.0)) for k in range(3)]
    mj = [leaf(be, np.where(np.asarray(aj) != 0, np.asarray(muj)[:, k], 0.0)) for k in range(3)]
    qi_, qj_ = leaf(be, qi + z), leaf(be, qj + z)
    e2s_ = leaf(be, e2s + z)
    sq = [dl[k] * dl[k] for k in range(3)]
    rsq = sq[0] + sq[1] + sq[2]
    r2inv = _inv(rsq)
    rinv = _sqrt(r2inv)
    r = _inv(rinv)
    r3inv = r2inv * rinv
    # --- charge-dipole
    if ew:
        b1, b2 = _ewald_b12(rsq, g_ewald, molok)
        pi_r, pj_r = _dot(mi, dl), _dot(mj, dl)
        cd = [e2s_ * qj_ * (b1 * mi[k] - b2 * pi_r * dl[k]) - e2s_ * qi_ * (b1 * mj[k] - b2 * pj_r * dl[k]) for k in range(3)]
        uef = Sum(be, be.arr(z))
    else:
        fs = leaf(be, f_shift + z)
        M = {}
        for p in range(3):
            a, b = (p + 1) % 3, (p + 2) % 3
            M[p, p] = (-2 * sq[p] + sq[a] + sq[b]) * r2inv + fs * (sq[a] + sq[b])
            for q in range(p + 1, 3):
                M[p, q] = M[q, p] = -3 * (dl[p] * dl[q]) * r2inv - fs * (dl[p] * dl[q])
        cfj, cfi = qj_ * e2s_ * r3inv, qi_ * e2s_ * r3inv
        cd = [cfj * (mi[0] * M[0, k] + mi[1] * M[1, k] + mi[2] * M[2, k]) -
              cfi * (mj[0] * M[0, k] + mj[1] * M[1, k] + mj[2] * M[2, k]) for k in range(3)]
        ef_temp = (_inv(rsq) + fs) * _inv(r) * e2s_
        ei = [ef_temp * qj_ * dl[k] for k in range(3)]
        ej = [ef_temp * qi_ * dl[k] for k in range(3)]
        uef = -_dot(mi, ei) + _dot(mj, ej)
    out["cd"], out["uef"] = cd, uef
    # --- dipole-dipole
    r5inv = r3inv * r2inv
    r7inv = r5inv * r2inv
    pdotp, pidotr, pjdotr = _dot(mi, mj), _dot(mi, dl), _dot(mj, dl)
    if damp == 0:
        pd_ = leaf(be, pd + z)
        t1 = _exp(-(pd_ * r), damp=True)
        t2 = 1 + pd_ * r + 0.5 * (pd_ * pd_ * r * r)
        t3 = t2 + _sixth(be) * (pd_ * pd_ * pd_ * r * r * r)
        g2, g3 = 1 - t1 * t2, 1 - t1 * t3
        pre1 = 3 * (r5inv * pdotp * g2) - 15 * (r7inv * pidotr * pjdotr * g3)
        pre2 = 3 * (r5inv * pjdotr * g3)
        pre3 = 3 * (r5inv * pidotr * g3)
        pre4 = -(pdotp * r3inv * (-(t1 * (pd_ * rinv + pd_ * pd_)) + t1 * pd_ * t2 * rinv))
        pre5 = 3 * (pidotr * pjdotr * r5inv * (-(t1 * (pd_ * rinv + pd_ * pd_ + 0.5 * (r * pd_ * pd_ * pd_))) + t1 * pd_ * t3 * rinv))
        dd = [pre1 * dl[k] + pre2 * mi[k] + pre3 * mj[k] + pre4 * dl[k] + pre5 * dl[k] for k in range(3)]
        udd = r3inv * pdotp * g2 - 3 * (r5inv * pidotr * pjdotr * g3)
    else:
        pre1 = 3 * (r5inv * pdotp) - 15 * (r7inv * pidotr * pjdotr)
        pre2 = 3 * (r5inv * pjdotr)
        pre3 = 3 * (r5inv * pidotr)
        dd = [pre1 * dl[k] + pre2 * mi[k] + pre3 * mj[k] for k in range(3)]
        udd = r3inv * pdotp - 3 * (r5inv * pidotr * pjdotr)
    out["dd"], out["udd"] = dd, udd
    return out


def to_f64(v, be=None):
    be = be or backend()
    return be.f64(v)


def err_over(got, ref, denom, be=None):
    """|got - ref| / denom as FP64, the difference taken in the backend's precision.  got: FP64 array."""
    be = be or backend()
    diff = np.abs(be.f64(be.arr(got) - ref))
    return diff / denom


EPS = math.ldexp(1.0, -53)
