"""High-precision reference for polar_point_grad_pair_ew (csrc/polar_ewald_point_grad.hpp): ONE atom's terms of the gradient of
the real-space Ewald field at a point, on the `Sum` backends of tests/pair_ref.py (value and scale = the sum of the absolute
terms), written from the definition: g_static_ab = e2s q_j (B1 delta_ab - B2 d_a d_b) with pair_ref's B1 and B2.  The induced
terms are tests/point_grad_ref.py's.  pair_ref.py itself stays as it is; what is added here is the gradient and, for excluded
atoms very close to the point, B1 and B2 to the precision of their VALUE (the scale of the closed form is that of its
cancelling terms): their Taylor series in x = g r at the backend's precision."""
import math

import numpy as np

import pair_ref as pr
import point_grad_ref as pgr

COMP = pgr.COMP


def static_grad_terms(d, q, kept, e2s, g, be=None):
    """six Sums, one atom per row at r > 0, before the cutoff selects"""
    be = be or pr.backend()
    d = np.asarray(d, np.float64)
    z = np.zeros(len(d))
    dl = [pr.leaf(be, d[:, k]) for k in range(3)]
    q_, e2s_ = pr.leaf(be, q + z), pr.leaf(be, e2s + z)
    rsq = dl[0] * dl[0] + dl[1] * dl[1] + dl[2] * dl[2]
    b1, b2 = pr._ewald_b12(rsq, g, np.asarray(kept, bool))
    out = []
    for a, b in COMP:
        t = -(e2s_ * q_ * (b2 * dl[a] * dl[b]))
        if a == b:
            t = t + e2s_ * q_ * b1
        out.append(t)
    return out


def grad_pair_ew(d, q, mu, alpha, kept, induced, cut_coul, dd_cutoff, pd, e2s, g, damp, be=None):
    """The cutoffs applied (decided on the FP64 rsq the kernel sees).  kept / induced as polar_point_grad_pair_ew; an atom on the
    point is left to the caller (its limit is a closed expression).  Returns dict(st_on, in_on, gs, gi)."""
    be = be or pr.backend()
    d = np.asarray(d, np.float64)
    rsq64 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
    on = rsq64 == 0
    st_on = ~on & (rsq64 <= cut_coul * cut_coul)
    safe = np.where(on[:, None], 1.0, d)
    gs = [c.where(st_on) for c in static_grad_terms(safe, q, np.asarray(kept, bool) & ~on, e2s, g, be)]
    ind = pgr.grad_pair(d, q, mu, alpha, np.zeros(len(d), bool), cut_coul, dd_cutoff, pd, e2s, damp, be)
    in_on = ind["in_on"] & (np.asarray(induced) != 0)
    return dict(st_on=st_on, in_on=in_on, gs=gs, gi=[c.where(in_on) for c in ind["gi"]])


def excluded_b12_series(rsq, g, be=None, terms=40):
    """(B1, B2) of the erf form as backend arrays, by their series in x^2 = g^2 r^2 (x < 1):
    B1 = g^3 2/sqrt(pi) sum_{n>=1} (-1)^n x^(2n-2) 2n / ((2n+1) n!), B2 = g^5 2/sqrt(pi) sum_{n>=2} (-1)^n x^(2n-4) 4n(1-n) / ((2n+1) n!)"""
    be = be or pr.backend()
    g_ = be.arr(g + np.zeros(len(rsq)))
    t = g_ * g_ * be.arr(rsq)
    b1, b2 = 0 * t, 0 * t
    for n in range(terms, 0, -1):
        b1 = b1 * t
        b2 = b2 * t if n >= 2 else b2
        f = be.arr(np.array([-1.0 if n % 2 else 1.0]))[0] / ((2 * n + 1) * math.factorial(n))   # (the quotient in the backend's precision)
        b1 = b1 + f * (2 * n)
        if n >= 2:
            b2 = b2 + f * (4 * n * (1 - n))
    c = be.two_over_sqrtpi
    return g_ * g_ * g_ * c * b1, g_ * g_ * g_ * g_ * g_ * c * b2
