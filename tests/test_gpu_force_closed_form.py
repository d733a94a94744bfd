"""The closed-form pair arithmetic of the polarization force kernels (csrc/polar_force_pair.hpp, the product library) against
the term-by-term form it replaced (csrc/lab/force_pair_literal.hpp: the lab library with POLAR_FORCE_LITERAL=1), on the same
inputs.

Both libraries solve the same dipoles under settings whose runs repeat bit for bit (exact mode; list mode with
`fixed_iteration yes` and `deterministic yes`), so only the force arithmetic differs.  Bounds: the two forms agree to ~1e-12
per pair (the term-by-term form's cancellation at short range, tests/test_force_pair_host.py) and a row has at most ~1,000
pairs: per-atom force <= 1e-10 of the largest force, eng_pol <= 1e-12 relative, virial <= 1e-10 relative."""
import os

import numpy as np
import pytest

from helpers import GOLD

pytestmark = pytest.mark.gpu

FIXED = ["use_previous", "no", "fixed_iteration", "yes", "max_iterations", "10"]
LIST = ["dd_cutoff", "9.0", "deterministic", "yes"]
CASES = [
    ("bulk_h2", "exact", []),
    ("bulk_h2", "list", []),           # box = 2 cut_coul exactly: pairs sit right at the strict rsq < cut_coulsq boundary
    ("mof5_h2", "exact", []),
    ("mof5_h2", "list", []),
    ("mof5_h2", "exact", ["damp_type", "none", "max_iterations", "4"]),   # undamped: a few sweeps, before it diverges
    ("mof5_h2", "list", ["damp_type", "none", "max_iterations", "4"]),
    ("mof5_h2", "exact", ["polar_ewald", "1e-6"]),
    ("mof5_h2", "list", ["polar_ewald", "1e-6"]),
]


def _run(pkg, s, lab, eflag, vflag):
    p = pkg.pair_from_system(s, lab=lab)
    try:
        return p.compute(eflag=eflag, vflag=vflag)
    finally:
        p.close()


@pytest.mark.parametrize("eflag,vflag", [(1, 2), (3, 5)])
@pytest.mark.parametrize("case,mode,extra", CASES)
def test_closed_form_forces_match_the_term_by_term_form(case, mode, extra, eflag, vflag, wl, pkg, monkeypatch):
    args = FIXED + (LIST if mode == "list" else []) + extra
    if "polar_ewald" in extra:
        vflag &= ~4    # polar_ewald refuses the per-atom virial (no pairwise reciprocal-space virial): 3/5 becomes 3/1 there
    s, _ = wl.load_fixture(os.path.join(GOLD, case + ".npz"), extra_args=args)
    new = _run(pkg, s, False, eflag, vflag)
    monkeypatch.setenv("POLAR_FORCE_LITERAL", "1")
    old = _run(pkg, s, True, eflag, vflag)
    assert new["status"] == old["status"]
    assert np.all(np.isfinite(new["f"])) and np.all(np.isfinite(old["f"]))
    mumax, fmax = np.max(np.abs(old["mu"])), np.max(np.abs(old["f"]))
    dmu = np.max(np.abs(new["mu"] - old["mu"])) / mumax
    df = np.max(np.abs(new["f"] - old["f"])) / fmax
    de = abs(new["eng_pol"] - old["eng_pol"]) / abs(old["eng_pol"])
    dv = np.max(np.abs(np.asarray(new["virial"]) - np.asarray(old["virial"]))) / np.max(np.abs(old["virial"]))
    print("%s %s %s eflag %d vflag %d: dmu %.2e  df %.2e  deng_pol %.2e  dvirial %.2e" % (case, mode, extra[:2], eflag, vflag, dmu, df, de, dv))
    # the lab run really took the term-by-term path: two different arithmetics do not agree in every bit of every force
    assert not np.array_equal(new["f"], old["f"])
    assert dmu <= 1e-12          # the premise: the same dipoles go into both force kernels
    assert df <= 1e-10
    assert de <= 1e-12
    assert dv <= 1e-10
    for k in ("vatom", "eatom"):
        if old[k] is not None:
            d = np.max(np.abs(new[k] - old[k])) / np.max(np.abs(old[k]))
            print("   %s %.2e" % (k, d))
            assert d <= 1e-10
