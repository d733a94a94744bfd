"""The shortest solves: 1 to 3 sweeps (`max_iterations` 0, 1, 2), where the end-of-sweep schedule (csrc/polar_plan.hpp,
sweep_end) has its edges: the count of k_solver_step after the last two sweeps of a fixed-iteration Gauss-Seidel solve, "no
mixing after the last sweep", "all-reduce once sw >= iterations_max".  On one handle and through the in-library driver
(polar_dist_step) with the one rank a test box has, which exchanges every third row with itself.

bulk_h2 (750 atoms), `use_previous no`.  The counters (sweeps, iterations, status) are the CPU oracle's; dipoles and E_pol are
held against it where the iteration does not depend on the order of the rows (Jacobi, the fallback alpha * E of a solve that
did not converge) or follows the oracle's order (exact mode)."""
import os

import numpy as np
import pytest

from helpers import GOLD, rel

pytestmark = pytest.mark.gpu

TOL = 1e-7
BASE = ["use_previous", "no"]
LIST = BASE + ["dd_cutoff", "9.0"]
_cache = {}


def _system(wl, extra):
    key = tuple(extra)
    if key not in _cache:
        _cache[key] = [wl.load_fixture(os.path.join(GOLD, "bulk_h2.npz"), extra_args=list(extra))[0], None]
    return _cache[key][0]


def _oracle(wl, oracle, extra):
    """The oracle's result for these keywords: computed once, shared, never written to."""
    s = _system(wl, extra)
    if _cache[tuple(extra)][1] is None:
        _cache[tuple(extra)][1] = oracle.compute(s, eflag=1, vflag=2)
    return _cache[tuple(extra)][1]


def _counters(out):
    return (out["sweeps"], out["iterations"], out["status"])


def _one_handle(pkg, s):
    p = pkg.pair_from_system(s)
    out = p.compute(eflag=1, vflag=2)
    p.close()
    return out


def _driver(pkg, s, schedules=("sweep", "phase"), reduce_every=1):
    """polar_dist_step with one rank per schedule: one exchange per sweep, then per colour phase (set_schedule(0, 0, 1))."""
    p = pkg.pair_from_system(s)
    p._ck(p.L.polar_set_list_style(p.h, 0))
    d = pkg.PolarDist(pkg.PolarDist.unique_id(), 0, 1, device=0)
    rows = np.arange(0, s.nlocal, 3, dtype=np.int32)
    d.set_halo(p, [0], [rows], [rows])
    d.set_cadence(reduce_every=reduce_every, check_every=4)
    outs = {}
    for sched in schedules:
        if sched == "phase":
            d.set_schedule(0, 0, 1)
        out = d.step(p, eflag=1, vflag=2)
        out["mu"] = p.download("mu", 3 * s.nlocal).reshape(-1, 3)
        outs[sched] = out
    d.close()
    p.close()
    return outs


def _close(a, b):
    return np.max(np.abs(a - b)) / np.max(np.abs(b)) < TOL


@pytest.mark.parametrize("M", [0, 1, 2])
def test_fixed_iteration_gauss_seidel_on_one_handle_and_through_the_driver(M, wl, pkg, oracle):
    """Cases 1 and 2: M + 1 sweeps, M iterations, status 0 as the oracle; the driver's one rank, exchanging with itself, runs the
    same iteration on both schedules (fixed-iteration runs take the deterministic commit): the same dipoles."""
    extra = LIST + ["polar_gs_ranked", "yes", "fixed_iteration", "yes", "max_iterations", str(M)]
    ref = _oracle(wl, oracle, extra)
    s = _system(wl, extra)
    one = _one_handle(pkg, s)
    assert _counters(one) == _counters(ref) == (M + 1, M, 0)
    for sched, out in _driver(pkg, s).items():
        assert _counters(out) == (M + 1, M, 0), sched
        assert _close(out["mu"], one["mu"]), sched


@pytest.mark.parametrize("M", [0, 1, 2])
def test_fixed_iteration_jacobi(M, wl, pkg, oracle):
    """Case 3: Jacobi does not depend on the order of the rows: dipoles and E_pol are the oracle's."""
    extra = LIST + ["polar_gs_ranked", "no", "polar_gs", "no", "fixed_iteration", "yes", "max_iterations", str(M)]
    ref = _oracle(wl, oracle, extra)
    s = _system(wl, extra)
    for name, out in [("one handle", _one_handle(pkg, s)), ("driver", _driver(pkg, s, schedules=("sweep",))["sweep"])]:
        assert _counters(out) == _counters(ref) == (M + 1, M, 0), name
        assert _close(out["mu"], ref["mu"]), name
        assert rel(out["eng_pol"], ref["eng_pol"], 1e-9) < TOL, name


@pytest.mark.parametrize("M", [0, 1, 2])
def test_precision_mode_that_cannot_converge(M, wl, pkg, oracle):
    """Case 4: the default precision is out of reach in M + 1 sweeps: M + 1 iterations, status 1, and the dipoles are the
    fallback alpha * E, whatever the order of the rows.  The driver with the change all-reduced after every sweep and after
    every second one -- the last sweep (sw >= iterations_max) reduces either way, or no rank would see the end."""
    extra = LIST + ["polar_gs_ranked", "yes", "fixed_iteration", "no", "max_iterations", str(M)]
    ref = _oracle(wl, oracle, extra)
    s = _system(wl, extra)
    runs = [("one handle", _one_handle(pkg, s))]
    for r in (1, 2):
        runs += [(f"driver reduce_every {r} {k}", o) for k, o in _driver(pkg, s, reduce_every=r).items()]
    for name, out in runs:
        assert _counters(out) == _counters(ref) == (M + 1, M + 1, 1), name
        assert _close(out["mu"], ref["mu"]), name
        assert rel(out["eng_pol"], ref["eng_pol"], 1e-9) < TOL, name


@pytest.mark.parametrize("M", [1, 2])
def test_polar_accel_with_fixed_iteration_gauss_seidel(M, wl, pkg, oracle):
    """Case 5: mixing after every sweep but the last; the counters are those of the plain solve (no claim on the dipoles)."""
    plain = LIST + ["polar_gs_ranked", "yes", "fixed_iteration", "yes", "max_iterations", str(M)]
    ref = _oracle(wl, oracle, plain)
    s = _system(wl, plain + ["polar_accel", "3"])
    for name, out in [("one handle", _one_handle(pkg, s)), ("driver", _driver(pkg, s, schedules=("sweep",))["sweep"])]:
        assert _counters(out) == _counters(ref) == (M + 1, M, 0), name
        assert np.all(np.isfinite(out["mu"])), name


@pytest.mark.parametrize("form", ["dense", "matrix_free"])
@pytest.mark.parametrize("fixed", ["yes", "no"])
@pytest.mark.parametrize("M", [0, 1])
def test_exact_mode(M, fixed, form, wl, pkg, oracle, monkeypatch):
    """Case 6: exact mode (no dd_cutoff) sweeps in the oracle's order, on the HBM-resident tensor and matrix-free."""
    extra = BASE + ["polar_gs_ranked", "yes", "fixed_iteration", fixed, "max_iterations", str(M)]
    ref = _oracle(wl, oracle, extra)
    if form == "matrix_free":
        monkeypatch.setenv("POLAR_NO_DENSE_GS", "1")
    out = _one_handle(pkg, _system(wl, extra))
    assert _counters(out) == _counters(ref) == ((M + 1, M, 0) if fixed == "yes" else (M + 1, M + 1, 1))
    assert _close(out["mu"], ref["mu"])
    assert rel(out["eng_pol"], ref["eng_pol"], 1e-9) < TOL
