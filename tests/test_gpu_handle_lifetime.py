"""Lifetime of a handle: what polar_create took from the runtime goes back with polar_destroy, whatever the handle was doing
(csrc/polar_own.hpp: the members free themselves, ~polar_handle only waits for the streams first).  The smallest golden
example, bulk_h2; every case is an ordinary use that has to end clean and leave the next handle of the process working.

List mode (dd_cutoff 9, `deterministic yes`: the setting under which the suite asks two runs for the same numbers) is held
against the oracle in the same truncated model, as test_gpu_parity does for list mode; the reference's own golden file is an
exact-mode run and is held against an exact-mode handle."""
import ctypes as C
import os

import numpy as np
import pytest

from helpers import GOLD, force_rel_err, golden_refs, load_ref_system, rel

pytestmark = pytest.mark.gpu

TOL = 1e-7            # test_gpu_parity's bar against the reference and the oracle
RUN_TO_RUN = 1e-12    # ... and between two runs on the same input
LIST_ARGS = ["use_previous", "no", "polar_gs_ranked", "yes", "dd_cutoff", "9.0", "deterministic", "yes", "precision", "1e-12",
             "max_iterations", "100"]
POLAR_OK, POLAR_ERR_NO_DEVICE = 0, -2


@pytest.fixture(scope="module")
def listed(wl, oracle):
    """bulk_h2 in list mode and what the oracle says about it (computed once, read only)."""
    s, _ = wl.load_fixture(os.path.join(GOLD, "bulk_h2.npz"), extra_args=LIST_ARGS)
    return s, oracle.compute(s, eflag=1, vflag=2)


def _check_listed(out, s, ref, oracle):
    assert out["status"] == 0 and ref["status"] == 0
    f = oracle.fold_ghost_forces(out["f"], s.owner, s.nlocal)
    assert force_rel_err(f, oracle.fold_ghost_forces(ref["f"], s.owner, s.nlocal)) < TOL
    assert np.max(np.abs(out["mu"] - ref["mu"])) / np.max(np.abs(ref["mu"])) < TOL
    for k in ("eng_vdwl", "eng_coul", "eng_pol"):
        assert rel(out[k], ref[k], 1e-9) < TOL, k
    assert np.max(np.abs(out["virial"] - ref["virial"])) < TOL * max(1.0, np.max(np.abs(ref["virial"])))


def _fresh_handle_computes(pkg, s, ref, oracle):
    p = pkg.pair_from_system(s)
    out = p.compute()
    assert p.L.polar_destroy(p.h) == POLAR_OK
    p.h = C.c_void_p()
    _check_listed(out, s, ref, oracle)


def _same(outs):
    for b in outs[1:]:
        for k in ("eng_vdwl", "eng_coul", "eng_pol", "u_self", "u_ef", "u_dd"):
            assert rel(b[k], outs[0][k], 1e-9) < RUN_TO_RUN, k
        assert np.max(np.abs(b["mu"] - outs[0]["mu"])) <= RUN_TO_RUN * np.max(np.abs(outs[0]["mu"]))
        assert b["iterations"] == outs[0]["iterations"]


def test_create_compute_destroy_three_times_in_list_mode(pkg, listed, oracle):
    s, ref = listed
    outs = []
    for _ in range(3):
        p = pkg.pair_from_system(s)
        outs.append(p.compute())
        assert p.L.polar_destroy(p.h) == POLAR_OK
        p.h = C.c_void_p()
    _same(outs)
    for out in outs:
        _check_listed(out, s, ref, oracle)


def test_create_compute_destroy_three_times_against_the_golden_file(wl, pkg, oracle):
    path, info = [(p, i) for p, i in golden_refs("bulk_h2") if i["variant"] == "ranked"][0]
    z = np.load(path)
    s, _ = load_ref_system(wl, info)
    outs = []
    for _ in range(3):
        p = pkg.pair_from_system(s, modify_args=info.get("modify_args", ()))
        outs.append(p.compute(eflag=info.get("eflag", 1), vflag=info.get("vflag", 2)))
        assert p.L.polar_destroy(p.h) == POLAR_OK
        p.h = C.c_void_p()
    _same(outs)
    for out in outs:
        assert force_rel_err(oracle.fold_ghost_forces(out["f"], s.owner, s.nlocal), z["f"]) < TOL
        assert np.max(np.abs(out["mu"] - z["mu"])) / max(np.max(np.abs(z["mu"])), 1e-30) < TOL
        assert np.max(np.abs(out["ef_static"] - z["ef_static"])) / np.max(np.abs(z["ef_static"])) < TOL
        for k, e in zip(("eng_vdwl", "eng_coul", "eng_pol"), z["energies"]):
            assert rel(out[k], e, 1e-6) < TOL, k
        assert np.max(np.abs(out["virial"] - z["virial"])) < TOL * max(1.0, np.max(np.abs(z["virial"])))
        assert (out["status"] == 1) == bool(info["warnings"])


def test_destroy_while_the_list_is_still_on_its_way(pkg, listed, oracle):
    """polar_set_neighbors returns when the rows are packed, not when they have arrived (their own stream)."""
    s, ref = listed
    p = pkg.pair_from_system(s)          # ... ends with the upload of the list
    assert p.L.polar_destroy(p.h) == POLAR_OK
    p.h = C.c_void_p()
    _fresh_handle_computes(pkg, s, ref, oracle)


def test_destroy_in_the_middle_of_a_step(pkg, listed, oracle):
    s, ref = listed
    p = pkg.pair_from_system(s)
    p._ck(p.L.polar_step_begin(p.h, 1, 2))
    assert p.L.polar_destroy(p.h) == POLAR_OK        # no polar_step_finish
    p.h = C.c_void_p()
    _fresh_handle_computes(pkg, s, ref, oracle)


def test_a_stream_of_the_caller_outlives_the_handle(pkg, listed, oracle):
    import torch

    s, ref = listed
    stream = torch.cuda.Stream()
    p = pkg.pair_from_system(s)
    p._ck(p.L.polar_set_stream(p.h, C.c_void_p(stream.cuda_stream)))
    out = p.compute()
    assert p.L.polar_destroy(p.h) == POLAR_OK
    p.h = C.c_void_p()
    _check_listed(out, s, ref, oracle)
    with torch.cuda.stream(stream):                  # the stream is the caller's: still there, still working
        t = torch.arange(1024, device="cuda", dtype=torch.float64)
        total = (2.0 * t).sum()
    stream.synchronize()
    assert float(total) == 1023.0 * 1024.0


def test_a_handle_without_a_device_fails_loudly_and_goes_quietly(pkg, listed):
    s, _ = listed
    p = pkg.PolarPair(device=pkg.device_count())     # one past the last
    assert p.h
    p.load_system(s)                                 # the host mirror works
    with pytest.raises(pkg.PolarError) as e:
        p.set_atoms(s.nlocal, s.nghost, s.x, s.q, s.alpha, s.type, s.molecule)
    assert e.value.code == POLAR_ERR_NO_DEVICE
    nall = s.nlocal + s.nghost
    f, mu, res = np.zeros((nall, 3)), np.zeros((s.nlocal, 3)), pkg.Result()
    dp = C.POINTER(C.c_double)
    assert p.L.polar_compute(p.h, 1, 2, f.ctypes.data_as(dp), mu.ctypes.data_as(dp), None, C.byref(res)) == POLAR_ERR_NO_DEVICE
    assert p.L.polar_compute_resident(p.h, 1, 2, C.byref(res)) == POLAR_ERR_NO_DEVICE
    assert b"no CPU fallback" in p.L.polar_last_error(p.h)
    assert p.L.polar_destroy(p.h) == POLAR_OK
    p.h = C.c_void_p()
