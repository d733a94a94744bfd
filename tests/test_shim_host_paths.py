"""The host-side paths of the LAMMPS shim run INSIDE the reference's own Pair base class, next to the reference's pair style
(tests/shim_host/shim_host_harness.cpp): init / cutsq / single() / extract() must agree with the reference's, and the restart
records must be interchangeable with the reference's in both directions.  The harnesses are compiled by build()
(oracle/Makefile `ref`, into oracle/_ref/) where the reference's sources are present; without them these skip.  No GPU needed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILT = os.path.join(ROOT, "oracle", "_ref")
PKG = os.path.join(ROOT, "lammps-induced-dipole-polarization-pair-style_amd")
LIB = os.path.join(PKG, "libpolar_mi355x.so")
HARNESSES = ["libshimhost.so", "libshimcompute.so", "atomvec_check", "atomvec_check_asan"]

pytestmark = pytest.mark.skipif(not os.path.exists(LIB) or not all(os.path.exists(os.path.join(BUILT, h)) for h in HARNESSES),
                                reason="oracle/_ref harnesses not built (build() makes them where the reference's sources are present)")


@pytest.fixture(scope="module")
def harness(tmp_path_factory, pkg):
    d = tmp_path_factory.mktemp("shimhost")
    os.environ["POLAR_HOST_PATHS_ONLY"] = "1"   # init_style would otherwise (rightly) refuse a machine without a GPU
    pkg.lib()   # the library's own load order (torch first), before the harness maps it
    L = C.CDLL(os.path.join(BUILT, "libshimhost.so"))
    L.shimhost_check.restype = C.c_int
    return L, str(d)


def _strs(a):
    arr = (C.c_char_p * len(a))(*[s.encode() for s in a])
    return arr


CASES = {
    "mof_like": (["2.5", "12.8345", "precision", "1e-11", "max_iterations", "100", "damp_type", "exponential", "damp", "2.1304",
                  "polar_gs_ranked", "yes", "debug", "no", "use_previous", "yes"], [],
                 ["1 1 0.123980 2.462000 6.155000", "1 2 0.086237 2.790000 6.975000", "2 2 0.059984 3.118000 7.795000",
                  "2 3 0.051368 2.844500", "3 3 0.043989 2.571000 6.427500", "1 3 0.0 1.0"]),
    "mixed_shifted_notable": (["9.0", "10.5"], ["mix", "arithmetic", "shift", "yes", "table", "0"],
                              ["1 1 0.10 3.0", "2 2 0.20 3.5 8.0", "3 3 0.05 2.8"]),
    "tabinner": (["2.5", "9.0", "damp_type", "none"], ["table", "10", "tabinner", "2.0", "mix", "geometric"],
                 ["* * 0.07 3.1", "2 3 0.2 2.0 12.0"]),
}


@pytest.mark.parametrize("case", list(CASES))
def test_shim_host_paths_agree_with_the_reference(case, harness):
    L, tmp = harness
    style, mod, rows = CASES[case]
    rep = (C.c_double * 8)()
    msg = C.create_string_buffer(512)
    rc = L.shimhost_check(tmp.encode(), 3, C.c_double(0.195492), C.c_double(332.06371), len(style), _strs(style),
                          len(mod), _strs(mod), len(rows), _strs(rows), rep, msg, 512)
    assert rc == 0, msg.value.decode()
    r = list(rep)
    # cutsq identical, single() to rounding (the library evaluates the same formulas and reads the base class's own tables)
    assert 0.0 <= r[0] < 1e-14, r
    assert 0.0 <= r[1] < 1e-14, r     # the reference's restart file read by the shim
    assert 0.0 <= r[2] < 1e-14, r     # the shim's restart file read by the reference
    assert r[3] == 0.0, r             # restart_polar yes: every polarization keyword came back
    assert r[5] > 1.0 and r[6] > 1.0, r   # the comparisons saw real energies and forces (kcal/mol, charges 0.4 / -0.7)
    assert r[7] == 0.0, r             # write_data / write_data_all: the reference's text
    assert r[4] == 0.0, r             # extract("cut_coul" | "epsilon" | "sigma") as the reference's, unknown names -> NULL


FAULTS = [
    ([], [], 0, 0),
    (["9", "9", "zodid", "yes"], [], 0, 0),
    (["9", "9", "polar_gs", "yes"], [], 0, 0),
    (["9", "precision", "1e-8"], [], 0, 0),
    (["9", "9", "damp_type", "thole"], [], 0, 0),
    (["9", "9", "debug", "maybe"], [], 0, 0),
    (["9", "9", "max_iterations", "3.5"], [], 0, 0),
    (["9", "9", "nonsense", "1"], [], 0, 0),
    (["9", "9"], ["1 1 0.1"], 0, 0),
    (["9", "9"], ["1 4 0.1 3.0"], 0, 0),
    (["9", "9"], ["1 1 0.1 3.0 x"], 0, 0),
    (["9", "9"], ["1 1 0.1 3.0"], 1, 0),                      # init with unset coefficients
    (["9", "9"], ["* * 0.1 3.0"], 1, 1),                      # no charges
    (["9", "9"], ["* * 0.1 3.0"], 1, 2),                      # no polarizability attribute
    (["9", "9"], ["* * 0.1 3.0"], 1, 4),                      # no KSpace style
    (["9", "9", "polar_gs_ranked", "no", "polar_gs", "yes"], ["* * 0.1 3.0", "1 2 0.2 3.1 7.0"], 1, 0),   # accepted by both
]


@pytest.mark.parametrize("style,rows,do_init,flags", FAULTS)
def test_faulty_input_gets_the_reference_error_text(style, rows, do_init, flags, harness):
    """The same input through the reference's pair style and through the shim, in one process: both accept it, or both stop
    with the same error->all text."""
    L, _ = harness
    L.shimhost_message.restype = C.c_int
    out = []
    for which in (0, 1):
        msg = C.create_string_buffer(512)
        rc = L.shimhost_message(which, 3, flags, len(style), _strs(style), len(rows), _strs(rows), do_init, msg, 512)
        out.append((rc, msg.value.decode()))
    assert out[0] == out[1], out


def test_halo_map_of_the_one_rank_per_gpu_path(harness):
    """build_halo_map: LAMMPS order -> [own | one ghost per foreign tag | other ghosts], half list re-indexed, special bits kept."""
    L, _ = harness
    msg = C.create_string_buffer(1024)
    assert L.shimhost_halo_map(msg, 1024) == 0, msg.value.decode()


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan"])
def test_atom_style_round_trips_inside_the_reference_atom_vec(sanitize):
    """lammps_shim/atom_vec_full_polar.cpp on top of the reference's AtomVec / AtomVecFull (tests/shim_host/
    atom_vec_harness.cpp): grow, copy, exchange, border (with velocities, with a grow inside the stock unpack), restart records
    with and without fixes' per-atom data behind the stock fields, create_atom, property names."""
    # (the asan build: -fsanitize=address,undefined without vptr checks, which need the typeinfo of LAMMPS classes the
    # harness does not build; oracle/Makefile)
    exe = os.path.join(BUILT, "atomvec_check_asan" if sanitize else "atomvec_check")
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and r.stdout.split()[0] == "0", (r.stdout, r.stderr[-3000:])


def test_shim_compute_marshalling_against_a_recording_stub():
    """PairLJCutCoulLongPolarizationMI355X::compute() EXECUTED (inside the reference's Pair base class:
    ev_setup and virial_fdotr_compute are src/pair.cpp's) against a recording stub of the C-ABI
    (tests/shim_host/shim_compute_harness.cpp), for eflag 0-3 x vflag {0,1,2,4,5,6} x device_neigh {no, yes} x
    neighbor->ago {0, 3} x {converged, not converged}: call sequence, pointer identities, the eflag / vflag mapping, lists
    handed over only on reneighbor steps, f += semantics, eng_vdwl / eng_coul / eng_pol / virial write-back,
    virial_fdotr_compute reached exactly when the reference's compute() reaches it (PS.cpp:644), warning ->
    error->warning, library error -> error->all."""
    L = C.CDLL(os.path.join(BUILT, "libshimcompute.so"))
    n = C.c_int(0)
    msg = C.create_string_buffer(1024)
    rc = L.shimcompute_check(C.byref(n), msg, 1024)
    assert rc == 0, msg.value.decode()
    assert n.value == 2 * 2 * 2 * 4 * 6
    # one MPI rank per GPU (comm->nprocs > 1 -> compute_sharded): library order [own | halo | other ghosts], row range, the
    # re-indexed list, the per-sweep sequence around MPI_Allreduce and Comm::forward_comm_pair (emulated through the shim's own
    # pack_forward_comm / unpack_forward_comm), the stop at the sweep the library reports, results back in LAMMPS order;
    # device_neigh {no, yes} x fixed_iteration {no, yes} x eflag {0, 3} x vflag {0, 2, 4, 6}, and the two refusals
    n2 = C.c_int(0)
    rc = L.shimsharded_check(C.byref(n2), msg, 1024)
    assert rc == 0, msg.value.decode()
    assert n2.value == 2 * 2 * 2 * 4 + 2   # + rccl_halo yes with device_neigh {no, yes}: this rank's share of energies / virial, not the sums over the ranks
