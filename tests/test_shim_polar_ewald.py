"""The LAMMPS shim with `polar_ewald` (no GPU): compute() executed inside the base class of the LAMMPS sources the shim
harnesses are built against (oracle/Makefile's REF), against the recording stub of the C-ABI
(tests/shim_host/shim_ewald_harness.cpp).  The reciprocal forces land in atom->f but their virial is not sum f.x: the shim
must ask the library for the global virial instead of leaving it to virial_fdotr_compute.  Skips where those sources are
absent, like the other shim harnesses."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE = os.path.join(ROOT, "oracle")


def _ref_dir():
    r = subprocess.run(["make", "-s", "-C", ORACLE, "--no-print-directory", "--eval=print-ref: ; @echo $(REF)", "print-ref"],
                       capture_output=True, text=True)
    return r.stdout.strip()


REF = _ref_dir()
pytestmark = pytest.mark.skipif(not REF or not os.path.exists(os.path.join(REF, "pair.cpp")),
                                reason="the LAMMPS sources of oracle/Makefile's REF are not present")


def test_shim_hands_the_global_virial_to_the_library_with_polar_ewald(tmp_path):
    so = str(tmp_path / "libshimewald.so")
    cmd = ["g++", "-O1", "-fPIC", "-shared", "-std=c++11", "-w", f"-I{REF}", f"-I{REF}/STUBS", f"-I{ROOT}/include",
           f"-I{ROOT}/lammps_shim", f"-I{ORACLE}/ref_seam", "-o", so,
           os.path.join(ROOT, "tests", "shim_host", "shim_ewald_harness.cpp"),
           os.path.join(ROOT, "lammps_shim", "pair_lj_cut_coul_long_polarization_mi355x.cpp"),
           os.path.join(REF, "pair_lj_cut_coul_long_polarization.cpp"), os.path.join(REF, "pair.cpp"),
           os.path.join(REF, "memory.cpp"), "-x", "c", os.path.join(REF, "STUBS", "mpi.c")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    L = C.CDLL(so)
    n = C.c_int(0)
    msg = C.create_string_buffer(1024)
    rc = L.shimewald_check(C.byref(n), msg, 1024)
    assert rc == 0, msg.value.decode()
    assert n.value == 2 * 3
