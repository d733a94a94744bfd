"""Builds tests/ewald_kspace_probe/ewald_kspace_probe.hip for gfx950 with the library's own flags and wraps its two entry
points (tests/test_gpu_ewald_kspace.py; the plan entry also in tests/test_gpu_polar_ewald.py).

POLAR_EWALD_PROBE_CSRC (environment) points the include path at another copy of csrc: the way to check that a deliberately
broken kernel header fails the probe's tests."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
E2S = float(np.sqrt(332.06371))
PLAN_KEYS = ("nk", "nrow", "nm", "tile", "kb", "nchunk", "chunk")
NOTILT = (0.0, 0.0, 0.0)

# The boxes of tests/test_gpu_ewald_kspace.py with what polar_plan.hpp makes of them (asserted from the probe's plan entry,
# without a GPU in tests/test_ewald_kspace_ref_host.py): nm = the largest index bound, nk k-vectors, the tile of ewald_tile.
#        prd                 tilt              g     acc    nm  nk     tile
CASES = {
    "z16": ((8.0, 8.0, 37.0), NOTILT, 0.32, 1e-8, 16, 414, 32),
    "z17": ((8.0, 8.0, 39.0), NOTILT, 0.32, 1e-8, 17, 443, 32),
    "z31": ((8.0, 8.0, 71.5), NOTILT, 0.32, 1e-8, 31, 809, 31),
    "z32": ((8.0, 8.0, 74.0), NOTILT, 0.32, 1e-8, 32, 830, 30),
    "x33": ((76.0, 8.0, 8.0), NOTILT, 0.32, 1e-8, 33, 859, 29),
    "y48": ((8.0, 110.0, 9.0), NOTILT, 0.32, 1e-8, 48, 1384, 20),
    "tilted": ((14.0, 11.0, 40.0), (3.1, -2.2, 4.5), 0.32, 1e-8, 17, 1066, 32),
    "cube20": ((20.0, 20.0, 20.0), NOTILT, 0.6, 1e-12, 20, 16940, 32),
    "none": ((8.0, 8.0, 8.0), NOTILT, 0.32, 0.9, 0, 0, None),
}
AXIS_BOUNDS = {"z16": (3, 3, 16), "z17": (3, 3, 17), "z31": (3, 3, 31), "z32": (3, 3, 32), "x33": (33, 3, 3), "y48": (3, 48, 3),
               "tilted": (6, 4, 17), "cube20": (20, 20, 20)}


def load(pkg, directory):
    """compile into `directory`, load after the library (and with it torch's HIP runtime, see pkg.lib)"""
    pkg.lib()
    csrc = os.environ.get("POLAR_EWALD_PROBE_CSRC") or os.path.join(os.path.dirname(pkg.__file__), "csrc")
    so = os.path.join(str(directory), "libewald_kspace_probe.so")
    subprocess.check_call([pkg.HIPCC] + pkg.HIP_FLAGS + ["-Wno-unused-function", "-I", csrc, "-o", so,
                           os.path.join(HERE, "ewald_kspace_probe", "ewald_kspace_probe.hip")])
    lib = C.CDLL(so)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    lib.ewald_kspace_probe_plan.restype = C.c_int
    lib.ewald_kspace_probe_plan.argtypes = [dp, dp, C.c_double, C.c_double, C.c_int] + [ip] * 7
    lib.ewald_kspace_probe_run.restype = C.c_int
    lib.ewald_kspace_probe_run.argtypes = ([dp, dp, C.c_double, C.c_double, C.c_double, C.c_int, dp, dp, dp, dp, C.c_int, ip, dp, dp,
                                            C.c_int, C.c_int, dp, ip, ip] + [dp] * 5)

    def d(a):
        return a.ctypes.data_as(dp)

    def c(a):
        return np.ascontiguousarray(a, dtype=np.float64)

    class Probe:
        @staticmethod
        def plan(prd, tilt, g, acc, n):
            """host only: the table's sizes and the plan's tiling for n atoms"""
            prd, tilt = c(prd), c(tilt)
            v = [C.c_int(0) for _ in PLAN_KEYS]
            assert lib.ewald_kspace_probe_plan(d(prd), d(tilt), g, acc, n, *[C.byref(i) for i in v]) == 0
            return dict(zip(PLAN_KEYS, (i.value for i in v)))

        @staticmethod
        def run(sysd, tile=0, chunk=0, cur=0, perm=None, f0=None, muA=None, muB=None):
            """The six kernels on sysd (prd, tilt, g, acc, n, x, q, mu, ef_s); both records carry sysd's dipoles unless muA /
            muB say otherwise; tile / chunk 0: the plan's.  Asserts that no HIP call failed and that every guard word
            behind the device buffers is intact."""
            n = sysd["n"]
            pl = Probe.plan(sysd["prd"], sysd["tilt"], sysd["g"], sysd["acc"], n)
            nk, nrow = pl["nk"], pl["nrow"]
            prd, tilt = c(sysd["prd"]), c(sysd["tilt"])
            x, q, ef_s = c(sysd["x"]), c(sysd["q"]), c(sysd["ef_s"])
            muA = c(sysd["mu"] if muA is None else muA)
            muB = c(sysd["mu"] if muB is None else muB)
            f0 = np.zeros((n, 3)) if f0 is None else c(f0)
            assert x.shape == muA.shape == muB.shape == ef_s.shape == f0.shape == (n, 3) and q.shape == (n,)
            pm = None
            if perm is not None:
                pm = np.ascontiguousarray(perm, dtype=np.int32)
                assert sorted(pm.tolist()) == list(range(n))              # (f is indexed with it)
            kv, hkl, rows = np.zeros((nk, 4)), np.zeros((nk, 4), np.int32), np.zeros((nrow + 1, 4), np.int32)
            S, M, erec, f, out = np.zeros((nk, 2)), np.zeros((nk, 2)), np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(7)
            rc = lib.ewald_kspace_probe_run(d(prd), d(tilt), sysd["g"], sysd["acc"], E2S, n, d(x), d(q), d(muA), d(muB), int(cur),
                                            None if pm is None else pm.ctypes.data_as(ip), d(ef_s), d(f0), int(tile), int(chunk),
                                            d(kv), hkl.ctypes.data_as(ip), rows.ctypes.data_as(ip), d(S), d(M), d(erec), d(f), d(out))
            if rc > 0:          # after a HIP error nothing more goes to this GPU: the session ends here
                pytest.exit("HIP error %d in ewald_kspace_probe_run" % rc, returncode=3)
            assert rc == 0, "a guard word behind a device buffer of the probe was overwritten"
            return dict(plan=pl, kv=kv, hkl=hkl, rows=rows, S=S, M=M, erec=erec, f=f, out=out, f0=f0)
    return Probe
