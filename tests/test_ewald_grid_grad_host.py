"""polar_ewald_field_grad_grid without a GPU: the plain-C++ arithmetic of its kernels (csrc/polar_ewald_grid_grad.hpp) and the
layout arithmetic (csrc/polar_plan.hpp), built by g++ with libm (tests/ewald_grid_grad/ewald_grid_grad.cpp).

1. The three-stage gradient sums against the direct NumPy sum (tests/ewald_point_grad_numpy.py::recip_grad_sums) at the grid's
   points: the tilted 60-atom box of tests/test_ewald_grid_host.py (seed 620, every charge raised by 0.05, origin at
   (-3.5, 7.25, 41)), 917 and 16,926 k-vectors, five grids.  Bound: 1e-12 of sum_k c_k |k|^2 |S(k)| -- the bound
   tests/test_ewald_grid_host.py uses for the field with sum_k c_k |k| |S|, by the same argument: a phase is the product of three
   table entries, each one sincospi of an argument rounded to 2^-53 of it, and no recurrence.  The field sums of the same call
   are held to that test's bound as well.
2. The field part has the bits of ew_grid_recip_eval of tests/ewald_grid/ewald_grid.cpp on the same inputs.
3. Passes of 37, 5 and 1 points with runs of 1 and 2 lines give the bits of one pass; without the field outputs the gradient bits
   are the same.
4. The trace gxx + gyy + gzz against sum_k c_k |k|^2 Re(e^{ik.p} conj S) summed directly, within the same bound: this pins the
   component order (the diagonal first) and, with item 1, the order of the other three.  The sign is that of
   g_recip_ab = Re sum_k (k_a k_b U_k) e^{ik.p}, whose trace is PLUS sum_k c_k |k|^2 Re(e^{ik.p} conj S): d/dx_b of
   e_a = sum_k c_k k_a Im(e^{ik.p} conj S) is sum_k c_k k_a k_b Re(e^{ik.p} conj S), the reciprocal term of
   tests/ewald_point_grad_numpy.py and of DESIGN section 6i.
5. The layout: nine sets, 144 bytes per element of T and V, V per run within 64 MB.
6. The harness as a stand-alone program under the address and undefined-behaviour sanitizers.
7. The package binds the entry point, has the two compositions, and refuses an unknown ``recip`` before any library call."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ewald_point_grad_numpy as egn
import ewald_point_numpy as epn
import test_ewald_grid_host as gh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "lammps-induced-dipole-polarization-pair-style_amd")
SRC = os.path.join(ROOT, "tests", "ewald_grid_grad", "ewald_grid_grad.cpp")
SRC4 = os.path.join(ROOT, "tests", "ewald_grid", "ewald_grid.cpp")
LO = gh.LO
GRIDS = gh.GRIDS + [((3, 1, 130), (0.0, 0.25, 0.9))]
IDS = ["8x6x4", "5x7x3_offset", "67x3x2", "1x1x1", "3x1x130_offset"]
TABLES = [(0.32, 1e-6), (0.6, 1e-12)]

_dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))   # noqa: E731
_ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))      # noqa: E731


def _gxx(out, src, extra):
    return subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", f"-I{PKG}/csrc", "-o", out, src] + extra,
                          capture_output=True, text=True)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("ewald_grid_grad") / "libewald_grid_grad.so")
    r = _gxx(so, SRC, ["-fPIC", "-shared"])
    assert r.returncode == 0, r.stderr[-3000:]
    L = C.CDLL(so)
    dp, ip, llp = C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_longlong)
    L.ew_gg_recip_eval.restype = C.c_longlong
    L.ew_gg_recip_eval.argtypes = [C.c_int, ip, dp, dp, dp, dp, C.c_int, ip, dp, dp, C.c_longlong, C.c_longlong, dp]
    L.ew_gg_sizes_eval.restype = None
    L.ew_gg_sizes_eval.argtypes = [C.c_int, ip, ip, llp]
    return L


@pytest.fixture(scope="module")
def lib4(tmp_path_factory):
    """the four-set harness of polar_ewald_field_grid"""
    so = str(tmp_path_factory.mktemp("ewald_grid4") / "libewald_grid.so")
    r = _gxx(so, SRC4, ["-fPIC", "-shared"])
    assert r.returncode == 0, r.stderr[-3000:]
    L = C.CDLL(so)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    L.ew_grid_recip_eval.restype = C.c_longlong
    L.ew_grid_recip_eval.argtypes = [C.c_int, ip, dp, dp, dp, dp, C.c_int, ip, dp, dp, C.c_longlong, C.c_longlong, dp]
    return L


@pytest.fixture(scope="module")
def tables():
    x, q, H = gh._box()
    out = {}
    for g, accuracy in TABLES:
        k, c, n, rows, kv = gh._table(H, g, accuracy)
        S = epn.structure_factors(x, q, k)
        out[(g, accuracy)] = (k, c, n, rows, kv, np.ascontiguousarray(np.stack([S.real, S.imag], axis=1)), S)
    return x, q, H, out


def _recip(lib, H, rows, kv, S2, shape, offset, field=1, chunk=None, lpr=0, fill=0.0):
    n3, off = np.array(shape, np.int32), np.array(offset, np.float64)
    box, cell = gh._geometry(H)
    npts = int(np.prod(shape))
    out = np.full((npts, 9), fill)
    out[:, 3:] = 0.0
    vmax = lib.ew_gg_recip_eval(field, _ip(n3), _dp(off), _dp(LO), _dp(box), _dp(cell), len(rows) - 1, _ip(rows), _dp(kv), _dp(S2),
                                chunk or npts, lpr, _dp(out))
    return out, vmax


@pytest.fixture(scope="module")
def one_pass(lib, tables):
    """(table, grid) -> the nine sums of one pass, computed once for the tests below"""
    x, q, H, tabs = tables
    out = {}
    for key in TABLES:
        k, c, n, rows, kv, S2, S = tabs[key]
        for shape, offset in GRIDS:
            out[(key, shape)] = _recip(lib, H, rows, kv, S2, shape, offset)
    return out


@pytest.mark.parametrize("shape,offset", GRIDS, ids=IDS)
@pytest.mark.parametrize("g,accuracy", TABLES, ids=["hundreds", "ten_thousands"])
def test_three_stage_gradient_sums_against_the_numpy_reciprocal_sums(tables, one_pass, g, accuracy, shape, offset):
    x, q, H, tabs = tables
    k, c, n, rows, kv, S2, S = tabs[(g, accuracy)]
    assert len(k) == (917 if accuracy == 1e-6 else 16926), len(k)
    pts = gh._grid_points(shape, offset, H)
    g_ref, scale_ab, scale = egn.recip_grad_sums(pts, x, q, H, g, accuracy)
    e_ref, _, scale_e = epn.recip_sums(pts, x, q, H, g, accuracy)
    out, vmax = one_pass[((g, accuracy), shape)]
    err = np.max(np.abs(out[:, 3:] - g_ref)) / scale
    err_ab = np.max(np.max(np.abs(out[:, 3:] - g_ref), axis=0) / scale_ab)
    err_e = np.max(np.abs(out[:, :3] - e_ref)) / scale_e
    print("nk %d rows %d grid %s offset %s: gradient %.2e of sum c |k|^2 |S| (per component %.2e of sum c |k_a k_b| |S|), field %.2e of sum c |k| |S|"
          % (len(k), len(rows) - 1, shape, offset, err, err_ab, err_e))
    assert err <= 1e-12 and err_e <= 1e-12
    assert vmax <= 64 << 20


@pytest.mark.parametrize("shape,offset", GRIDS, ids=IDS)
@pytest.mark.parametrize("g,accuracy", TABLES, ids=["hundreds", "ten_thousands"])
def test_the_field_sets_have_the_bits_of_the_four_set_stages(lib4, tables, one_pass, g, accuracy, shape, offset):
    x, q, H, tabs = tables
    k, c, n, rows, kv, S2, S = tabs[(g, accuracy)]
    out, _ = one_pass[((g, accuracy), shape)]
    n3, off = np.array(shape, np.int32), np.array(offset, np.float64)
    box, cell = gh._geometry(H)
    for phi in (0, 1):
        f4 = np.zeros((len(out), 4))
        lib4.ew_grid_recip_eval(phi, _ip(n3), _dp(off), _dp(LO), _dp(box), _dp(cell), len(rows) - 1, _ip(rows), _dp(kv), _dp(S2), len(out), 0, _dp(f4))
        assert np.array_equal(f4[:, :3], out[:, :3]), phi


@pytest.mark.parametrize("shape,offset", GRIDS, ids=IDS)
@pytest.mark.parametrize("g,accuracy", TABLES, ids=["hundreds", "ten_thousands"])
def test_passes_and_line_runs_of_any_size_and_the_field_switch_leave_the_bits(lib, tables, one_pass, g, accuracy, shape, offset):
    x, q, H, tabs = tables
    k, c, n, rows, kv, S2, S = tabs[(g, accuracy)]
    out, _ = one_pass[((g, accuracy), shape)]
    for chunk, lpr in ((37, 1), (5, 2), (1, 0)):
        part, _ = _recip(lib, H, rows, kv, S2, shape, offset, chunk=chunk, lpr=lpr)
        assert np.array_equal(part, out), (chunk, lpr)
    nof, _ = _recip(lib, H, rows, kv, S2, shape, offset, field=0, chunk=37, lpr=2, fill=7.0)
    assert np.array_equal(nof[:, 3:], out[:, 3:]) and np.all(nof[:, :3] == 7.0)


@pytest.mark.parametrize("shape,offset", GRIDS, ids=IDS)
@pytest.mark.parametrize("g,accuracy", TABLES, ids=["hundreds", "ten_thousands"])
def test_trace_against_the_direct_sum_pins_the_component_order(tables, one_pass, g, accuracy, shape, offset):
    x, q, H, tabs = tables
    k, c, n, rows, kv, S2, S = tabs[(g, accuracy)]
    out, _ = one_pass[((g, accuracy), shape)]
    pts = gh._grid_points(shape, offset, H)
    w = c * np.sum(k * k, axis=1)
    trace = np.real(np.exp(1j * (pts @ k.T)) * np.conj(S)[None, :]) @ w
    scale = float(np.sum(w * np.abs(S)))
    err = np.max(np.abs(out[:, 3] + out[:, 4] + out[:, 5] - trace)) / scale
    print("nk %d grid %s: trace %.2e of sum c |k|^2 |S|" % (len(k), shape, err))
    assert err <= 1e-12
    assert np.max(np.abs(trace)) > 1e3 * 1e-12 * scale          # (the trace is not small: a wrong sign or a wrong diagonal would show)
    # the off-diagonal sets, one by one: xy, xz, yz each against its own direct sum
    for col, (a, b) in ((6, (0, 1)), (7, (0, 2)), (8, (1, 2))):
        ref = np.real(np.exp(1j * (pts @ k.T)) * np.conj(S)[None, :]) @ (c * k[:, a] * k[:, b])
        assert np.max(np.abs(out[:, col] - ref)) <= 1e-12 * scale, col


@pytest.mark.parametrize("g,accuracy", TABLES, ids=["hundreds", "ten_thousands"])
def test_layout_sizes_with_nine_sets(lib, tables, g, accuracy):
    _, _, H, tabs = tables
    k, c, n, rows, kv, S2, S = tabs[(g, accuracy)]
    nrow = len(rows) - 1
    hmax = int(n[:, 0].max())
    for shape in ((8, 6, 4), (64, 64, 64), (3, 1, 130)):
        sizes = np.zeros(5, np.int64)
        lib.ew_gg_sizes_eval(nrow, _ip(rows), _ip(np.array(shape, np.int32)), sizes.ctypes.data_as(C.POINTER(C.c_longlong)))
        sets, t, v_line, lpr, hm = (int(v) for v in sizes)
        assert sets == 9 and hm == hmax
        assert t * 16 == nrow * shape[2] * 144            # T: 144 bytes per (row, g_z)
        assert v_line == (hmax + 1) * 144                  # V: 144 bytes per (h, line)
        assert lpr == max(1, (64 << 20) // v_line) and lpr * v_line <= 64 << 20


def test_the_same_code_as_a_program_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    exe = str(tmp_path / "ewald_grid_grad_san")
    r = _gxx(exe, SRC, ["-DEWALD_GRID_GRAD_MAIN", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout.strip())
    assert r.returncode == 0, (r.returncode, r.stdout[-1000:], r.stderr[-3000:])
    m = re.match(r"grids 5 k-vectors 77 rows 18 checks (\d+) failures (\d+)", r.stdout)
    assert m and int(m.group(1)) == 1116 and int(m.group(2)) == 0, r.stdout


def test_the_package_binds_the_entry_point_and_has_the_compositions(pkg):
    assert "polar_ewald_field_grad_grid" in pkg.EXPORTS
    assert hasattr(pkg.lib(), "polar_ewald_field_grad_grid")
    hdr = open(os.path.join(ROOT, "include", "polar_mi355x.h")).read()
    assert re.search(r"\bint polar_ewald_field_grad_grid\s*\(", hdr)
    assert callable(pkg.PolarPair.ewald_probe_grid) and callable(pkg.PolarPair.ewald_probe_force_grid)

    class NoLibrary:
        def __getattr__(self, name):
            raise AssertionError("the library was called: " + name)

    p = pkg.PolarPair.__new__(pkg.PolarPair)
    p.L, p.h = NoLibrary(), None
    with pytest.raises(ValueError):
        p.ewald_field_grad_grid((4, 4, 4), recip="mesh")
