"""Distance classes of the symmetrised LJ/Coulomb rows (csrc/polar_skin.hpp) on the host.

The header is plain C++ and is the text the kernels compile: g++ builds tests/skin/skin_host.cpp around it, a stand-alone
program (with the address and undefined-behaviour sanitizers where the toolchain has them).  For d_max in {0, 0.01, 0.3, 1.0,
1.2, 3.0} A it draws 10^5 triples (r0, displacement of i, displacement of j), half of them with both atoms moving straight
towards each other by the whole d_max, and checks that no pair whose new distance is below r_cmax lies outside the walked
classes -- without exception --, that d_max = 0 walks class 0 alone, that a drift beyond the last shell walks every class,
and the classes and walks exactly on the class bounds and at r0 = r_cmax.  Nothing is loaded into Python, no GPU is needed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "lammps-induced-dipole-polarization-pair-style_amd")
SRC = os.path.join(ROOT, "tests", "skin", "skin_host.cpp")


@pytest.fixture(scope="module")
def skin_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("skin") / "skin_host")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", f"-I{PKG}/csrc", "-o", exe, SRC]
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    built = "with -fsanitize=address,undefined"
    if r.returncode != 0 and "sanitize" in r.stderr:      # a toolchain without the sanitizer runtimes: the plain program
        print("skin_host: the sanitized build failed, building without sanitizers:\n" + r.stderr[-1500:])
        built = "WITHOUT sanitizers"
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    print("skin_host built " + built)
    return exe


# 12.8345: the headline's cut_coul; 2.5: a cutoff of the size of the shells' span; 40: a long one
@pytest.mark.parametrize("r_cmax,seed", [(12.8345, 1), (12.0, 2), (2.5, 3), (40.0, 4)])
def test_no_pair_inside_the_cutoff_is_skipped_and_the_edges_hold(skin_exe, r_cmax, seed):
    p = subprocess.run([skin_exe, repr(r_cmax), str(seed)], capture_output=True, text=True)
    lines = p.stdout.splitlines()
    bad = [ln for ln in lines if ln.startswith("FAIL")]
    assert not bad and p.returncode == 0, (bad[:10], p.stderr[-2000:])
    names = {ln.split()[1] for ln in lines if ln.startswith("ok")}
    # every kind of check really ran
    for want in ("no_pair_inside_cutoff_is_skipped", "dmax0_walks_class0_only", "beyond_last_shell_walks_all", "class_on_bound",
                 "class_at_r_cmax", "bound_reached_is_walked", "bound_not_reached_is_skipped"):
        assert want in names, want
    assert sum(ln.split()[1] == "no_pair_inside_cutoff_is_skipped" for ln in lines) == 6
    # the draws do put pairs inside the cutoff and beyond the walk (the check is not vacuous)
    for ln in lines:
        if ln.startswith("info"):
            t = ln.split()
            assert int(t[6]) > 1000, ln
            if int(t[4]) < 8:
                assert int(t[8]) < 100000, ln
