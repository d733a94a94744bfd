"""LJ/Coulomb rows of the symmetrised list walked by distance class (csrc/polar_skin.hpp, k_sym_count / k_sym_fill / k_lj_walk):
skin entries the drift since the list's upload keeps outside every cutoff are left out whole, and nothing else changes.

Two child processes (tests/skin/skin_child.py), one with POLAR_LJ_SKIN=1 and one with 0 -- the variable is read when a handle
is created --, drive the 1,349-atom MOF-5 + H2 cell with its handed-over half list (ghosts included) through displacement
fields of largest norm 0, 0.1, 0.5 and 1.5 x skin / 2 (polar_set_positions, ghosts moved with their owners), back to the
start, through polar_set_atoms with no new list and through a list handed over again; both forms of the kernel
(POLAR_LJ_PERS=2 / 0), newton on and off.  A full-list handle and a device_neigh handle ride along.

Tolerances.  Between the two handles the same pairs contribute in another order: E_vdwl, E_coul to 1e-12 relative, forces to
1e-12 of the largest force.  The virial is sum f.x over locals and ghosts (fdotr): an FP64 sum of N = 12,935 terms in any
order is off by at most N 2^-53 sum |f_k x_k| = 1.44e-12 of that sum, two such sums differ by at most twice that: 3e-12 of
sum |f_k x_k| per component.  Against the oracle: the 1e-7 of the golden tests (tests/test_gpu_parity.py)."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import force_rel_err, rel

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CHILD = os.path.join(HERE, "skin", "skin_child.py")
_spec = importlib.util.spec_from_file_location("skin_child", CHILD)
sc = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(sc)

TOL = 1e-7          # against the oracle, as the golden tests
AB = 1e-12          # between the two handles
SHELL, NCLASS, GUARD = 0.25, 8, 1e-12   # csrc/polar_skin.hpp


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """{skin setting: arrays of its child}: both children at once, each a fresh process."""
    d = tmp_path_factory.mktemp("lj_skin")
    procs = {}
    for skin in (1, 0):
        env = dict(os.environ, POLAR_LJ_SKIN=str(skin))
        env.pop("POLAR_LJ_PERS", None)
        out = str(d / f"skin{skin}.npz")
        procs[skin] = (subprocess.Popen([sys.executable, CHILD, out], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True), out)
    res = {}
    try:
        for skin, (p, out) in procs.items():
            log, _ = p.communicate(timeout=600)
            assert p.returncode == 0, (skin, p.returncode, log[-3000:])
            res[skin] = dict(np.load(out))
    finally:   # whatever happened -- a time limit, a failed child -- no child stays behind with the GPU open
        for p, _ in procs.values():
            if p.poll() is None:
                p.kill()
                p.communicate()
    return res


@pytest.fixture(scope="module")
def case(wl, oracle):
    """Per newton setting: the system, r_cmax, the oracle at every displacement, and the pair distances of the entries the
    kernel's rows hold -- computed once, read by every test."""
    cache = {}

    def get(newton):
        if newton in cache:
            return cache[newton]
        s = sc.load(wl, newton)
        n = s.nlocal
        rc = float(np.sqrt(s.tables["cutsq"][1:, 1:].max()))
        i = np.repeat(np.arange(n), s.numneigh)        # rows are stored in atom order (firstneigh ascending with i)
        assert np.array_equal(s.firstneigh, np.concatenate(([0], np.cumsum(s.numneigh)[:-1])))
        j = s.neigh & 0x3FFFFFFF
        # entries of the walked rows per pair of the half list: newton on -- the rows of i and of j (ghost rows too);
        # newton off -- local rows only
        mult = np.full(len(j), 2) if newton else 1 + (j < n).astype(np.int64)
        orc = {sc_: oracle.compute(sc.moved(s, sc_), eflag=1, vflag=2) for sc_ in sc.SCALES}
        cache[newton] = dict(s=s, rc=rc, i=i, j=j, mult=mult, orc=orc, skin=sc.skin_of(s))
        return cache[newton]
    return get


def _r(c, scale):
    x = sc.positions(c["s"], scale)
    d = x[c["i"]] - x[c["j"]]
    return np.sqrt(np.einsum("ij,ij->i", d, d))


def _count_below(c, r, bound):
    return int(np.sum(c["mult"][r < bound]))


def _against_oracle(out_f, out_e, out_vir, ref, s, locals_only=False):
    fr = np.zeros((s.nlocal, 3))
    np.add.at(fr, s.owner, ref["f"])
    if locals_only:
        f = out_f[:s.nlocal]
    else:
        f = np.zeros((s.nlocal, 3))
        np.add.at(f, s.owner, out_f)
    assert force_rel_err(f, fr) < TOL
    for k, name in enumerate(("eng_vdwl", "eng_coul", "eng_pol")):
        assert rel(out_e[k], ref[name], 1e-9) < TOL, name
    assert np.max(np.abs(out_vir - ref["virial"])) < TOL * max(1.0, np.max(np.abs(ref["virial"])))


@pytest.mark.parametrize("newton", [1, 0], ids=["newton_on", "newton_off"])
@pytest.mark.parametrize("pers", sc.PERS, ids=["persistent", "wave_per_row"])
def test_skipped_skin_entries_change_nothing_and_are_really_skipped(pers, newton, runs, case):
    c = case(newton)
    s, rc, half_skin = c["s"], c["rc"], 0.5 * c["skin"]
    total = int(np.sum(c["mult"]))
    for stage, scale in sc.STAGES:
        tag = f"n{newton}_p{pers}_{stage}"
        on, off = ({k: runs[sk][f"{tag}_{k}"] for k in ("f", "e", "virial", "count")} for sk in (1, 0))
        x = sc.positions(s, scale)
        print(tag, "walked/total on", on["count"], "off", off["count"],
              "dE", [rel(on["e"][k], off["e"][k]) for k in (0, 1)], "df", np.max(np.abs(on["f"] - off["f"])) / np.max(np.abs(off["f"])),
              "dvir", np.max(np.abs(on["virial"] - off["virial"])), "of", np.sum(np.abs(off["f"] * x), axis=0))
        # the two handles agree
        assert rel(on["e"][0], off["e"][0]) < AB and rel(on["e"][1], off["e"][1]) < AB
        assert np.max(np.abs(on["f"] - off["f"])) < AB * np.max(np.abs(off["f"]))
        fx = np.abs(off["f"][:, [0, 1, 2, 1, 2, 2]] * x[:, [0, 1, 2, 0, 0, 1]]).sum(axis=0)   # the terms of k_virial_fdotr's six sums
        assert np.all(np.abs(on["virial"] - off["virial"]) < 3 * AB * fx)
        # ... and each agrees with the oracle
        for h in (on, off):
            _against_oracle(h["f"], h["e"], h["virial"], c["orc"][scale], s)
        # the counters
        assert off["count"][1] == total and off["count"][0] == total          # POLAR_LJ_SKIN=0 walks every entry
        assert on["count"][1] == total
        walked = int(on["count"][0])
        # distances when the classes were made: at the upload's positions, for "relist" at the moved ones; drift since then
        r0 = _r(c, 0.1 if stage == "relist" else 0.0)
        drift = 0.0 if stage == "relist" else scale * half_skin
        if stage == "atoms_no_list":
            assert walked == total                                            # per-atom arrays replaced, no new list: the whole rows
            continue
        if scale == 1.5:
            assert walked == total                                            # 2 d_max beyond the last shell: every class
            continue
        if drift == 0.0:
            # exactly class 0 (r0^2 < r_cmax^2 (1 + guard); an entry within a rounding of that bound may fall either way)
            edge = rc * np.sqrt(1.0 + GUARD)
            assert _count_below(c, r0, edge * (1 - 1e-13)) <= walked <= _count_below(c, r0, edge * (1 + 1e-13))
            # the skip really happens: at least half of the entries a whole shell beyond r_cmax are left out
            far = total - _count_below(c, r0, rc + SHELL)
            assert far > 0.1 * total and walked <= total - far / 2
        else:
            # every entry the drift can bring inside is walked; nothing is walked a whole shell beyond that
            assert _count_below(c, r0, rc + 2 * drift - 1e-9) <= walked <= _count_below(c, r0, rc + 2 * drift + SHELL + 1e-6)
            assert walked < total
        # nothing inside the cutoff NOW lies beyond the walk (what makes the skip exact)
        assert _count_below(c, _r(c, scale), rc) <= walked


@pytest.mark.parametrize("pers", sc.PERS, ids=["persistent", "wave_per_row"])
def test_full_list_and_device_built_list_walk_every_entry(pers, runs, case):
    c = case(1)
    s = c["s"]
    for kind in ("full", "devneigh"):
        tag = f"p{pers}_{kind}"
        on, off = ({k: runs[sk][f"{tag}_{k}"] for k in ("f", "e", "virial", "count")} for sk in (1, 0))
        assert np.all(on["f"][s.nlocal:] == 0.0)                # these lists leave no force on ghosts
        for h in (on, off):
            _against_oracle(h["f"], h["e"], h["virial"], c["orc"][0.0], s, locals_only=True)
            assert h["count"][0] == h["count"][1] > 0             # the counter reports the total
        assert np.array_equal(on["count"], off["count"])
        assert rel(on["e"][0], off["e"][0]) < AB and rel(on["e"][1], off["e"][1]) < AB
        assert np.max(np.abs(on["f"] - off["f"])) < AB * np.max(np.abs(off["f"]))
    assert runs[1][f"p{pers}_full_count"][1] == runs[1][f"p{pers}_full_nneigh"][0]
