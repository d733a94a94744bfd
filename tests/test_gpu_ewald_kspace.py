"""The reciprocal-space kernels of `polar_ewald` (csrc/polar_ewald.hpp: k_ew_sfac<false / true>, k_ew_fold, k_ew_field,
k_ew_force, k_ew_kvirial, k_ew_finish) on the MI355X against the long-double reference of tests/ewald_kspace_ref.py.

tests/ewald_kspace_probe/ewald_kspace_probe.hip launches the six kernels as polar_step.hip does, on records filled from
plain arrays, with the plan's tiling or an overridden one.  The boxes are the smallest that reach every branch: the long
axis on x, y and z in turn, power-table indices on the segment seams m = 16, 32 and 48, both branches of ewald_tile (the
48 KB cap bites from nm = 31 on), an l-recurrence of 65 steps (z32), a cubic table of 16,940 vectors, and no k-vector at all.

Every figure is "of scale": |got - reference| over the sum of the absolute values of the reference's terms (the reference
returns it beside each value).  Bound: 1e-12 of scale for every output, the ledger's figure for ew_point_rows, which is the
same construction.  Expected: a cmul step of a recurrence adds about 3 eps at |p| = 1, sincospi a few ulp; 3 x 97 x eps =
3e-14 for the longest row (97 entries, in y48), about 150 eps for a product of three table entries.

Measured on the MI355X, the worst over every run below: S 4.1e-15, M 3.4e-15 (x33), erec 1.7e-15 (z17, 513 atoms),
f 1.6e-15 (z31), u_ef 4.1e-17, virial 1.7e-16 (y48); k-vectors within 1.1 ulp, c_k within 1.7 ulp (the ledger of DESIGN
section 4 has the rows).

tests/ewald_kspace_load.py builds the probe (and says how to point it at a deliberately broken copy of csrc)."""
import os

import numpy as np
import pytest

import ewald_kspace_load as kl
import ewald_kspace_ref as kr

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not kr.available(), reason="np.longdouble has no 64-bit mantissa here")]

E2S = kl.E2S
TOL = 1e-12
EPS = float(np.finfo(np.float64).eps)

CASES, AXIS_BOUNDS = kl.CASES, kl.AXIS_BOUNDS
OUTPUTS = ("S", "M", "erec", "f", "out")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b, keys=OUTPUTS):
    for k in keys:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k


def _system(case, n=70, seed=11):
    """n atoms, seeded: q ~ N(0, 0.4) not neutralised, 30 % without a dipole, a third of those without a charge either,
    fractional coordinates uniform in [-0.5, 1.5] (atoms outside the cell included), a random ef_s"""
    prd, tilt, g, acc = CASES[case][:4]
    rng = np.random.default_rng(seed)
    q, mu = rng.normal(0, 0.4, n), rng.normal(0, 0.3, (n, 3))
    u = rng.uniform(size=n)
    if n > 1:
        mu[u < 0.3] = 0.0
        q[u < 0.1] = 0.0
    H = np.array([[prd[0], tilt[0], tilt[1]], [0.0, prd[1], tilt[2]], [0.0, 0.0, prd[2]]])
    x = rng.uniform(-0.5, 1.5, (n, 3)) @ H.T
    return dict(case=case, prd=prd, tilt=tilt, g=g, acc=acc, n=n, x=np.ascontiguousarray(x), q=q, mu=mu, ef_s=rng.normal(0, 1.0, (n, 3)))


@pytest.fixture(scope="module")
def probe(pkg, tmp_path_factory):
    if not os.path.exists(pkg.HIPCC):
        pytest.skip("hipcc not available")
    return kl.load(pkg, tmp_path_factory.mktemp("ewald_kspace_probe"))


@pytest.fixture(scope="module")
def bench(probe):
    """Systems, probe runs with the default arguments and references, each made once and shared by the tests below."""
    systems, runs, refs = {}, {}, {}

    class Bench:
        @staticmethod
        def system(case, n=70):
            if (case, n) not in systems:
                systems[case, n] = _system(case, n)
            return systems[case, n]

        @staticmethod
        def run(case, n=70, tile=0, chunk=0):
            key = (case, n, tile, chunk)
            if key not in runs:
                runs[key] = probe.run(Bench.system(case, n), tile=tile, chunk=chunk)
            return runs[key]

        @staticmethod
        def ref(sysd, out):
            """the reference of a system, from the table as the probe returned it; cached for the shared systems"""
            key = (sysd["case"], sysd["n"])
            shared = systems.get(key) is sysd
            if shared and key in refs:
                return refs[key]
            r = kr.reference(sysd["prd"], sysd["tilt"], sysd["g"], E2S, sysd["x"], sysd["q"], sysd["mu"], sysd["ef_s"], out["hkl"], out["kv"])
            if shared:
                refs[key] = r
            return r
    return Bench


def _of_scale(diff, scale):
    """max |diff| / scale; where the scale is zero (no term at all) the difference has to be zero"""
    diff, scale = np.abs(np.asarray(diff, dtype=kr.LD)), np.broadcast_to(np.asarray(scale, dtype=kr.LD), np.shape(diff))
    assert np.all(np.isfinite(diff))
    zero = scale == 0
    assert not np.any(diff[zero]), "an output without a single term is not zero"
    return float(np.max(diff[~zero] / scale[~zero])) if np.any(~zero) else 0.0


def _errors(out, ref, f_slack=0.0):
    """every output of a probe run against the reference, of scale; f is compared as f - f0"""
    w, ws = ref["w_atom"] + ref["w_k"], ref["w_atom_scale"] + ref["w_k_scale"]
    df = np.abs((out["f"].astype(kr.LD) - out["f0"].astype(kr.LD)) - ref["f"])
    if np.ndim(f_slack) or f_slack:
        df = np.maximum(df - f_slack, 0)
    return dict(S=_of_scale(out["S"] - ref["S"], ref["S_scale"]), M=_of_scale(out["M"] - ref["M"], ref["M_scale"][:, None]),
                erec=_of_scale(out["erec"] - ref["erec"], ref["erec_scale"]), f=_of_scale(df, ref["f_scale"][:, None]),
                u_ef=_of_scale(out["out"][0] - ref["u_ef"], ref["u_ef_scale"]), virial=_of_scale(out["out"][1:7] - w, ws))


WORST = {}     # quantity -> (figure, label): the worst of every comparison of this module, printed when it is through


@pytest.fixture(scope="module", autouse=True)
def worst_figures():
    yield
    for k, (v, label) in WORST.items():
        print("\nworst %-6s %.2e of scale (%s)" % (k, v, label), end="")
    print()


def _check(label, out, ref, **kw):
    err = _errors(out, ref, **kw)
    print("%-28s of scale: " % label + "  ".join("%s %.2e" % kv for kv in err.items()))
    for k, v in err.items():
        if v > WORST.get(k, (-1.0, ""))[0]:
            WORST[k] = (v, label)
    for k, v in err.items():
        assert v <= TOL, (label, k, v)
    return err


# ---- the cases are the ones meant -------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(CASES))
def test_plan_and_table(case, probe, bench):
    """nm, nk and the tile of the plan are the figures the cases were chosen for (a drift of polar_plan.hpp or of a box is
    noticed here, not by a branch silently no longer taken); the table is 2 pi hkl H^-1 and c_k's formula to 4 ulp."""
    prd, tilt, g, acc, nm, nk, tile = CASES[case]
    pl = probe.plan(prd, tilt, g, acc, 70)
    assert (pl["nm"], pl["nk"]) == (nm, nk)
    out = bench.run(case)
    assert len(out["kv"]) == nk and out["rows"][-1].tolist() == [0, 0, 0, nk]
    if tile is None:
        return
    assert pl["tile"] == tile
    assert tuple(np.abs(out["hkl"][:, :3]).max(0)) == AXIS_BOUNDS[case]
    dk, dc = kr.kvectors_check(prd, tilt, g, out["hkl"], out["kv"])
    print("%s: k-vectors %.2f ulp of the sum of their terms, c_k %.2f ulp" % (case, dk, dc))
    assert dk <= 4.0 and dc <= 4.0


# ---- accuracy -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tiling", ["plan", "tile7_chunk17"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_accuracy(case, tiling, bench):
    """S, M, erec, f, u_ef and the six virial sums within 1e-12 of scale, at the plan's tiling and with tiles of 7, 7 and 3
    atoms in chunks of 17 (70 atoms: a last chunk of 2)."""
    tile, chunk = (0, 0) if tiling == "plan" else (7, 17)
    out = bench.run(case, tile=tile, chunk=chunk)
    _check("%s %s" % (case, tiling), out, bench.ref(bench.system(case), out))


@pytest.mark.parametrize("case", ["z17", "y48", "tilted"])
def test_tile_size_does_not_touch_the_bits(case, bench):
    """One chunking (24 atoms), tiles of 1, 2, 7, 24 atoms and the plan's: every output bit for bit the same.  The tile only
    decides how many atoms' power tables sit in LDS at once; a stale or half-filled table cannot survive this."""
    base = bench.run(case, tile=0, chunk=24)
    for tile in (1, 2, 7, 24):
        _same_bits(bench.run(case, tile=tile, chunk=24), base)


@pytest.mark.parametrize("case", ["z17", "y48", "tilted"])
def test_chunking(case, probe, bench):
    """chunks of 1, 17 and 70 atoms: each within the bound (the fold adds the partials in chunk order, so the bits may differ
    between chunkings); the same chunking twice gives the same S bit for bit (no atomics anywhere)."""
    for chunk in (1, 17, 70):
        out = bench.run(case, tile=0, chunk=chunk)
        _check("%s chunk %d" % (case, chunk), out, bench.ref(bench.system(case), out))
        again = probe.run(bench.system(case), tile=0, chunk=chunk)
        _same_bits(again, out)


# ---- what an atom without charge and dipole may and may not do ----------------------------------------------------------
@pytest.mark.parametrize("case", ["z17", "tilted"])
def test_atoms_without_weight(case, probe, bench):
    """40 more atoms with q = 0 and mu = 0 behind the 70, same chunk and tile: S and M keep their bits, the f rows of the 70
    too; the new atoms' f rows keep the bits of f0 (k_ew_force skips them), and their erec rows are written all the same."""
    s = bench.system(case)
    n, m = s["n"], 40
    rng = np.random.default_rng(5)
    f0 = rng.normal(0, 3.0, (n + m, 3))
    prd, tilt = CASES[case][:2]
    H = np.array([[prd[0], tilt[0], tilt[1]], [0.0, prd[1], tilt[2]], [0.0, 0.0, prd[2]]])
    big = dict(s, n=n + m, x=np.vstack([s["x"], rng.uniform(-0.5, 1.5, (m, 3)) @ H.T]), q=np.concatenate([s["q"], np.zeros(m)]),
               mu=np.vstack([s["mu"], np.zeros((m, 3))]), ef_s=np.vstack([s["ef_s"], rng.normal(0, 1.0, (m, 3))]))
    a = probe.run(s, tile=7, chunk=24, f0=f0[:n])
    b = probe.run(big, tile=7, chunk=24, f0=f0)
    _same_bits(a, b, keys=("S", "M"))
    assert np.array_equal(_bits(b["f"][:n]), _bits(a["f"]))
    assert np.array_equal(_bits(b["f"][n:]), _bits(f0[n:]))
    assert np.array_equal(_bits(b["erec"][:n]), _bits(a["erec"]))
    ref = bench.ref(big, b)
    assert np.any(ref["erec"][n:] != 0)
    _check("%s + 40 weightless atoms" % case, b, ref, f_slack=EPS * np.abs(f0))


def test_perm_and_accumulation(probe, bench):
    """f goes to row perm[i] with the bits of the unpermuted row i, and is added to what f held: f - f0 within the bound plus
    the rounding of the one addition, eps |f0|."""
    s = bench.system("z17")
    base = bench.run("z17")
    rng = np.random.default_rng(3)
    perm = rng.permutation(s["n"])
    assert np.any(perm != np.arange(s["n"]))
    out = probe.run(s, perm=perm)
    assert np.array_equal(_bits(out["f"][perm]), _bits(base["f"]))
    _same_bits(out, base, keys=("S", "M", "erec", "out"))
    f0 = rng.normal(0, 50.0, (s["n"], 3))
    acc = probe.run(s, f0=f0)
    assert np.abs(f0).min() > 0 and np.abs(f0).max() > 10 * np.abs(base["f"]).max()
    _check("z17 f0 random", acc, bench.ref(s, acc), f_slack=EPS * np.abs(f0))


def test_cur_selects_the_dipoles(probe, bench):
    """Scal.cur picks the records M, f and out take their dipoles from: NaN dipoles in the other records leave no trace.
    S and erec never read a dipole."""
    s = bench.system("z17")
    base = bench.run("z17")
    nan = np.full((s["n"], 3), np.nan)
    for cur, kw in ((1, dict(muA=nan)), (0, dict(muB=nan))):
        out = probe.run(s, cur=cur, **kw)
        for k in OUTPUTS:
            assert np.all(np.isfinite(out[k])), (cur, k)
        _same_bits(out, base)
    both = probe.run(s, cur=0, muA=nan)                 # (and the test can see a NaN: the records in use do reach M, f, out)
    assert np.all(np.isnan(both["M"])) and np.any(np.isnan(both["f"])) and np.isnan(both["out"][0])
    _same_bits(both, base, keys=("S", "erec"))


# ---- edges --------------------------------------------------------------------------------------------------------------
def test_one_atom_and_no_atom(probe, bench):
    out = bench.run("z17", n=1)
    s1 = bench.system("z17", n=1)
    assert s1["q"][0] != 0 and np.all(s1["mu"] != 0)
    _check("z17 n = 1", out, bench.ref(s1, out))
    none = bench.run("z17", n=0)
    assert none["erec"].shape == none["f"].shape == (0, 3)
    for k in ("S", "M", "out"):
        assert not np.any(none[k]), k


def test_no_kvector(probe, bench):
    """accuracy 0.9 leaves no k-vector: erec = 0, f = f0 bit for bit, no virial, u_ef = -sum mu . ef_s"""
    s = bench.system("none")
    f0 = np.random.default_rng(9).normal(0, 3.0, (s["n"], 3))
    out = probe.run(s, f0=f0)
    assert out["plan"]["nk"] == 0 and out["S"].shape == (0, 2)
    assert not np.any(out["erec"]) and not np.any(out["out"][1:7])
    assert np.array_equal(_bits(out["f"]), _bits(f0))
    _check("none", out, bench.ref(s, out))
    empty = probe.run(bench.system("none", n=0))
    assert not np.any(empty["out"])


@pytest.mark.parametrize("n", [257, 513])
def test_more_than_one_workgroup_of_atoms(n, bench):
    """257 and 513 atoms: two and three workgroups of k_ew_force and k_ew_field, the last with a single atom, their partials
    through k_ew_finish; 9 and 17 chunks of whole tiles in k_ew_sfac"""
    out = bench.run("z17", n=n)
    assert out["plan"]["nchunk"] > 1 and out["plan"]["chunk"] <= out["plan"]["tile"]
    _check("z17 n = %d" % n, out, bench.ref(bench.system("z17", n), out))
