"""Register / scratch budgets of the point kernels -- k_field_at (csrc/polar_field_at.hpp), k_field_grad_at
(csrc/polar_field_grad_at.hpp), k_probe_lj (csrc/polar_probe_at.hpp), k_ew_point_real / k_ew_point_recip
(csrc/polar_ewald_field_at.hpp) and the kernels of csrc/polar_ewald_field_grid.hpp -- read from hipcc's resource remarks
(cross-compiles for gfx950 without a GPU).  polar_step.hip holds the launchers, hence every kernel's instances: it is compiled
once per build flavour, product and lab, and each family's test reads its kernels out of that one compile.  The kernels share
their walk (csrc/polar_point_walk.hpp); what each parks in vector registers is its own, and these tests are what notices when a
compiler, or a change to the shared walk, decides otherwise."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lammps-induced-dipole-polarization-pair-style_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FIELDS = ("VGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill")
# k_field_at<ALLPAIRS, DAMP, PHI>: the VGPR column of the table of DESIGN section 6d
FIELD_AT_VGPRS = {"Lb1ELi0ELb1E": 62, "Lb1ELi0ELb0E": 62, "Lb1ELi1ELb1E": 58, "Lb1ELi1ELb0E": 52,
                  "Lb0ELi0ELb1E": 94, "Lb0ELi0ELb0E": 92, "Lb0ELi1ELb1E": 64, "Lb0ELi1ELb0E": 58}
GRID_KERNELS = {"k_ew_grid_points": 1, "k_ew_grid_tab": 1, "k_ew_grid_l": 1, "k_ew_grid_k": 1, "k_ew_grid_hI": 2}
# (ALLPAIRS, PHI) -> vector registers of k_ew_point_real, either damping type; PHI -> those of k_ew_point_recip
POINT_REAL = {("1", "1"): 156, ("1", "0"): 152, ("0", "1"): 186, ("0", "0"): 182}
POINT_RECIP = {"1": 59, "0": 57}


@pytest.fixture(scope="module", params=[[], ["-DPOLAR_LAB"]], ids=["product", "lab"])
def remarks(request, tmp_path_factory):
    """kernel name -> {remark: value} of every kernel of polar_step.hip"""
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
        pytest.skip("hipcc not available")
    obj = tmp_path_factory.mktemp("point_resources") / "step.o"
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-function", "--cuda-device-only", "-c",
                        "-o", str(obj), os.path.join(CSRC, "polar_step.hip"), "-Rpass-analysis=kernel-resource-usage"] + request.param,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    res, cur = {}, None
    for ln in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            cur = res.setdefault(m.group(1), {})
        m = re.search(r"remark:.*\s(VGPRs|SGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|SGPRs Spill|VGPRs Spill|LDS Size \[bytes/block\]): (\d+)", ln)
        if m and cur is not None:
            cur[m.group(1)] = int(m.group(2))
    return res


def _family(remarks, mark):
    return {k: v for k, v in remarks.items() if mark in k}


def _no_scratch_no_spill(k, v):
    assert all(f in v for f in FIELDS), (k, v)
    assert v["ScratchSize [bytes/lane]"] == 0 and v["SGPRs Spill"] == 0 and v["VGPRs Spill"] == 0, (k, v)


def _four_waves(res):
    for k, v in sorted(res.items()):
        print(k[:48], v)
        _no_scratch_no_spill(k, v)
        assert v["VGPRs"] <= 128, (k, v)
        assert v["Occupancy [waves/SIMD]"] >= 4, (k, v)


def test_every_instance_of_k_field_at_keeps_its_budget(remarks):
    """Every instance -- exact / list mode x damping type x with / without the potentials -- stays within 128 vector registers
    (four waves per SIMD at least), uses no scratch and spills no register, vector or scalar.  The list-mode instances hold more
    wave-uniform state than a wave has scalar registers; the kernel parks part of it in vector registers on purpose (in_vgpr).
    The eight instances have the vector register counts of the table of DESIGN section 6d."""
    res = _family(remarks, "k_field_atI")
    assert len(res) == 8, sorted(res)          # ALLPAIRS x DAMP x PHI
    _four_waves(res)
    for k, v in sorted(res.items()):
        inst = re.search(r"k_field_atI((?:L[bi]\dE){3})", k).group(1)
        assert v["VGPRs"] == FIELD_AT_VGPRS[inst], (inst, v)


def test_every_instance_of_k_field_grad_at_keeps_its_budget(remarks):
    """Each of the four instances -- exact / list mode x damping type -- stays within 128 vector registers (four waves per SIMD
    at least), uses no scratch and spills no register, vector or scalar.  The damped list-mode instance carries 18 sums on top
    of k_field_at's wave-uniform state and is the tight one (122 registers); it parks the table pointers in vector registers as
    well, without which two scalar registers are spilled."""
    res = _family(remarks, "k_field_grad_atI")
    assert len(res) == 4, sorted(res)          # ALLPAIRS x DAMP
    _four_waves(res)


def test_every_instance_of_k_probe_lj_keeps_its_budget(remarks):
    """Every instance -- exact / list mode x with / without the force -- stays within 128 vector registers (four waves per SIMD
    at least), uses no scratch and spills no register, vector or scalar.  The undamped k_field_at instances with a comparable
    walk sit at 52-64 vector registers; this kernel carries less state."""
    res = _family(remarks, "k_probe_ljI")
    assert len(res) == 4, sorted(res)          # ALLPAIRS x FORCE
    _four_waves(res)


def test_every_kernel_of_ewald_field_at_keeps_its_budget(remarks):
    """k_ew_point_real, eight instances (exact / list mode x damping type x with / without the potentials): no scratch, no
    spilled register, vector or scalar, and at most 256 vector registers -- two waves per SIMD.  erfc, erf and the Gaussian per
    pair are register-heavy (k_ew_static_field of the step needs 158): the compiler keeps the four exact-mode instances, damped
    and undamped, within 168 (152 / 156: three waves per SIMD), which is asserted for all four, and takes 182 to 186 in list
    mode (DESIGN section 6e has the table), where it does not allow 168 and 256 is asserted.  The list-mode instances park
    wave-uniform state in vector registers on purpose (in_vgpr), list the stencil's runs in LDS before the pair loops and walk
    the records once for the induced and once for the static sums.
    k_ew_point_recip, two instances: at most 64 vector registers (eight waves per SIMD), no scratch, no spill."""
    res = _family(remarks, "k_ew_point_")
    real, recip = _family(res, "k_ew_point_realI"), _family(res, "k_ew_point_recipI")
    assert len(real) == 8, sorted(res)          # ALLPAIRS x DAMP x PHI
    assert len(recip) == 2, sorted(res)         # PHI
    for k, v in sorted(res.items()):
        print(k[:56], v)
        _no_scratch_no_spill(k, v)
    for k, v in real.items():
        exact = "k_ew_point_realILb1E" in k          # ALLPAIRS
        assert v["VGPRs"] <= (168 if exact else 256), (k, v)
        assert v["Occupancy [waves/SIMD]"] >= (3 if exact else 2), (k, v)
    assert sum("k_ew_point_realILb1E" in k for k in real) == 4
    for k, v in recip.items():
        assert v["VGPRs"] <= 64 and v["Occupancy [waves/SIMD]"] >= 8, (k, v)


def test_every_kernel_of_ewald_field_grid_keeps_its_budget(remarks):
    """k_ew_grid_points, k_ew_grid_tab, k_ew_grid_l, k_ew_grid_k and the two instances of k_ew_grid_h (with / without the
    potential): no scratch, no spilled register, vector or scalar, no LDS, and at most 64 vector registers -- eight waves per
    SIMD, the cap asserted for k_ew_point_recip: these are streaming kernels whose loads are hidden by the waves in flight.
    hipcc reports 18 to 30 (DESIGN section 6f has the table).
    The grid call launches the k_ew_point_real instances: their vector-register counts, and k_ew_point_recip's, are the ones
    DESIGN section 6e records."""
    grid = _family(remarks, "k_ew_grid_")
    for name, count in GRID_KERNELS.items():
        assert sum(name in k for k in grid) == count, (name, sorted(grid))
    assert len(grid) == sum(GRID_KERNELS.values()), sorted(grid)
    for k, v in sorted(grid.items()):
        print(k[:40], v)
        _no_scratch_no_spill(k, v)
        assert "LDS Size [bytes/block]" in v and v["LDS Size [bytes/block]"] == 0, (k, v)
        assert v["VGPRs"] <= 64 and v["Occupancy [waves/SIMD]"] >= 8, (k, v)
    # the per-point kernels beside them: as recorded
    real, recip = _family(remarks, "k_ew_point_realI"), _family(remarks, "k_ew_point_recipI")
    assert len(real) == 8 and len(recip) == 2, sorted(real) + sorted(recip)
    for k, v in sorted(real.items()):
        m = re.search(r"k_ew_point_realILb([01])ELi[01]ELb([01])E", k)
        assert m and v["VGPRs"] == POINT_REAL[(m.group(1), m.group(2))], (k, v)
        _no_scratch_no_spill(k, v)
    for k, v in sorted(recip.items()):
        m = re.search(r"k_ew_point_recipILb([01])E", k)
        assert m and v["VGPRs"] == POINT_RECIP[m.group(1)], (k, v)
