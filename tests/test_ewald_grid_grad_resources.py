"""Register / scratch budgets of the kernels of csrc/polar_ewald_field_grad_grid.hpp -- k_ew_gg_l, k_ew_gg_k and the two instances
of k_ew_gg_h -- read from hipcc's resource remarks (cross-compiles for gfx950 without a GPU), in the way of
tests/test_ewald_grad_resources.py: polar_step.hip holds the launchers, hence every instance; it is compiled once per build
flavour, product and lab.  The counts are those of the table of DESIGN section 6j: every kernel inside the 64-register step,
eight waves per SIMD, the cap the k_ew_grid_* kernels meet."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lammps-induced-dipole-polarization-pair-style_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FIELDS = ("VGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill", "LDS Size [bytes/block]")
# kernel -> vector registers.  k_ew_gg_h: FIELD = true (eighteen FMAs per h), FIELD = false (twelve)
VGPRS = {"k_ew_gg_l": 62, "k_ew_gg_k": 44, "k_ew_gg_hILb1E": 32, "k_ew_gg_hILb0E": 26}
CAP, WAVES = 64, 8


@pytest.fixture(scope="module", params=[[], ["-DPOLAR_LAB"]], ids=["product", "lab"])
def remarks(request, tmp_path_factory):
    """kernel name -> {remark: value} of every kernel of polar_step.hip"""
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
        pytest.skip("hipcc not available")
    obj = tmp_path_factory.mktemp("ewald_grid_grad_resources") / "step.o"
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


def test_every_k_ew_gg_kernel_keeps_its_budget(remarks):
    """Four kernels: no scratch, no spilled register, vector or scalar, no LDS; the recorded vector registers, all within 64, and
    eight waves per SIMD.  Stage 3 holds nine sums, one table entry and its addresses in 32 registers; its V column -- nine
    16-byte values per h, two h's in flight -- sits in scalar registers."""
    res = {k: v for k, v in remarks.items() if "k_ew_gg_" in k}
    assert len(res) == 4, sorted(res)
    seen = set()
    for k, v in sorted(res.items()):
        print(k[:44], v)
        assert all(f in v for f in FIELDS), (k, v)
        assert v["ScratchSize [bytes/lane]"] == 0 and v["SGPRs Spill"] == 0 and v["VGPRs Spill"] == 0, (k, v)
        assert v["LDS Size [bytes/block]"] == 0, (k, v)
        (name,) = [n for n in VGPRS if n in k]
        seen.add(name)
        assert v["VGPRs"] == VGPRS[name] and v["VGPRs"] <= CAP and v["Occupancy [waves/SIMD]"] == WAVES, (k, v)
    assert seen == set(VGPRS)


def test_the_new_kernels_stay_out_of_the_existing_counts(remarks):
    """The kernels other resource tests count by name: none of the new ones matches."""
    for k in remarks:
        if "k_ew_gg_" in k:
            assert not any(s in k for s in ("k_ew_grid_", "k_ew_grad_real", "k_ew_grad_recip", "k_ew_grad_fold")), k
