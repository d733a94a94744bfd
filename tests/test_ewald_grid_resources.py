"""Register / scratch budget of the kernels of polar_ewald_field_grid (csrc/polar_ewald_field_grid.hpp), read from hipcc's
resource remarks (cross-compiles for gfx950 without a GPU), in the pattern of tests/test_ewald_field_at_resources.py.

k_ew_grid_points, k_ew_grid_tab, k_ew_grid_l, k_ew_grid_k and the two instances of k_ew_grid_h (with / without the potential):
no scratch, no spilled register, vector or scalar, no LDS, and at most 64 vector registers -- eight waves per SIMD, the cap
that file asserts for k_ew_point_recip: these are streaming kernels whose loads are hidden by the waves in flight.  hipcc
reports 18 to 30 (DESIGN section 6f has the table).
The kernels of polar_ewald_field_at sit in the same translation unit and the grid call launches its k_ew_point_real instances:
their vector-register counts are the ones DESIGN section 6e records."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lammps-induced-dipole-polarization-pair-style_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FIELDS = ("VGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill", "LDS Size [bytes/block]")
GRID_KERNELS = {"k_ew_grid_points": 1, "k_ew_grid_tab": 1, "k_ew_grid_l": 1, "k_ew_grid_k": 1, "k_ew_grid_hI": 2}
# (ALLPAIRS, PHI) -> vector registers of k_ew_point_real, either damping type; PHI -> those of k_ew_point_recip
POINT_REAL = {("1", "1"): 156, ("1", "0"): 152, ("0", "1"): 186, ("0", "0"): 182}
POINT_RECIP = {"1": 59, "0": 57}


@pytest.mark.parametrize("flags", [[], ["-DPOLAR_LAB"]], ids=["product", "lab"])
def test_every_kernel_of_ewald_field_grid_keeps_its_budget(flags, tmp_path):
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
        pytest.skip("hipcc not available")
    # polar_step.hip holds the launchers (ewald_field_grid_begin, ewald_field_grid_pass), hence the kernels' instances
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-function", "--cuda-device-only", "-c",
                        "-o", str(tmp_path / "step.o"), os.path.join(CSRC, "polar_step.hip"), "-Rpass-analysis=kernel-resource-usage"] + flags,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    res, cur = {}, None
    for ln in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            cur = res.setdefault(m.group(1), {}) if ("k_ew_grid_" in m.group(1) or "k_ew_point_" in m.group(1)) else None
        m = re.search(r"remark:.*\s(VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|SGPRs Spill|VGPRs Spill|LDS Size \[bytes/block\]): (\d+)", ln)
        if m and cur is not None:
            cur[m.group(1)] = int(m.group(2))
    grid = {k: v for k, v in res.items() if "k_ew_grid_" in k}
    for name, count in GRID_KERNELS.items():
        assert sum(name in k for k in grid) == count, (name, sorted(grid))
    assert len(grid) == sum(GRID_KERNELS.values()), sorted(grid)
    for k, v in sorted(grid.items()):
        print(k[:40], v)
        assert all(f in v for f in FIELDS), (k, v)
        assert v["ScratchSize [bytes/lane]"] == 0 and v["SGPRs Spill"] == 0 and v["VGPRs Spill"] == 0 and v["LDS Size [bytes/block]"] == 0, (k, v)
        assert v["VGPRs"] <= 64 and v["Occupancy [waves/SIMD]"] >= 8, (k, v)
    # the per-point kernels beside them: as recorded
    real = {k: v for k, v in res.items() if "k_ew_point_realI" in k}
    recip = {k: v for k, v in res.items() if "k_ew_point_recipI" in k}
    assert len(real) == 8 and len(recip) == 2, sorted(res)
    for k, v in sorted(real.items()):
        m = re.search(r"k_ew_point_realILb([01])ELi[01]ELb([01])E", k)
        assert m and v["VGPRs"] == POINT_REAL[(m.group(1), m.group(2))], (k, v)
        assert v["ScratchSize [bytes/lane]"] == 0 and v["SGPRs Spill"] == 0 and v["VGPRs Spill"] == 0, (k, v)
    for k, v in sorted(recip.items()):
        m = re.search(r"k_ew_point_recipILb([01])E", k)
        assert m and v["VGPRs"] == POINT_RECIP[m.group(1)], (k, v)
