"""Register / scratch budget of k_probe_lj (csrc/polar_probe_at.hpp), read from hipcc's resource remarks (cross-compiles for
gfx950 without a GPU): every instance -- exact / list mode x with / without the force -- stays within 128 vector registers (four
waves per SIMD at least), uses no scratch and spills no register, vector or scalar, in the product and in the lab build.  The
undamped k_field_at instances with a comparable walk sit at 52-64 vector registers; this kernel carries less state."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lammps-induced-dipole-polarization-pair-style_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FIELDS = ("VGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill")


@pytest.mark.parametrize("flags", [[], ["-DPOLAR_LAB"]], ids=["product", "lab"])
def test_every_instance_of_k_probe_lj_keeps_its_budget(flags, tmp_path):
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
        pytest.skip("hipcc not available")
    # polar_step.hip holds the launcher (probe_at_pass), hence the kernel's instances
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-function", "--cuda-device-only", "-c",
                        "-o", str(tmp_path / "step.o"), os.path.join(CSRC, "polar_step.hip"), "-Rpass-analysis=kernel-resource-usage"] + flags,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    res, cur = {}, None
    for ln in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            cur = res.setdefault(m.group(1), {}) if "k_probe_ljI" in m.group(1) else None
        m = re.search(r"remark:\s+(VGPRs|SGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|SGPRs Spill|VGPRs Spill): (\d+)", ln)
        if m and cur is not None:
            cur[m.group(1)] = int(m.group(2))
    assert len(res) == 4, sorted(res)          # ALLPAIRS x FORCE
    for k, v in sorted(res.items()):
        print(k[:48], v)
        assert all(f in v for f in FIELDS), (k, v)
        assert v["VGPRs"] <= 128, (k, v)
        assert v["ScratchSize [bytes/lane]"] == 0 and v["SGPRs Spill"] == 0 and v["VGPRs Spill"] == 0, (k, v)
        assert v["Occupancy [waves/SIMD]"] >= 4, (k, v)
