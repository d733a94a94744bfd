"""Register / scratch budget of k_field_at (csrc/polar_field_at.hpp), read from hipcc's resource remarks (cross-compiles for
gfx950 without a GPU): every instance -- exact / list mode x damping type x with / without the potentials -- stays within 128
vector registers (four waves per SIMD at least), uses no scratch and spills no register, vector or scalar.  The list-mode
instances hold more wave-uniform state than a wave has scalar registers; the kernel parks part of it in vector registers
on purpose (in_vgpr), and this test is what notices when a compiler decides otherwise."""
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
def test_every_instance_of_k_field_at_keeps_its_budget(flags, tmp_path):
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
        pytest.skip("hipcc not available")
    # polar_step.hip holds the launcher (field_at_pass), hence the kernel's instances
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-function", "--cuda-device-only", "-c",
                        "-o", str(tmp_path / "step.o"), os.path.join(CSRC, "polar_step.hip"), "-Rpass-analysis=kernel-resource-usage"] + flags,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    res, cur = {}, None
    for ln in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            cur = res.setdefault(m.group(1), {}) if "k_field_atI" in m.group(1) else None
        m = re.search(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|SGPRs Spill|VGPRs Spill): (\d+)", ln)
        if m and cur is not None:
            cur[m.group(1)] = int(m.group(2))
    assert len(res) == 8, sorted(res)          # ALLPAIRS x DAMP x PHI
    for k, v in sorted(res.items()):
        print(k[:48], v)
        assert all(f in v for f in FIELDS), (k, v)
        assert v["VGPRs"] <= 128, (k, v)
        assert v["ScratchSize [bytes/lane]"] == 0 and v["SGPRs Spill"] == 0 and v["VGPRs Spill"] == 0, (k, v)
        assert v["Occupancy [waves/SIMD]"] >= 4, (k, v)
