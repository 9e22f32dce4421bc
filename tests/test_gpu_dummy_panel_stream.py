"""The 8-pivot stream of the joint panel column that ends in dummy unknowns (panel8x1_dpp, tools/gen_panel_asm.py
JOINT_DUMMY_PIVOTS) leaves L and 1 / L_jj as the 16-pivot stream does: tools/microbench/dummy_panel_probe.hip factors the
same panel, with the dummy structure, with both."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "paper_gorbani_2025_humanoids_multi-rate-mpc-ironcub_amd"


@pytest.mark.gpu
def test_dummy_panel_stream_matches_the_sixteen_pivot_stream(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "dummy_panel_probe")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-I", os.path.join(ROOT, PKG, "csrc"), "-o", exe,
                    os.path.join(ROOT, "tools", "microbench", "dummy_panel_probe.hip")], check=True, capture_output=True, text=True)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "equal to the 16-pivot stream" in res.stdout, res.stdout
