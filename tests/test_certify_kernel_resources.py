"""Resources of certify_kernel (csrc/vsmpc_certify.hip), read from the code object of the current build with
tools/kernel_resources.py: no spilled vector register, no private (scratch) segment, no static LDS beside the dynamic
block the launcher sizes, one 256-thread workgroup."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as kr  # noqa: E402


@pytest.fixture(scope="module")
def kernel(solver_mod):
    ks = kr.all_kernels()
    assert ks, "no code objects under <pkg>/build: build first (python __graft_entry__.py)"
    hit = {k: v for k, v in ks.items() if re.search(r"\bcertify_kernel\(", k)}
    assert len(hit) == 1, list(hit)
    return next(iter(hit.values()))


def test_certify_kernel_does_not_spill(kernel):
    assert kernel["vgpr_spill_count"] == 0, kernel
    assert kernel.get("sgpr_spill_count", 0) == 0, kernel
    assert kernel["private_segment_fixed_size"] == 0, kernel        # no scratch segment at all


def test_certify_kernel_shape(kernel):
    assert kernel["max_flat_workgroup_size"] == 256, kernel
    assert kernel["group_segment_fixed_size"] == 0, kernel          # LDS: the launcher's dynamic block and nothing else
    assert kernel["vgpr_count"] + kernel.get("agpr_count", 0) <= 128, kernel    # at least four wavefronts per SIMD
