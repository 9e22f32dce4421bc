"""Resources of the adjoint kernels (adjoint_kernel_rt, adjoint_kernel_rt_tuned), read from the code objects of the current
build with tools/kernel_resources.py: like the runtime-sized solve kernels whose phases they run first, no spilled vector
register and no scratch segment -- the five adjoint phases behind the solve must not cost the condensing its registers."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as kr  # noqa: E402


@pytest.fixture(scope="module")
def kernels(solver_mod):
    ks = kr.all_kernels()
    assert ks, "no code objects under <pkg>/build: build first (python __graft_entry__.py)"
    return ks


def one(kernels, pattern):
    hit = {k: v for k, v in kernels.items() if re.search(pattern, k)}
    assert len(hit) == 1, (pattern, list(hit))
    return next(iter(hit.values()))


@pytest.mark.parametrize("name", ["adjoint_kernel_rt", "adjoint_kernel_rt_tuned"])
def test_adjoint_kernels_do_not_spill(kernels, name):
    r = one(kernels, rf"\b{name}\(")
    assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, r
    assert r["group_segment_fixed_size"] == 0, r                 # LDS: the dynamic block the launcher sizes, nothing else
    assert r["max_flat_workgroup_size"] == 256, r
