"""Resources of the record-adjoint kernels (adjoint_record_kernel_rt, adjoint_record_kernel_rt_tuned), read from the code
objects of the current build with tools/kernel_resources.py: like the adjoint kernels whose phases they run first, no spilled
vector register and no scratch segment -- the two record phases behind them (the per-thread accumulators of dL/d(A | Bj | Bt |
c), the 3 x 3 algebra of the transposed linearisation) must not cost the condensing its registers."""
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


def test_layout_names_the_kernels(layout):
    assert layout.ADJOINT_RECORD_KERNEL_NAMES == ("adjoint_record_kernel_rt", "adjoint_record_kernel_rt_tuned")


@pytest.mark.parametrize("name", ["adjoint_record_kernel_rt", "adjoint_record_kernel_rt_tuned"])
def test_record_adjoint_kernels_do_not_spill(kernels, name):
    r = one(kernels, rf"\b{name}\(")
    assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, r
    assert r["group_segment_fixed_size"] == 0, r                 # LDS: the dynamic block the launcher sizes, nothing else
    assert r["max_flat_workgroup_size"] == 256, r
