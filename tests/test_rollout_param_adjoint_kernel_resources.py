"""Resources of the two instantiations of advance_adjoint_kernel, read from the code objects of the current build with
tools/kernel_resources.py: the one that also accumulates the parameter and track gradients (PT) spills no vector register,
has no scratch segment and keeps its LDS -- the parameter cotangent and the touched track samples beside what the sweep
already holds -- under the workgroup limit; the plain one keeps the LDS it had."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as kr  # noqa: E402

LDS_WORKGROUP_LIMIT = 64 * 1024        # static LDS one workgroup may declare
PLAIN_LDS = 16040                      # of advance_adjoint_kernel before the second instantiation existed


@pytest.fixture(scope="module")
def kernels(solver_mod):
    ks = kr.all_kernels()
    assert ks, "no code objects under <pkg>/build: build first (python __graft_entry__.py)"
    return ks


def one(kernels, pattern):
    hit = {k: v for k, v in kernels.items() if re.search(pattern, k)}
    assert len(hit) == 1, (pattern, list(hit))
    return next(iter(hit.values()))


def test_both_instantiations_exist_and_no_third(kernels):
    assert len([k for k in kernels if "advance_adjoint_kernel" in k]) == 2


def test_param_instantiation_does_not_spill(kernels):
    r = one(kernels, r"advance_adjoint_kernel<true>\(")
    assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, r
    assert PLAIN_LDS < r["group_segment_fixed_size"] < LDS_WORKGROUP_LIMIT, r
    # 249 doubles of parameters, 6 per window slot, the alpha elements: a few KB beside the plain kernel's
    assert r["group_segment_fixed_size"] - PLAIN_LDS <= 8 * (250 + 6 * 41 + 6), r
    assert r["max_flat_workgroup_size"] == 64, r


def test_plain_instantiation_is_what_it_was(kernels):
    r = one(kernels, r"advance_adjoint_kernel<false>\(")
    assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, r
    assert r["group_segment_fixed_size"] == PLAIN_LDS, r
