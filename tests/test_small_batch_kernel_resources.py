"""Resources of the small-batch kind of the solve kernel (solve_kernel_small, csrc/vsmpc_kernels.hip), read from the
code-object metadata of the current build as tests/test_kernel_resources.py does for the shipped kernels.  The kind runs one
workgroup per CU on purpose, so it may take the registers and the LDS of a whole CU -- but a spilled vector register or a
scratch segment is a global-memory round trip on the serial instruction stream of every instance there too, and the LDS it
asks for at launch has to fit the 160 KB a CU has.  (The dynamic LDS size is a launch argument, not metadata: the library
reports it per tabled horizon, without a device.)"""
import importlib
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as kr  # noqa: E402

PKG = "paper_gorbani_2025_humanoids_multi-rate-mpc-ironcub_amd"
CU_LDS_BYTES = 160 * 1024


@pytest.fixture(scope="module")
def small_kernels(solver_mod):
    ks = kr.all_kernels()
    assert ks, "no code objects under <pkg>/build: build first (python __graft_entry__.py)"
    return {k: v for k, v in ks.items() if "solve_kernel_small<" in k}


def test_the_paper_horizon_has_both_instantiations(small_kernels):
    """production (STAMPS = false) and diagnostic (true), and no other horizon of the default table has the kind"""
    names = sorted(small_kernels)
    assert len(names) == 2, names
    assert all("Dims<17, 7, 12>" in n for n in names), names
    assert any(", false>" in n for n in names) and any(", true>" in n for n in names), names


def test_small_kind_does_not_spill_and_has_no_scratch(small_kernels):
    for name, r in small_kernels.items():
        assert r["vgpr_spill_count"] == 0, (name, r)
        assert r["private_segment_fixed_size"] == 0, (name, r)
        assert r["max_flat_workgroup_size"] == 256, (name, r)
        assert r["vgpr_count"] + r.get("agpr_count", 0) <= 512, (name, r)      # one wavefront per SIMD at the most


def test_launch_lds_fits_one_cu(solver_mod):
    lib = importlib.import_module(PKG + "._lib").load()
    small = lib.vsmpc_small_batch_lds_bytes(17, 7, 12)
    assert 80 * 1024 < small <= CU_LDS_BYTES, small          # more than a two-per-CU kernel may take, no more than a CU has
    assert small % 8 == 0
    for horizon in ((34, 14, 24), (21, 9, 15), (13, 5, 8)):   # long horizon, SYRK-only horizon, not in the table
        assert lib.vsmpc_small_batch_lds_bytes(*horizon) == 0, horizon
