"""CPU side of the kinematic-tree plant's new entries (vsmpc_tree_jacobian_batch[_device], vsmpc_rollout_set_tree_ex): the
header declares them, libvsmpc.so exports them, layout.py carries the header's constants, the NULL and size refusals come
back before any device call, and the code objects of the current build (tools/kernel_resources.py) show the new kernels
without a spilled vector register or a scratch segment -- tree_jacobian_kernel walks its bodies by run-time tables, which
is what would put its per-body frames into scratch if they were not staged in LDS.  No device call."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as kr  # noqa: E402

NEW = ("vsmpc_tree_jacobian_batch", "vsmpc_tree_jacobian_batch_device", "vsmpc_rollout_set_tree_ex")
LDS_WORKGROUP_LIMIT = 64 * 1024


def _text():
    return open(os.path.join(ROOT, "include", "vsmpc.h")).read()


def _prototype(name):
    m = re.search(rf"\bint\s+{name}\s*\(([^)]*)\)\s*;", re.sub(r"/\*.*?\*/", "", _text(), flags=re.S))
    assert m, name
    return [a.strip() for a in m.group(1).split(",")]


def test_header_prototypes_and_constants(layout):
    host, dev = _prototype(NEW[0]), _prototype(NEW[1])
    assert [a.split()[-1] for a in host] == ["h", "tree", "q", "thrust", "batch", "terms", "jac"]
    assert [a.split()[-1].replace("d_", "", 1) for a in dev] == ["h", "tree", "q", "thrust", "batch", "terms", "jac", "stream"]
    assert [a.split()[-1] for a in _prototype(NEW[2])] == ["r", "tree", "flags"] and _prototype(NEW[2])[2].startswith("unsigned")
    defs = dict(re.findall(r"#define\s+VSMPC_(TT_[A-Z]+)\s+(\d+)", _text()))
    assert defs == {"TT_AMOM": "0", "TT_LLIN": "24", "TT_LANG": "48", "TT_IB": "72", "TT_SIZE": "81", "TT_NDIR": "12"}
    for key, val in defs.items():
        assert getattr(layout, key) == int(val), key
    assert re.search(r"#define\s+VSMPC_TREE_ADJOINT\s+1u", _text()) and layout.TREE_ADJOINT == 1


def test_header_states_the_scope():
    flat = re.sub(r"\s*\n \* ", " ", _text())
    assert "Supported: the parametric plant, and the kinematic-tree plant when the tree was set with VSMPC_TREE_ADJOINT" in flat
    assert "gradients to it are not computed" in flat and "kept by value with the tape" in flat
    assert "INERTIA_B, AMOM0, DJ -- are +0.0" in flat


def test_new_symbols_exported(solver_mod, pkg):
    from importlib import import_module
    _lib = import_module(pkg.__name__ + "._lib")
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in NEW:
        assert name in _lib.EXPORTS and name in exported, name
        assert len(getattr(_lib.load(), name).argtypes) == len(_prototype(name)), name


def test_entry_points_validate_without_a_device(solver_mod, pkg):
    from importlib import import_module
    lib = import_module(pkg.__name__ + "._lib").load()
    RT = import_module(pkg.__name__ + ".robot_tree")
    tree = ctypes.byref(RT.to_c(RT.default_tree()))
    buf = (ctypes.c_double * (81 * 13))()
    p = ctypes.cast(buf, ctypes.c_void_p)
    # without a device there is no handle: every call here comes back at the first check, before any device call.  The checks
    # behind it (tree, q, thrust, batch, an invalid tree) are held with a live handle in tests/test_gpu_tree_jacobian.py
    for fn, tail in ((lib.vsmpc_tree_jacobian_batch, ()), (lib.vsmpc_tree_jacobian_batch_device, (None,))):
        assert fn(None, tree, p, p, 1, p, p, *tail) == -1
        assert fn(None, None, None, None, 0, None, None, *tail) == -1
    assert lib.vsmpc_rollout_set_tree_ex(None, tree, 1) == -1
    assert lib.vsmpc_rollout_set_tree_ex(None, None, 0) == -1
    assert lib.vsmpc_rollout_set_tree_ex(None, tree, 2) == -1        # an unknown flag
    assert lib.vsmpc_strerror(-1) == b"invalid argument"


@pytest.fixture(scope="module")
def kernels(solver_mod):
    ks = kr.all_kernels()
    assert ks, "no code objects under <pkg>/build: build first (python __graft_entry__.py)"
    return ks


def _one(kernels, pattern):
    hit = {k: v for k, v in kernels.items() if re.search(pattern, k)}
    assert len(hit) == 1, (pattern, list(hit))
    return next(iter(hit.values()))


def test_tree_jacobian_kernel_keeps_its_frames_out_of_scratch(kernels):
    r = _one(kernels, r"\btree_jacobian_kernel\(")
    assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, r
    # the staged frames: 183 values per instance and 183 derivatives per direction lane, four instances of eight lanes
    assert 8 * 183 * (4 + 32) <= r["group_segment_fixed_size"] < LDS_WORKGROUP_LIMIT, r
    assert r["max_flat_workgroup_size"] == 64, r


@pytest.mark.parametrize("pt", ["false", "true"])
def test_tree_instantiations_of_the_sweep_do_not_spill(kernels, pt):
    r = _one(kernels, rf"advance_tree_adjoint_kernel<{pt}>\(")
    plain = _one(kernels, rf"advance_adjoint_kernel<{pt}>\(")
    assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, r
    # tau, its Jacobian and the sub-steps' cotangent of I_B beside what the parametric plant's kernel holds
    extra = r["group_segment_fixed_size"] - plain["group_segment_fixed_size"]
    assert 8 * (81 + 81 * 12 + 9) <= extra <= 8 * (81 + 81 * 12 + 9 + 4), (extra, r)
    assert r["group_segment_fixed_size"] < LDS_WORKGROUP_LIMIT and r["max_flat_workgroup_size"] == 64, r
