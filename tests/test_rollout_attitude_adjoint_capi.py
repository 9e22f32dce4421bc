"""CPU side of the entries behind the rollout adjoint's attitude-track gradients (vsmpc_rollout_set_attitude_tracks_ex with
VSMPC_ATTITUDE_ADJOINT, vsmpc_rollout_backward_attitude[_device], vsmpc_rollout_att_grad_size): the header declares them and
the flag, libvsmpc.so exports them, the ctypes prototypes of _lib.py match the header, calls without a rollout and with unknown
flag bits are refused, build.py lists the two new units, and the four new kernels have the resources they were given -- read
from the code objects of the current build with tools/kernel_resources.py -- while the old kernel names count what they did.
No device call."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as kr  # noqa: E402

NEW = ("vsmpc_rollout_set_attitude_tracks_ex", "vsmpc_rollout_backward_attitude", "vsmpc_rollout_backward_attitude_device",
       "vsmpc_rollout_att_grad_size")
ATT_ARGS = ["r", "log_bar", "state_bar", "grad_state0", "grad_cfg", "grad_params", "grad_traj", "grad_att", "flags", "stream"]
UNITS = ("vsmpc_rollout_attitude_adjoint.hip", "vsmpc_rollout_attitude_tree_adjoint.hip")
LDS_WORKGROUP_LIMIT = 64 * 1024
MAX_SLOTS = 41                          # MAX_STAGES + 1 window slots of one launch
# What ATT adds to the LDS of an instantiation: the attitude slots, 6 doubles each (PT only: the other instantiation has no track
# rows, and one placeholder double), and what att_column leaves per slot for the reductions over the columns, 9 doubles each
# (the shares of roll, pitch, yaw | ybar | v); at most one double of alignment beside each of the two arrays.
ATT_SLOT, ATT_COL = 6, 9
LDS_EXCESS_MAX = 8 * (ATT_SLOT * MAX_SLOTS + ATT_COL * MAX_SLOTS + 2)
# (new kernel, its counterpart without ATT): the instantiations with the track rows, where the attitude slots live
PAIRS = ((r"advance_attitude_adjoint_kernel<true>\(", r"advance_adjoint_kernel<true>\("),
         (r"advance_attitude_tree_adjoint_kernel<true>\(", r"advance_tree_adjoint_kernel<true>\("))
PLAIN_PAIRS = ((r"advance_attitude_adjoint_kernel<false>\(", r"advance_adjoint_kernel<false>\("),
               (r"advance_attitude_tree_adjoint_kernel<false>\(", r"advance_tree_adjoint_kernel<false>\("))


def _text():
    return open(os.path.join(ROOT, "include", "vsmpc.h")).read()


def _header():
    return re.sub(r"/\*.*?\*/", "", _text(), flags=re.S)


def _prototype(name):
    m = re.search(rf"\bint\s+{name}\s*\(([^)]*)\)\s*;", _header())
    assert m, name
    return [a.strip() for a in m.group(1).split(",")]


def test_header_prototypes_and_flag():
    assert re.search(r"#define\s+VSMPC_ATTITUDE_ADJOINT\s+1u", _header())
    ex = _prototype(NEW[0])
    assert [a.split()[-1] for a in ex] == ["r", "traj_rpy", "traj_rpy_dot", "flags"]
    assert ex[1].startswith("const double*") and ex[2].startswith("const double*") and ex[3].startswith("unsigned")
    assert [a.split()[-1] for a in _prototype("vsmpc_rollout_set_attitude_tracks")] == ["r", "traj_rpy", "traj_rpy_dot"]
    host, dev = _prototype(NEW[1]), _prototype(NEW[2])
    assert [a.split()[-1] for a in host] == ATT_ARGS
    assert [a.split()[-1].replace("d_", "", 1) for a in dev] == ATT_ARGS
    for a in host[1:3] + dev[1:3]:
        assert a.startswith("const double*"), a
    for a in host[3:8] + dev[3:8]:
        assert a.startswith("double*"), a
    assert host[8].startswith("int*") and dev[8].startswith("int*")
    # the `_full` entries keep their signatures: grad_att sits between grad_traj and flags of a new entry
    assert [a.split()[-1] for a in _prototype("vsmpc_rollout_backward_full")] == [a for a in ATT_ARGS if a != "grad_att"]
    assert [a.split()[-1] for a in _prototype(NEW[3])] == ["r"]


def test_header_states_what_is_accepted_returned_and_refused():
    flat = re.sub(r"\s*\n \* ", " ", _text())
    assert "or with an RPYDot track -- alone or beside such a tree -- is refused" not in flat      # the old sentences
    assert "the jet plant option or an RPYDot track is refused by name" not in flat
    assert "with an RPYDot track set without VSMPC_ATTITUDE_ADJOINT" in flat
    assert "allocates batch x 6 n_traj doubles" in flat and "W^T R I_B^T R^T w" in flat
    assert "Still refused under the flag: the jet plant option, and a tree set without VSMPC_TREE_ADJOINT" in flat


def test_new_symbols_exported(solver_mod, pkg):
    from importlib import import_module
    _lib = import_module(pkg.__name__ + "._lib")
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in NEW:
        assert name in _lib.EXPORTS and name in exported, name


def test_ctypes_prototypes_match_header(solver_mod, pkg):
    from importlib import import_module
    lib = import_module(pkg.__name__ + "._lib").load()
    for name in NEW:
        decl = _prototype(name)
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int, name
        assert len(fn.argtypes) == len(decl), name
        for arg, t in zip(decl, fn.argtypes):
            if "*" in arg:
                assert t is ctypes.c_void_p or issubclass(t, ctypes._Pointer), (name, arg, t)
            else:
                assert arg.startswith("unsigned") and t is ctypes.c_uint, (name, arg, t)


def test_layout_names_the_blocks_of_grad_att(pkg):
    from importlib import import_module
    L = import_module(pkg.__name__ + ".layout")
    blocks = L.att_grad_blocks(24)
    assert list(blocks) == ["rpy", "rpy_dot"]
    assert blocks["rpy"] == (0, 72, (24, 3)) and blocks["rpy_dot"] == (72, 72, (24, 3))
    assert L.ATTITUDE_ADJOINT == 1


def test_entry_points_validate_without_a_device(solver_mod, pkg):
    from importlib import import_module
    lib = import_module(pkg.__name__ + "._lib").load()
    buf = (ctypes.c_double * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for fn in (lib.vsmpc_rollout_backward_attitude, lib.vsmpc_rollout_backward_attitude_device):
        assert fn(None, None, None, None, None, None, None, None, None, None) == -1
        assert fn(None, p, p, p, p, p, p, p, None, None) == -1
    assert lib.vsmpc_rollout_att_grad_size(None) == -1
    for flags in (0, 1, 2, 0x80000000):
        assert lib.vsmpc_rollout_set_attitude_tracks_ex(None, p, p, flags) == -1
    assert lib.vsmpc_strerror(-1) == b"invalid argument"


def test_build_lists_the_two_units(pkg):
    from importlib import import_module
    build = import_module(pkg.__name__ + ".build")
    for unit in UNITS:
        assert unit in build.SOURCES and os.path.exists(os.path.join(build.CSRC, unit)), unit
        assert any(u[1] == unit for u in build._units()), unit


@pytest.fixture(scope="module")
def kernels(solver_mod):
    ks = kr.all_kernels()
    assert ks, "no code objects under <pkg>/build: build first (python __graft_entry__.py)"
    return ks


def one(kernels, pattern):
    hit = {k: v for k, v in kernels.items() if re.search(pattern, k)}
    assert len(hit) == 1, (pattern, list(hit))
    return next(iter(hit.values()))


@pytest.mark.parametrize("new, old", PAIRS + PLAIN_PAIRS)
def test_new_kernels_resources(kernels, new, old):
    r, base = one(kernels, new), one(kernels, old)
    assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, r
    assert r["max_flat_workgroup_size"] == 64, r
    assert r["group_segment_fixed_size"] < LDS_WORKGROUP_LIMIT, r
    excess = r["group_segment_fixed_size"] - base["group_segment_fixed_size"]
    assert 8 * ATT_SLOT * MAX_SLOTS <= excess <= LDS_EXCESS_MAX, (new, excess)


def test_old_kernel_names_count_what_they_did(kernels):
    assert len([k for k in kernels if "advance_adjoint_kernel" in k]) == 2
    assert len([k for k in kernels if "advance_tree_adjoint_kernel" in k]) == 2
    assert len([k for k in kernels if "advance_attitude_adjoint_kernel" in k]) == 2
    assert len([k for k in kernels if "advance_attitude_tree_adjoint_kernel" in k]) == 2
    assert one(kernels, r"advance_adjoint_kernel<false>\(")["group_segment_fixed_size"] == 16040
