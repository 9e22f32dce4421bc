"""CPU side of the entries behind the rollout adjoint's parameter and track gradients (vsmpc_rollout_backward_full[_device],
vsmpc_rollout_traj_grad_size, vsmpc_rollout_set_trajectories): the header declares them, libvsmpc.so exports them, the ctypes
prototypes of _lib.py match the header, and calls without a rollout are refused.  No device call."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vsmpc_rollout_backward_full", "vsmpc_rollout_backward_full_device", "vsmpc_rollout_traj_grad_size",
       "vsmpc_rollout_set_trajectories")
FULL_ARGS = ["r", "log_bar", "state_bar", "grad_state0", "grad_cfg", "grad_params", "grad_traj", "flags", "stream"]


def _text():
    return open(os.path.join(ROOT, "include", "vsmpc.h")).read()


def _header():
    return re.sub(r"/\*.*?\*/", "", _text(), flags=re.S)


def _prototype(name):
    m = re.search(rf"\bint\s+{name}\s*\(([^)]*)\)\s*;", _header())
    assert m, name
    return [a.strip() for a in m.group(1).split(",")]


def test_header_prototypes():
    host, dev = _prototype(NEW[0]), _prototype(NEW[1])
    assert [a.split()[-1] for a in host] == FULL_ARGS
    assert [a.split()[-1].replace("d_", "", 1) for a in dev] == FULL_ARGS
    for a in host[1:3] + dev[1:3]:
        assert a.startswith("const double*"), a
    for a in host[3:7] + dev[3:7]:
        assert a.startswith("double*"), a
    assert host[7].startswith("int*") and dev[7].startswith("int*")
    # the old entries keep their signatures: the new arguments sit between grad_cfg and flags of a new entry
    old = [a.split()[-1] for a in _prototype("vsmpc_rollout_backward")]
    assert old == [a for a in FULL_ARGS if a not in ("grad_params", "grad_traj")]
    assert [a.split()[-1] for a in _prototype(NEW[2])] == ["r"]
    st = _prototype(NEW[3])
    assert [a.split()[-1] for a in st] == ["r", "traj_pos", "traj_vel", "traj_alpha"]
    assert all(a.startswith("const double*") for a in st[1:])


def test_header_states_the_memory_the_scope_and_the_alpha_track():
    flat = re.sub(r"\s*\n \* ", " ", _text())
    assert re.search(r"batch x \(VSMPC_PLANT_PARAMS \+ 6 n_traj \+ n_alpha\) doubles", flat)
    assert "held fixed" in flat and "VSMPC_ERR_ALLOC and leaves the rollout and its tape usable" in flat
    assert "and the alpha track are structural" not in flat          # the sentence the old header had: alpha is differentiated
    assert "Gradients with respect to the plant parameters and the trajectories are not returned" not in flat


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
            assert "*" in arg and (t is ctypes.c_void_p or issubclass(t, ctypes._Pointer)), (name, arg, t)


def test_layout_names_the_blocks_of_grad_traj(pkg):
    from importlib import import_module
    L = import_module(pkg.__name__ + ".layout")
    blocks = L.traj_grad_blocks(24, 4)
    assert list(blocks) == ["pos", "vel", "alpha"]
    assert blocks["pos"] == (0, 72, (24, 3)) and blocks["vel"] == (72, 72, (24, 3)) and blocks["alpha"] == (144, 4, (4,))
    fields = {name: (off, n) for name, off, n in L.PARAM_GRAD_FIELDS}
    assert fields["MASS"] == (L.PP_MASS, 1) and fields["DJ"] == (L.PP_DJ, 192) and fields["DIST_TAU"] == (L.PP_DIST_TAU, 3)
    assert sum(n for _, n in fields.values()) == L.PLANT_PARAMS - 3      # all but DIST_T0, DIST_T1, TICK0


def test_entry_points_validate_without_a_device(solver_mod, pkg):
    from importlib import import_module
    lib = import_module(pkg.__name__ + "._lib").load()
    buf = (ctypes.c_double * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for fn in (lib.vsmpc_rollout_backward_full, lib.vsmpc_rollout_backward_full_device):
        assert fn(None, None, None, None, None, None, None, None, None) == -1
        assert fn(None, p, p, p, p, p, p, None, None) == -1
    assert lib.vsmpc_rollout_traj_grad_size(None) == -1
    assert lib.vsmpc_rollout_set_trajectories(None, p, p, p) == -1
    assert lib.vsmpc_strerror(-1) == b"invalid argument"
