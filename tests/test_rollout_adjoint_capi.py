"""CPU side of the rollout-adjoint entries (vsmpc_rollout_run_taped, vsmpc_rollout_backward[_device]): the header declares
them, libvsmpc.so exports them, the ctypes prototypes of _lib.py match the header, the build lists the new unit and the
shared header, and calls without a rollout are refused.  No device call."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vsmpc_rollout_run_taped", "vsmpc_rollout_backward", "vsmpc_rollout_backward_device")
BACKWARD_ARGS = ["r", "log_bar", "state_bar", "grad_state0", "grad_cfg", "flags", "stream"]


def _header():
    text = open(os.path.join(ROOT, "include", "vsmpc.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _prototype(name):
    m = re.search(rf"\bint\s+{name}\s*\(([^)]*)\)\s*;", _header())
    assert m, name
    return [a.strip() for a in m.group(1).split(",")]


def test_header_prototypes():
    assert [a.split()[-1] for a in _prototype(NEW[0])] == [a.split()[-1] for a in _prototype("vsmpc_rollout_run")]
    assert _prototype(NEW[0]) == _prototype("vsmpc_rollout_run")                 # the same arguments as the untaped run
    host, dev = _prototype(NEW[1]), _prototype(NEW[2])
    assert [a.split()[-1] for a in host] == BACKWARD_ARGS
    assert [a.split()[-1].replace("d_", "", 1) for a in dev] == BACKWARD_ARGS
    for a in host[1:3] + dev[1:3]:
        assert a.startswith("const double*"), a
    for a in host[3:5] + dev[3:5]:
        assert a.startswith("double*"), a
    assert host[5].startswith("int*") and dev[5].startswith("int*")


def test_header_states_the_tape_size():
    text = open(os.path.join(ROOT, "include", "vsmpc.h")).read()
    assert re.search(r"VSMPC_PLANT_STATE \+ n_in \+ VSMPC_FM_SIZE doubles plus one int", re.sub(r"\s*\n \* ", " ", text))


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
                assert arg.startswith("int ") and t is ctypes.c_int, (name, arg, t)


def test_build_lists_the_new_unit(pkg):
    from importlib import import_module
    build = import_module(pkg.__name__ + ".build")
    assert "vsmpc_rollout_adjoint.hip" in build.SOURCES and "vsmpc_rollout_device.hpp" in build.HEADERS
    for f in ("vsmpc_rollout_adjoint.hip", "vsmpc_rollout_device.hpp"):
        assert os.path.exists(os.path.join(build.CSRC, f)), f


def test_entry_points_validate_without_a_device(solver_mod, pkg):
    from importlib import import_module
    lib = import_module(pkg.__name__ + "._lib").load()
    buf = (ctypes.c_double * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.vsmpc_rollout_run_taped(None, 3, None, None) == -1
    assert lib.vsmpc_rollout_run_taped(None, -1, p, None) == -1
    for fn in (lib.vsmpc_rollout_backward, lib.vsmpc_rollout_backward_device):
        assert fn(None, None, None, None, None, None, None) == -1
        assert fn(None, p, p, p, p, None, None) == -1
    assert lib.vsmpc_strerror(-1) == b"invalid argument"
