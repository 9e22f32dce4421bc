"""CPU side of the adjoint entry (vsmpc_adjoint_batch, adjoint_kernel_rt[_tuned]): the header declares the entry points and
the VSMPC_GRAD_* / VSMPC_ADJ_* constants, layout.py mirrors them, libvsmpc.so exports the symbols, the ctypes prototypes of
_lib.py match the header, and calls without a handle are refused.  No device call."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vsmpc_adjoint_batch", "vsmpc_adjoint_batch_device")
ARGS = ["h", "in", "tunables", "xbar", "fmbar", "batch", "x", "first_move", "status", "iters", "grad_x0", "grad_cfg", "active",
        "adj_flags", "stream"]


def _header():
    text = open(os.path.join(ROOT, "include", "vsmpc.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _prototype(name):
    m = re.search(rf"\bint\s+{name}\s*\(([^)]*)\)\s*;", _header())
    assert m, name
    return [a.strip() for a in m.group(1).split(",")]


def _define(name):
    m = re.search(rf"#define VSMPC_{name}\s+(0x[0-9a-fA-F]+|\d+)u?\b", _header())
    assert m, name
    return int(m.group(1), 0)


def test_header_constants_match_layout(layout):
    names = ["CREATE_ADJOINT", "ADJ_DEGENERATE", "ADJ_UNSOLVED", "GRAD_SIZE"] + \
            [n for n in dir(layout) if n.startswith("GRAD_W_") or n.startswith("GRAD_THROTTLE_")]
    assert len(names) == 4 + 12
    for name in names:
        assert _define(name) == getattr(layout, name), name
    # the create flags stay distinct bits, and 0x10 stays unused
    flags = [layout.CREATE_RUNTIME_FALLBACK, layout.CREATE_RUNTIME_ONLY, layout.CREATE_SENSITIVITY, layout.CREATE_TUNABLES,
             layout.CREATE_CERTIFY, layout.CREATE_ADJOINT]
    assert sum(flags) == 0x6f and len(set(flags)) == 6
    assert layout.ADJ_DEGENERATE == layout.SENS_DEGENERATE and layout.ADJ_UNSOLVED == layout.SENS_UNSOLVED


def test_gradient_row_follows_the_config_fields(layout):
    """entries 0..30 in the order of the tunable fields of vsmpc_config (the ctypes image), entry 31 unused"""
    tunable = [(n, t) for n, t in layout.CConfig._fields_ if n.startswith("w_") or n.startswith("throttle_")]
    off = 0
    for (name, t), (gname, goff, glen) in zip(tunable, layout.GRAD_FIELDS):
        n = ctypes.sizeof(t) // ctypes.sizeof(ctypes.c_double)
        assert (gname, goff, glen) == (name, off, n)
        assert getattr(layout, "GRAD_" + name.upper()) == off
        off += n
    assert len(tunable) == len(layout.GRAD_FIELDS) and off == 31 and layout.GRAD_SIZE == 32


def test_header_prototypes():
    host, dev = _prototype("vsmpc_adjoint_batch"), _prototype("vsmpc_adjoint_batch_device")
    assert [a.split()[-1] for a in host] == ARGS
    assert [a.split()[-1].replace("d_", "", 1) for a in dev] == ARGS
    for a in host[1:5]:
        assert a.startswith("const double*"), a


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


def test_entry_points_validate_without_a_device(solver_mod, pkg):
    from importlib import import_module
    lib = import_module(pkg.__name__ + "._lib").load()
    tail = [None] * 9
    assert lib.vsmpc_adjoint_batch(None, None, None, None, None, 4, *tail) == -1
    assert lib.vsmpc_adjoint_batch_device(None, None, None, None, None, 4, *tail) == -1
    assert lib.vsmpc_strerror(-1) == b"invalid argument"
