"""CPU side of the record-adjoint entry (vsmpc_adjoint_record_batch, adjoint_record_kernel_rt[_tuned]): the header declares
the entry points, the create flag and the VSMPC_GRAD_MODEL_* constants, layout.py mirrors them and its field table tiles the
record, libvsmpc.so exports the symbols, the ctypes prototypes of _lib.py match the header, and calls without a handle are
refused.  No device call."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vsmpc_adjoint_record_batch", "vsmpc_adjoint_record_batch_device")
ARGS = ["h", "in", "tunables", "xbar", "fmbar", "batch", "x", "first_move", "status", "iters", "grad_x0", "grad_cfg", "active",
        "adj_flags", "grad_in", "grad_model", "stream"]


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
    names = ["CREATE_ADJOINT_RECORD", "GRAD_MODEL_A", "GRAD_MODEL_BJ", "GRAD_MODEL_BT", "GRAD_MODEL_C", "GRAD_MODEL_SIZE"]
    for name in names:
        assert _define(name) == getattr(layout, name), name
    # the blocks of grad_model are A [26][26] | Bj [26][8] | Bt [26][4] | c [26], as linearize() returns them
    nx, nj, nt = layout.N_STATES, layout.N_JOINTS, layout.N_THRUSTS
    assert (layout.GRAD_MODEL_A, layout.GRAD_MODEL_BJ, layout.GRAD_MODEL_BT, layout.GRAD_MODEL_C, layout.GRAD_MODEL_SIZE) == \
        (0, nx * nx, nx * nx + nx * nj, nx * nx + nx * nj + nx * nt, nx * nx + nx * nj + nx * nt + nx)
    # a free bit of its own: the create flags stay distinct, and 0x10 stays unused
    flags = [layout.CREATE_RUNTIME_FALLBACK, layout.CREATE_RUNTIME_ONLY, layout.CREATE_SENSITIVITY, layout.CREATE_TUNABLES,
             layout.CREATE_CERTIFY, layout.CREATE_ADJOINT, layout.CREATE_ADJOINT_RECORD]
    assert sum(flags) == 0xef and len(set(flags)) == 7


def test_field_table_tiles_the_record(layout):
    """layout.record_fields: every field at its VSMPC_IN_* offset, no gap, no overlap, the window last"""
    cfg = layout.paper_config()
    off = 0
    for name, o, n in layout.record_fields(cfg):
        assert o == off == _define("IN_" + name) == getattr(layout, "IN_" + name), name
        off += n
    assert off == cfg.n_in and layout.record_fields(cfg)[-1] == ("XREF", layout.IN_XREF, 12 * cfg.n_ref_cols)


def test_header_prototypes():
    host, dev = _prototype(NEW[0]), _prototype(NEW[1])
    assert [a.split()[-1] for a in host] == ARGS
    assert [a.split()[-1].replace("d_", "", 1) for a in dev] == ARGS
    for a in host[1:5]:
        assert a.startswith("const double*"), a
    # vsmpc_adjoint_batch's arguments, then the two new outputs in front of the stream
    base = [a.split()[-1] for a in _prototype("vsmpc_adjoint_batch")]
    assert ARGS == base[:-1] + ["grad_in", "grad_model", "stream"]


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
    tail = [None] * 11
    assert lib.vsmpc_adjoint_record_batch(None, None, None, None, None, 4, *tail) == -1
    assert lib.vsmpc_adjoint_record_batch_device(None, None, None, None, None, 4, *tail) == -1
    assert lib.vsmpc_strerror(-1) == b"invalid argument"
