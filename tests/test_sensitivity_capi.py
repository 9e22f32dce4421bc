"""CPU side of the sensitivity entry (vsmpc_sensitivity_batch, sens_kernel_rt): the header declares the entry points and
constants, libvsmpc.so exports them, the ctypes prototypes of _lib.py match the header, and the kernel's code object has
no spilled vector register and no scratch segment.  No device call."""
import ctypes
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

NEW = ("vsmpc_num_throttle_unknowns", "vsmpc_sensitivity_batch", "vsmpc_sensitivity_batch_device")


def _header(strip_comments=True):
    text = open(os.path.join(ROOT, "include", "vsmpc.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S) if strip_comments else text


def _prototype(name):
    m = re.search(rf"\bint\s+{name}\s*\(([^)]*)\)\s*;", _header())
    assert m, name
    return [a.strip() for a in m.group(1).split(",")]


def test_header_constants_match_layout(layout):
    text = _header()
    for name in ("CREATE_SENSITIVITY", "SENS_DEGENERATE", "SENS_UNSOLVED"):
        m = re.search(rf"#define VSMPC_{name}\s+(0x[0-9a-fA-F]+|\d+)u?\b", text)
        assert m, name
        assert int(m.group(1), 0) == getattr(layout, name), name
    for name in ("SENS_GRAD_TOL", "SENS_BOUND_TOL"):
        m = re.search(rf"#define VSMPC_{name}\s+([0-9.eE+-]+)", text)
        assert m and float(m.group(1)) == getattr(layout, name), name
    flags = [layout.CREATE_RUNTIME_FALLBACK, layout.CREATE_RUNTIME_ONLY, layout.CREATE_SENSITIVITY]
    assert sum(flags) == 0x7 and len(set(flags)) == 3            # distinct bits


def test_header_prototypes():
    assert _prototype("vsmpc_num_throttle_unknowns") == ["const vsmpc_handle* h"]
    host = _prototype("vsmpc_sensitivity_batch")
    dev = _prototype("vsmpc_sensitivity_batch_device")
    assert len(host) == len(dev) == 12
    assert [a.split()[-1] for a in host] == ["h", "in", "batch", "x", "first_move", "status", "iters", "dx_dx0", "dfm_dx0",
                                             "active", "sens_flags", "stream"]


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
    assert lib.vsmpc_num_throttle_unknowns(None) == -1
    args = [None] * 9
    assert lib.vsmpc_sensitivity_batch(None, None, 4, *args) == -1
    assert lib.vsmpc_sensitivity_batch_device(None, None, 4, *args) == -1


def test_sens_kernel_resources(solver_mod):
    import kernel_resources as kr
    ks = {k: v for k, v in kr.all_kernels().items() if "sens_kernel_rt" in k}
    assert ks, "sens_kernel_rt not in the build"
    for name, r in ks.items():
        assert r["vgpr_spill_count"] == 0, (name, r)
        assert r["private_segment_fixed_size"] == 0, (name, r)
        assert r["max_flat_workgroup_size"] == 256, (name, r)
