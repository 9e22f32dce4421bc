"""Host side of the duals / certificate entries (vsmpc_certify_batch, vsmpc_certify_batch_device): declarations, the
VSMPC_CERT_* offsets, exports, ctypes prototypes and argument validation without a device."""
import ctypes
import os
import re
import subprocess
from importlib import import_module

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vsmpc_certify_batch", "vsmpc_certify_batch_device")
OFFSETS = {"STATIONARITY": 0, "STAT_SCALE": 1, "PRIMAL": 2, "COMPLEMENTARITY": 3, "OBJECTIVE": 4, "DUAL_MAX": 5, "SIZE": 8}


def _header(strip=True):
    text = open(os.path.join(ROOT, "include", "vsmpc.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S) if strip else text


def _prototype(name):
    m = re.search(rf"\bint\s+{name}\s*\(([^)]*)\)\s*;", _header())
    assert m, name
    return [a.strip() for a in m.group(1).split(",")]


def test_header_declares_the_entries_and_offsets(layout, solver_mod):
    text = _header()
    for name, value in OFFSETS.items():
        m = re.search(rf"#define VSMPC_CERT_{name}\s+(\d+)", text)
        assert m and int(m.group(1)) == value == getattr(layout, "CERT_" + name), name
        assert getattr(solver_mod, "CERT_" + name) == value
    m = re.search(r"#define VSMPC_CREATE_CERTIFY\s+(0x[0-9a-fA-F]+)u", text)
    assert m and int(m.group(1), 0) == 0x20 == layout.CREATE_CERTIFY
    flags = [layout.CREATE_RUNTIME_FALLBACK, layout.CREATE_RUNTIME_ONLY, layout.CREATE_SENSITIVITY, layout.CREATE_TUNABLES,
             layout.CREATE_CERTIFY]
    assert sum(flags) == 0x2F and len(set(flags)) == 5             # distinct bits
    host = [a.split()[-1] for a in _prototype("vsmpc_certify_batch")]
    assert host == ["h", "in", "x", "tunables", "batch", "y", "cert"]
    dev = [a.split()[-1] for a in _prototype("vsmpc_certify_batch_device")]
    assert dev == ["h", "d_in", "d_x", "d_tunables", "batch", "d_y", "d_cert", "stream"]
    full = _header(strip=False)
    for cited in ("solve_exact", "kkt_certificate", "oracle/vsmpc_ref.py", "OSQP", "zero by the construction of y"):
        assert cited in full, cited


def test_new_symbols_exported(solver_mod, pkg):
    _lib = import_module(pkg.__name__ + "._lib")
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in NEW:
        assert name in _lib.EXPORTS and name in exported, name
    assert any("certify_kernel" in line for line in
               subprocess.run(["nm", "-C", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout.splitlines())


def test_ctypes_prototypes_match_header(solver_mod, pkg):
    lib = import_module(pkg.__name__ + "._lib").load()
    for name in NEW:
        decl = _prototype(name)
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int, name
        assert len(fn.argtypes) == len(decl), name
        for arg, t in zip(decl, fn.argtypes):
            if "*" in arg:
                assert t is ctypes.c_void_p, (name, arg, t)
            else:
                assert arg.startswith("int ") and t is ctypes.c_int, (name, arg, t)


def test_null_handle_is_an_invalid_argument(solver_mod, pkg):
    lib = import_module(pkg.__name__ + "._lib").load()
    assert lib.vsmpc_certify_batch(None, None, None, None, 4, None, None) == -1
    assert lib.vsmpc_certify_batch_device(None, None, None, None, 4, None, None, None) == -1
    assert lib.vsmpc_strerror(-1).decode() == "invalid argument"
