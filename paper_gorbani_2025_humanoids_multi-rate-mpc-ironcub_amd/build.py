"""Builds the HIP library in-tree: csrc/*.hip -> build/*.o -> libvsmpc.so (gfx950 only).

hipcc cross-compiles without a GPU, so this runs in the build container; the resulting .so is
git-ignored but travels with the tree to the GPU box.
"""
from __future__ import annotations

import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB_PATH = os.path.join(HERE, "libvsmpc.so")
SOLVE = "vsmpc_kernels.hip"     # the per-horizon unit: production / diagnostic / per-instance-tunables instantiations
SOURCES = [SOLVE, "vsmpc_dispatch.hip", "vsmpc_rollout.hip", "vsmpc_rollout_adjoint.hip", "vsmpc_rollout_tree_adjoint.hip",
           "vsmpc_rollout_attitude_adjoint.hip", "vsmpc_rollout_attitude_tree_adjoint.hip", "vsmpc_capi.hip", "vsmpc_capi_solve.hip", "vsmpc_capi_debug.hip",
           "vsmpc_capi_rollout.hip", "vsmpc_jet.hip", "vsmpc_provider.hip", "vsmpc_tree_jacobian.hip", "vsmpc_runtime.hip", "vsmpc_certify.hip"]
HEADERS = ["vsmpc_device.hpp", "vsmpc_launch.hpp", "vsmpc_host.hpp", "vsmpc_p0.hpp", "vsmpc_smem.hpp", "vsmpc_p1_syrk.hpp", "vsmpc_p1_struct.hpp",
           "vsmpc_p3.hpp", "vsmpc_p4.hpp", "vsmpc_p5.hpp", "vsmpc_panel_asm.inc",
           "vsmpc_structure.hpp", "vsmpc_rt_core.hpp", "vsmpc_rt_sens.hpp", "vsmpc_rt_adjoint.hpp", "vsmpc_rt_adjoint_record.hpp", "vsmpc_solve_body.inc", "vsmpc_jet_device.hpp", "vsmpc_rollout_device.hpp", "vsmpc_noise_device.hpp", "vsmpc_rollout_adjoint_device.hpp", "vsmpc_horizons.def", os.path.join("..", "..", "include", "vsmpc.h"),
           os.path.join("..", "..", "include", "vsmpc_jet.h")]


# Horizons (nIter, nIterSmall, controlHorizon) that get a kernel instantiation.  The kernels are straight-line code per
# horizon (variableSamplingMPC.cpp:24-45 sizes the reference from its XML at run time; here the table is fixed at build
# time): BASELINE.json's two configurations, plus one odd size that exercises the general paths (controlHorizon odd:
# joint rows share a tile with throttle rows; three throttle tile rows).  VSMPC_HORIZONS="17,7,12;25,10,18" overrides.
DEFAULT_HORIZONS = ((17, 7, 12), (34, 14, 24), (21, 9, 15))
HORIZONS_DEF = os.path.join(CSRC, "vsmpc_horizons.def")


def horizons():
    env = os.environ.get("VSMPC_HORIZONS", "").strip()
    if not env:
        return DEFAULT_HORIZONS
    out = []
    for item in env.split(";"):
        n, ns, hc = (int(v) for v in item.split(","))
        out.append((n, ns, hc))
    return tuple(out)


def write_horizons_def() -> bool:
    """(Re)writes csrc/vsmpc_horizons.def when the requested table differs; returns True if it changed."""
    text = ("// Horizons (nIter, nIterSmall, controlHorizon) with a kernel instantiation: one X(...) line each.\n"
            "// Written by build.py (DEFAULT_HORIZONS or VSMPC_HORIZONS); the first two are BASELINE.json's configurations.\n"
            + "".join(f"X({n}, {ns}, {hc})\n" for n, ns, hc in horizons()))
    old = open(HORIZONS_DEF).read() if os.path.exists(HORIZONS_DEF) else None
    if old != text:
        with open(HORIZONS_DEF, "w") as f:
            f.write(text)
        return True
    return False


def _hipcc() -> str:
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found: the vsmpc HIP library cannot be built")


OBJ_DIR = os.path.join(HERE, "build")


SCHED_MAX_ILP = ["-mllvm", "-amdgpu-sched-strategy=max-ilp"]
# the small-batch kind of the paper horizon: 32.4-32.8 us per 256-launch with max-ilp, 32.8-33.2 with the default strategy
SMALL_SCHED = SCHED_MAX_ILP


def _units():
    """(object name, source, extra flags): vsmpc_kernels.hip is compiled five times per horizon (production, diagnostic, the
    two condensing forms of the per-instance-tunables kind and the small-batch kind, see the note on the launchers in the
    file), everything else once.  Which horizons have a structured form is decided in the C++ (Dims::STRUCT_P1), so the structured unit is
    listed for every horizon: where the horizon has none (21,9,15 of the default table) it holds no kernel, only a
    launcher that returns hipErrorInvalidValue and that the dispatcher never calls."""
    units = []
    for n, ns, hc in horizons():
        # Machine scheduler strategy per horizon (measured on MI355X, default against -amdgpu-sched-strategy=max-ilp): the
        # short-horizon kernels (<= 256 registers, two workgroups per CU) gain 2-3 % with max-ilp -- 36.6 -> 35.7 us per 256-launch,
        # 327 -> 317 us per 4096 -- the long-horizon kernel (512 registers, tiles in AGPRs) loses 2.6 % (1,593 -> 1,634 us).
        sched = SCHED_MAX_ILP if n <= 24 else []
        for name, kind in (("prod", "PRODUCTION"), ("diag", "DIAGNOSTIC")):
            units.append((f"kernels_{n}_{ns}_{hc}_{name}", SOLVE,
                          [f"-DVS_TU_HORIZON={n},{ns},{hc}", f"-DVS_TU_KIND=VS_KIND_{kind}"] + sched))
        for form in (0, 1):     # the per-instance-tunables kind: one unit per condensing form (1 = structured)
            units.append((f"kernels_{n}_{ns}_{hc}_tuned_{'struct' if form else 'syrk'}", SOLVE,
                          [f"-DVS_TU_HORIZON={n},{ns},{hc}", "-DVS_TU_KIND=VS_KIND_TUNED", f"-DVS_TU_FORM={form}"] + sched))
        # the small-batch kind (solve_kernel_small, production + diagnostic; a horizon without it gets a launcher that
        # refuses and that the dispatcher never calls).  Scheduler strategy: see SMALL_SCHED
        units.append((f"kernels_{n}_{ns}_{hc}_small", SOLVE,
                      [f"-DVS_TU_HORIZON={n},{ns},{hc}", "-DVS_TU_KIND=VS_KIND_SMALL"] + SMALL_SCHED))
    for src in SOURCES:
        if src != SOLVE:
            units.append((os.path.splitext(src)[0], src, []))
    return units


def _deps(src):
    return [os.path.join(CSRC, src)] + [os.path.join(CSRC, h) for h in HEADERS] + [os.path.abspath(__file__)]


def _extra_flags():
    """VSMPC_HIPCC_FLAGS: measurement builds, e.g. -DVS_DIAG_P3 (tools/gpu_phases.py)"""
    return os.environ.get("VSMPC_HIPCC_FLAGS", "").split()


def _unit_options(unit):
    """what hipcc is given for one unit of _units() besides the paths: what the code in its object depends on"""
    return ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c"] + _extra_flags() + unit[2]


def _stamp(unit):
    """(path, text now) of the unit's .flags stamp, written beside its object when it has compiled.  Neither the place of
    the tree nor the compiler's is in the text: a tree that was copied with its library stays built."""
    return os.path.join(OBJ_DIR, unit[0] + ".o.flags"), " ".join(_unit_options(unit) + [unit[1]])


def _stamped(unit) -> bool:
    path, text = _stamp(unit)
    return os.path.exists(path) and open(path).read() == text


def needs_build() -> bool:
    """True when the library is missing, older than a source, or was built with other flags than a build would use now
    (VSMPC_HIPCC_FLAGS: a measurement build must not pass for the production library, nor the reverse)"""
    if not os.path.exists(LIB_PATH):
        return True
    t = os.path.getmtime(LIB_PATH)
    deps = [os.path.join(CSRC, s) for s in SOURCES + HEADERS] + [os.path.abspath(__file__)]
    return any(os.path.getmtime(d) > t for d in deps) or not all(_stamped(u) for u in _units())


def build_library(force: bool = False, verbose: bool = False, jobs: int | None = None) -> str:
    """Objects under build/ (git-ignored), one hipcc process each, `jobs` at a time (default: the CPUs of the machine, at
    most 8); an object is rebuilt when its source, a header or this file is newer, or when its flags changed."""
    from concurrent.futures import ThreadPoolExecutor
    changed = write_horizons_def()
    if not force and not changed and not needs_build():
        return LIB_PATH
    os.makedirs(OBJ_DIR, exist_ok=True)
    hipcc = _hipcc()
    todo, objs = [], []
    for unit in _units():
        obj = os.path.join(OBJ_DIR, unit[0] + ".o")
        stamp, flagtext = _stamp(unit)
        cmd = ([hipcc] + (["-Rpass-analysis=kernel-resource-usage"] if verbose else []) + _unit_options(unit)
               + [os.path.join(CSRC, unit[1]), "-o", obj])
        objs.append(obj)
        fresh = (not force and os.path.exists(obj) and _stamped(unit)
                 and all(os.path.getmtime(d) <= os.path.getmtime(obj) for d in _deps(unit[1])))
        if not fresh:
            todo.append((cmd, stamp, flagtext))

    def run(item):
        cmd, stamp, flagtext = item
        res = subprocess.run(cmd, capture_output=True, text=True)
        if res.returncode == 0:
            with open(stamp, "w") as f:
                f.write(flagtext)
        return cmd, res

    jobs = jobs or int(os.environ.get("VSMPC_BUILD_JOBS", "0")) or min(8, os.cpu_count() or 1)
    with ThreadPoolExecutor(max_workers=jobs) as pool:
        results = list(pool.map(run, todo))
    for cmd, res in results:
        if res.returncode != 0:
            raise RuntimeError("hipcc failed: " + " ".join(cmd) + "\n" + res.stdout + res.stderr)
        if verbose:
            print(res.stderr)
    keep = {os.path.basename(o) for o in objs}
    for f in os.listdir(OBJ_DIR):           # objects of horizons that left the table
        if f.endswith(".o") and f not in keep:
            os.remove(os.path.join(OBJ_DIR, f))
    link = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-Wl,-rpath,/opt/rocm/lib", "-o", LIB_PATH] + objs
    res = subprocess.run(link, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError("link failed:\n" + res.stdout + res.stderr)
    return LIB_PATH


def build_bindings(force: bool = False) -> str | None:
    """pybind11 shim `bindingsMPC` (reference Python surface, MPCPyBindings.cpp:12-91); host-only g++ build that links
    libvsmpc.so.  Returns the module path, or None when pybind11 is not available."""
    try:
        import pybind11
    except ImportError:
        return None
    import sysconfig
    src = os.path.join(CSRC, "bindings_mpc.cpp")
    out = os.path.join(HERE, "bindingsMPC" + (sysconfig.get_config_var("EXT_SUFFIX") or ".so"))
    deps = [src, os.path.join(HERE, "..", "include", "VariableSamplingMPC.hpp"), os.path.join(HERE, "..", "include", "vsmpc.h")]
    if not force and os.path.exists(out) and all(os.path.getmtime(d) <= os.path.getmtime(out) for d in deps):
        return out
    build_library()
    cmd = ["g++", "-O2", "-std=c++17", "-shared", "-fPIC", f"-I{pybind11.get_include()}",
           f"-I{sysconfig.get_paths()['include']}", src, "-o", out, f"-L{HERE}", "-lvsmpc",
           "-Wl,-rpath,$ORIGIN", "-Wl,-rpath,/opt/rocm/lib"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError("bindingsMPC build failed:\n" + res.stdout + res.stderr)
    return out


if __name__ == "__main__":
    print(build_library(force=True, verbose=True))
