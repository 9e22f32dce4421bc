"""CPU side of the runtime-sized solve kernel (csrc/vsmpc_runtime.hip, vsmpc_create_ex):
  * tests/runtime_model.py -- the kernel's algorithm in numpy (full joint blocks, Cholesky of the joint columns, then
    block principal pivoting on the throttle Schur complement) -- lands on the oracle's optimum with the oracle's
    active-set iteration count, for tabled, untabled and edge horizons and non-default settings;
  * the C-ABI: vsmpc_create_ex is declared, exported and bound, and the flag values agree between header and layout.py;
  * the runtime kernel's code object has no spilled vector register and no scratch segment."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import relerr
from config_cases import NON_DEFAULT
import runtime_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))



def _cases(layout, synth, ref, horizon, settings, n_per_workload=2):
    kw = dict(n_iter=horizon[0], n_iter_small=horizon[1], control_horizon=horizon[2], **settings)
    cfg, rcfg = layout.MPCConfig(**kw), ref.Config(**kw)
    recs = [synth.make_batch(cfg, n_per_workload, workload=w, first_index=3) for w in ("hover", "takeoff")]
    sat = synth.make_batch(cfg, 2, workload="hover", first_index=40)     # saturated throttles on a free tick
    sat[:, layout.IN_HOLD] = 0.0
    sat[:, layout.IN_XREF + 2::12] += 30.0
    sat[:, 22] = sat[:, 2] - sat[:, layout.IN_XREF + 2]
    held = synth.make_batch(cfg, 1, workload="takeoff", first_index=7)   # the hold pin on
    held[:, layout.IN_HOLD] = 1.0
    return rcfg, np.concatenate(recs + [sat, held])


# (40, 2, 40): 156 throttles; the oracle is a dense 1542-variable solve per instance, so defaults only
CASES = [(h, s) for h in ((17, 7, 12), (20, 5, 9), (6, 2, 3), (12, 12, 12)) for s in ("default", "non_default")] + \
        [((40, 2, 40), "default")]
SATURATING = {(17, 7, 12), (20, 5, 9), (40, 2, 40)}   # horizons whose pushed instances hit the throttle box


@pytest.mark.parametrize("horizon, settings", CASES)
def test_runtime_model_matches_oracle(layout, synth, ref, horizon, settings):
    rcfg, recs = _cases(layout, synth, ref, horizon, {} if settings == "default" else NON_DEFAULT,
                        n_per_workload=1 if horizon == (40, 2, 40) else 2)
    multi = 0
    for b, rec in enumerate(recs):
        xr, _, itr, _ = ref.solve_instance(rcfg, rec)
        x, fm, st, it = rm.solve(rcfg, rec)
        assert st == rm.SOLVED, (b, st)
        assert relerr(x, xr) < 1e-10, (b, relerr(x, xr))
        assert relerr(fm, ref.first_move_vector(rcfg, xr)) < 1e-10
        assert it == itr, (b, it, itr)
        multi += itr > 1
    if horizon in SATURATING:
        assert multi > 0   # the saturated instances need more than the hold-only solve


def test_runtime_model_hold_pins_v0(layout, synth, ref):
    cfg = layout.MPCConfig(n_iter=20, n_iter_small=5, control_horizon=9)
    rcfg = ref.Config(n_iter=20, n_iter_small=5, control_horizon=9)
    rec = synth.make_batch(cfg, 1, workload="takeoff")[0]
    rec[layout.IN_HOLD] = 1.0
    x, _, st, _ = rm.solve(rcfg, rec)
    vprev = [ref.v_of_throttle(rec[layout.IN_UPREV + r]) for r in range(4)]
    assert st == rm.SOLVED and np.array_equal(x[rcfg.off_throttle:rcfg.off_throttle + 4], vprev)


def _header():
    return open(os.path.join(ROOT, "include", "vsmpc.h")).read()


def test_create_ex_flags_match_layout(layout):
    text = _header()
    for name, val in (("RUNTIME_FALLBACK", layout.CREATE_RUNTIME_FALLBACK), ("RUNTIME_ONLY", layout.CREATE_RUNTIME_ONLY)):
        m = re.search(rf"#define VSMPC_CREATE_{name}\s+(0x[0-9a-fA-F]+|\d+)u?", text)
        assert m, name
        assert int(m.group(1), 0) == val
    assert layout.RUNTIME_MODES == {"never": 0, "fallback": 1, "always": 2}
    assert re.search(r"int vsmpc_create_ex\(const vsmpc_config\* cfg, int device, int max_batch, unsigned flags,", text)


def test_create_ex_exported_and_bound(solver_mod, pkg):
    from importlib import import_module
    _lib = import_module(pkg.__name__ + "._lib")
    assert "vsmpc_create_ex" in _lib.EXPORTS
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "vsmpc_create_ex" in {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_runtime_mode_argument_is_checked(solver_mod, layout):
    with pytest.raises(ValueError):
        solver_mod.BatchedVSMPC(layout.paper_config(), device=0, max_batch=1, runtime="sometimes")


def test_runtime_kernel_does_not_spill(solver_mod):
    import kernel_resources as kr
    ks = {k: v for k, v in kr.all_kernels().items() if "solve_kernel_rt" in k}
    assert ks, "runtime kernel not in the build"
    for name, r in ks.items():
        assert r["vgpr_spill_count"] == 0, (name, r)
        assert r["private_segment_fixed_size"] == 0, (name, r)
