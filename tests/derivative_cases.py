"""The record families the derivative kernels (sens_kernel_rt, adjoint_kernel_rt[_tuned]) are held to, with their CPU
references (plain helper module, imported by tests).

test_gpu_sensitivity._records() draws from synth.make_batch, whose records tie together what the derivative phases read
through index arithmetic of their own (tests/record_cases.py lists the ties): a window read one column late, or a hold
read as == 1.0, changes nothing on them.  The families here are the ones the solve kernels are already held to:

  RECORDS   record_cases.records() -- six all-distinct records and the edge records (HELD = 2.5, -1, 1e-300 and -0.0 in the
            hold flag, a window 30 m apart from column to column, every throttle on the upper bound at mass_480) -- at the
            paper horizon, at (20, 5, 9) with NON_DEFAULT and at (6, 2, 3)
  TABLES    the tables of boxqp_pass_cases picked by what the later passes of the box QP do: bounds added in a later pass,
            lower and upper bounds in one instance, the three-tile-row horizon (34, 14, 24) with 44 throttles

The references of an instance (both routes of adjoint_model and of sensitivity_model) are computed once per process, keyed
by (family, instance, cotangent seed), and never written to; tests/test_derivative_cases.py keeps the families honest on
the CPU.
"""
import numpy as np

import adjoint_model as am
import boxqp_pass_cases as bp
import config_cases as cc
import record_cases as rc
import sensitivity_model as sm

RECORDS = [((17, 7, 12), {}), ((20, 5, 9), cc.NON_DEFAULT), ((6, 2, 3), {})]
TABLES = ("shrinking", "growing", "H21_box", "H34")
SEED = 5                                    # of the cotangents (test_gpu_adjoint._cotangents' default)


def _records_name(horizon):
    return "records_%d_%d_%d" % tuple(horizon)


FAMILIES = tuple(_records_name(h) for h, _ in RECORDS) + TABLES
SIZES = dict(zip(FAMILIES, (20, 20, 20, 5, 4, 3, 8)))
# the `runtime` argument of the handle that solves a family, by horizon ("fallback" elsewhere): the solve in front of the
# derivative phases is the tuned kernel's at the paper horizon and the runtime-sized one at the others
RUNTIME = {(17, 7, 12): "never", (21, 9, 15): "always", (34, 14, 24): "always"}

_families = {}
_refs = {}


def runtime_of(cfg):
    return RUNTIME.get((cfg.n_iter, cfg.n_iter_small, cfg.control_horizon), "fallback")


def family(ref, name):
    """(name, MPCConfig, oracle Config, records, names) of one family; the arrays are shared and read-only"""
    if name not in _families:
        if name in TABLES:
            cfg, rcfg, recs = bp.batch(ref, name)
            names = [f"{name}[{i}]" for i in range(len(recs))]
        else:
            horizon, settings = RECORDS[[_records_name(h) for h, _ in RECORDS].index(name)]
            cfg, rcfg = cc.configs(ref, horizon, settings)
            names, recs = rc.records(cfg)
        recs = np.ascontiguousarray(recs)
        recs.setflags(write=False)
        assert len(recs) == SIZES[name] and len(names) == len(recs), name
        _families[name] = (name, cfg, rcfg, recs, list(names))
    return _families[name]


def families(ref):
    return [family(ref, name) for name in FAMILIES]


def cotangents(B, n_var, seed=SEED):
    """(xbar [B, n_var], fmbar [B, 24]): standard normal, fixed seed"""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((B, n_var)), rng.standard_normal((B, 24))


def _frozen(d):
    for v in d.values() if isinstance(d, dict) else d:
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def adjoint_refs(ref, name, b, seed=SEED):
    """(kkt_adjoint, condensed_adjoint) of instance b of a family under the family's cotangents"""
    key = (name, b, seed)
    if key not in _refs:
        _, _, rcfg, recs, _ = family(ref, name)
        xbar, fmbar = cotangents(len(recs), rcfg.n_var, seed)
        _refs[key] = (_frozen(am.kkt_adjoint(rcfg, recs[b], xbar[b], fmbar[b])),
                      _frozen(am.condensed_adjoint(rcfg, recs[b], xbar[b], fmbar[b])))
    return _refs[key]


def jacobian_refs(ref, name, b):
    """((x, J, active) of kkt_jacobian, condensed_jacobian's dict) of instance b of a family"""
    key = (name, b, None)
    if key not in _refs:
        _, _, rcfg, recs, _ = family(ref, name)
        _refs[key] = (_frozen(sm.kkt_jacobian(rcfg, recs[b])), _frozen(sm.condensed_jacobian(rcfg, recs[b])))
    return _refs[key]


# ---- adjoint_kernel_rt_tuned: the records at (20, 5, 9) on a handle of the default configuration, instance b under
# configuration b % 3 of: the handle's own, NON_DEFAULT without period_small (a structural field), the box 30..85
TUNED_HORIZON = (20, 5, 9)
TUNED_SETTINGS = ({}, {k: v for k, v in cc.NON_DEFAULT.items() if k != "period_small"}, bp.BOX_30_85)


def tuned_cases(ref):
    """(handle's MPCConfig, records, names, one MPCConfig per instance, one oracle Config per instance)"""
    if "tuned" not in _families:
        both = [cc.configs(ref, TUNED_HORIZON, s) for s in TUNED_SETTINGS]
        names, recs = rc.records(both[0][0])
        recs = np.ascontiguousarray(recs)
        recs.setflags(write=False)
        _families["tuned"] = (both[0][0], recs, list(names), [both[b % 3][0] for b in range(len(recs))],
                              [both[b % 3][1] for b in range(len(recs))])
    return _families["tuned"]


def tuned_refs(ref, b, seed=SEED):
    """(kkt_adjoint, condensed_adjoint) of instance b of tuned_cases() under its own configuration"""
    key = ("tuned", b, seed)
    if key not in _refs:
        _, recs, _, _, rcfgs = tuned_cases(ref)
        xbar, fmbar = cotangents(len(recs), rcfgs[b].n_var, seed)
        _refs[key] = (_frozen(am.kkt_adjoint(rcfgs[b], recs[b], xbar[b], fmbar[b])),
                      _frozen(am.condensed_adjoint(rcfgs[b], recs[b], xbar[b], fmbar[b])))
    return _refs[key]


# ---- affine exactness of the shipped Jacobian (test_gpu_sensitivity.test_affine_exactness_on_the_production_path's step)
AFFINE_RECORDS = [f"all_distinct_{i}" for i in range(6)] + ["lateral_30m", "mass_12.3"]
AFFINE_KEEP_MIN = 6          # how many of them must keep their active set under the step


def affine_cases(ref):
    """(MPCConfig, oracle Config, records, names, step d [B, 26]) at the paper horizon"""
    _, cfg, rcfg, recs, names = family(ref, FAMILIES[0])
    recs = recs[[names.index(n) for n in AFFINE_RECORDS]]
    d = 1e-5 * (1.0 + np.abs(recs[:, :26])) * np.random.default_rng(3).standard_normal((len(recs), 26))
    return cfg, rcfg, recs, list(AFFINE_RECORDS), d


def field_errors(got_x0, got_cfg, want_x0, want_cfg):
    """worst |err| / (1e-6 |field|_inf + 1e-12 max |all gradient entries|) over grad_x0 and the fields of grad_cfg: the bar
    of tests/test_adjoint_model.py (b) is 1 (test_gpu_adjoint._field_errors, on arrays)"""
    gall = np.abs(np.concatenate([want_x0, want_cfg])).max()
    worst = np.abs(got_x0 - want_x0).max() / (1e-6 * np.abs(want_x0).max() + 1e-12 * gall)
    for _, off, n in am.GRAD_FIELDS:
        f = want_cfg[off:off + n]
        worst = max(worst, np.abs(got_cfg[off:off + n] - f).max() / (1e-6 * np.abs(f).max() + 1e-12 * gall))
    return float(worst)


def kinds(active):
    """what a final throttle-state vector holds: a subset of {"lower", "upper", "free", "pinned"}"""
    a = np.asarray(active)
    return {k for k, s in (("lower", sm.LOWER), ("upper", sm.UPPER), ("free", sm.FREE), ("pinned", sm.PINNED)) if (a == s).any()}
