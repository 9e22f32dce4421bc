"""The instances the record adjoint (adjoint_record_kernel_rt[_tuned], tests/adjoint_record_model.py) is held to, with their
CPU references (plain helper module, imported by tests/test_adjoint_record_model.py and tests/test_gpu_adjoint_record.py).

The families, records and cotangents are derivative_cases' (the 80 instances the adjoint kernels are held to); on top:
  DENSE      the instances compared with the dense route on the GPU: the five (6, 2, 3) records that are also compared with
             central differences of the oracle's solve, one instance per table, one hold record at the paper horizon
  FD         the instances compared with central differences of vsmpc_ref.solve_instance
  EDGE       (2, 2, 2) -- one throttle block, a window of one column -- and (40, 2, 40), the largest horizon
  tuned      derivative_cases.tuned_cases: (20, 5, 9), instance b under configuration b % 3

Every reference is computed once per process, keyed by instance, and never written to.
"""
import numpy as np

import adjoint_record_model as arm
import config_cases as cc
import derivative_cases as dc
import record_cases as rc

FD = [("records_6_2_3", b) for b in (0, 3, 7, 12, 19)] + [("shrinking", 0), ("H21_box", 0)]
DENSE = [("records_6_2_3", b) for b in (0, 3, 7, 12, 19)] + [(t, 0) for t in dc.TABLES] + [("records_17_7_12", 1)]
EDGE = ((2, 2, 2), (40, 2, 40))
TUNED_DENSE = (0, 1, 2, 3, 4, 5)            # instances of tuned_cases() compared with the dense route: each configuration twice

_refs = {}
_edge = {}


def instance(ref, name, b):
    """(oracle Config, record, xbar, fmbar) of instance b of a family of derivative_cases"""
    _, _, rcfg, recs, _ = dc.family(ref, name)
    xbar, fmbar = dc.cotangents(len(recs), rcfg.n_var)
    return rcfg, recs[b], xbar[b], fmbar[b]


def _cached(key, make):
    if key not in _refs:
        _refs[key] = dc._frozen(make())
    return _refs[key]


def mirror(ref, name, b):
    return _cached(("mirror", name, b), lambda: arm.condensed_record_adjoint(*instance(ref, name, b)))


def dense(ref, name, b, model=False):
    return _cached(("dense", name, b, model), lambda: arm.kkt_record_adjoint(*instance(ref, name, b), model=model))


def edge(ref, horizon):
    """(MPCConfig, oracle Config, records, xbar, fmbar) of an edge horizon: all-distinct records, a released and a held one
    at (2, 2, 2), one at (40, 2, 40)"""
    if horizon not in _edge:
        cfg, rcfg = cc.configs(ref, horizon, {})
        _, recs = rc.records(cfg)
        recs = np.ascontiguousarray(recs[:1] if horizon == (40, 2, 40) else recs[:2])
        recs.setflags(write=False)
        xbar, fmbar = dc.cotangents(len(recs), rcfg.n_var)
        _edge[horizon] = (cfg, rcfg, recs, xbar, fmbar)
    return _edge[horizon]


def edge_mirror(ref, horizon, b):
    _, rcfg, recs, xbar, fmbar = edge(ref, horizon)
    return _cached(("mirror", horizon, b), lambda: arm.condensed_record_adjoint(rcfg, recs[b], xbar[b], fmbar[b]))


def edge_dense(ref, horizon, b):
    _, rcfg, recs, xbar, fmbar = edge(ref, horizon)
    return _cached(("dense", horizon, b), lambda: arm.kkt_record_adjoint(rcfg, recs[b], xbar[b], fmbar[b]))


def tuned_instance(ref, b):
    _, recs, _, _, rcfgs = dc.tuned_cases(ref)
    xbar, fmbar = dc.cotangents(len(recs), rcfgs[b].n_var)
    return rcfgs[b], recs[b], xbar[b], fmbar[b]


def tuned_mirror(ref, b):
    return _cached(("mirror", "tuned", b), lambda: arm.condensed_record_adjoint(*tuned_instance(ref, b)))


def tuned_dense(ref, b):
    return _cached(("dense", "tuned", b), lambda: arm.kkt_record_adjoint(*tuned_instance(ref, b)))
