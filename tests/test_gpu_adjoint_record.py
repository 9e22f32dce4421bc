"""The adjoint of the record on the GPU (vsmpc_adjoint_record_batch, adjoint_record_kernel_rt[_tuned]): gradients to every
record entry and to the linearisation against tests/adjoint_record_model.py (the numpy mirror on all 80 instances of
derivative_cases, the dense route on a subset), the adjoint entry's outputs bit for bit, the edge horizons, per-instance
tunables, the failure inputs, optional outputs and guard words, determinism, chunking, the create flag, and PlanFunction
with a differentiable record.  The references are computed once per process (tests/adjoint_record_cases.py)."""
from ctypes import c_void_p
from importlib import import_module

import numpy as np
import pytest

import adjoint_record_cases as cases
import adjoint_record_model as arm
import config_cases as cc
import derivative_cases as dc
import record_cases as rc

pytestmark = pytest.mark.gpu

GUARD = 7.25e77          # guard words around output buffers
# The mirror runs the kernel's recursions: only rounding and summation order differ.  1e-4 of the bar of
# test_adjoint_record_model.py (b), the allowance the adjoint kernels have against their mirror (test_gpu_adjoint.MIRROR_BAR).
MIRROR_BAR = 1e-4
ADJOINT_KEYS = ("x", "first_move", "status", "iters", "grad_x0", "grad_cfg", "active", "flags")
_runs = {}


def _model_errors(got, want):
    """worst block error of grad_model in units of 1e-6 |block|_inf + 1e-12 max |grad_model|"""
    gall = np.abs(want).max()
    worst = 0.0
    for lo, hi in ((arm.GM_A, arm.GM_BJ), (arm.GM_BJ, arm.GM_BT), (arm.GM_BT, arm.GM_C), (arm.GM_C, arm.GRAD_MODEL_SIZE)):
        w = want[lo:hi]
        worst = max(worst, float(np.abs(got[lo:hi] - w).max() / (1e-6 * np.abs(w).max() + 1e-12 * gall)))
    return worst


def _family_run(solver_mod, ref, name):
    """(outputs of solve_adjoint_record, outputs of solve_adjoint) of a family on one handle: computed once"""
    if name not in _runs:
        _, cfg, rcfg, recs, _ = dc.family(ref, name)
        xbar, fmbar = dc.cotangents(len(recs), rcfg.n_var)
        m = solver_mod.BatchedVSMPC(cfg, device=0, max_batch=len(recs), runtime=dc.runtime_of(cfg), adjoint_record=True)
        try:
            assert m.uses_runtime_kernel == (dc.runtime_of(cfg) != "never")
            _runs[name] = (m.solve_adjoint_record(recs, xbar, fmbar), m.solve_adjoint(recs, xbar, fmbar))
        finally:
            m.close()
    return _runs[name]


def _against_mirror(layout, rcfg, out, b, c):
    """error of instance b against the mirror in units of the bar, or None where a flagged instance settled elsewhere"""
    assert out["status"][b] == layout.STATUS_SOLVED and c["solved"], b
    if not np.array_equal(out["active"][b], c["active"]):
        assert out["flags"][b] & layout.ADJ_DEGENERATE, b
        return None
    return max(arm.field_errors(rcfg, out["grad_in"][b], c["grad_in"]), _model_errors(out["grad_model"][b], c["grad_model"]))


@pytest.mark.parametrize("name", dc.FAMILIES)
def test_all_instances_match_the_mirror(solver_mod, ref, layout, name):
    _, cfg, rcfg, recs, names = dc.family(ref, name)
    out, adj = _family_run(solver_mod, ref, name)
    for k in ADJOINT_KEYS:                                   # the adjoint entry's outputs, bit for bit
        np.testing.assert_array_equal(out[k], adj[k], err_msg=k)
    np.testing.assert_array_equal(out["grad_in"][:, :26], out["grad_x0"])
    assert out["grad_in"].shape == (len(recs), cfg.n_in) and out["grad_model"].shape == (len(recs), layout.GRAD_MODEL_SIZE)
    checked, worst = 0, 0.0
    for b in range(len(recs)):
        e = _against_mirror(layout, rcfg, out, b, cases.mirror(ref, name, b))
        if e is None:
            continue
        assert e <= MIRROR_BAR, (names[b], e)
        worst, checked = max(worst, e), checked + 1
        for i in arm.dead(rcfg) + [layout.IN_HOLD]:
            assert out["grad_in"][b, i] == 0.0 and not np.signbit(out["grad_in"][b, i]), (names[b], i)
    print(f"{name}: {checked} of {len(recs)} instances, worst {worst:.2e} of the bar against the mirror")
    assert checked >= len(recs) - 1


@pytest.mark.parametrize("name, b", cases.DENSE)
def test_subset_matches_the_dense_route(solver_mod, ref, layout, name, b):
    rcfg = cases.instance(ref, name, b)[0]
    out, _ = _family_run(solver_mod, ref, name)
    k = cases.dense(ref, name, b)
    assert out["status"][b] == layout.STATUS_SOLVED
    if out["flags"][b] & layout.ADJ_DEGENERATE and not np.array_equal(out["active"][b], k["active"]):
        pytest.fail("a subset instance is degenerate: choose another one")
    np.testing.assert_array_equal(out["active"][b], k["active"])
    e = arm.field_errors(rcfg, out["grad_in"][b], k["grad_in"])
    print(f"{name}[{b}]: {e:.2e} of the bar against the dense route")
    assert e <= 1.0, (name, b, e)


@pytest.mark.parametrize("horizon", cases.EDGE)
def test_edge_horizons(solver_mod, ref, layout, horizon):
    """(2, 2, 2): one throttle block, a window of one column; (40, 2, 40): the LDS limit, without and with tunables"""
    cfg, rcfg, recs, xbar, fmbar = cases.edge(ref, horizon)
    m = solver_mod.BatchedVSMPC(cfg, device=0, max_batch=len(recs), runtime="fallback", adjoint_record=True)
    try:
        out = m.solve_adjoint_record(recs, xbar, fmbar)
        own = m.solve_adjoint_record(recs, xbar, fmbar, configs=[cfg] * len(recs))
    finally:
        m.close()
    for k in out:
        np.testing.assert_array_equal(own[k], out[k], err_msg=k)
    for b in range(len(recs)):
        e = _against_mirror(layout, rcfg, out, b, cases.edge_mirror(ref, horizon, b))
        print(f"{horizon}[{b}]: {e} of the bar against the mirror")
        assert e is not None and e <= MIRROR_BAR, (horizon, b, e)
    if horizon == (2, 2, 2):
        assert (out["grad_in"][:, layout.IN_XREF:] != 0.0).all()       # the one column is live


def test_per_instance_tunables(solver_mod, ref, layout):
    """adjoint_record_kernel_rt_tuned: instance b under configuration b % 3, against both routes under that configuration"""
    hcfg, recs, names, cfgs, rcfgs = dc.tuned_cases(ref)
    B = len(recs)
    xbar, fmbar = dc.cotangents(B, rcfgs[0].n_var)
    m = solver_mod.BatchedVSMPC(hcfg, device=0, max_batch=B, runtime="fallback", adjoint_record=True)
    try:
        out = m.solve_adjoint_record(recs, xbar, fmbar, configs=cfgs)
        adj = m.solve_adjoint(recs, xbar, fmbar, configs=cfgs)
        none = m.solve_adjoint_record(recs, xbar, fmbar)
    finally:
        m.close()
    for k in ADJOINT_KEYS:
        np.testing.assert_array_equal(out[k], adj[k], err_msg=k)
    assert not np.array_equal(out["grad_in"], none["grad_in"])
    checked = 0
    for b in range(B):
        e = _against_mirror(layout, rcfgs[b], out, b, cases.tuned_mirror(ref, b))
        if e is not None:
            assert e <= MIRROR_BAR, (names[b], e)
            checked += 1
    assert checked >= B - 1
    for b in cases.TUNED_DENSE:
        k = cases.tuned_dense(ref, b)
        np.testing.assert_array_equal(out["active"][b], k["active"])
        e = arm.field_errors(rcfgs[b], out["grad_in"][b], k["grad_in"])
        print(f"configuration {b % 3}, {names[b]}: {e:.2e} of the bar against the dense route")
        assert e <= 1.0, (b, e)


def test_without_the_jet_dynamics(solver_mod, ref, layout):
    cfg, rcfg = cc.configs(ref, (6, 2, 3), {"use_jet_dynamic": False})
    _, recs = rc.records(cfg)
    recs = recs[[0, 3]]
    xbar, fmbar = dc.cotangents(len(recs), rcfg.n_var)
    m = solver_mod.BatchedVSMPC(cfg, device=0, max_batch=len(recs), runtime="fallback", adjoint_record=True)
    try:
        out = m.solve_adjoint_record(recs, xbar, fmbar)
    finally:
        m.close()
    for b in range(len(recs)):
        c = arm.condensed_record_adjoint(rcfg, recs[b], xbar[b], fmbar[b])
        assert _against_mirror(layout, rcfg, out, b, c) <= MIRROR_BAR
        for f, off, n in arm.fields(rcfg):
            if f in arm.JET_FIELDS:
                assert not out["grad_in"][b, off:off + n].any(), f
        assert out["grad_in"][b, layout.IN_UPREV:layout.IN_UPREV + 4].any()


def _small(ref):
    """(MPCConfig, oracle Config, records, xbar, fmbar) at (6, 2, 3)"""
    _, cfg, rcfg, recs, _ = dc.family(ref, "records_6_2_3")
    xbar, fmbar = dc.cotangents(len(recs), rcfg.n_var)
    return cfg, rcfg, recs, xbar, fmbar


def test_failure_inputs(solver_mod, ref, layout):
    cfg, rcfg, recs, xbar, fmbar = _small(ref)
    full, _ = _family_run(solver_mod, ref, "records_6_2_3")
    bad_rec, bad_bar, bad_fm = recs.copy(), xbar.copy(), fmbar.copy()
    bad_rec[1, layout.IN_MASS] = np.nan
    bad_bar[2, 100] = np.inf
    bad_fm[4, 3] = np.nan
    m = solver_mod.BatchedVSMPC(cfg, device=0, max_batch=len(recs), runtime="fallback", adjoint_record=True)
    try:
        out = m.solve_adjoint_record(bad_rec, bad_bar, bad_fm)
    finally:
        m.close()
    assert out["status"][1] != layout.STATUS_SOLVED and out["flags"][1] == layout.ADJ_UNSOLVED
    assert not out["grad_in"][1].any() and not out["grad_model"][1].any()
    assert not np.signbit(out["grad_in"][1]).any() and not np.signbit(out["grad_model"][1]).any()
    for b in (2, 4):
        assert np.isnan(out["grad_in"][b]).all() and np.isnan(out["grad_model"][b]).all(), b
    for b in [i for i in range(len(recs)) if i not in (1, 2, 4)]:
        for k in ("grad_in", "grad_model", "grad_x0", "grad_cfg"):
            np.testing.assert_array_equal(out[k][b], full[k][b], err_msg=f"{k}[{b}]")


def test_optional_outputs_and_guard_words(solver_mod, ref, layout):
    cfg, rcfg, recs, xbar, fmbar = _small(ref)
    full, _ = _family_run(solver_mod, ref, "records_6_2_3")
    B = len(recs)
    m = solver_mod.BatchedVSMPC(cfg, device=0, max_batch=B, runtime="fallback", adjoint_record=True)
    try:
        lib, P = m.lib, (lambda a: a.ctypes.data_as(c_void_p))
        inner = lambda a: c_void_p(a.ctypes.data + a.itemsize)
        st = np.full(B, -7, dtype=np.int32)
        none8 = [None] * 8
        # required arguments, batch 0, batch too large: the adjoint entry's rules
        assert lib.vsmpc_adjoint_record_batch(m._h, None, None, P(xbar), None, B, None, None, P(st), *none8) == -1
        assert lib.vsmpc_adjoint_record_batch(m._h, P(recs), None, None, None, B, None, None, P(st), *none8) == -1
        assert lib.vsmpc_adjoint_record_batch(m._h, P(recs), None, P(xbar), None, B, None, None, None, *none8) == -1
        assert lib.vsmpc_adjoint_record_batch(m._h, P(recs), None, P(xbar), None, 0, None, None, P(st), *none8) == 0
        assert (st == -7).all()
        with pytest.raises(Exception) as e:
            m.solve_adjoint_record(np.concatenate([recs, recs[:1]]), np.concatenate([xbar, xbar[:1]]))
        assert "max_batch" in str(e.value)
        # each of the two outputs alone, everything else NULL but the status
        gin, gmodel = np.full(B * cfg.n_in + 2, GUARD), np.full(B * layout.GRAD_MODEL_SIZE + 2, GUARD)
        assert lib.vsmpc_adjoint_record_batch(m._h, P(recs), None, P(xbar), P(fmbar), B, None, None, P(st), None, None, None,
                                              None, None, inner(gin), None, None) == 0
        assert lib.vsmpc_adjoint_record_batch(m._h, P(recs), None, P(xbar), P(fmbar), B, None, None, P(st), None, None, None,
                                              None, None, None, inner(gmodel), None) == 0
        np.testing.assert_array_equal(st, full["status"])
        for a, k in ((gin, "grad_in"), (gmodel, "grad_model")):
            assert a[0] == GUARD and a[-1] == GUARD, k
            np.testing.assert_array_equal(a[1:-1].reshape(full[k].shape), full[k], err_msg=k)
        # guard words around every output at once
        sizes = {"x": m.n_var, "first_move": 24, "grad_x0": 26, "grad_cfg": layout.GRAD_SIZE, "grad_in": cfg.n_in,
                 "grad_model": layout.GRAD_MODEL_SIZE}
        bufs = {k: np.full(B * n + 2, GUARD) for k, n in sizes.items()}
        ints = {k: np.full(B * n + 2, -7, dtype=np.int32)
                for k, n in (("status", 1), ("iters", 1), ("active", m.n_v), ("flags", 1))}
        assert lib.vsmpc_adjoint_record_batch(
            m._h, P(recs), None, P(xbar), P(fmbar), B, inner(bufs["x"]), inner(bufs["first_move"]), inner(ints["status"]),
            inner(ints["iters"]), inner(bufs["grad_x0"]), inner(bufs["grad_cfg"]), inner(ints["active"]), inner(ints["flags"]),
            inner(bufs["grad_in"]), inner(bufs["grad_model"]), None) == 0
        for k, a in list(bufs.items()) + list(ints.items()):
            assert a[0] == a[-1] and a[0] in (GUARD, -7), k
            np.testing.assert_array_equal(a[1:-1].reshape(full[k].shape), full[k], err_msg=k)
    finally:
        m.close()


def test_determinism(solver_mod, ref, layout):
    cfg, rcfg, recs, xbar, fmbar = _small(ref)
    a, _ = _family_run(solver_mod, ref, "records_6_2_3")
    B = len(recs)
    perm = np.random.default_rng(2).permutation(B)
    m = solver_mod.BatchedVSMPC(cfg, device=0, max_batch=B, runtime="fallback", adjoint_record=True)
    try:
        again = m.solve_adjoint_record(recs, xbar, fmbar)
        p = m.solve_adjoint_record(recs[perm], xbar[perm], fmbar[perm])
        alone = [m.solve_adjoint_record(recs[b:b + 1], xbar[b:b + 1], fmbar[b:b + 1]) for b in (0, 3, 19)]
    finally:
        m.close()
    for k in a:
        np.testing.assert_array_equal(again[k], a[k], err_msg=k)
        np.testing.assert_array_equal(p[k], a[k][perm], err_msg=k)
        for one, b in zip(alone, (0, 3, 19)):
            np.testing.assert_array_equal(one[k][0], a[k][b], err_msg=k)


def test_host_entry_over_two_chunks_equals_the_device_entry(solver_mod, synth, layout):
    """300 instances: more than one chunk of the host entry (256), against one launch of the device entry"""
    import torch
    cfg = layout.MPCConfig(n_iter=2, n_iter_small=2, control_horizon=2)
    B = 300
    recs = np.concatenate([synth.make_batch(cfg, B // 2, workload=w, first_index=3) for w in ("hover", "takeoff")])
    xbar, fmbar = dc.cotangents(B, cfg.n_var)
    dev = torch.device("cuda:0")
    f64 = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)
    m = solver_mod.BatchedVSMPC(cfg, device=0, max_batch=B, runtime="fallback", adjoint_record=True)
    try:
        whole = m.solve_adjoint_record(recs, xbar, fmbar)
        t = {"x": f64(B, m.n_var), "first_move": f64(B, 24), "status": i32(B), "iters": i32(B), "grad_x0": f64(B, 26),
             "grad_cfg": f64(B, layout.GRAD_SIZE), "active": i32(B, m.n_v), "flags": i32(B), "grad_in": f64(B, cfg.n_in),
             "grad_model": f64(B, layout.GRAD_MODEL_SIZE)}
        m.solve_adjoint_record_device(torch.from_numpy(recs).to(dev), None, torch.from_numpy(xbar).to(dev),
                                      torch.from_numpy(fmbar).to(dev), *[t[k] for k in ADJOINT_KEYS], t["grad_in"], t["grad_model"])
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy() for k, v in t.items()}
    finally:
        m.close()
    assert (whole["status"] == layout.STATUS_SOLVED).all() and whole["grad_in"].any(axis=1).all()
    for k in whole:
        np.testing.assert_array_equal(got[k], whole[k], err_msg=k)


def test_without_the_create_flag(solver_mod, ref, layout):
    cfg, rcfg, recs, xbar, fmbar = _small(ref)
    for kw in ({}, {"adjoint": True}):
        plain = solver_mod.BatchedVSMPC(cfg, device=0, max_batch=len(recs), runtime="fallback", **kw)
        try:
            with pytest.raises(Exception) as e:
                plain.solve_adjoint_record(recs, xbar, fmbar)
            assert "VSMPC_CREATE_ADJOINT_RECORD" in str(e.value) and "(-2)" in str(e.value)
        finally:
            plain.close()


def _plan_setup(solver_mod, ref):
    import torch
    ag = import_module(solver_mod.__name__.rsplit(".", 1)[0] + ".autograd")
    _, cfg, rcfg, recs, names = dc.family(ref, "records_17_7_12")
    return torch, ag, cfg, rcfg, recs, names, torch.device("cuda:0")


def test_plan_function_differentiates_the_record(solver_mod, ref, layout):
    torch, ag, cfg, rcfg, recs, names, dev = _plan_setup(solver_mod, ref)
    B = len(recs)
    c, d = dc.cotangents(B, cfg.n_var, seed=8)
    m = solver_mod.BatchedVSMPC(cfg, device=0, max_batch=B, adjoint_record=True)
    try:
        d_recs = torch.from_numpy(recs.copy()).to(dev).requires_grad_(True)
        x0 = d_recs.detach()[:, :26].clone().requires_grad_(True)
        gains = torch.from_numpy(np.tile(ag.gains_of(cfg), (B, 1))).to(dev).requires_grad_(True)
        info = {}
        x, fm, status = ag.plan(m, d_recs, x0, gains, info)
        ((torch.from_numpy(c).to(dev) * x).sum() + (torch.from_numpy(d).to(dev) * fm).sum()).backward()
        want = m.solve_adjoint_record(recs, c, d, configs=[cfg] * B)
        gin = want["grad_in"].copy()
        gin[:, :26] = 0.0                                    # x0 replaced these columns in the forward pass
        np.testing.assert_array_equal(d_recs.grad.cpu().numpy(), gin)
        np.testing.assert_array_equal(x0.grad.cpu().numpy(), want["grad_x0"])
        np.testing.assert_array_equal(gains.grad.cpu().numpy(), want["grad_cfg"])
        np.testing.assert_array_equal(info["flags"].cpu().numpy(), want["flags"])
        assert gin.any(axis=1).all()
    finally:
        m.close()


def test_gradient_step_on_the_window_lowers_a_loss_on_the_planned_com(solver_mod, ref, layout):
    """A quadratic loss on the planned CoM, targets 0.2 m above the plan.  One step along -dL/d window whose largest entry is
    1 % of the window's largest entry and at most 0.05 (within the 5 % the step may take; the plan follows the window with a
    gain below one, so a step of 5 cm cannot overshoot a target 0.2 m away) lowers it wherever the gradient is not negligible."""
    torch, ag, cfg, rcfg, recs, names, dev = _plan_setup(solver_mod, ref)
    B, N = len(recs), cfg.n_iter
    m = solver_mod.BatchedVSMPC(cfg, device=0, max_batch=B, adjoint_record=True)
    try:
        base = torch.from_numpy(recs.copy()).to(dev)
        x0 = base[:, :26].clone()
        target = None

        def com_loss(r):
            nonlocal target
            x, _, status = ag.plan(m, r, x0)
            com = x[:, :26 * (N + 1)].reshape(B, N + 1, 26)[:, 1:, 0:3]
            if target is None:
                target = com.detach() + torch.tensor([0.0, 0.0, 0.2], dtype=torch.float64, device=dev)
            return ((com - target) ** 2).sum(dim=(1, 2)), status

        r0 = base.clone().requires_grad_(True)
        before, status = com_loss(r0)
        before.sum().backward()
        g = r0.grad[:, layout.IN_XREF:]
        assert not r0.grad[:, :26].any()
        gmax = g.abs().amax(dim=1)
        solved = torch.from_numpy(np.asarray(status.cpu().numpy() == layout.STATUS_SOLVED)).to(dev)
        moved = solved & (gmax > 1e-6 * gmax.max())
        assert int(moved.sum()) >= B // 2, (gmax, names)
        step = base.clone()
        scale = torch.clamp(0.01 * base[:, layout.IN_XREF:].abs().amax(dim=1), max=0.05)
        step[:, layout.IN_XREF:] -= (scale / torch.where(gmax > 0, gmax, torch.ones_like(gmax)))[:, None] * g
        after, _ = com_loss(step)
        assert (after[moved] < before[moved]).all(), (before, after, names)
    finally:
        m.close()
