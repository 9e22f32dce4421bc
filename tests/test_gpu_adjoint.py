"""The adjoint of the solve on the GPU (vsmpc_adjoint_batch, adjoint_kernel_rt[_tuned]): gradients against
tests/adjoint_model.py (the numpy mirror and the dense-KKT route), grad_x0 against the shipped sensitivity entry, the solve
outputs against solve(), per-instance tunables, determinism, the contracts of the entry points, and PlanFunction.
Records away from the synthetic workloads and the box QP's tabled active sets: tests/test_gpu_adjoint_records.py."""
import dataclasses
from ctypes import c_void_p
from importlib import import_module

import numpy as np
import pytest

from conftest import relerr
from config_cases import NON_DEFAULT
import adjoint_model as am
from test_gpu_sensitivity import _cfgs, _records

pytestmark = pytest.mark.gpu

GUARD = 7.25e77          # guard words around output buffers
_shared = {}


def _cotangents(B, n_var, seed=5):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((B, n_var)), rng.standard_normal((B, 24))


def _field_errors(got, want_x0, want_cfg):
    """worst |err| / (1e-6 |field|_inf + 1e-12 max |all gradient entries|) over grad_x0 and the fields of grad_cfg: the bar
    of tests/test_adjoint_model.py (b) is 1"""
    gall = np.abs(np.concatenate([want_x0, want_cfg])).max()
    worst = np.abs(got["grad_x0"] - want_x0).max() / (1e-6 * np.abs(want_x0).max() + 1e-12 * gall)
    for name, off, n in am.GRAD_FIELDS:
        f = want_cfg[off:off + n]
        worst = max(worst, np.abs(got["grad_cfg"][off:off + n] - f).max() / (1e-6 * np.abs(f).max() + 1e-12 * gall))
    return worst


# the numpy mirror runs the kernel's algorithm: only rounding differs.  Measured on the device over the cases below: at
# most 3.8e-7 of the bar of test_adjoint_model.py (b) against the mirror (8.7e-4 of it against the dense route); the bar
# against the mirror is 100 times the measured value, rounded up to a power of ten.
MIRROR_BAR = 1e-4


@pytest.mark.parametrize("horizon, runtime, settings", [
    ((17, 7, 12), "never", {}), ((17, 7, 12), "never", NON_DEFAULT), ((17, 7, 12), "always", {}),
    ((20, 5, 9), "fallback", {}), ((20, 5, 9), "fallback", NON_DEFAULT), ((2, 2, 2), "fallback", {}),
    ((40, 2, 40), "fallback", {})])
def test_gradients_match_models(solver_mod, ref, synth, layout, horizon, runtime, settings):
    cfg, rcfg = _cfgs(layout, ref, horizon, **settings)
    recs = _records(layout, synth, cfg, n=1 if horizon == (40, 2, 40) else 2)
    xbar, fmbar = _cotangents(len(recs), cfg.n_var)
    m = solver_mod.BatchedVSMPC(cfg, device=0, max_batch=len(recs), runtime=runtime, adjoint=True)
    try:
        assert m.uses_runtime_kernel == (runtime != "never")
        out = m.solve_adjoint(recs, xbar, fmbar)
    finally:
        m.close()
    assert (out["status"] == layout.STATUS_SOLVED).all(), out["status"]
    assert (out["grad_cfg"][:, 31] == 0.0).all()
    checked = mirrored = 0
    for b, rec in enumerate(recs):
        key = (horizon, bool(settings), b)                    # the references: computed once, shared, left unchanged
        if key not in _shared:
            _shared[key] = (am.kkt_adjoint(rcfg, rec, xbar[b], fmbar[b]), am.condensed_adjoint(rcfg, rec, xbar[b], fmbar[b]))
        k, c = _shared[key]
        got = {"grad_x0": out["grad_x0"][b], "grad_cfg": out["grad_cfg"][b]}
        assert out["flags"][b] == c["flags"], b
        if np.array_equal(out["active"][b], c["active"]):
            e = _field_errors(got, c["grad_x0"], c["grad_cfg"])
            print(f"{horizon} {runtime} instance {b}: {e:.2e} of the bar against the mirror")
            assert e <= MIRROR_BAR, (b, e)
            mirrored += 1
        else:               # only a flagged instance may settle on another side than the mirror
            assert out["flags"][b] & layout.ADJ_DEGENERATE, b
        if out["flags"][b] & layout.ADJ_DEGENERATE and not np.array_equal(out["active"][b], k["active"]):
            continue   # a weakly or nearly active throttle may settle on either side in the two solvers
        np.testing.assert_array_equal(out["active"][b], k["active"])
        e = _field_errors(got, k["grad_x0"], k["grad_cfg"])
        print(f"{horizon} {runtime} instance {b}: {e:.2e} of the bar against the dense route")
        assert e <= 1.0, (b, e)
        checked += 1
    assert checked >= len(recs) - 1 and mirrored >= len(recs) - 1, (checked, mirrored, out["flags"])


def test_grad_x0_matches_the_sensitivity_entry(solver_mod, synth, layout):
    """dL/dX0 = dx_dx0^T xbar + dfm_dx0^T fmbar with the Jacobians the same handle ships: needs no oracle"""
    cfg = layout.paper_config()
    recs = _records(layout, synth, cfg)
    xbar, fmbar = _cotangents(len(recs), cfg.n_var, seed=6)
    m = solver_mod.BatchedVSMPC(cfg, device=0, max_batch=len(recs), sensitivity=True, adjoint=True)
    try:
        sens = m.solve_sensitivity(recs)
        out = m.solve_adjoint(recs, xbar, fmbar)
    finally:
        m.close()
    np.testing.assert_array_equal(out["active"], sens["active"])
    np.testing.assert_array_equal(out["flags"], sens["flags"])
    for b in range(len(recs)):
        want = sens["dx_dx0"][b].T @ xbar[b] + sens["dfm_dx0"][b].T @ fmbar[b]
        assert relerr(out["grad_x0"][b], want) < 1e-8, (b, relerr(out["grad_x0"][b], want))


def test_solve_outputs_unchanged(solver_mod, synth, layout):
    rcfg = layout.MPCConfig(n_iter=20, n_iter_small=5, control_horizon=9)
    recs = _records(layout, synth, rcfg)
    xbar, fmbar = _cotangents(len(recs), rcfg.n_var)
    m = solver_mod.BatchedVSMPC(rcfg, device=0, max_batch=len(recs), runtime="always", adjoint=True)
    try:                                     # runtime handle: the same phases, bit for bit
        x, fm, st, it = m.solve(recs)
        out = m.solve_adjoint(recs, xbar, fmbar)
        for k, v in (("x", x), ("first_move", fm), ("status", st), ("iters", it)):
            np.testing.assert_array_equal(out[k], v, err_msg=k)
    finally:
        m.close()
    cfg = layout.paper_config()
    recs = _records(layout, synth, cfg)
    xbar, fmbar = _cotangents(len(recs), cfg.n_var)
    tuned = solver_mod.BatchedVSMPC(cfg, device=0, max_batch=len(recs), adjoint=True)
    plain = solver_mod.BatchedVSMPC(cfg, device=0, max_batch=len(recs))
    try:                                     # tuned handle: another algorithm, to rounding, same iterations
        assert not tuned.uses_runtime_kernel
        x, fm, st, it = tuned.solve(recs)
        out = tuned.solve_adjoint(recs, xbar, fmbar)
        np.testing.assert_array_equal(out["status"], st)
        np.testing.assert_array_equal(out["iters"], it)
        for b in range(len(recs)):
            assert relerr(out["x"][b], x[b]) < 1e-12 and relerr(out["first_move"][b], fm[b]) < 1e-12, b
        for a, c in zip((x, fm, st, it), plain.solve(recs)):    # the flag does not change the plain solve
            np.testing.assert_array_equal(a, c)
    finally:
        tuned.close()
        plain.close()


def test_per_instance_tunables(solver_mod, synth, layout):
    cfg = layout.MPCConfig(n_iter=20, n_iter_small=5, control_horizon=9)
    other = dataclasses.replace(cfg, **{k: v for k, v in NON_DEFAULT.items() if k != "period_small"})
    third = dataclasses.replace(cfg, w_throttle=3e4, w_rpy=(900.0, 1100.0, 1300.0), throttle_max=80.0)
    recs = _records(layout, synth, cfg)
    B = len(recs)
    cfgs = [(cfg, other, third)[b % 3] for b in range(B)]
    xbar, fmbar = _cotangents(B, cfg.n_var)
    m = solver_mod.BatchedVSMPC(cfg, device=0, max_batch=B, runtime="fallback", adjoint=True)
    try:
        mixed = m.solve_adjoint(recs, xbar, fmbar, configs=cfgs)
        none = m.solve_adjoint(recs, xbar, fmbar)
        own = m.solve_adjoint(recs, xbar, fmbar, configs=[cfg] * B)
    finally:
        m.close()
    for k in none:                                           # rows packed from the handle's configuration == tunables=None
        np.testing.assert_array_equal(own[k], none[k], err_msg=k)
    for c in (cfg, other, third):                            # one handle per configuration, bit for bit
        sel = [b for b in range(B) if cfgs[b] is c]
        h = solver_mod.BatchedVSMPC(c, device=0, max_batch=B, runtime="fallback", adjoint=True)
        try:
            single = h.solve_adjoint(recs[sel], xbar[sel], fmbar[sel])
        finally:
            h.close()
        for k in single:
            np.testing.assert_array_equal(mixed[k][sel], single[k], err_msg=k)
    assert not np.array_equal(mixed["grad_cfg"], none["grad_cfg"])


def test_determinism(solver_mod, synth, layout):
    cfg = layout.paper_config()
    recs = _records(layout, synth, cfg)
    B = len(recs)
    xbar, fmbar = _cotangents(B, cfg.n_var)
    perm = np.random.default_rng(2).permutation(B)
    m = solver_mod.BatchedVSMPC(cfg, device=0, max_batch=B, adjoint=True)
    try:
        a = m.solve_adjoint(recs, xbar, fmbar)
        again = m.solve_adjoint(recs, xbar, fmbar)
        p = m.solve_adjoint(recs[perm], xbar[perm], fmbar[perm])
        alone = [m.solve_adjoint(recs[b:b + 1], xbar[b:b + 1], fmbar[b:b + 1]) for b in range(B)]
    finally:
        m.close()
    for k in ("grad_x0", "grad_cfg", "active", "flags", "x"):
        np.testing.assert_array_equal(again[k], a[k], err_msg=k)
        np.testing.assert_array_equal(p[k], a[k][perm], err_msg=k)
        for b in range(B):
            np.testing.assert_array_equal(alone[b][k][0], a[k][b], err_msg=k)


def test_contracts(solver_mod, synth, layout):
    import torch
    cfg = layout.MPCConfig(n_iter=20, n_iter_small=5, control_horizon=9)
    recs = _records(layout, synth, cfg)
    B = len(recs)
    xbar, fmbar = _cotangents(B, cfg.n_var)
    plain = solver_mod.BatchedVSMPC(cfg, device=0, max_batch=B, runtime="fallback")
    try:                                                     # a handle without the flag
        with pytest.raises(Exception) as e:
            plain.solve_adjoint(recs, xbar, fmbar)
        assert "unsupported" in str(e.value).lower() or "VSMPC_CREATE_ADJOINT" in str(e.value)
        assert "VSMPC_CREATE_ADJOINT" in str(e.value)
    finally:
        plain.close()
    m = solver_mod.BatchedVSMPC(cfg, device=0, max_batch=B, runtime="fallback", adjoint=True)
    try:
        lib, P = m.lib, (lambda a: a.ctypes.data_as(c_void_p))
        with pytest.raises(Exception) as e:
            m.solve_adjoint(np.concatenate([recs, recs[:1]]), np.concatenate([xbar, xbar[:1]]))
        assert "max_batch" in str(e.value)
        full = m.solve_adjoint(recs, xbar, fmbar)
        st = np.full(B, -7, dtype=np.int32)
        # NULL required arguments, batch 0
        tail = [None] * 5
        assert lib.vsmpc_adjoint_batch(m._h, None, None, P(xbar), None, B, None, None, P(st), None, *tail) == -1
        assert lib.vsmpc_adjoint_batch(m._h, P(recs), None, None, None, B, None, None, P(st), None, *tail) == -1
        assert lib.vsmpc_adjoint_batch(m._h, P(recs), None, P(xbar), None, B, None, None, None, None, *tail) == -1
        assert lib.vsmpc_adjoint_batch(m._h, P(recs), None, P(xbar), None, 0, None, None, P(st), None, *tail) == 0
        assert (st == -7).all()
        # optional outputs NULL: status only (and no fmbar)
        assert lib.vsmpc_adjoint_batch(m._h, P(recs), None, P(xbar), None, B, None, None, P(st), None, *tail) == 0
        np.testing.assert_array_equal(st, full["status"])
        # guard words around every output buffer
        sizes = {"x": m.n_var, "first_move": 24, "grad_x0": 26, "grad_cfg": layout.GRAD_SIZE}
        bufs = {k: np.full(B * n + 2, GUARD) for k, n in sizes.items()}
        ints = {k: np.full(B * n + 2, -7, dtype=np.int32) for k, n in (("status", 1), ("iters", 1), ("active", m.n_v), ("flags", 1))}
        inner = lambda a: c_void_p(a.ctypes.data + a.itemsize)
        assert lib.vsmpc_adjoint_batch(m._h, P(recs), None, P(xbar), P(fmbar), B, inner(bufs["x"]), inner(bufs["first_move"]),
                                       inner(ints["status"]), inner(ints["iters"]), inner(bufs["grad_x0"]),
                                       inner(bufs["grad_cfg"]), inner(ints["active"]), inner(ints["flags"]), None) == 0
        for k, a in list(bufs.items()) + list(ints.items()):
            assert a[0] == a[-1] and a[0] in (GUARD, -7), k
            np.testing.assert_array_equal(a[1:-1].reshape(full[k].shape), full[k], err_msg=k)
        # an unsolved instance (a non-finite record: status Numerical; the iteration cap is not settable through the API)
        # and a non-finite cotangent, each in its own instance only
        bad_rec, bad_bar = recs.copy(), xbar.copy()
        bad_rec[1, layout.IN_MASS] = np.nan
        bad_bar[2, 100] = np.inf
        out = m.solve_adjoint(bad_rec, bad_bar, fmbar)
        assert out["status"][1] != layout.STATUS_SOLVED and out["flags"][1] == layout.ADJ_UNSOLVED
        assert not out["grad_x0"][1].any() and not out["grad_cfg"][1].any()
        assert np.isnan(out["grad_x0"][2]).all() and np.isnan(out["grad_cfg"][2, :31]).all() and out["grad_cfg"][2, 31] == 0.0
        for b in (0, 3, 4, 5, 6, 7):
            np.testing.assert_array_equal(out["grad_x0"][b], full["grad_x0"][b])
            np.testing.assert_array_equal(out["grad_cfg"][b], full["grad_cfg"][b])
        # device entry == host entry, bit for bit
        dev = torch.device("cuda:0")
        f64 = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)
        i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)
        t = {"x": f64(B, m.n_var), "first_move": f64(B, 24), "status": i32(B), "iters": i32(B), "grad_x0": f64(B, 26),
             "grad_cfg": f64(B, layout.GRAD_SIZE), "active": i32(B, m.n_v), "flags": i32(B)}
        m.solve_adjoint_device(torch.from_numpy(recs).to(dev), None, torch.from_numpy(xbar).to(dev),
                               torch.from_numpy(fmbar).to(dev), t["x"], t["first_move"], t["status"], t["iters"],
                               t["grad_x0"], t["grad_cfg"], t["active"], t["flags"])
        torch.cuda.synchronize()
        for k, v in t.items():
            np.testing.assert_array_equal(v.cpu().numpy(), full[k], err_msg=k)
    finally:
        m.close()


def test_host_entry_over_two_chunks(solver_mod, synth, layout):
    """more instances than one chunk of the host entry (256), from pageable and from pinned buffers"""
    import torch
    cfg = layout.MPCConfig(n_iter=2, n_iter_small=2, control_horizon=2)
    B = 300
    recs = np.concatenate([synth.make_batch(cfg, B // 2, workload=w, first_index=3) for w in ("hover", "takeoff")])
    xbar, fmbar = _cotangents(B, cfg.n_var)
    m = solver_mod.BatchedVSMPC(cfg, device=0, max_batch=B, runtime="fallback", adjoint=True)
    try:
        whole = m.solve_adjoint(recs, xbar, fmbar)
        parts = [m.solve_adjoint(recs[s], xbar[s], fmbar[s]) for s in (slice(0, 256), slice(256, B))]
        pin = [torch.from_numpy(a).pin_memory().numpy() for a in (recs, xbar, fmbar)]
        pinned = m.solve_adjoint(*pin)
    finally:
        m.close()
    for k in whole:
        np.testing.assert_array_equal(whole[k], np.concatenate([p[k] for p in parts]), err_msg=k)
        np.testing.assert_array_equal(pinned[k], whole[k], err_msg=k)


def test_plan_function(solver_mod, synth, layout):
    import torch
    ag = import_module(solver_mod.__name__.rsplit(".", 1)[0] + ".autograd")
    cfg = layout.paper_config()
    recs = _records(layout, synth, cfg)
    B = len(recs)
    c, d = _cotangents(B, cfg.n_var, seed=8)
    dev = torch.device("cuda:0")
    m = solver_mod.BatchedVSMPC(cfg, device=0, max_batch=B, adjoint=True)
    try:
        d_recs = torch.from_numpy(recs).to(dev)
        x0 = d_recs[:, :26].clone().requires_grad_(True)
        gains = torch.from_numpy(np.tile(ag.gains_of(cfg), (B, 1))).to(dev).requires_grad_(True)
        info = {}
        x, fm, status = ag.plan(m, d_recs, x0, gains, info)
        assert (status.cpu().numpy() == layout.STATUS_SOLVED).all()
        loss = (torch.from_numpy(c).to(dev) * x).sum() + (torch.from_numpy(d).to(dev) * fm).sum()
        loss.backward()
        want = m.solve_adjoint(recs, c, d, configs=[cfg] * B)
        np.testing.assert_array_equal(x0.grad.cpu().numpy(), want["grad_x0"])
        np.testing.assert_array_equal(gains.grad.cpu().numpy(), want["grad_cfg"])
        np.testing.assert_array_equal(info["flags"].cpu().numpy(), want["flags"])
        with pytest.raises(ValueError):
            ag.plan(m, d_recs.clone().requires_grad_(True), x0, gains)
        # without gains: the handle's configuration, the tuned kernel in the forward pass
        x0b = d_recs[:, :26].clone().requires_grad_(True)
        xb, fmb, _ = ag.plan(m, d_recs, x0b)
        ((torch.from_numpy(c).to(dev) * xb).sum() + (torch.from_numpy(d).to(dev) * fmb).sum()).backward()
        np.testing.assert_array_equal(x0b.grad.cpu().numpy(), m.solve_adjoint(recs, c, d)["grad_x0"])
        # one step of gradient descent on w_throttle lowers a quadratic loss on the first-move throttle
        target = torch.full((B, 4), 50.0, dtype=torch.float64, device=dev)

        def throttle_loss(g):
            _, fmv, _ = ag.plan(m, d_recs, d_recs[:, :26].clone(), g)
            return ((fmv[:, layout.FM_THROTTLE:layout.FM_THROTTLE + 4] - target) ** 2).sum(dim=1)

        g0 = gains.detach().clone().requires_grad_(True)
        before = throttle_loss(g0)
        before.sum().backward()
        gw = g0.grad[:, layout.GRAD_W_THROTTLE]
        assert (gw != 0).any()
        step = g0.detach().clone()
        # a step that changes w_throttle by at most 5 % (the loss is smooth in the weight while the active set holds)
        step[:, layout.GRAD_W_THROTTLE] -= 0.05 * cfg.w_throttle * gw / gw.abs().max()
        after = throttle_loss(step)
        moved = gw.abs() > 1e-6 * gw.abs().max()
        assert (after[moved] < before[moved]).all(), (before, after)
    finally:
        m.close()
