"""Sensitivities of the solution to X0 on the GPU (vsmpc_sensitivity_batch, sens_kernel_rt): Jacobians against
tests/sensitivity_model.py, the solve outputs against solve(), affine exactness on the production path, the degeneracy
flag, and the contracts of the entry points.
Records away from the synthetic workloads and the box QP's tabled active sets: tests/test_gpu_sensitivity_records.py."""
import dataclasses
from ctypes import c_void_p

import numpy as np
import pytest

from conftest import relerr
from config_cases import NON_DEFAULT
import sensitivity_model as sm

pytestmark = pytest.mark.gpu



def _cfgs(layout, ref, horizon, **settings):
    kw = dict(n_iter=horizon[0], n_iter_small=horizon[1], control_horizon=horizon[2], **settings)
    return layout.MPCConfig(**kw), ref.Config(**kw)


def _records(layout, synth, cfg, n=2):
    """hover, take-off, saturated throttles on a free tick, the hold on, zero Lambda (no joint authority)"""
    hover = synth.make_batch(cfg, n, workload="hover", first_index=5)
    takeoff = synth.make_batch(cfg, n, workload="takeoff", first_index=5)
    sat = synth.make_batch(cfg, n, workload="hover", first_index=40)
    sat[:, layout.IN_HOLD] = 0.0
    sat[:, layout.IN_XREF + 2::12] += 30.0
    sat[:, 22] = sat[:, 2] - sat[:, layout.IN_XREF + 2]
    held = takeoff[:1].copy()
    held[:, layout.IN_HOLD] = 1.0
    zl = hover[:1].copy()
    zl[:, layout.IN_LLIN:layout.IN_LLIN + 48] = 0.0
    return np.concatenate([hover, takeoff, sat, held, zl])


@pytest.mark.parametrize("horizon, runtime, settings", [
    ((17, 7, 12), "never", {}), ((34, 14, 24), "never", {}), ((20, 5, 9), "fallback", {}), ((40, 2, 40), "fallback", {}),
    ((17, 7, 12), "never", NON_DEFAULT), ((20, 5, 9), "fallback", NON_DEFAULT)])
def test_jacobians_match_model(solver_mod, ref, synth, layout, horizon, runtime, settings):
    cfg, rcfg = _cfgs(layout, ref, horizon, **settings)
    recs = _records(layout, synth, cfg, n=1 if horizon == (40, 2, 40) else 2)
    m = solver_mod.BatchedVSMPC(cfg, device=0, max_batch=len(recs), runtime=runtime, sensitivity=True)
    try:
        assert m.uses_runtime_kernel == (runtime != "never")
        out = m.solve_sensitivity(recs)
    finally:
        m.close()
    assert (out["status"] == layout.STATUS_SOLVED).all(), out["status"]
    checked = 0
    for b, rec in enumerate(recs):
        x, J, active = sm.kkt_jacobian(rcfg, rec)
        if out["flags"][b] & layout.SENS_DEGENERATE and not np.array_equal(out["active"][b], active):
            continue   # a weakly or nearly active throttle may settle on either side in the two solvers
        # (flagged instances with the same final active set: the same affine piece, so the same Jacobian -- at (40, 2, 40)
        # the far throttle blocks of every record are weakly active)
        np.testing.assert_array_equal(out["active"][b], active)
        assert relerr(out["dx_dx0"][b], J) < 1e-8, (b, relerr(out["dx_dx0"][b], J))
        dfm = sm.first_move_jacobian(rcfg, x[rcfg.off_throttle:rcfg.off_throttle + 4], J)
        assert relerr(out["dfm_dx0"][b], dfm) < 1e-8, (b, relerr(out["dfm_dx0"][b], dfm))
        assert out["flags"][b] == sm.condensed_jacobian(rcfg, rec)["flags"], b
        checked += 1
    assert checked >= len(recs) - 1, out["flags"]


def test_solve_outputs_unchanged(solver_mod, synth, layout):
    rcfg = layout.MPCConfig(n_iter=20, n_iter_small=5, control_horizon=9)
    recs = _records(layout, synth, rcfg, n=3)
    m = solver_mod.BatchedVSMPC(rcfg, device=0, max_batch=len(recs), runtime="always", sensitivity=True)
    try:                                     # runtime handle: the same kernel body, bit for bit
        x, fm, st, it = m.solve(recs)
        out = m.solve_sensitivity(recs)
        for k, v in (("x", x), ("first_move", fm), ("status", st), ("iters", it)):
            np.testing.assert_array_equal(out[k], v, err_msg=k)
    finally:
        m.close()
    cfg = layout.paper_config()
    recs = _records(layout, synth, cfg, n=3)
    tuned = solver_mod.BatchedVSMPC(cfg, device=0, max_batch=len(recs), sensitivity=True)
    plain = solver_mod.BatchedVSMPC(cfg, device=0, max_batch=len(recs))
    try:                                     # tuned handle: another algorithm, to rounding, same iterations
        assert not tuned.uses_runtime_kernel
        x, fm, st, it = tuned.solve(recs)
        out = tuned.solve_sensitivity(recs)
        np.testing.assert_array_equal(out["status"], st)
        np.testing.assert_array_equal(out["iters"], it)
        for b in range(len(recs)):
            assert relerr(out["x"][b], x[b]) < 1e-12 and relerr(out["first_move"][b], fm[b]) < 1e-12, b
        for a, c in zip((x, fm, st, it), plain.solve(recs)):    # the flag does not change the plain solve
            np.testing.assert_array_equal(a, c)
    finally:
        tuned.close()
        plain.close()


def test_affine_exactness_on_the_production_path(solver_mod, synth, layout):
    cfg = layout.paper_config()
    recs = np.concatenate([synth.make_batch(cfg, 8, workload=w, first_index=11) for w in ("hover", "takeoff")])
    m = solver_mod.BatchedVSMPC(cfg, device=0, max_batch=len(recs), sensitivity=True)
    try:
        assert not m.uses_runtime_kernel
        out = m.solve_sensitivity(recs)
        d = 1e-5 * (1.0 + np.abs(recs[:, :26])) * np.random.default_rng(3).standard_normal((len(recs), 26))
        plus, minus = recs.copy(), recs.copy()
        plus[:, :26] += d
        minus[:, :26] -= d
        xp, _, stp, _ = m.solve(plus)
        xm, _, stm, _ = m.solve(minus)
        ap = m.solve_sensitivity(plus, jacobian=False)["active"]
        am = m.solve_sensitivity(minus, jacobian=False)["active"]
    finally:
        m.close()
    checked = 0
    for b in range(len(recs)):
        if out["flags"][b] or not (np.array_equal(ap[b], out["active"][b]) and np.array_equal(am[b], out["active"][b])):
            continue
        assert stp[b] == stm[b] == layout.STATUS_SOLVED
        Jd = out["dx_dx0"][b] @ d[b]
        err = np.abs((xp[b] - xm[b]) / 2.0 - Jd).max() / np.abs(Jd).max()
        assert err <= 1e-7, (b, err)
        checked += 1
    assert checked >= len(recs) // 2, checked


def test_degeneracy_flag(solver_mod, synth, layout):
    """throttleMax placed on the largest free throttle of a plain hover solution (the box then changes nothing): the
    instance is flagged; the plain hover instance is not"""
    from importlib import import_module
    JetModel = import_module(solver_mod.__name__.rsplit(".", 1)[0] + ".jet_model").JetModel
    cfg = layout.paper_config()
    rec = synth.make_batch(cfg, 1, workload="hover", first_index=5)
    rec[:, layout.IN_HOLD] = 0.0
    m = solver_mod.BatchedVSMPC(cfg, device=0, max_batch=1, sensitivity=True)
    try:
        out = m.solve_sensitivity(rec)
    finally:
        m.close()
    assert out["status"][0] == layout.STATUS_SOLVED and out["flags"][0] == 0
    v = out["x"][0, cfg.off_throttle:cfg.off_throttle + m.n_v]
    top = int(np.argmax(v))
    assert out["active"][0, top] == layout.ACTIVE_FREE
    capped = dataclasses.replace(cfg, throttle_max=float(JetModel().destandardizeThrottle_u2T(v[top])))
    m = solver_mod.BatchedVSMPC(capped, device=0, max_batch=1, sensitivity=True)
    try:
        out2 = m.solve_sensitivity(rec)
    finally:
        m.close()
    assert out2["status"][0] == layout.STATUS_SOLVED
    assert out2["flags"][0] & layout.SENS_DEGENERATE, (out2["flags"], out2["active"])
    assert relerr(out2["x"][0], out["x"][0]) < 1e-9


@pytest.mark.parametrize("jacobian", [True, False])
def test_host_entry_over_two_chunks_equals_the_device_entry(solver_mod, synth, layout, jacobian):
    """257 instances at (2, 2, 2): one chunk of the host entry (256) and a second of a single instance, against one launch
    of the device entry -- the same kernel, so every output is equal bit for bit (NaN == NaN).  Hover and take-off records,
    one held tick and one with a NaN in X0 among them, both in the first chunk."""
    import torch
    cfg = layout.MPCConfig(n_iter=2, n_iter_small=2, control_horizon=2)
    B = 257
    recs = np.concatenate([synth.make_batch(cfg, 129, workload="hover", first_index=3),
                           synth.make_batch(cfg, 128, workload="takeoff", first_index=3)])
    recs[70, layout.IN_HOLD] = 1.0
    recs[200, layout.IN_X0 + 4] = np.nan
    dev = torch.device("cuda:0")
    f64 = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)
    m = solver_mod.BatchedVSMPC(cfg, device=0, max_batch=B, runtime="always", sensitivity=True)
    try:
        whole = m.solve_sensitivity(recs, jacobian=jacobian)
        t = {"x": f64(B, m.n_var), "first_move": f64(B, 24), "status": i32(B), "iters": i32(B),
             "dx_dx0": f64(B, m.n_var, 26) if jacobian else None, "dfm_dx0": f64(B, 24, 26), "active": i32(B, m.n_v),
             "flags": i32(B)}
        m.solve_sensitivity_device(torch.from_numpy(recs).to(dev), *t.values())
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy() for k, v in t.items() if v is not None}
    finally:
        m.close()
    assert (np.delete(whole["status"], 200) == layout.STATUS_SOLVED).all() and np.isnan(whole["x"][200]).any()
    assert sorted(whole) == sorted(got) and ("dx_dx0" in whole) == jacobian
    for k in whole:
        assert np.array_equal(got[k], whole[k], equal_nan=True), (
            k, [b for b in range(B) if not np.array_equal(got[k][b], whole[k][b], equal_nan=True)])


def test_contracts(solver_mod, synth, layout):
    import torch
    cfg = layout.MPCConfig(n_iter=20, n_iter_small=5, control_horizon=9)
    recs = _records(layout, synth, cfg, n=2)
    B = len(recs)
    plain = solver_mod.BatchedVSMPC(cfg, device=0, max_batch=B, runtime="fallback")
    try:
        with pytest.raises(Exception) as e:
            plain.solve_sensitivity(recs)
        assert "unsupported" in str(e.value).lower()
    finally:
        plain.close()
    m = solver_mod.BatchedVSMPC(cfg, device=0, max_batch=B, runtime="fallback", sensitivity=True)
    try:
        with pytest.raises(Exception) as e:
            m.solve_sensitivity(np.concatenate([recs, recs[:1]]))
        assert "max_batch" in str(e.value)
        full = m.solve_sensitivity(recs)                        # batch = max_batch
        one = m.solve_sensitivity(recs[1:2])                    # batch 1
        for k, v in one.items():
            np.testing.assert_array_equal(v[0], full[k][1], err_msg=k)
        # NULL optional outputs: status only
        st = np.empty(B, dtype=np.int32)
        rc = m.lib.vsmpc_sensitivity_batch(m._h, recs.ctypes.data_as(c_void_p), B, None, None,
                                           st.ctypes.data_as(c_void_p), None, None, None, None, None, None)
        assert rc == 0
        np.testing.assert_array_equal(st, full["status"])
        # device entry == host entry, bit for bit
        dev = torch.device("cuda:0")
        t = {"in": torch.from_numpy(recs).to(dev),
             "x": torch.empty((B, m.n_var), dtype=torch.float64, device=dev),
             "fm": torch.empty((B, 24), dtype=torch.float64, device=dev),
             "st": torch.empty(B, dtype=torch.int32, device=dev), "it": torch.empty(B, dtype=torch.int32, device=dev),
             "dx": torch.empty((B, m.n_var, 26), dtype=torch.float64, device=dev),
             "dfm": torch.empty((B, 24, 26), dtype=torch.float64, device=dev),
             "act": torch.empty((B, m.n_v), dtype=torch.int32, device=dev),
             "fl": torch.empty(B, dtype=torch.int32, device=dev)}
        m.solve_sensitivity_device(t["in"], t["x"], t["fm"], t["st"], t["it"], t["dx"], t["dfm"], t["act"], t["fl"])
        torch.cuda.synchronize()
        for k, name in (("x", "x"), ("fm", "first_move"), ("st", "status"), ("it", "iters"), ("dx", "dx_dx0"),
                        ("dfm", "dfm_dx0"), ("act", "active"), ("fl", "flags")):
            np.testing.assert_array_equal(t[k].cpu().numpy(), full[name], err_msg=name)
    finally:
        m.close()
