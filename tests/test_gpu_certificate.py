"""Duals and KKT certificate on the device (vsmpc_certify_batch, vsmpc_certify_batch_device; certify_kernel) against the
oracle: y against oracle/vsmpc_ref.py solve_exact at the project's 1e-8, every certificate field against kkt_certificate
on the same (x, y) with the arithmetic-only tolerances of tests/certificate_model.py field_tolerances.  Those are worst-case
rounding bounds (proportional to |y|_inf, up to 3e6), so at an optimum, where STATIONARITY and COMPLEMENTARITY are rounding
noise themselves, the per-field comparison only says "both are noise": it would not see such a field 100 times off.  What
pins the fields is test_certificate_sees_a_wrong_answer (values known in closed form, to 1e-6 and 1e-12 relative) and the
1e-9 bars of test_full_size_every_instance.  x is the library's own solve.  The oracle results are computed once per session (certificate_model.oracle_cases) and shared with
tests/test_certificate_model.py, which also checks on the CPU that the paper batches reach every branch."""
import numpy as np
import pytest

import certificate_model as cm
import config_cases as cc

pytestmark = pytest.mark.gpu

TOL_Y = 1e-8                      # the project's parity bar
TOL_CERT = 1e-9                   # the bar of test_gpu_parity._kkt_properties
S, SC, P, C, O, D = range(6)      # CERT_* columns


def make(solver_mod, cfg, max_batch, runtime="never", **kw):
    return solver_mod.BatchedVSMPC(cfg, device=0, max_batch=max_batch, runtime=runtime, certify=True, **kw)


def check_against_oracle(ref, rcfg, rec, x, y, cert, y_ref):
    H, g, Ac, lo, hi = ref.assemble_dense(rcfg, rec)
    err_y = float(np.abs(y - y_ref).max() / max(1.0, np.abs(y_ref).max()))
    want = ref.kkt_certificate(H, g, Ac, lo, hi, x, y)
    tol = cm.field_tolerances(H, g, Ac, x, y)
    scale = max(1.0, float(np.abs(g).max()), float(np.abs(H @ x).max()))
    oscale = max(1.0, abs(want["objective"]), 0.5 * float(x @ H @ x))
    figures = (err_y, abs(cert[S] - want["stationarity"]) / tol["stationarity"], abs(cert[SC] - scale) / scale,
               abs(cert[P] - want["primal"]) / tol["primal"], abs(cert[C] - want["complementarity"]) / tol["complementarity"],
               abs(cert[O] - want["objective"]) / oscale / tol["objective_rel"])
    print("y rel %.2e | stat %.2e of tol | scale rel %.1e | primal %.2e of tol | comp %.2e of tol | obj %.2e of tol" % figures)
    assert err_y <= TOL_Y
    assert figures[1] <= 1.0 and figures[3] <= 1.0 and figures[4] <= 1.0 and figures[5] <= 1.0
    assert figures[2] <= 4 * np.finfo(float).eps
    assert cert[D] == np.abs(y).max() and (cert[6:] == 0.0).all()
    r1 = 26 * (rcfg.n_iter + 1) + 4 * rcfg.n_vblocks
    assert r1 < y.size and (y[r1:] == 0.0).all()                      # the padding rows, exactly
    return want


@pytest.mark.parametrize("name, counts", [("paper", (48, 48)), ("h2x", (8, 0)), ("odd", (8, 0)), ("unlisted", (4, 0))])
def test_parity_with_the_oracle(solver_mod, ref, synth, layout, name, counts):
    """1: take-off (+ Monte-Carlo at the paper horizon) records; 20/5/9 is in no table and runs on a runtime handle"""
    cfg, rcfg = cm.case_configs(ref, layout, name)
    cases = cm.oracle_cases(ref, synth, layout, name, "takeoff", counts[0])
    if counts[1]:
        cases = cases + cm.oracle_cases(ref, synth, layout, name, "montecarlo", counts[1])
    recs = np.ascontiguousarray(np.stack([c[0] for c in cases]))
    mpc = make(solver_mod, cfg, len(cases), runtime="fallback" if name == "unlisted" else "never")
    assert mpc.uses_runtime_kernel == (name == "unlisted")
    x, _, st, _ = mpc.solve(recs)
    assert (st == layout.STATUS_SOLVED).all()
    y, cert = mpc.certify(recs, x)
    assert y.shape == (len(cases), rcfg.n_con) and cert.shape == (len(cases), layout.CERT_SIZE)
    worst = {"stationarity_rel": 0.0, "primal": 0.0, "complementarity": 0.0}
    for b, (rec, _, y_ref) in enumerate(cases):
        want = check_against_oracle(ref, rcfg, rec, x[b], y[b], cert[b], y_ref)
        for k in worst:
            worst[k] = max(worst[k], want[k])
    print(name, "oracle certificate of the device (x, y):", worst, "max |y|", np.abs(y).max())
    assert solver_mod.certified(cert, x, TOL_CERT).all()
    if name == "paper":            # the batch must not be an easy one
        held = recs[:, layout.IN_HOLD] != 0.0
        v = x[:, cfg.off_throttle:].reshape(len(cases), -1, 4)
        lo, hi = ref.throttle_bounds(rcfg)
        free_rows = np.ones(v.shape, dtype=bool)
        free_rows[held, 0, :] = False                                  # pinned by the hold
        assert (free_rows & (np.abs(v - lo) < 1e-12)).any(), "no non-pinned throttle on its lower bound"
        assert (free_rows & (np.abs(v - hi) < 1e-12)).any(), "no non-pinned throttle on its upper bound"
        assert held.any() and (~held).any()
        mu = y[:, 26 * (rcfg.n_iter + 1):][:, :v.shape[1] * 4].reshape(v.shape)
        assert (mu[free_rows & (np.abs(v - lo) < 1e-12)] < 0.0).all()      # OSQP's sign: lower-active negative
        assert (mu[free_rows & (np.abs(v - hi) < 1e-12)] > 0.0).all()
    mpc.close()


def test_per_instance_tunables(solver_mod, ref, synth, layout):
    """2: 8 instances under 4 configurations, solved and certified with the same rows; then the same x under the handle's
    configuration: the instances whose weights differ are not stationary for it"""
    settings = [{}, dict(throttle_min=10.0, throttle_max=90.0), dict(w_delta_joint=cc.JOINT_SPREAD),
                {k: v for k, v in cc.all_distinct(cc.PAPER).items() if not k.startswith("period")}]
    pairs = [cc.configs(ref, cc.PAPER, s) for s in settings]
    recs = np.ascontiguousarray(synth.make_batch(pairs[0][0], 8, workload="takeoff"))
    which = [0, 1, 2, 3, 1, 2, 3, 0]
    cfgs = [pairs[w][0] for w in which]
    mpc = make(solver_mod, pairs[0][0], 8, tunables=True)
    x, _, st, _ = mpc.solve(recs, configs=cfgs)
    assert (st == layout.STATUS_SOLVED).all()
    y, cert = mpc.certify(recs, x, configs=cfgs)
    for b, w in enumerate(which):
        _, y_ref, _, _ = ref.solve_instance(pairs[w][1], recs[b])
        check_against_oracle(ref, pairs[w][1], recs[b], x[b], y[b], cert[b], y_ref)
    assert solver_mod.certified(cert, x, TOL_CERT).all()
    rows = solver_mod.pack_tunables(mpc, cfgs)
    y2, cert2 = mpc.certify(recs, x, tunables=rows)
    assert np.array_equal(y, y2) and np.array_equal(cert, cert2)
    _, plain = mpc.certify(recs, x)
    rel = plain[:, S] / plain[:, SC]
    print("stationarity / scale under the handle's configuration:", rel)
    for b, w in enumerate(which):
        if w in (2, 3):
            assert rel[b] > 1e-6, (b, w, rel[b])
        if w == 0:
            assert np.array_equal(plain[b], cert[b])
    mpc.close()


def test_certificate_sees_a_wrong_answer(solver_mod, ref, synth, layout):
    """3: one solved take-off instance, three perturbations"""
    cfg, rcfg = cm.case_configs(ref, layout, "paper")
    recs = np.ascontiguousarray(synth.make_batch(cfg, 48, workload="takeoff"))
    mpc = make(solver_mod, cfg, 48)
    xs, _, st, _ = mpc.solve(recs)
    ys, certs = mpc.certify(recs, xs)
    lo, hi = mpc.assemble_dense(recs[0])[3:5]
    nvb, offV, r1 = cfg.n_vblocks, cfg.off_throttle, 26 * (cfg.n_iter + 1)
    # an instance with a non-pinned throttle on a bound (block >= 1 is never pinned)
    pick = None
    for b in range(48):
        v = xs[b, offV + 4:]
        at = np.nonzero((np.abs(v - lo[r1 + 4:r1 + 4 * nvb]) < 1e-12) | (np.abs(v - hi[r1 + 4:r1 + 4 * nvb]) < 1e-12))[0]
        if st[b] == layout.STATUS_SOLVED and at.size:
            pick, idx = b, 4 + int(at[0])
            break
    assert pick is not None
    rec, x, base = recs[pick:pick + 1], xs[pick], certs[pick]
    assert solver_mod.certified(base[None, :], x[None, :], TOL_CERT).all()
    delta = 1e-3
    # (a) one joint increment of block 0: only that row of the gradient moves, by its diagonal of H
    j = 5
    xa = x.copy()
    xa[cfg.off_joints + j] += delta
    ya, ca = mpc.certify(rec, xa[None, :])
    want = (cfg.w_delta_joint[j] + cfg.w_reg_joint_pos) * delta
    print(f"(a) stationarity {ca[0, S]:.9e}, wanted {want:.9e}; base {base[S]:.3e}")
    assert abs(ca[0, S] - want) <= 1e-6 * want
    assert np.array_equal(ya[0], ys[pick])                            # y depends on the states alone
    # (b) one entry of X_5
    xb = x.copy()
    xb[5 * 26 + 1] += delta
    _, cb = mpc.certify(rec, xb[None, :])
    print(f"(b) primal {cb[0, P]:.9e}; base {base[P]:.3e}")
    assert cb[0, P] >= delta * (1 - 1e-6)
    # (c) a bound-active throttle moved inside its box, states re-simulated with the library's own linearisation
    A, Bj, Bt, c, dt = (a[0] if a.ndim > 1 and a.shape[0] == 1 else a for a in mpc.linearize(rec))
    xc = x.copy()
    inward = delta if abs(x[offV + idx] - lo[r1 + idx]) < 1e-12 else -delta
    xc[offV + idx] += inward
    X = np.empty((cfg.n_iter + 1, 26))
    X[0] = rec[0, :26]
    U = xc[cfg.off_joints:offV].reshape(-1, 8)
    V = xc[offV:].reshape(-1, 4)
    for i in range(cfg.n_iter):
        X[i + 1] = X[i] + dt[i] * (A @ X[i] + Bj @ U[ref.joint_block_of_stage(rcfg, i)]
                                   + Bt @ V[ref.throttle_block_of_stage(rcfg, i)] + c)
    xc[:26 * (cfg.n_iter + 1)] = X.reshape(-1)
    yc, cc_ = mpc.certify(rec, xc[None, :])
    mu = abs(yc[0, r1 + idx])
    print(f"(c) primal {cc_[0, P]:.3e}, complementarity {cc_[0, C]:.6e}, |mu| delta {mu * delta:.6e}; base {base[C]:.3e}")
    assert cc_[0, P] <= TOL_CERT * max(1.0, np.abs(xc).max())
    assert mu > 0.0 and cc_[0, C] >= mu * delta * (1 - 1e-6)
    assert cc_[0, C] > base[C]
    # The moved row need not be the maximum: y is defined from x, so the neighbouring blocks of the moved throttle take a
    # multiplier of w_throttle * delta = 80 with a slack of order 1, which can exceed |mu| delta.  The field is therefore
    # pinned from both sides against the definition evaluated on the host from the returned y and the same x and box.
    vb, mub = xc[offV + 4:], yc[0, r1 + 4:r1 + 4 * nvb]
    lob, hib = lo[r1 + 4:r1 + 4 * nvb], hi[r1 + 4:r1 + 4 * nvb]
    want_c = np.maximum(np.maximum(mub, 0.0) * (hib - vb), np.maximum(-mub, 0.0) * (vb - lob)).max()
    if rec[0, layout.IN_HOLD] == 0.0:                                  # block 0 counts on an unheld tick
        v0, mu0 = xc[offV:offV + 4], yc[0, r1:r1 + 4]
        want_c = max(want_c, np.maximum(np.maximum(mu0, 0.0) * (hi[r1 + 4] - v0), np.maximum(-mu0, 0.0) * (v0 - lo[r1 + 4])).max())
    print(f"    complementarity by its definition on the host: {want_c:.9e}")
    assert abs(cc_[0, C] - want_c) <= 1e-12 * want_c
    mpc.close()


def certify_device(mpc, layout, recs, x, rows=None, duals=True):
    import torch
    dev = torch.device("cuda:0")
    B = recs.shape[0]
    d_in, d_x = torch.from_numpy(recs).to(dev), torch.from_numpy(x).to(dev)
    d_tun = None if rows is None else torch.from_numpy(rows).to(dev)
    d_y = torch.full((B, mpc.n_con), -7.0, dtype=torch.float64, device=dev) if duals else None
    d_c = torch.full((B, layout.CERT_SIZE), -7.0, dtype=torch.float64, device=dev)
    mpc.certify_device(d_in, d_x, d_tun, d_y, d_c)
    torch.cuda.synchronize()
    return (d_y.cpu().numpy() if duals else None), d_c.cpu().numpy()


def test_determinism(solver_mod, synth, layout):
    """4: repeated and permuted batches bit-identical; host and device entries bit-identical"""
    cfg = layout.paper_config()
    recs = np.ascontiguousarray(np.concatenate([synth.make_batch(cfg, 24, workload="takeoff"),
                                                synth.make_batch(cfg, 24, workload="montecarlo")]))
    mpc = make(solver_mod, cfg, 96)
    x = mpc.solve(recs)[0]
    y, cert = mpc.certify(recs, x)
    y2, cert2 = mpc.certify(recs, x)
    assert np.array_equal(y, y2) and np.array_equal(cert, cert2)
    perm = np.random.default_rng(5).permutation(48)
    big_r = np.ascontiguousarray(np.concatenate([recs[perm], recs]))
    big_x = np.ascontiguousarray(np.concatenate([x[perm], x]))
    yp, cp = mpc.certify(big_r, big_x)
    assert np.array_equal(yp[:48], y[perm]) and np.array_equal(cp[:48], cert[perm])
    assert np.array_equal(yp[48:], y) and np.array_equal(cp[48:], cert)
    yd, cd = certify_device(mpc, layout, recs, x)
    assert np.array_equal(yd, y) and np.array_equal(cd, cert)
    mpc.close()


def test_full_size_every_instance(solver_mod, synth, layout):
    """5: 4096 distinct take-off records at the paper horizon, every one certified at the 1e-9 of _kkt_properties"""
    cfg = layout.paper_config()
    B = 4096
    recs = np.ascontiguousarray(synth.make_batch(cfg, B, workload="takeoff"))
    mpc = make(solver_mod, cfg, B)
    x, _, st, _ = mpc.solve(recs)
    assert (st == layout.STATUS_SOLVED).all()
    _, cert = mpc.certify(recs, x, duals=False)
    xs = np.maximum(1.0, np.abs(x).max(axis=1))
    print("worst stationarity / scale %.3e, primal / |x| %.3e, complementarity / max(1, |y|) %.3e, max |y| %.3e" % (
        (cert[:, S] / cert[:, SC]).max(), (cert[:, P] / xs).max(), (cert[:, C] / np.maximum(1.0, cert[:, D])).max(),
        cert[:, D].max()))
    assert np.isfinite(cert).all()
    assert (cert[:, S] <= TOL_CERT * cert[:, SC]).all()
    assert (cert[:, P] <= TOL_CERT * xs).all()
    assert (cert[:, C] <= TOL_CERT * np.maximum(1.0, cert[:, D])).all()
    assert solver_mod.certified(cert, x, TOL_CERT).all() and cert.shape[0] == B
    mpc.close()


def test_edge_cases(solver_mod, synth, layout):
    """6: batch 0, 1, above the handle; a handle without the create flag; y == NULL; a NaN record"""
    from importlib import import_module
    _lib = import_module(solver_mod.__name__.rsplit(".", 1)[0] + "._lib")
    cfg = layout.paper_config()
    recs = np.ascontiguousarray(synth.make_batch(cfg, 8, workload="takeoff"))
    mpc = make(solver_mod, cfg, 8)
    x = mpc.solve(recs)[0]
    y, cert = mpc.certify(recs, x)
    lib, p = mpc.lib, solver_mod._ptr
    guard_y, guard_c = np.full((9, mpc.n_con), -7.0), np.full((9, layout.CERT_SIZE), -7.0)
    assert lib.vsmpc_certify_batch(mpc._h, p(recs), p(x), None, 0, p(guard_y), p(guard_c)) == 0
    assert (guard_y == -7.0).all() and (guard_c == -7.0).all()
    big_r, big_x = np.tile(recs, (2, 1))[:9].copy(), np.tile(x, (2, 1))[:9].copy()
    assert lib.vsmpc_certify_batch(mpc._h, p(big_r), p(big_x), None, 9, p(guard_y), p(guard_c)) == -3
    assert (guard_y == -7.0).all() and (guard_c == -7.0).all()
    y1, c1 = mpc.certify(recs[:1], x[:1])
    assert np.array_equal(y1[0], y[0]) and np.array_equal(c1[0], cert[0])
    none_y, c_only = mpc.certify(recs, x, duals=False)
    assert none_y is None and np.array_equal(c_only, cert)
    yd, cd = certify_device(mpc, layout, recs, x, duals=False)
    assert yd is None and np.array_equal(cd, cert)
    # a NaN in one record
    bad = recs.copy()
    bad[3, layout.IN_INERTIA] = np.nan
    yb, cb = mpc.certify(bad, x)
    assert not np.isfinite(cb[3, S]) and not np.isfinite(cb[3, P])
    keep = [b for b in range(8) if b != 3]
    assert np.array_equal(yb[keep], y[keep]) and np.array_equal(cb[keep], cert[keep])
    assert not solver_mod.certified(cb, x, TOL_CERT)[3] and solver_mod.certified(cb, x, TOL_CERT)[keep].all()
    # a NaN in x, in a place no maximum would keep
    xn = x.copy()
    xn[5, cfg.off_joints + 2] = np.nan
    _, cn = mpc.certify(recs, xn)
    assert not np.isfinite(cn[5, S]) and not np.isfinite(cn[5, P]) and np.array_equal(cn[keep[:4]], cert[keep[:4]])
    mpc.close()
    plain = solver_mod.BatchedVSMPC(cfg, device=0, max_batch=8)
    assert lib.vsmpc_certify_batch(plain._h, p(recs), p(x), None, 8, p(guard_y), p(guard_c)) == -2
    assert "VSMPC_CREATE_CERTIFY" in lib.vsmpc_strerror(-2).decode()
    with pytest.raises(_lib.VsmpcError, match="VSMPC_CREATE_CERTIFY"):
        plain.certify(recs, x)
    yd, cd = certify_device(plain, layout, recs, x)                   # the device entry needs no staging, hence no flag
    assert np.array_equal(yd, y) and np.array_equal(cd, cert)
    plain.close()
