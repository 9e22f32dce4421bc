"""The solve kernels on rank-deficient and vanishing Lambda (tests/lambda_cases.py): p0_joint_reduction's path without a
reflector (csrc/vsmpc_kernels.hip: nz = sk > 1e-300, beta = 0, zero columns of R^T) and joint_expand on the way back in P6.

At the three tabled horizons every variant, on a free and on a held tie-broken record, is solved by
  * the tuned kernel in both condensing forms where the horizon has both,
  * its shipped and small-batch kinds where the horizon has the kind,
  * the per-instance-tunables instantiation under config_cases.JOINT_SPREAD rows, in both forms,
  * the runtime-sized kernel,
and compared with the oracle by test_gpu_config_parity._check_solution (1e-8 per output group, equal statuses and iteration
counts).  The joint block is also compared on its own, relative to its own maximum (with Lambda = 0 the joints are 1e-5
beside states of 200, and a bar relative to |x| cannot see them), and the joints whose column of Lambda is zero with their
closed form U[k] = -w_reg q_err[k] / (w_dq[k] + w_reg) at 100 times what the numpy route reaches
(lambda_cases.CLOSED_FORM_BAR).  Every result is then certified by certify_kernel at 1e-9.

vsmpc_debug_condensed against algo_model.reduced_condensed, at test_gpu_record_parity.py's bars: the whole of M, the
gradient row and L where the QR is determined by the data (DETERMINED: full rank, or pivot columns that are exactly zero
and get no reflector on either side).  Where a pivot column is rounding noise (rank3_lin_eq_ang, rank5_combination,
one_joint_only) its reflector, and with it every later column of Q and R, is an arbitrary orthogonal completion that two
correct implementations choose differently; what does not depend on the choice is the factor of the Schur complement on the
throttles, L22, and the throttle part of L^-1 g, and those are compared for every variant.  At scaled_1e-140 the numpy
model's own reflector update underflows (it forms outer(v, v'A), 1e-141 x 1e-282, before it multiplies by beta = 1e280; its
reduced gradient differs from the unscaled record's by 8.5e-3, where the two are equal in exact arithmetic), so it is no
reference for the gradient row there: the device's joint gradient is compared with the model's Q'b of the UNSCALED record,
which a QR is invariant to, and M with the model's (Lambda's share of it is 1e-280 on both sides).
tests/test_lambda_cases.py is the reference side, on the CPU."""
import numpy as np
import pytest

from conftest import relerr
import config_cases as cc
import lambda_cases as lc
import record_cases as rc
from test_gpu_config_parity import _check_solution

pytestmark = pytest.mark.gpu
TOL_CERT = 1e-9
DETERMINED = {"zero", "lin_zero", "ang_zero", "rank5_row1_zero", "first_pivot_zero", "last_pivot_zero",
              "two_joint_columns_zero", "scaled_1e-8", "scaled_1e-152"}


def _check(ref, solver_mod, layout, rcfg, names, recs, sol, xs_ref, cert_mpc, label, cfgs=None):
    x, fm, st, it = sol
    print(label)
    if xs_ref is None:                      # the oracle's solutions and iteration counts, computed once per configuration
        xs_ref = (_check_solution(ref, rcfg, layout, recs, x, fm, st, it), it.copy())
    else:
        _check_solution_against(ref, rcfg, layout, recs, sol, *xs_ref)
    xs = xs_ref[0]
    worst = {"joints": 0.0}
    for b, name in enumerate(names):
        variant = name.split("/")[0]
        e = lc.joint_block_error(rcfg, x[b], xs[b])
        worst["joints"] = max(worst["joints"], e)
        assert e <= lc.JOINT_BLOCK_BAR, (label, name, e)
        joints = lc.CLOSED_FORM_JOINTS.get(variant)
        if joints is not None:
            want = lc.closed_form_joints(rcfg, layout, recs[b], joints)
            U = x[b, rcfg.off_joints:rcfg.off_throttle].reshape(-1, 8)
            e = float(np.abs(U[:, joints] - want).max() / np.abs(want).max())
            worst["closed form " + variant] = max(worst.get("closed form " + variant, 0.0), e)
            assert e <= lc.CLOSED_FORM_BAR[variant], (label, name, e, lc.CLOSED_FORM_BAR[variant])
    _, cert = cert_mpc.certify(recs, x, configs=cfgs, duals=False)
    ok = solver_mod.certified(cert, x, TOL_CERT)
    worst["stationarity / scale"] = float((cert[:, 0] / cert[:, 1]).max())
    worst["primal / |x|"] = float((cert[:, 2] / np.maximum(1.0, np.abs(x).max(axis=1))).max())
    worst["complementarity / max(1, |y|)"] = float((cert[:, 3] / np.maximum(1.0, cert[:, 5])).max())
    print("  ", {k: f"{v:.2e}" for k, v in worst.items()})
    assert ok.all(), (label, [n for n, o in zip(names, ok) if not o])
    return xs_ref


def _check_solution_against(ref, rcfg, layout, recs, sol, xs, iters):
    """_check_solution with the oracle's solutions at hand: the same groups, bars and iteration counts"""
    x, fm, st, it = sol
    assert (st == layout.STATUS_SOLVED).all(), st
    np.testing.assert_array_equal(it, iters)              # the oracle's, checked by _check_solution on the first solve
    oj, ov = rcfg.off_joints, rcfg.off_throttle
    worst = {}
    for b in range(len(recs)):
        X, Xr = x[b, :oj].reshape(-1, 26), xs[b][:oj].reshape(-1, 26)
        for k, v in (("x", relerr(x[b], xs[b])), ("thrust", relerr(X[:, 12:16], Xr[:, 12:16])),
                     ("thrust_dot", relerr(X[:, 16:20], Xr[:, 16:20])), ("traj", relerr(X[:, 0:12], Xr[:, 0:12])),
                     ("v", relerr(x[b, ov:], xs[b][ov:])), ("dq", relerr(x[b, oj:ov], xs[b][oj:ov])),
                     ("fm", relerr(fm[b], ref.first_move_vector(rcfg, xs[b])))):
            worst[k] = max(worst.get(k, 0.0), v)
    print("worst vs oracle:", {k: f"{v:.2e}" for k, v in worst.items()})
    for k, v in worst.items():
        assert v < 1e-8, (k, v)


@pytest.mark.parametrize("horizon", cc.HORIZONS, ids=lambda h: "%d-%d-%d" % tuple(h))
def test_rank_deficient_lambda(solver_mod, ref, layout, horizon):
    import algo_model
    cfg, rcfg = cc.configs(ref, horizon, {})
    spread, rspread = cc.configs(ref, horizon, dict(w_delta_joint=cc.JOINT_SPREAD))
    names, recs = lc.records(cfg, layout)
    base = rc.distinct_records(cfg)
    n = len(recs)
    paper = tuple(horizon) == cc.PAPER
    m = solver_mod.BatchedVSMPC(cfg, device=0, max_batch=n, tunables=True, certify=True)
    rt = solver_mod.BatchedVSMPC(cfg, device=0, max_batch=n, runtime="always")
    try:
        assert "solve_kernel" in m.kernel_name and not m.uses_runtime_kernel and rt.uses_runtime_kernel
        forms = []
        for form in (solver_mod.KERNEL_FORM_STRUCTURED, solver_mod.KERNEL_FORM_SYRK):
            try:
                m.set_kernel_form(form)
                forms.append(form)
            except ValueError:
                assert tuple(horizon) == (21, 9, 15) and form == solver_mod.KERNEL_FORM_STRUCTURED, (horizon, form)
        assert solver_mod.KERNEL_FORM_SYRK in forms
        xs = xs_spread = None
        bM, bL = (1e-12, 1e-11) if paper else (1e-11, 1e-10)
        for form in forms:
            m.set_kernel_form(form)
            kinds = ["never"]
            try:                                      # the kind is the structured form's (include/vsmpc.h): SYRK keeps the shipped kernel
                m.set_small_batch_kernel("always")
                if form == solver_mod.KERNEL_FORM_STRUCTURED:
                    kinds.append("always")
                else:
                    assert not m.uses_small_batch_kernel(n)
            except ValueError:
                assert not paper
            assert kinds == ["never", "always"] or not (paper and form == solver_mod.KERNEL_FORM_STRUCTURED)
            for kind in kinds:
                m.set_small_batch_kernel(kind)
                assert m.uses_small_batch_kernel(n) == (kind == "always")
                xs = _check(ref, solver_mod, layout, rcfg, names, recs, m.solve(recs), xs, m, f"{horizon} form {form} small-batch {kind}:")
            m.set_small_batch_kernel("auto")
            # the per-instance-tunables instantiation, W read per instance
            cfgs = [spread] * n
            xs_spread = _check(ref, solver_mod, layout, rspread, names, recs, m.solve(recs, configs=cfgs), xs_spread, m,
                               f"{horizon} form {form} tunables, JOINT_SPREAD rows:", cfgs=cfgs)
            # P1-P3 of this form
            assert xs[1].max() > 1
            for b, name in enumerate(names):
                if name.endswith("/held") and name.split("/")[0] not in ("zero", "rank5_combination", "scaled_1e-140"):
                    continue
                M, Lf = m.debug_condensed(recs[b])[:2]
                Me, ge, Le = algo_model.reduced_condensed(rcfg, ref, recs[b])
                nz = Me.shape[0]
                nu = nz - 4 * rcfg.n_vblocks
                lge = np.linalg.solve(Le, ge)
                eS = relerr(np.tril(Lf[nu:nz, nu:nz]), Le[nu:, nu:])
                eSg = relerr(Lf[nz, nu:nz], lge[nu:])
                Mh = np.tril(M[:nz, :nz])
                Mh = Mh + np.tril(Mh, -1).T
                eM, eg = relerr(Mh, Me), relerr(M[nz, :nz], ge)
                eL, eLg = relerr(np.tril(Lf[:nz, :nz]), Le), relerr(Lf[nz, :nz], lge)
                print(f"form {form} {name}: L22 {eS:.2e} (L^-1 g)_v {eSg:.2e} | M {eM:.2e} g {eg:.2e} L {eL:.2e} L^-1 g {eLg:.2e}")
                assert eS < bL and eSg < bL, (form, name, eS, eSg)
                if name.split("/")[0] == "scaled_1e-140":
                    gy = algo_model.reduced_model(rcfg, ref, base[2 if name.endswith("/free") else 3])[1]["gy"]
                    want = ge.copy()
                    want[:6 * rcfg.control_horizon] = np.tile(gy, rcfg.control_horizon)
                    eg = relerr(M[nz, :nz], want)
                    print(f"    against the unscaled record's Q'b: g {eg:.2e}")
                    assert eM < bM and eg < bM, (form, name, eM, eg)
                if name.split("/")[0] in DETERMINED:
                    assert eM < bM and eg < bM, (form, name, eM, eg)
                    assert eL < bL and eLg < bL, (form, name, eL, eLg)
        m.set_kernel_form(solver_mod.KERNEL_FORM_AUTO)
        _check(ref, solver_mod, layout, rcfg, names, recs, rt.solve(recs), xs, m, f"{horizon} runtime kernel:")
    finally:
        m.close()
        rt.close()
