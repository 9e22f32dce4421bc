"""The numpy model of certify_kernel (tests/certificate_model.py) against the oracle, on the oracle's own optimum: the
duals of the structured route against oracle/vsmpc_ref.py solve_exact, the certificate against kkt_certificate.  No GPU.

Bar on y: the project's 1e-8, as |y_model - y_ref|_inf / max(1, |y_ref|_inf).  Measured worst value over the cases below
(paper horizon: 48 take-off, 48 Monte-Carlo, 48 hover; 34/14/24, 21/9/15 and 20/5/9: 4 take-off each): 1.9e-15 at the paper
horizon (take-off; Monte-Carlo 1.1e-15, hover 1.8e-15) and 8.7e-16 at the others: both routes are at rounding level, seven
orders below the bar.  Which of the two is the less accurate one shows in the certificate: solve_exact gets its equality
duals from a dense LU of the 468 x 468 Ax^T, the recursion only ever multiplies by I + dt A, and with the model's y the
stationarity residual over ALL entries of Hx + g + Ac'y is the smaller one on 40 / 32 / 26 of the 48 take-off / Monte-Carlo
/ hover records (printed and asserted for at least half).  The oracle's LU sets the floor, such as it is.
"""
import numpy as np
import pytest

import certificate_model as cm

TOL_Y = 1e-8


def compare(ref, rcfg, rec, x, y_ref):
    H, g, Ac, lo, hi = ref.assemble_dense(rcfg, rec)
    y, cert = cm.certify(ref, rcfg, rec, x)
    err_y = float(np.abs(y - y_ref).max() / max(1.0, np.abs(y_ref).max()))
    want = ref.kkt_certificate(H, g, Ac, lo, hi, x, y)
    tol = cm.field_tolerances(H, g, Ac, x, y)
    assert abs(cert[cm.CERT_STATIONARITY] - want["stationarity"]) <= tol["stationarity"]
    scale = max(1.0, float(np.abs(g).max()), float(np.abs(H @ x).max()))
    assert abs(cert[cm.CERT_STAT_SCALE] - scale) <= 4 * np.finfo(float).eps * scale
    assert abs(cert[cm.CERT_PRIMAL] - want["primal"]) <= tol["primal"]
    assert abs(cert[cm.CERT_COMPLEMENTARITY] - want["complementarity"]) <= tol["complementarity"]
    oscale = max(1.0, abs(want["objective"]), 0.5 * float(x @ H @ x))
    assert abs(cert[cm.CERT_OBJECTIVE] - want["objective"]) <= tol["objective_rel"] * oscale
    assert cert[cm.CERT_DUAL_MAX] == np.abs(y).max() and (cert[6:] == 0.0).all()
    # the padding rows behind the last throttle block
    r1 = 26 * (rcfg.n_iter + 1) + 4 * rcfg.n_vblocks
    assert (y[r1:] == 0.0).all() and (y_ref[r1:] == 0.0).all()
    # which route is the less accurate one: the full stationarity residual with either y
    own = ref.kkt_certificate(H, g, Ac, lo, hi, x, y_ref)
    return err_y, want["stationarity"], own["stationarity"]


@pytest.mark.parametrize("workload", ["takeoff", "montecarlo", "hover"])
def test_model_matches_the_oracle_at_the_paper_horizon(ref, synth, layout, workload):
    _, rcfg = cm.case_configs(ref, layout, "paper")
    worst, n_better = 0.0, 0
    cases = cm.oracle_cases(ref, synth, layout, "paper", workload, 48)
    for rec, x, y_ref in cases:
        err, stat_model, stat_ref = compare(ref, rcfg, rec, x, y_ref)
        worst = max(worst, err)
        n_better += stat_model <= stat_ref
    print(f"{workload}: worst |y_model - y_ref| / max(1, |y_ref|) = {worst:.3e}; model's y has the smaller full "
          f"stationarity residual on {n_better} of {len(cases)}")
    assert worst <= TOL_Y
    assert n_better >= len(cases) // 2          # the oracle's dense route sets the floor (module docstring)


@pytest.mark.parametrize("name", ["h2x", "odd", "unlisted"])
def test_model_matches_the_oracle_at_other_horizons(ref, synth, layout, name):
    _, rcfg = cm.case_configs(ref, layout, name)
    worst = 0.0
    for rec, x, y_ref in cm.oracle_cases(ref, synth, layout, name, "takeoff", 4):
        worst = max(worst, compare(ref, rcfg, rec, x, y_ref)[0])
    print(f"{cm.HORIZONS[name]}: worst |y_model - y_ref| / max(1, |y_ref|) = {worst:.3e}")
    assert worst <= TOL_Y


def test_the_paper_batches_reach_every_branch(ref, synth, layout):
    """What tests/test_gpu_certificate.py relies on, for exactly its 48 + 48 records: bound-active non-pinned throttles
    on both sides, held and unheld records"""
    _, rcfg = cm.case_configs(ref, layout, "paper")
    vmin, vmax = ref.throttle_bounds(rcfg)
    counts = {}
    for workload in ("takeoff", "montecarlo"):
        lower = upper = held = 0
        for rec, x, _ in cm.oracle_cases(ref, synth, layout, "paper", workload, 48):
            hold = rec[layout.IN_HOLD] != 0.0
            held += hold
            v = x[rcfg.off_throttle:].reshape(-1, 4)[1 if hold else 0:]
            lower += int((v == vmin).sum())
            upper += int((v == vmax).sum())
        counts[workload] = (lower, upper, held)
    print(counts)
    assert counts["takeoff"] == (100, 1, 45)
    assert counts["montecarlo"][1:] == (8, 45)


def test_model_sees_a_wrong_answer(ref, synth, layout):
    """the three perturbations of tests/test_gpu_certificate.py on the model"""
    _, rcfg = cm.case_configs(ref, layout, "paper")
    rec, x, _ = cm.oracle_cases(ref, synth, layout, "paper", "takeoff", 48)[0]
    _, base = cm.certify(ref, rcfg, rec, x)
    xa = x.copy()
    xa[rcfg.off_joints + 3] += 1e-3
    _, ca = cm.certify(ref, rcfg, rec, xa)
    want = (rcfg.w_delta_joint[3] + rcfg.w_reg_joint_pos) * 1e-3
    assert abs(ca[cm.CERT_STATIONARITY] - want) <= 1e-6 * want
    seen = np.abs(ref.linearize(rcfg, rec)[1][:, 3]).max() * ref.dt_schedule(rcfg)[0] * 1e-3
    assert ca[cm.CERT_PRIMAL] >= seen * (1 - 1e-6) > 0.0          # (the dynamics rows of stage 0 see the increment too)
    xb = x.copy()
    xb[5 * 26 + 2] += 1e-3
    _, cb = cm.certify(ref, rcfg, rec, xb)
    assert cb[cm.CERT_PRIMAL] >= 1e-3 * (1 - 1e-6) and base[cm.CERT_PRIMAL] < 1e-9
