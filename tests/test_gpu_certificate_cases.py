"""certify_kernel (csrc/vsmpc_certify.hip) away from the optimum: the cases of tests/certificate_cases.py on the device.

At an optimum three of the certificate's fields are rounding noise, and four of the six are maxima that see one entry: a
lane range that skips rows, blocks or the second pass of phase B's strided loop makes the certificate report too little,
which tests/test_gpu_certificate.py cannot see.  Here every field has a known value on a chosen row (spotlights: closed
form), y is compared per row class with the numpy model at the measured bars certificate_cases.Y_BAR (1.5e-12 for the
costate and initial rows, 1.7e-9 for the throttle rows; at the optima also with solve_exact at the project's 1e-8), every
field with oracle/vsmpc_ref.py kkt_certificate on the device's own (x, y) inside certificate_model.field_tolerances, at the
three tabled horizons (tuned handles) and at six more (runtime handles), among them (2, 2, 2), (12, 12, 12), (40, 2, 2)
and (40, 2, 40), where phase B makes its second pass.  tests/test_certificate_cases.py is the reference side, on the CPU:
the model alone uses a fifth of every bound, the oracle's maximum sits on the intended row of every spotlight, and sixteen
one-line mistakes in a copy of the model each miss these checks by ten bars or more
(profiles/certificate_cases_mutations.txt)."""
import numpy as np
import pytest

import certificate_cases as ccs
import certificate_model as cm
import config_cases as cc
from test_gpu_certificate import certify_device

pytestmark = pytest.mark.gpu
TOL_CERT = 1e-9
S, SC, P, C, O, D = range(6)


def check_case(ref, solver_mod, rcfg, case, y, cert, worst, x=None, off_optimum=None):
    """one instance of a launch: y and cert are the device's; x: the primal that was certified if not the case's own"""
    if x is not None:
        case = dict(case, x=x)
    x = case["x"]
    y_model, _ = cm.certify(ref, rcfg, case["rec"], x)
    err = ccs.class_errors(rcfg, y, y_model) / ccs.Y_BAR
    fig, _ = ccs.field_figures(ref, rcfg, case, y, cert)
    fig["y class"] = float(err.max())
    if case["y_ref"] is not None:
        fig["y optimum"] = float(np.abs(y - case["y_ref"]).max() / max(1.0, np.abs(case["y_ref"]).max())) / 1e-8
    for k, v in fig.items():
        worst[k] = max(worst.get(k, 0.0), v)
    tag = (case["family"], case["name"], case["rec_name"])
    for k, v in fig.items():
        assert v <= 1.0, (tag, k, v)
    assert cert[D] == np.abs(y).max() and (cert[6:] == 0.0).all(), tag
    r1 = 26 * (rcfg.n_iter + 1) + 4 * rcfg.n_vblocks
    assert (y[r1:] == 0.0).all(), tag                                   # the padding rows, exactly
    optimum = case["family"] == "optimum" if off_optimum is None else not off_optimum
    margin = float(ccs.certified_margins(cert, x).max())
    worst["certified " + ("optima" if optimum else "others, least")] = (
        max(worst.get("certified optima", 0.0), margin) if optimum else min(worst.get("certified others, least", np.inf), margin))
    assert bool(solver_mod.certified(cert[None, :], x[None, :], TOL_CERT)[0]) == optimum, (tag, margin)


def run_group(ref, solver_mod, layout, mpc, rcfg, cases, label, device_entry=False, permuted=False):
    recs = np.ascontiguousarray(np.stack([c["rec"] for c in cases]))
    xs = np.ascontiguousarray(np.stack([c["x"] for c in cases]))
    y, cert = mpc.certify(recs, xs)
    assert y.shape == (len(cases), rcfg.n_con) and cert.shape == (len(cases), layout.CERT_SIZE)
    worst = {}
    for b, case in enumerate(cases):
        check_case(ref, solver_mod, rcfg, case, y[b], cert[b], worst)
    print(label, len(cases), "cases; worst, in bars:", {k: f"{v:.2e}" for k, v in worst.items()})
    # the optima again, from the library's own solve of the same records
    opt = [b for b, c in enumerate(cases) if c["family"] == "optimum"]
    xl, _, st, _ = mpc.solve(recs[opt])
    assert (st == layout.STATUS_SOLVED).all(), st
    yl, cl = mpc.certify(recs[opt], xl)
    worst = {}
    for k, b in enumerate(opt):
        check_case(ref, solver_mod, rcfg, cases[b], yl[k], cl[k], worst, x=xl[k])
    print(label, "the library's own optima; worst, in bars:", {k: f"{v:.2e}" for k, v in worst.items()})
    if device_entry:
        yd, cd = certify_device(mpc, layout, recs, xs)
        assert np.array_equal(yd, y) and np.array_equal(cd, cert)
    if permuted:
        perm = np.random.default_rng(5).permutation(len(cases))
        yp, cp = mpc.certify(np.ascontiguousarray(recs[perm]), np.ascontiguousarray(xs[perm]))
        assert np.array_equal(yp, y[perm]) and np.array_equal(cp, cert[perm])


@pytest.mark.parametrize("horizon", ccs.HORIZONS, ids=lambda h: "%d-%d-%d" % h)
def test_certificate_cases(solver_mod, ref, layout, horizon):
    tuned = horizon in ccs.TUNED
    for n, config in enumerate(ccs.config_names(horizon)):
        cfg, rcfg = cc.configs(ref, horizon, ccs.settings_of(horizon, config))
        cases = ccs.cases(ref, horizon, config)
        mpc = solver_mod.BatchedVSMPC(cfg, device=0, max_batch=len(cases), runtime="never" if tuned else "fallback", certify=True)
        try:
            assert mpc.uses_runtime_kernel == (not tuned)
            run_group(ref, solver_mod, layout, mpc, rcfg, cases, f"{horizon} {config}:", device_entry=n == 0,
                      permuted=n == 0 and horizon == (40, 2, 40))
        finally:
            mpc.close()


def test_per_instance_rows(solver_mod, ref, layout):
    """one batch at the paper horizon, every instance under its own row of tunables: five distinct rows"""
    items = ccs.tunable_cases(ref)
    cfgs = [cfg for cfg, _, _ in items]
    mpc = solver_mod.BatchedVSMPC(cfgs[0], device=0, max_batch=len(items), tunables=True, certify=True)
    try:
        rows = solver_mod.pack_tunables(mpc, cfgs)
        assert len({r.tobytes() for r in rows}) == len(ccs.TUNABLE_SETTINGS) >= 4
        recs = np.ascontiguousarray(np.stack([c["rec"] for _, _, c in items]))
        xs = np.ascontiguousarray(np.stack([c["x"] for _, _, c in items]))
        y, cert = mpc.certify(recs, xs, tunables=rows)
        worst = {}
        for b, (_, rcfg, case) in enumerate(items):
            check_case(ref, solver_mod, rcfg, case, y[b], cert[b], worst)
        print(len(items), "cases; worst, in bars:", {k: f"{v:.2e}" for k, v in worst.items()})
        yd, cd = certify_device(mpc, layout, recs, xs, rows=rows)
        assert np.array_equal(yd, y) and np.array_equal(cd, cert)
    finally:
        mpc.close()


def test_boxqp_table_at_the_long_horizon(solver_mod, ref, layout):
    """table H34 of tests/boxqp_pass_cases.py: 44 throttles, lower and upper bounds active at the optimum"""
    cfg, rcfg, cases = ccs.boxqp_cases(ref)
    mpc = solver_mod.BatchedVSMPC(cfg, device=0, max_batch=len(cases), certify=True)
    try:
        run_group(ref, solver_mod, layout, mpc, rcfg, cases, "H34:")
    finally:
        mpc.close()
