"""The records of tests/lambda_cases.py on the CPU: the reference side of tests/test_gpu_lambda_cases.py.  No GPU.

The oracle (dense, no joint reduction) solves every variant; the numpy model of the kernels' algorithm with the joint
reduction in front (algo_model.solve_model(reduce=True), its rank-deficient path: no reflector for a pivot column below
1e-300) agrees with it in both condensing forms with equal iteration counts, at the three tabled horizons, under the default
weights and under config_cases.JOINT_SPREAD (with non-uniform W the column scaling of a matrix with zero columns matters).
Bars here: 1e-10 on x and on the joint block relative to its own maximum (a hundredth of the device's 1e-8), and the joints
whose column of Lambda is zero against their closed form at lambda_cases.CLOSED_FORM_WORST, whose hundredfold is the
device's bar (profiles/lambda_cases.txt, written by `python tests/test_lambda_cases.py`)."""
import importlib
import os
import sys

import numpy as np
import pytest

import config_cases as cc
import lambda_cases as lc

SETTINGS = {"default": {}, "joint_spread": dict(w_delta_joint=cc.JOINT_SPREAD)}


def measure(ref, layout, horizon, config, forms=(None, "structured")):
    import algo_model
    import condense_model
    cfg, rcfg = cc.configs(ref, horizon, SETTINGS[config])
    names, recs = lc.records(cfg, layout)
    worst = {"x": 0.0, "joints": 0.0, "closed form, oracle": 0.0, "cond(M)": 0.0}
    worst.update({"closed form, model, " + v: 0.0 for v in lc.CLOSED_FORM_JOINTS})
    iters = []
    for name, rec in zip(names, recs):
        xo, _, ito, _ = ref.solve_instance(rcfg, rec)
        iters.append(ito)
        variant = name.split("/")[0]
        joints = lc.CLOSED_FORM_JOINTS.get(variant)
        if joints is not None:
            want = lc.closed_form_joints(rcfg, layout, rec, joints)
            U = xo[rcfg.off_joints:rcfg.off_throttle].reshape(-1, 8)
            worst["closed form, oracle"] = max(worst["closed form, oracle"], float(np.abs(U[:, joints] - want).max() / np.abs(want).max()))
        for form in forms:
            cond = None if form is None else condense_model.condense_structured
            xm, status, itm = algo_model.solve_model(rcfg, ref, rec, reduce=True, condense=cond)
            assert status == 1 and itm == ito, (name, form, status, itm, ito)
            worst["x"] = max(worst["x"], float(np.abs(xm - xo).max() / max(1.0, np.abs(xo).max())))
            worst["joints"] = max(worst["joints"], lc.joint_block_error(rcfg, xm, xo))
            if joints is not None:
                U = xm[rcfg.off_joints:rcfg.off_throttle].reshape(-1, 8)
                key = "closed form, model, " + variant
                worst[key] = max(worst[key], float(np.abs(U[:, joints] - want).max() / np.abs(want).max()))
        if variant == "zero":
            M, _, _ = algo_model.reduced_condensed(rcfg, ref, rec)
            worst["cond(M)"] = max(worst["cond(M)"], float(np.linalg.cond(M)))
    return worst, iters


@pytest.mark.parametrize("config", list(SETTINGS))
@pytest.mark.parametrize("horizon", cc.HORIZONS, ids=lambda h: "%d-%d-%d" % tuple(h))
def test_model_with_the_joint_reduction_matches_the_oracle(ref, layout, horizon, config):
    worst, iters = measure(ref, layout, horizon, config)
    print(horizon, config, {k: f"{v:.2e}" for k, v in worst.items()}, "iterations", min(iters), "to", max(iters))
    assert worst["x"] <= 1e-10 and worst["joints"] <= 1e-10
    assert worst["closed form, oracle"] <= 1e-15
    for v, ceiling in lc.CLOSED_FORM_WORST.items():
        assert worst["closed form, model, " + v] <= ceiling, v
    assert max(iters) > 1


def _reduced_gradients(ref, layout, variant):
    """(Q'b of the unscaled base record, Q'b of the variant of it) by algo_model.joint_reduction"""
    import algo_model
    import record_cases as rc
    cfg, rcfg = cc.configs(ref, cc.PAPER, {})
    names, recs = lc.records(cfg, layout)
    base = algo_model.reduced_model(rcfg, ref, rc.distinct_records(cfg)[2])[1]["gy"]
    return base, algo_model.reduced_model(rcfg, ref, recs[names.index(variant + "/free")])[1]["gy"]


def test_the_model_is_no_reference_for_the_gradient_at_1e_140(ref, layout):
    """A QR does not see a scaling of its matrix: Q, and with it the reduced gradient Q'b, is the unscaled record's.  The numpy
    model keeps that at 1e-8 and loses it at 1e-140, where its reflector update forms outer(v, v'A) (1e-141 x 1e-282, which
    underflows) before it multiplies by beta (1e280).  The optimum does not notice (Lambda's share of the problem is 1e-140),
    but tests/test_gpu_lambda_cases.py cannot hold the device's gradient row to this model there: it uses the unscaled
    record's Q'b instead.  If the model is ever made to keep the order beta (v'A) first, this test says so."""
    base, small = _reduced_gradients(ref, layout, "scaled_1e-8")
    assert np.abs(small - base).max() <= 1e-15 * max(1.0, np.abs(base).max())
    base, tiny = _reduced_gradients(ref, layout, "scaled_1e-140")
    print("model's Q'b at 1e-140 against the unscaled record's:", np.abs(tiny - base).max(), "of", np.abs(base).max())
    assert np.abs(tiny - base).max() >= 1e-6


def write_profile(root):
    import vsmpc_ref as ref
    from conftest import PKG
    layout = importlib.import_module(PKG + ".layout")
    lines = ["Reference side of tests/test_gpu_lambda_cases.py (python tests/test_lambda_cases.py), CPU only: the 13 variants of",
             "tests/lambda_cases.py on a free and a held tie-broken record.  algo_model.solve_model(reduce=True), SYRK and",
             "structured condensing, against oracle/vsmpc_ref.py solve_instance (equal iteration counts asserted):",
             "x relative to max(1, |x|_inf); the joint block relative to its own maximum; the joints whose column of Lambda",
             "is zero against U[k] = -w_reg q_err[k] / (w_dq[k] + w_reg), relative to the largest of them; cond(M) of the",
             "reduced condensed Hessian at Lambda = 0.", ""]
    top = {v: 0.0 for v in lc.CLOSED_FORM_WORST}
    for h in cc.HORIZONS:
        for config in SETTINGS:
            worst, iters = measure(ref, layout, h, config)
            for v in top:
                top[v] = max(top[v], worst["closed form, model, " + v])
            lines.append(f"{str(tuple(h)):13s} {config:13s} " + "  ".join(f"{k} {v:.1e}" for k, v in worst.items())
                         + f"  iterations {min(iters)}..{max(iters)}")
    lines += ["", "closed form, worst over the above / ceiling asserted (lambda_cases.CLOSED_FORM_WORST) / device's bar (100 times):"]
    lines += [f"  {v:24s} {top[v]:.2e} / {lc.CLOSED_FORM_WORST[v]:.1e} / {lc.CLOSED_FORM_BAR[v]:.1e}" for v in top]
    base, tiny = _reduced_gradients(ref, layout, "scaled_1e-140")
    lines += ["", "scaled_1e-140: the model's reduced gradient Q'b differs from the unscaled record's (equal in exact arithmetic) by",
              f"{np.abs(tiny - base).max():.1e} of {np.abs(base).max():.1e}: outer(v, v'A) underflows in the model's reflector update.  The optimum does not",
              "depend on it; the device's gradient row is held to the unscaled record's Q'b there (tests/test_gpu_lambda_cases.py)."]
    with open(os.path.join(root, "profiles", "lambda_cases.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "oracle"), os.path.join(root, "tests")):
        sys.path.insert(0, p)
    write_profile(root)
