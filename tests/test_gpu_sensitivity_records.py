"""The sensitivity kernel (sens_kernel_rt) on records away from the synthetic workloads and on the active sets the box-QP
tests were built around (tests/derivative_cases.py; tests/test_derivative_cases.py keeps the families and their
references honest on the CPU).

Every instance of every family is compared with tests/sensitivity_model.py -- none is skipped: the references raise no
flag and agree on every active set -- and the shipped Jacobian is held to central differences of the production solve on
tie-broken records."""
import numpy as np
import pytest

from conftest import relerr
import derivative_cases as dc
import sensitivity_model as sm

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", dc.FAMILIES)
def test_jacobians_match_model_on_every_record(solver_mod, ref, layout, name):
    _, cfg, rcfg, recs, names = dc.family(ref, name)
    assert len(recs) <= 20
    runtime = dc.runtime_of(cfg)
    m = solver_mod.BatchedVSMPC(cfg, device=0, max_batch=len(recs), runtime=runtime, sensitivity=True)
    try:
        assert m.uses_runtime_kernel == (runtime != "never")
        out = m.solve_sensitivity(recs)
    finally:
        m.close()
    assert (out["status"] == layout.STATUS_SOLVED).all(), out["status"]
    worst, checked = (0.0, None), 0
    for b in range(len(recs)):
        (x, J, active), c = dc.jacobian_refs(ref, name, b)
        assert c["flags"] == 0 and out["flags"][b] == c["flags"], (names[b], out["flags"][b])
        np.testing.assert_array_equal(out["active"][b], active, err_msg=names[b])
        np.testing.assert_array_equal(out["active"][b], c["active"], err_msg=names[b])
        assert relerr(out["x"][b], x) < 1e-8, (names[b], relerr(out["x"][b], x))
        e = relerr(out["dx_dx0"][b], J)
        assert e < 1e-8, (names[b], e)
        dfm = sm.first_move_jacobian(rcfg, x[rcfg.off_throttle:rcfg.off_throttle + 4], J)
        ef = relerr(out["dfm_dx0"][b], dfm)
        assert ef < 1e-8, (names[b], ef)
        worst = max(worst, (e, names[b]), (ef, names[b]))
        checked += 1
    print(f"{name}: Jacobians worst {worst[0]:.2e} ({worst[1]}) on {checked} records")
    assert checked == len(recs) == dc.SIZES[name]


def test_affine_exactness_on_distinct_records(solver_mod, ref, layout):
    """test_gpu_sensitivity.test_affine_exactness_on_the_production_path, its step and its bar, on the six all-distinct
    records, lateral_30m and mass_12.3: needs no Python model.  On the oracle all eight keep their active set under the
    step (test_derivative_cases.test_affine_step_keeps_enough_active_sets)."""
    cfg, _, recs, names, d = dc.affine_cases(ref)
    assert cfg == layout.paper_config() and len(recs) == 8
    m = solver_mod.BatchedVSMPC(cfg, device=0, max_batch=len(recs), sensitivity=True)
    try:
        assert not m.uses_runtime_kernel
        out = m.solve_sensitivity(recs)
        plus, minus = recs.copy(), recs.copy()
        plus[:, :26] += d
        minus[:, :26] -= d
        xp, _, stp, _ = m.solve(plus)
        xm, _, stm, _ = m.solve(minus)
        ap = m.solve_sensitivity(plus, jacobian=False)["active"]
        am = m.solve_sensitivity(minus, jacobian=False)["active"]
    finally:
        m.close()
    assert (out["status"] == layout.STATUS_SOLVED).all(), out["status"]
    checked = 0
    for b in range(len(recs)):
        if out["flags"][b] or not (np.array_equal(ap[b], out["active"][b]) and np.array_equal(am[b], out["active"][b])):
            continue
        assert stp[b] == stm[b] == layout.STATUS_SOLVED
        Jd = out["dx_dx0"][b] @ d[b]
        err = np.abs((xp[b] - xm[b]) / 2.0 - Jd).max() / np.abs(Jd).max()
        print(f"{names[b]}: {err:.2e}")
        assert err <= 1e-7, (names[b], err)
        checked += 1
    assert checked >= dc.AFFINE_KEEP_MIN, checked
