"""CPU checks of tests/sensitivity_model.py, the reference that sens_kernel_rt (vsmpc_sensitivity_batch) is tested against:
  * the KKT route equals central differences of the oracle's exact solve with the initial-state bounds lo = hi perturbed;
  * the condensed route (the kernel's algorithm in numpy) equals the KKT route;
  * the solution is affine in X0 while the active set holds: x*(X0 + d) - x*(X0) = J d."""
import numpy as np
import pytest

from conftest import relerr
from config_cases import NON_DEFAULT
import sensitivity_model as sm

CASES = [(h, s) for h in ((17, 7, 12), (20, 5, 9)) for s in ("default", "non_default")]


def _cases(layout, synth, ref, horizon, settings):
    """hover and take-off (hold on and off), saturated throttles on a free tick"""
    kw = dict(n_iter=horizon[0], n_iter_small=horizon[1], control_horizon=horizon[2],
              **({} if settings == "default" else NON_DEFAULT))
    cfg, rcfg = layout.MPCConfig(**kw), ref.Config(**kw)
    hover = synth.make_batch(cfg, 2, workload="hover", first_index=3)
    takeoff = synth.make_batch(cfg, 2, workload="takeoff", first_index=3)
    hover[1, layout.IN_HOLD] = 0.0
    takeoff[1, layout.IN_HOLD] = 1.0
    sat = synth.make_batch(cfg, 2, workload="hover", first_index=40)
    sat[:, layout.IN_HOLD] = 0.0
    sat[:, layout.IN_XREF + 2::12] += 30.0
    sat[:, 22] = sat[:, 2] - sat[:, layout.IN_XREF + 2]
    return rcfg, np.concatenate([hover, takeoff, sat])


def _solve_x0(ref, rcfg, qp, j, h):
    H, g, Ac, lo, hi = qp
    r = 26 * rcfg.n_iter + j                  # initial-state row j
    lo, hi = lo.copy(), hi.copy()
    lo[r] += h
    hi[r] += h
    return ref.solve_exact(rcfg, H, g, Ac, lo, hi)[0]


@pytest.mark.parametrize("horizon, settings", CASES)
def test_kkt_route_matches_central_differences(layout, synth, ref, horizon, settings):
    rcfg, recs = _cases(layout, synth, ref, horizon, settings)
    nv = 4 * rcfg.n_vblocks
    off = rcfg.off_throttle
    bound = 0
    for b, rec in enumerate(recs):
        x, J, active = sm.kkt_jacobian(rcfg, rec)
        bound += int((active != sm.FREE).sum())
        qp = ref.assemble_dense(rcfg, rec)
        fd = np.zeros_like(J)
        for j in range(26):
            h = 1e-4 * (1.0 + abs(rec[j]))
            xp, xm = _solve_x0(ref, rcfg, qp, j, h), _solve_x0(ref, rcfg, qp, j, -h)
            for xs in (xp, xm):                # the step keeps the active set
                assert np.array_equal(xs[off:off + nv] == x[off:off + nv], active != sm.FREE), (b, j)
            fd[:, j] = (xp - xm) / (2.0 * h)
        assert relerr(fd, J) < 1e-6, (b, relerr(fd, J))
    assert bound > 0


@pytest.mark.parametrize("horizon, settings", CASES)
def test_condensed_route_matches_kkt_route(layout, synth, ref, horizon, settings):
    rcfg, recs = _cases(layout, synth, ref, horizon, settings)
    for b, rec in enumerate(recs):
        x, J, active = sm.kkt_jacobian(rcfg, rec)
        c = sm.condensed_jacobian(rcfg, rec)
        assert c["status"] == 1 and c["flags"] == 0, (b, c["status"], c["flags"])
        np.testing.assert_array_equal(c["active"], active)
        assert relerr(c["J"], J) < 1e-10, (b, relerr(c["J"], J))
        v0 = x[rcfg.off_throttle:rcfg.off_throttle + 4]
        assert relerr(sm.first_move_jacobian(rcfg, c["v"][:4], c["J"]), sm.first_move_jacobian(rcfg, v0, J)) < 1e-10


@pytest.mark.parametrize("horizon", [(17, 7, 12), (20, 5, 9)])
def test_solution_is_affine_in_x0(layout, synth, ref, horizon):
    rcfg, recs = _cases(layout, synth, ref, horizon, "default")
    rng = np.random.default_rng(7)
    for b, rec in enumerate(recs):
        x, J, active = sm.kkt_jacobian(rcfg, rec)
        d = 1e-3 * (1.0 + np.abs(rec[:26])) * rng.standard_normal(26)
        moved = rec.copy()
        moved[:26] += d
        x2, _, active2 = sm.kkt_jacobian(rcfg, moved)
        np.testing.assert_array_equal(active2, active)
        Jd = J @ d
        assert np.abs((x2 - x) - Jd).max() <= 1e-9 * np.abs(Jd).max(), b


def test_first_move_throttle_rows_vanish_on_the_clamp(ref):
    assert sm.dthrottle_dv(ref.v_of_throttle(50.0)) > 0.0
    lo, hi = ref.v_of_throttle(-1.0), ref.v_of_throttle(101.0)       # percent outside [0, 100]
    assert sm.dthrottle_dv(lo) == 0.0 and sm.dthrottle_dv(hi) == 0.0
    v = ref.v_of_throttle(40.0)
    h = 1e-6
    fd = (ref.destd_throttle(v + h) - ref.destd_throttle(v - h)) / (2 * h)
    assert abs(fd - sm.dthrottle_dv(v)) < 1e-6 * abs(fd)
