"""CPU checks of tests/adjoint_model.py, the reference that adjoint_kernel_rt (vsmpc_adjoint_batch) is tested against:
  (a) the dense-KKT route equals central differences of the oracle's exact solve, for X0, for every config field of a
      gradient row (weights through dataclasses.replace on the oracle Config) and for the throttle limits in percent;
  (b) the condensed route (the kernel's algorithm in numpy) equals the dense-KKT route;
  (c) grad_x0 equals J^T xbar + (dfm/dX0)^T fmbar with J from sensitivity_model.kkt_jacobian;
  (d) with fmbar alone, the throttle-percent rows contribute nothing on the clamp."""
import dataclasses

import numpy as np
import pytest

from config_cases import NON_DEFAULT
import adjoint_model as am
import sensitivity_model as sm
from test_sensitivity_model import _cases

_kkt = {}


def _cotangents(rcfg, b):
    rng = np.random.default_rng(100 + b)
    return rng.standard_normal(rcfg.n_var), rng.standard_normal(24)


def _loss(ref, rcfg, x, xbar, fmbar):
    return float(xbar @ x + fmbar @ ref.first_move_vector(rcfg, x))


def _solve(ref, rcfg, rec):
    """(x, active) of the oracle, the active set read by comparing the throttles with the bounds"""
    H, g, Ac, lo, hi = ref.assemble_dense(rcfg, rec)
    x = ref.solve_exact(rcfg, H, g, Ac, lo, hi)[0]
    nxs, nv = 26 * (rcfg.n_iter + 1), 4 * rcfg.n_vblocks
    tlo, thi = lo[nxs:nxs + nv], hi[nxs:nxs + nv]
    return x, sm.throttle_states(x[rcfg.off_throttle:rcfg.off_throttle + nv], tlo, thi, tlo == thi)


def _field_bar(field, grad_all, rel):
    """|err| <= rel |field|_inf + 1e-12 max |all gradient entries|: the absolute term is the level at which an entry that is
    exactly zero on one route sits on the other (a dense solve's rounding, 2e-15 of the largest entry measured)"""
    return rel * np.abs(field).max() + 1e-12 * np.abs(grad_all).max()


def _fd_cases(layout, synth, ref):
    out = []
    for settings in ("default", "non_default"):
        rcfg, recs = _cases(layout, synth, ref, (17, 7, 12), settings)
        out += [(rcfg, rec) for rec in recs]
    rcfg, recs = _cases(layout, synth, ref, (20, 5, 9), "non_default")
    out.append((rcfg, recs[5]))     # saturated: a lower-active and an upper-active free throttle
    return out


def test_kkt_route_matches_central_differences(layout, synth, ref):
    kinds = set()
    for b, (rcfg, rec) in enumerate(_fd_cases(layout, synth, ref)):
        xbar, fmbar = _cotangents(rcfg, b)
        if rcfg.throttle_max == 100.0 or rcfg.throttle_min == 0.0:
            # the limits coincide with the clamp of the throttle-percent output: with a first throttle on such a limit the
            # loss itself has a kink in that limit (the percent rows are covered by the other configuration and by (c), (d))
            fmbar[12:16] = 0.0
        k = am.kkt_adjoint(rcfg, rec, xbar, fmbar)
        active = k["active"]
        kinds |= {int(s) for s in active}

        def fd(cfg_p, rec_p, cfg_m, rec_m, h):
            (xp, ap), (xm, am_) = _solve(ref, cfg_p, rec_p), _solve(ref, cfg_m, rec_m)
            assert np.array_equal(ap, active) and np.array_equal(am_, active), b     # the step keeps the active set
            return (_loss(ref, cfg_p, xp, xbar, fmbar) - _loss(ref, cfg_m, xm, xbar, fmbar)) / (2.0 * h)

        g0 = np.zeros(26)
        for j in range(26):
            h = 1e-4 * (1.0 + abs(rec[j]))
            rp, rm_ = rec.copy(), rec.copy()
            rp[j] += h
            rm_[j] -= h
            g0[j] = fd(rcfg, rp, rcfg, rm_, h)
        err = np.abs(g0 - k["grad_x0"]).max()
        print(f"case {b}: grad_x0 rel {err / np.abs(k['grad_x0']).max():.2e}")
        assert err <= 1e-6 * np.abs(k["grad_x0"]).max(), (b, err)
        for name, off, n in am.GRAD_FIELDS:
            gf = np.zeros(n)
            for i in range(n):
                val = getattr(rcfg, name)
                if name.startswith("throttle_"):
                    # 1e-5 on the warped bound, as a step in percent
                    h = 1e-5 / am.dv_dthrottle(val)
                    cp, cm = dataclasses.replace(rcfg, **{name: val + h}), dataclasses.replace(rcfg, **{name: val - h})
                elif n == 1:
                    h = 1e-4 * max(1.0, abs(val))
                    if name == "w_reg_joint_pos" and val == 0.0:
                        # The one exception to the step above.  At w_reg_joint_pos = 0 (NON_DEFAULT) the gradient is 1e-4 of
                        # the row's largest entry and the step 1e-4 leaves the quotient at its rounding level: 5.6e-9 on
                        # 1.8e-4, 3.1e-5 relative on the first such record, whatever the adjoint returns.  The weight is
                        # added to joint weights of 200 and more, so a step of 0.1 has a truncation error of
                        # (0.1 / 200)^2 = 2.5e-7 relative and a thousandth of the rounding.
                        h = 0.1
                    cp, cm = dataclasses.replace(rcfg, **{name: val + h}), dataclasses.replace(rcfg, **{name: val - h})
                else:
                    h = 1e-4 * max(1.0, abs(val[i]))
                    vp, vm = list(val), list(val)
                    vp[i] += h
                    vm[i] -= h
                    cp, cm = dataclasses.replace(rcfg, **{name: tuple(vp)}), dataclasses.replace(rcfg, **{name: tuple(vm)})
                gf[i] = fd(cp, rec, cm, rec, h)
            field = k["grad_cfg"][off:off + n]
            err = np.abs(gf - field).max()
            print(f"case {b}: {name} rel {err / max(np.abs(field).max(), 1e-300):.2e} of {np.abs(field).max():.3e}")
            assert err <= 1e-5 * np.abs(field).max(), (b, name, err, field)
        assert k["grad_cfg"][31] == 0.0
    assert sm.LOWER in kinds and sm.UPPER in kinds, kinds     # both box gradients are exercised


@pytest.mark.parametrize("horizon", [(2, 2, 2), (17, 7, 12), (20, 5, 9), (34, 14, 24), (40, 2, 40)])
def test_condensed_route_matches_kkt_route(layout, synth, ref, horizon):
    for settings in ("default", "non_default"):
        rcfg, recs = _cases(layout, synth, ref, horizon, settings)
        if horizon[0] >= 34:
            recs = recs[[0, 3, 5]]           # hover, take-off with the hold, saturated
        for b, rec in enumerate(recs):
            xbar, fmbar = _cotangents(rcfg, b)
            k = am.kkt_adjoint(rcfg, rec, xbar, fmbar)
            c = am.condensed_adjoint(rcfg, rec, xbar, fmbar)
            assert c["status"] == 1
            if c["flags"] & am.DEGENERATE and not np.array_equal(c["active"], k["active"]):
                continue                     # a weakly active throttle may settle on either side in the two solvers
            np.testing.assert_array_equal(c["active"], k["active"])
            assert c["flags"] == k["flags"], (settings, b)
            gall = np.concatenate([k["grad_x0"], k["grad_cfg"]])
            assert np.abs(c["grad_x0"] - k["grad_x0"]).max() <= _field_bar(k["grad_x0"], gall, 1e-6), b
            for name, off, n in am.GRAD_FIELDS:
                f = k["grad_cfg"][off:off + n]
                err = np.abs(c["grad_cfg"][off:off + n] - f).max()
                assert err <= _field_bar(f, gall, 1e-6), (settings, b, name, err, f)


@pytest.mark.parametrize("settings", ["default", "non_default"])
def test_grad_x0_agrees_with_the_jacobian(layout, synth, ref, settings):
    rcfg, recs = _cases(layout, synth, ref, (17, 7, 12), settings)
    for b, rec in enumerate(recs):
        xbar, fmbar = _cotangents(rcfg, b)
        x, J, _ = sm.kkt_jacobian(rcfg, rec)
        D = sm.first_move_jacobian(rcfg, x[rcfg.off_throttle:rcfg.off_throttle + 4], J)
        want = J.T @ xbar + D.T @ fmbar
        for route in (am.kkt_adjoint, am.condensed_adjoint):
            got = route(rcfg, rec, xbar, fmbar)["grad_x0"]
            assert np.abs(got - want).max() <= 1e-8 * max(1.0, np.abs(want).max()), (b, route.__name__)


def test_first_move_cotangent_alone(layout, synth, ref):
    """fmbar without xbar; the throttle-percent rows vanish where the clamp to [0, 100] is active"""
    rcfg = ref.Config(throttle_min=-5.0, throttle_max=100.0)      # a lower limit below the clamp
    cfg = layout.MPCConfig(throttle_min=-5.0, throttle_max=100.0)
    rec = synth.make_batch(cfg, 1, workload="hover", first_index=3)[0]
    zero = np.zeros(rcfg.n_var)
    fmbar = np.random.default_rng(9).standard_normal(24)
    x, J, _ = sm.kkt_jacobian(rcfg, rec)
    D = sm.first_move_jacobian(rcfg, x[rcfg.off_throttle:rcfg.off_throttle + 4], J)
    got = am.condensed_adjoint(rcfg, rec, zero, fmbar)
    assert np.abs(got["grad_x0"] - D.T @ fmbar).max() <= 1e-8 * max(1.0, np.abs(D.T @ fmbar).max())
    # on the clamp: d throttle / dv = 0, so a cotangent on the percent rows alone folds to nothing
    only = np.zeros(24)
    only[12:16] = fmbar[12:16]
    v_clamped = np.full(4, ref.v_of_throttle(-1.0))
    assert np.array_equal(am.fold_first_move(rcfg, v_clamped, zero, only), zero)
    v_inside = np.full(4, ref.v_of_throttle(40.0))
    folded = am.fold_first_move(rcfg, v_inside, zero, only)
    assert np.array_equal(folded[rcfg.off_throttle:rcfg.off_throttle + 4], sm.dthrottle_dv(v_inside) * only[12:16])
    assert np.count_nonzero(folded) == 4
