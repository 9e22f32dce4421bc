"""tests/derivative_cases.py: the families the derivative kernels are tested on (test_gpu_adjoint_records.py,
test_gpu_sensitivity_records.py) are ones on which the CPU references need no allowance -- both routes of adjoint_model
and of sensitivity_model settle on the same active set, neither raises a flag, the mirrors sit inside the dense routes'
bars -- and together they hold every kind of active set the GPU tests are there for.  The dense-KKT adjoint is held to
central differences of the oracle on three of the tie-broken records.  Conditions on the tests' inputs and references,
not on the kernels."""
import dataclasses

import numpy as np
import pytest

from conftest import relerr
import adjoint_model as am
import boxqp_pass_cases as bp
import derivative_cases as dc
import sensitivity_model as sm
from test_adjoint_model import _loss, _solve

# worst distance of the mirror from the dense route per family, in units of test_adjoint_model.py (b)'s bar, as
# test_references_agree_on_every_record prints it: records_17_7_12 1.4e-4 (hold_-1), records_20_5_9 2.4e-5,
# records_6_2_3 4.4e-5, shrinking 2.3e-5, growing 1.7e-4, H21_box 2.4e-4 (H21_box[0]), H34 2.1e-5


@pytest.mark.parametrize("name", dc.FAMILIES)
def test_references_agree_on_every_record(ref, name):
    _, cfg, rcfg, recs, names = dc.family(ref, name)
    assert (cfg.n_iter, cfg.n_iter_small, cfg.control_horizon) == (rcfg.n_iter, rcfg.n_iter_small, rcfg.control_horizon)
    assert len(recs) == dc.SIZES[name] <= 20 and len({r.tobytes() for r in recs}) == len(recs)
    worst, worst_j = (0.0, None), 0.0
    for b in range(len(recs)):
        k, c = dc.adjoint_refs(ref, name, b)
        assert c["status"] == 1 and k["flags"] == 0 and c["flags"] == 0, (names[b], c["status"], k["flags"], c["flags"])
        np.testing.assert_array_equal(c["active"], k["active"], err_msg=names[b])
        e = dc.field_errors(c["grad_x0"], c["grad_cfg"], k["grad_x0"], k["grad_cfg"])
        worst = max(worst, (e, names[b]))
        assert e <= 1.0, (names[b], e)
        (x, J, active), cj = dc.jacobian_refs(ref, name, b)
        assert cj["status"] == 1 and cj["flags"] == 0, (names[b], cj["status"], cj["flags"])
        np.testing.assert_array_equal(active, k["active"], err_msg=names[b])
        np.testing.assert_array_equal(cj["active"], active, err_msg=names[b])
        ej = relerr(cj["J"], J)
        worst_j = max(worst_j, ej)
        assert ej < 1e-8, (names[b], ej)
        v0 = x[rcfg.off_throttle:rcfg.off_throttle + 4]
        assert relerr(sm.first_move_jacobian(rcfg, cj["v"][:4], cj["J"]), sm.first_move_jacobian(rcfg, v0, J)) < 1e-8, names[b]
    print(f"{name}: mirror against the dense route {worst[0]:.2e} of the bar ({worst[1]}), Jacobians {worst_j:.2e}")


def test_families_cover_the_active_sets(ref):
    """over the families together, so that a later edit of a table cannot empty the GPU tests without notice"""
    seen = set()
    box_grads = {}
    for name, cfg, rcfg, recs, names in dc.families(ref):
        horizon = (cfg.n_iter, cfg.n_iter_small, cfg.control_horizon)
        lo, hi = box_grads.get(horizon, (False, False))
        for b, rec in enumerate(recs):
            k, _ = dc.adjoint_refs(ref, name, b)
            a = k["active"]
            kd = dc.kinds(a) - {"pinned"}
            seen.add("all-bound" if "free" not in kd else "free-only" if kd == {"free"} else
                     "mixed" if {"lower", "upper"} <= kd else "lower-only" if "lower" in kd else "upper-only")
            held = rec[ref.IN_HOLD] != 0.0
            assert (a[:4] == sm.PINNED).all() if held else not (a == sm.PINNED).any(), names[b]
            g = k["grad_cfg"]
            lo, hi = lo or g[29] != 0.0, hi or g[30] != 0.0
            assert (g[29] != 0.0) == (a == sm.LOWER).any() and (g[30] != 0.0) == (a == sm.UPPER).any(), names[b]
        box_grads[horizon] = (lo, hi)
        if name.startswith("records"):
            for hold_name, value in (("all_distinct_1", 2.5), ("hold_-1", -1.0), ("hold_1e-300", 1e-300)):
                b = names.index(hold_name)
                assert recs[b][ref.IN_HOLD] == value and (dc.adjoint_refs(ref, name, b)[0]["active"][:4] == sm.PINNED).all()
            b = names.index("hold_-0.0")
            assert recs[b][ref.IN_HOLD] == 0.0 and np.signbit(recs[b][ref.IN_HOLD])
            assert not (dc.adjoint_refs(ref, name, b)[0]["active"] == sm.PINNED).any()
    assert seen == {"lower-only", "upper-only", "mixed", "free-only", "all-bound"}, seen
    assert set(box_grads) == {(17, 7, 12), (20, 5, 9), (6, 2, 3), (21, 9, 15), (34, 14, 24)}
    for horizon, both in box_grads.items():
        assert both == (True, True) or horizon == (6, 2, 3), (horizon, both)
    # lower and upper bounds in one instance, away from the records too; the three-tile-row horizon has 44 throttles
    assert any({"lower", "upper"} <= dc.kinds(dc.adjoint_refs(ref, t, b)[0]["active"])
               for t in ("growing", "H21_box") for b in range(dc.SIZES[t]))
    assert len(dc.adjoint_refs(ref, "H34", 0)[0]["active"]) == 44
    # a bound added in a later pass: the final set is not the first violated set, nor a subset of it
    _, _, rcfg, recs, _ = dc.family(ref, "growing")
    for rec in recs:
        sets, _ = bp.sequence(ref, rcfg, rec)
        assert sets[-1] != sets[0] and not set(sets[-1]) <= set(sets[0]), sets


def test_tuned_groups_are_flag_free(ref):
    """the inputs of test_gpu_adjoint_records.test_tuned_rows_match_the_dense_route: every record under its own
    configuration is as clean as the families are, and the third group has throttles on both limits of its box"""
    cfg, recs, names, cfgs, rcfgs = dc.tuned_cases(ref)
    _, _, _, family_recs, family_names = dc.family(ref, "records_20_5_9")
    assert len(recs) == 20 and names == family_names
    np.testing.assert_array_equal(recs, family_recs)              # the family's records: period_small builds none of them
    assert len({id(c) for c in cfgs}) == 3 and cfgs[0] is cfg
    lo = hi = False
    for b in range(len(recs)):
        k, c = dc.tuned_refs(ref, b)
        assert c["status"] == 1 and k["flags"] == 0 and c["flags"] == 0, (names[b], c["status"], k["flags"], c["flags"])
        np.testing.assert_array_equal(c["active"], k["active"], err_msg=names[b])
        assert dc.field_errors(c["grad_x0"], c["grad_cfg"], k["grad_x0"], k["grad_cfg"]) <= 1.0, names[b]
        if b % 3 == 2:
            assert (rcfgs[b].throttle_min, rcfgs[b].throttle_max) == (30.0, 85.0)
            lo, hi = lo or k["grad_cfg"][29] != 0.0, hi or k["grad_cfg"][30] != 0.0
    assert lo and hi
    # the factor from the warped limit to percent differs between the groups by far more than the bar's 1e-6 (0.8 % at
    # the upper limit, more at the lower)
    assert min(abs(am.dv_dthrottle(30.0) / am.dv_dthrottle(0.0) - 1.0), abs(am.dv_dthrottle(85.0) / am.dv_dthrottle(100.0) - 1.0)) > 5e-3


def test_affine_step_keeps_enough_active_sets(ref):
    """the inputs of test_gpu_sensitivity_records.test_affine_exactness_on_distinct_records, on the oracle"""
    _, rcfg, recs, names, d = dc.affine_cases(ref)
    assert len(recs) == 8
    kept = 0
    for b, rec in enumerate(recs):
        plus, minus = rec.copy(), rec.copy()
        plus[:26] += d[b]
        minus[:26] -= d[b]
        a = sm.kkt_jacobian(rcfg, rec)[2]
        kept += int(all(np.array_equal(sm.kkt_jacobian(rcfg, r)[2], a) for r in (plus, minus)))
    print(f"{kept} of {len(recs)} keep their active set")
    assert kept >= dc.AFFINE_KEEP_MIN, kept


# (family, record name): one HELD all-distinct record, the window 30 m apart from column to column, one record with
# lower and upper bounds (growing[3]: 1 lower, 3 upper).  Each keeps its active set under every step below.
FD_RECORDS = [("records_17_7_12", "all_distinct_3"), ("records_17_7_12", "lateral_30m"), ("growing", "growing[3]")]


@pytest.mark.parametrize("name, record", FD_RECORDS)
def test_kkt_route_matches_central_differences_on_distinct_records(ref, name, record):
    """test_adjoint_model.test_kkt_route_matches_central_differences, its steps and its bars, on tie-broken records: holds
    the dense route to something outside adjoint_model.py where the window, the hold value and the box are not special"""
    _, _, rcfg, recs, names = dc.family(ref, name)
    b = names.index(record)
    rec = recs[b]
    xbar, fmbar = (a[b].copy() for a in dc.cotangents(len(recs), rcfg.n_var))
    if rcfg.throttle_max == 100.0 or rcfg.throttle_min == 0.0:
        fmbar[12:16] = 0.0          # a limit on the clamp of the throttle-percent output: the loss has a kink in the limit
        k = am.kkt_adjoint(rcfg, rec, xbar, fmbar)
    else:
        k = dc.adjoint_refs(ref, name, b)[0]
    active = k["active"]

    def fd(cfg_p, rec_p, cfg_m, rec_m, h):
        (xp, ap), (xm, am_) = _solve(ref, cfg_p, rec_p), _solve(ref, cfg_m, rec_m)
        assert np.array_equal(ap, active) and np.array_equal(am_, active), record     # the step keeps the active set
        return (_loss(ref, cfg_p, xp, xbar, fmbar) - _loss(ref, cfg_m, xm, xbar, fmbar)) / (2.0 * h)

    g0 = np.zeros(26)
    for j in range(26):
        h = 1e-4 * (1.0 + abs(rec[j]))
        rp, rm_ = rec.copy(), rec.copy()
        rp[j] += h
        rm_[j] -= h
        g0[j] = fd(rcfg, rp, rcfg, rm_, h)
    err = np.abs(g0 - k["grad_x0"]).max()
    print(f"{record}: grad_x0 rel {err / np.abs(k['grad_x0']).max():.2e}")
    assert err <= 1e-6 * np.abs(k["grad_x0"]).max(), (record, err)
    for field, off, n in am.GRAD_FIELDS:
        gf = np.zeros(n)
        for i in range(n):
            val = getattr(rcfg, field)
            if field.startswith("throttle_"):
                h = 1e-5 / am.dv_dthrottle(val)          # 1e-5 on the warped bound, as a step in percent
                cp, cm = dataclasses.replace(rcfg, **{field: val + h}), dataclasses.replace(rcfg, **{field: val - h})
            elif n == 1:
                h = 1e-4 * max(1.0, abs(val))
                cp, cm = dataclasses.replace(rcfg, **{field: val + h}), dataclasses.replace(rcfg, **{field: val - h})
            else:
                h = 1e-4 * max(1.0, abs(val[i]))
                vp, vm = list(val), list(val)
                vp[i] += h
                vm[i] -= h
                cp, cm = dataclasses.replace(rcfg, **{field: tuple(vp)}), dataclasses.replace(rcfg, **{field: tuple(vm)})
            gf[i] = fd(cp, rec, cm, rec, h)
        want = k["grad_cfg"][off:off + n]
        err = np.abs(gf - want).max()
        print(f"{record}: {field} rel {err / max(np.abs(want).max(), 1e-300):.2e} of {np.abs(want).max():.3e}")
        assert err <= 1e-5 * np.abs(want).max(), (record, field, err, want)
    assert k["grad_cfg"][31] == 0.0
