"""The executable model of the record adjoint (tests/adjoint_record_model.py) on the CPU: the dense route against central
differences of the oracle's solve, the numpy mirror of adjoint_record_kernel_rt against the dense route on the 80 instances
of derivative_cases and at the edge horizons, consistency with adjoint_model, the exact zeros, and planted defects.

Bars.  (a) Dense route against central differences of vsmpc_ref.solve_instance, loss xbar' x + fmbar' first_move: per field
|err| <= 1e-5 |field|_inf + 2e-8 max |grad_in|.  Measured with steps 1e-5 and 1e-6 times max(1, |p|) on the seven instances
of adjoint_record_cases.FD: the whole record agrees to 3.6e-10 (step 1e-5) and 2.3e-9 (step 1e-6) of max |grad_in| -- the
difference quotient of a solve that is exact to ~1e-13 carries noise ~1e-13 |L| / h, which grows as the step shrinks -- and
above that noise no field differs by more than 1e-8 of itself.  The floor is 5 times the worst whole-record figure, rounded
up; 1e-5 is the bar the project holds its weight gradients to (test_adjoint_model.py).  The test runs step 1e-5.
(b) Mirror against the dense route: the project's bar form, per field 1e-6 |field|_inf + 1e-12 max |gradient|."""
import numpy as np
import pytest

import adjoint_model as am
import adjoint_record_cases as cases
import adjoint_record_model as arm
import config_cases as cc
import derivative_cases as dc
import record_cases as rc

FD_BAR, FD_FLOOR, FD_STEP = 1e-5, 2e-8, 1e-5
MUTATION_MISS = 100.0        # a planted defect misses bar (b) by at least this factor on some family


def _loss(ref, rcfg, rec, xbar, fmbar):
    x = ref.solve_instance(rcfg, rec)[0]
    return float(xbar @ x + fmbar @ ref.first_move_vector(rcfg, x))


@pytest.mark.parametrize("name, b", cases.FD)
def test_dense_route_matches_central_differences_of_the_solve(ref, name, b):
    rcfg, rec, xbar, fmbar = cases.instance(ref, name, b)
    k = cases.dense(ref, name, b)
    fd = np.zeros(rcfg.n_in)
    for i in range(rcfg.n_in):
        if i == ref.IN_HOLD:
            continue
        h = FD_STEP * max(1.0, abs(rec[i]))
        p, m = rec.copy(), rec.copy()
        p[i] += h
        m[i] -= h
        fd[i] = (_loss(ref, rcfg, p, xbar, fmbar) - _loss(ref, rcfg, m, xbar, fmbar)) / (2.0 * h)
    e = arm.field_errors(rcfg, k["grad_in"], fd, FD_BAR, FD_FLOOR)
    nonzero = int((k["grad_in"] != 0.0).sum())
    print(f"{name}[{b}]: {e:.2e} of the bar; whole record {np.abs(fd - k['grad_in']).max() / np.abs(fd).max():.2e}; "
          f"{nonzero} of {rcfg.n_in - len(arm.dead(rcfg)) - 1} live entries non-zero")
    assert e <= 1.0, (name, b, e)
    assert nonzero >= rcfg.n_in - len(arm.dead(rcfg)) - 1 - 4          # (alpha = 0 zeroes the gravity entries)


def test_one_central_difference_is_exact_off_the_nonlinear_fields(ref):
    """kkt_record_adjoint extrapolates only on MASS, INERTIA, RPY: everywhere else the assembly is affine or quadratic in
    the entry, so the second difference quotient changes nothing but rounding (~1e-16 |Ac| / h of the terms summed)"""
    rcfg, rec, xbar, fmbar = cases.instance(ref, "records_6_2_3", 0)
    one = cases.dense(ref, "records_6_2_3", 0)["grad_in"]
    two = arm.kkt_record_adjoint(rcfg, rec, xbar, fmbar, richardson=True)["grad_in"]
    e = arm.field_errors(rcfg, one, two, 1e-9, 1e-12)
    print(f"one quotient against two: {e:.2e} of 1e-9 |field| + 1e-12 max")
    assert e <= 1.0


def _mirror_against_dense(rcfg, c, k, flags):
    """worst field error of the mirror against the dense route in units of bar (b), or None where a flagged instance settled
    on another side in the two solvers"""
    assert c["solved"]
    if not np.array_equal(c["active"], k["active"]):
        assert flags & am.DEGENERATE
        return None
    return arm.field_errors(rcfg, c["grad_in"], k["grad_in"])


@pytest.mark.parametrize("name", dc.FAMILIES)
def test_mirror_matches_dense_route(ref, name):
    _, _, rcfg, recs, names = dc.family(ref, name)
    checked, worst = 0, 0.0
    for b in range(len(recs)):
        flags = dc.adjoint_refs(ref, name, b)[1]["flags"]
        e = _mirror_against_dense(rcfg, cases.mirror(ref, name, b), cases.dense(ref, name, b), flags)
        if e is None:
            continue
        assert e <= 1.0, (names[b], e)
        worst, checked = max(worst, e), checked + 1
    print(f"{name}: {checked} of {len(recs)} instances, worst {worst:.2e} of the bar")
    assert checked >= len(recs) - 1


@pytest.mark.parametrize("horizon", cases.EDGE)
def test_mirror_matches_dense_route_at_the_edge_horizons(ref, horizon):
    _, rcfg, recs, xbar, fmbar = cases.edge(ref, horizon)
    for b in range(len(recs)):
        c, k = cases.edge_mirror(ref, horizon, b), cases.edge_dense(ref, horizon, b)
        np.testing.assert_array_equal(c["active"], k["active"])
        e = arm.field_errors(rcfg, c["grad_in"], k["grad_in"])
        print(f"{horizon}[{b}]: {e:.2e} of the bar")
        assert e <= 1.0, (horizon, b, e)
    if horizon == (2, 2, 2):       # a window of one column: every node tracks it, nothing of it is dead
        assert arm.dead(rcfg) == [ref.IN_RPY + 2]
        assert (k["grad_in"][ref.IN_XREF:] != 0.0).all()


@pytest.mark.parametrize("name, b", [("records_6_2_3", 0), ("records_6_2_3", 3)])
def test_consistent_with_the_adjoint_model(ref, name, b):
    """grad_in[X0] is kkt_adjoint's grad_x0; grad_model is the dense route with A, Bj, Bt, c moved directly"""
    rcfg, rec, xbar, fmbar = cases.instance(ref, name, b)
    k = cases.dense(ref, name, b, model=True)
    c = cases.mirror(ref, name, b)
    x0 = dc.adjoint_refs(ref, name, b)[0]["grad_x0"]
    gall = np.abs(k["grad_in"]).max()
    assert np.abs(k["grad_in"][:26] - x0).max() <= 1e-6 * np.abs(x0).max() + 1e-12 * gall
    np.testing.assert_array_equal(c["grad_in"][:26], dc.adjoint_refs(ref, name, b)[1]["grad_x0"])
    mall = np.abs(k["grad_model"]).max()
    for lo, hi in ((arm.GM_A, arm.GM_BJ), (arm.GM_BJ, arm.GM_BT), (arm.GM_BT, arm.GM_C), (arm.GM_C, arm.GRAD_MODEL_SIZE)):
        want = k["grad_model"][lo:hi]
        assert np.abs(c["grad_model"][lo:hi] - want).max() <= 1e-6 * np.abs(want).max() + 1e-12 * mall, (lo, hi)
    assert c["grad_model"].shape == (1014,) and (c["grad_model"] != 0.0).sum() > 900


def test_exact_zeros(ref):
    """the dead entries and the hold flag on both routes; the jet entries with use_jet_dynamic = False"""
    for name, b in (("records_6_2_3", 0), ("records_6_2_3", 3), ("records_17_7_12", 1)):
        rcfg = cases.instance(ref, name, b)[0]
        for g in (cases.dense(ref, name, b)["grad_in"], cases.mirror(ref, name, b)["grad_in"]):
            assert len(arm.dead(rcfg)) == 13
            for i in arm.dead(rcfg) + [ref.IN_HOLD]:
                assert g[i] == 0.0 and not np.signbit(g[i]), (name, b, i)
    cfg, rcfg = cc.configs(ref, (6, 2, 3), {"use_jet_dynamic": False})
    _, recs = rc.records(cfg)
    xbar, fmbar = dc.cotangents(len(recs), rcfg.n_var)
    for b in (0, 3):
        k = arm.kkt_record_adjoint(rcfg, recs[b], xbar[b], fmbar[b])
        c = arm.condensed_record_adjoint(rcfg, recs[b], xbar[b], fmbar[b])
        assert arm.field_errors(rcfg, c["grad_in"], k["grad_in"]) <= 1.0
        for f, off, n in arm.fields(rcfg):
            if f in arm.JET_FIELDS:
                assert not k["grad_in"][off:off + n].any() and not c["grad_in"][off:off + n].any(), f
        assert c["grad_in"][ref.IN_UPREV:ref.IN_UPREV + 4].any()          # the direct part stays


def mutation_table(ref):
    """{mutation: {family: worst error of the mutated mirror against the dense route, in units of bar (b)}}"""
    table = {}
    for mut in arm.MUTATIONS:
        table[mut] = {}
        for name in dc.FAMILIES:
            _, _, rcfg, recs, _ = dc.family(ref, name)
            worst = 0.0
            for b in range(len(recs)):
                k = cases.dense(ref, name, b)
                c = arm.condensed_record_adjoint(*cases.instance(ref, name, b), mutation=mut)
                if np.array_equal(c["active"], k["active"]):
                    worst = max(worst, arm.field_errors(rcfg, c["grad_in"], k["grad_in"]))
            table[mut][name] = worst
    return table


def test_planted_defects_miss_the_bar(ref):
    """each defect of adjoint_record_model.MUTATIONS, planted in the mirror, misses bar (b) by orders of magnitude on at least
    one family (which families catch which: profiles/adjoint_record_mutations.txt)"""
    table = mutation_table(ref)
    for mut, row in table.items():
        print(mut, {k: f"{v:.1e}" for k, v in row.items()})
        assert max(row.values()) >= MUTATION_MISS, (mut, row)
    held = [n for n in dc.FAMILIES if table["drop_pin"][n] >= MUTATION_MISS]
    assert held, "no family with a hold record catches the dropped pin term"
