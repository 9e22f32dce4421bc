"""The solve kernels on records away from the synthetic workloads (tests/record_cases.py).

Every record synth.make_batch builds ties together fields that the kernels read through index arithmetic and duplicated
formulas of their own (IN_T0 and X0's thrusts, IN_RPY and X0's RPY, IN_PREF / IN_RPYINIT and the window's first column,
a window that is zero or constant on nine of its twelve rows, gravity along z, a symmetric inertia, wR_b = R(IN_RPY)).
Here the three HIP implementations that read the record -- the tuned kernels in both condensing forms, solve_kernel_rt
and sens_kernel_rt -- are compared with the oracle on records without those ties, on edge records, and with one entry
of the record changed at a time, at the project's bars (test_gpu_config_parity.py's header): solution and first move
1e-8 relative with equal active-set iteration counts and statuses, linearisation 1e-13, condensed M and gradient row
1e-12 (paper horizon) / 1e-11, factor L 1e-11 / 1e-10, form against form 1e-13 (M) and 1e-12 / 1e-11 (L), runtime
kernel against tuned 1e-10.  The reference side sits at 3e-12 or better on every one of these records
(tests/test_record_cases.py)."""
import numpy as np
import pytest

from conftest import relerr
import config_cases as cc
import record_cases as rc
from test_gpu_config_parity import _check_entry_points, _check_solution, _tuned

pytestmark = pytest.mark.gpu


def _cfgs(ref, horizon, config="default"):
    return cc.configs(ref, horizon, cc.all_distinct(horizon) if config == "ALL_DISTINCT" else {})


@pytest.mark.parametrize("config", ["default", "ALL_DISTINCT"])
@pytest.mark.parametrize("horizon", cc.HORIZONS)
def test_kernels_match_oracle_phase_by_phase(solver_mod, ref, layout, horizon, config):
    """all-distinct + edge records; config ALL_DISTINCT breaks the configuration's ties at the same time"""
    import algo_model
    cfg, rcfg = _cfgs(ref, horizon, config)
    names, recs = rc.records(cfg)
    paper = tuple(horizon) == cc.PAPER
    probe = [1, 2, names.index("pitch_1.45_roll_0.7"), names.index("lateral_30m")]    # held, free + saturated, two edges
    m = _tuned(solver_mod, cfg, len(recs))
    rt = solver_mod.BatchedVSMPC(cfg, device=0, max_batch=len(recs), runtime="always")
    try:
        # P0: the linearisation of every record
        A, Bj, Bt, c, dt = m.linearize(recs)
        np.testing.assert_allclose(dt, ref.dt_schedule(rcfg), rtol=0, atol=cc.dt_atol(rcfg))
        worst = 0.0
        for b, rec in enumerate(recs):
            Ar, Bjr, Btr, cr = ref.linearize(rcfg, rec)
            e = (relerr(A[b], Ar), relerr(Bj[b], Bjr), relerr(Bt[b], Btr), relerr(c[b], cr))
            worst = max(worst, *e)
            assert e[0] < 1e-13 and e[1] < 1e-14 and e[2] < 1e-13 and e[3] < 1e-13, (names[b], e)
        print(f"linearisation worst {worst:.2e}")
        # the reference-ordered dense QP
        for b in probe:
            H, g, Ac, lo, hi = m.assemble_dense(recs[b])
            Hr, gr, Acr, lor, hir = ref.assemble_dense(rcfg, recs[b])
            np.testing.assert_array_equal(H, Hr)
            assert relerr(g, gr) < 1e-14 and relerr(Ac, Acr) < 1e-13, names[b]
            assert relerr(lo, lor) < 1e-13 and relerr(hi, hir) < 1e-13, names[b]
            assert np.array_equal(Ac == 0, Acr == 0)
        # P1-P3: condensed Hessian, gradient row and factor, in both condensing forms where the horizon has both
        prev = m.set_kernel_form(solver_mod.KERNEL_FORM_AUTO)
        try:
            forms = {}
            for form in (solver_mod.KERNEL_FORM_STRUCTURED, solver_mod.KERNEL_FORM_SYRK):
                try:
                    m.set_kernel_form(form)
                except ValueError:
                    assert tuple(horizon) == (21, 9, 15) and form == solver_mod.KERNEL_FORM_STRUCTURED, (horizon, form)
                    continue
                forms[form] = (m.solve(recs), [m.debug_condensed(recs[b])[:2] for b in probe])
        finally:
            m.set_kernel_form(prev)
        assert solver_mod.KERNEL_FORM_SYRK in forms and (len(forms) == 2 or tuple(horizon) == (21, 9, 15))
        bM, bL = (1e-12, 1e-11) if paper else (1e-11, 1e-10)
        for k, b in enumerate(probe):
            Me, ge, Le = algo_model.reduced_condensed(rcfg, ref, recs[b])
            nz = Me.shape[0]
            for form, (_, cond) in forms.items():
                M, Lf = cond[k]
                Mh = np.tril(M[:nz, :nz])
                Mh = Mh + np.tril(Mh, -1).T
                eM, eg = relerr(Mh, Me), relerr(M[nz, :nz], ge)
                eL, eLg = relerr(np.tril(Lf[:nz, :nz]), Le), relerr(Lf[nz, :nz], np.linalg.solve(Le, ge))
                print(f"form {form} {names[b]}: M {eM:.2e} g {eg:.2e} L {eL:.2e} L^-1 g {eLg:.2e}")
                assert eM < bM and eg < bM, (form, names[b], eM, eg)
                assert eL < bL and eLg < bL, (form, names[b], eL, eLg)
            if len(forms) == 2:
                (Ma, La), (Mb, Lb) = (forms[f][1][k] for f in (solver_mod.KERNEL_FORM_STRUCTURED, solver_mod.KERNEL_FORM_SYRK))
                assert relerr(np.tril(Ma[:nz + 1, :nz]), np.tril(Mb[:nz + 1, :nz])) < 1e-13, names[b]
                assert relerr(np.tril(La[:nz + 1, :nz]), np.tril(Lb[:nz + 1, :nz])) < bL / 10, names[b]
        xs = None
        for form, (sol, _) in forms.items():             # each form's solve against the oracle, per output group
            print(f"form {form}:")
            xs = _check_solution(ref, rcfg, layout, recs, *sol)
        if len(forms) == 2:
            a, b_ = forms[solver_mod.KERNEL_FORM_STRUCTURED][0], forms[solver_mod.KERNEL_FORM_SYRK][0]
            np.testing.assert_array_equal(a[2], b_[2])
            np.testing.assert_array_equal(a[3], b_[3])
            assert relerr(a[0], b_[0]) < bL and relerr(a[1], b_[1]) < bL
        # the handle's own (automatic) form
        x, fm, st, it = m.solve(recs)
        print("automatic form:")
        xs = _check_solution(ref, rcfg, layout, recs, x, fm, st, it)
        v = x[:, rcfg.off_throttle:]
        vmin, vmax = ref.throttle_bounds(rcfg)
        held = recs[:, layout.IN_HOLD] != 0.0
        assert held[names.index("hold_1e-300")] and held[names.index("hold_-1")] and not held[names.index("hold_-0.0")]
        assert v[:, 4:].min() >= vmin and v[:, 4:].max() <= vmax
        assert v[~held, :4].min() >= vmin and v[~held, :4].max() <= vmax
        vprev = ref.v_of_throttle(recs[:, layout.IN_UPREV:layout.IN_UPREV + 4])
        np.testing.assert_allclose(v[held, :4], vprev[held], rtol=0, atol=1e-15)       # the pin, whatever the flag's value
        assert it.max() > 1
        # the runtime-sized kernel: an independent HIP implementation of the same solve, against the oracle and the tuned one
        xr_, fmr, str_, itr_ = rt.solve(recs)
        assert rt.uses_runtime_kernel
        np.testing.assert_array_equal(st, str_)
        np.testing.assert_array_equal(it, itr_)
        assert relerr(xr_, xs) < 1e-8, relerr(xr_, xs)
        assert relerr(xr_, x) < 1e-10 and relerr(fmr, fm) < 1e-10, (relerr(xr_, x), relerr(fmr, fm))
    finally:
        m.close()
        rt.close()


def _one_at_a_time(solver_mod, ref, layout, horizon, cases, runtime):
    cfg, rcfg = _cfgs(ref, horizon)
    base = cases[0][2]
    recs = np.array([base] + [r for _, r, _ in cases])
    m = solver_mod.BatchedVSMPC(cfg, device=0, max_batch=len(recs), runtime=runtime)
    try:
        assert m.uses_runtime_kernel == (runtime == "always")
        x, fm, st, it = m.solve(recs)                     # one launch for all of them
    finally:
        m.close()
    xs = _check_solution(ref, rcfg, layout, recs, x, fm, st, it)
    moved = [relerr(xs[b], xs[0]) for b in range(1, len(recs))]
    print(f"{len(cases)} cases, least response of the oracle {min(moved):.2e}")
    for (name, _, _), mv in zip(cases, moved):            # per case: one that proves nothing fails loudly
        assert mv >= 1e-5, (name, mv)


def test_one_entry_at_a_time(solver_mod, ref, layout):
    """Every live entry of the record on its own, tuned kernel, paper horizon: the kernel follows the oracle, and the
    oracle's solution differs from the base record's by at least 1e-5 relative -- an entry the kernel ignored, or read
    from its twin's slot (which holds another value in the all-distinct base), cannot pass."""
    cfg, _ = _cfgs(ref, cc.PAPER)
    cases = list(rc.one_at_a_time(cfg))
    assert len(cases) == 281
    _one_at_a_time(solver_mod, ref, layout, cc.PAPER, cases, "never")


@pytest.mark.parametrize("horizon, runtime", [(cc.PAPER, "always"), ((21, 9, 15), "never"), ((34, 14, 24), "never")])
def test_one_entry_per_field_on_the_other_kernels(solver_mod, ref, layout, horizon, runtime):
    """solve_kernel_rt, the SYRK-only kernel and the STRUCT_LONG kernel: one entry (or a few) of every field"""
    cfg, _ = _cfgs(ref, horizon)
    cases = rc.one_per_field(cfg)
    assert len(cases) == len(rc.REPRESENTATIVE)
    _one_at_a_time(solver_mod, ref, layout, horizon, cases, runtime)


@pytest.mark.parametrize("horizon, runtime", [(cc.PAPER, "never"), (cc.PAPER, "always"), ((34, 14, 24), "never")])
def test_dead_entries_change_nothing(solver_mod, ref, layout, horizon, runtime):
    """the yaw of IN_RPY and the last window column: every output bit-identical to the base record's -- solve and
    sensitivity kernels"""
    cfg, _ = _cfgs(ref, horizon)
    cases = list(rc.dead_cases(cfg))
    assert len(cases) == 13
    recs = np.array([cases[0][2]] + [r for _, r, _ in cases])
    m = solver_mod.BatchedVSMPC(cfg, device=0, max_batch=len(recs), runtime=runtime, sensitivity=True)
    try:
        assert m.uses_runtime_kernel == (runtime == "always")
        out = dict(zip(("x", "first_move", "status", "iters"), m.solve(recs)))
        sens = m.solve_sensitivity(recs)
    finally:
        m.close()
    assert (out["status"] == layout.STATUS_SOLVED).all() and (sens["status"] == layout.STATUS_SOLVED).all()
    assert set(sens) >= {"x", "first_move", "status", "iters", "dx_dx0", "dfm_dx0", "active", "flags"}
    for res in (out, sens):
        for key, val in res.items():
            for b in range(1, len(recs)):
                np.testing.assert_array_equal(val[b], val[0], err_msg=f"{key} {cases[b - 1][0]}")


@pytest.mark.parametrize("horizon, runtime", [(cc.PAPER, "never"), (cc.PAPER, "always"), ((34, 14, 24), "never")])
def test_sensitivities_on_all_distinct_records(solver_mod, ref, layout, horizon, runtime):
    """test_gpu_sensitivity.test_jacobians_match_model's checks and its rule for flagged instances, on the all-distinct
    records"""
    import sensitivity_model as sm
    cfg, rcfg = _cfgs(ref, horizon)
    recs = rc.distinct_records(cfg)
    m = solver_mod.BatchedVSMPC(cfg, device=0, max_batch=len(recs), runtime=runtime, sensitivity=True)
    try:
        assert m.uses_runtime_kernel == (runtime != "never")
        out = m.solve_sensitivity(recs)
    finally:
        m.close()
    assert (out["status"] == layout.STATUS_SOLVED).all(), out["status"]
    checked, worst = 0, 0.0
    for b, rec in enumerate(recs):
        x, J, active = sm.kkt_jacobian(rcfg, rec)
        if out["flags"][b] & layout.SENS_DEGENERATE and not np.array_equal(out["active"][b], active):
            continue   # a weakly or nearly active throttle may settle on either side in the two solvers
        np.testing.assert_array_equal(out["active"][b], active)
        assert relerr(out["x"][b], x) < 1e-8, b
        assert relerr(out["dx_dx0"][b], J) < 1e-8, (b, relerr(out["dx_dx0"][b], J))
        dfm = sm.first_move_jacobian(rcfg, x[rcfg.off_throttle:rcfg.off_throttle + 4], J)
        assert relerr(out["dfm_dx0"][b], dfm) < 1e-8, (b, relerr(out["dfm_dx0"][b], dfm))
        assert out["flags"][b] == sm.condensed_jacobian(rcfg, rec)["flags"], b
        worst = max(worst, relerr(out["dx_dx0"][b], J), relerr(out["dfm_dx0"][b], dfm))
        checked += 1
    print(f"Jacobians worst {worst:.2e} on {checked} records")
    assert checked >= len(recs) - 1, out["flags"]


def test_entry_points_are_bit_identical_on_all_distinct_records(solver_mod, ref, layout):
    """solve_device, the pinned direct-store path and tick against solve on one all-distinct batch"""
    cfg, _ = _cfgs(ref, cc.PAPER)
    recs = np.concatenate([rc.distinct_records(cfg, seed) for seed in (rc.SEED, 101, 202, 303)])
    assert len(recs) == 24 and len({r.tobytes() for r in recs}) == 24
    _, _, _, it = _check_entry_points(solver_mod, layout, cfg, recs)
    assert it.max() > 1
