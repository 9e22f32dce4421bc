"""The executable model of the rollout adjoint on the kinematic-tree plant (tests/rollout_tree_adjoint_model.py) on the CPU:
the numpy sweep against central differences of the whole loop -- rollout_adjoint_model.forward under
rollout_model.set_tree -- entry by entry, on the five loops of tests/rollout_tree_adjoint_cases.py at horizon (6, 2, 3),
ratio 4, nine ticks, on loop 1 under a joint selector that is not the default, and on loop 0 with one tick that does not
consume its move; and planted defects.

Bars: those of tests/test_rollout_adjoint_model.py (grad_state0 and grad_cfg: FD_BAR = 7.8e-8 of |field|_inf + 1e-3 max
|gradient|, step 1e-2 of the entry's scale, Richardson extrapolated) and of tests/test_rollout_param_adjoint_model.py
(grad_params and grad_traj: 9.2e-7 under the same rule), imported from there and unchanged.  Measured here, in units of
the bar: state and gains 0.004 .. 0.28 (worst: the hover loop with a tick that is not Solved, w_reg_joint_pos), parameters
0.054 .. 0.062 and tracks 0.072 .. 0.097.  Every planted
defect misses its bar by more than MUTATION_MISS = 10 on some loop: profiles/rollout_tree_adjoint_mutations.txt.

The quotients are formed in worker processes (71 entries of four loop evaluations each per scenario), a scenario each."""
import concurrent.futures
import os

import numpy as np
import pytest

import adjoint_model as am
import rollout_adjoint_model as ram
import rollout_param_adjoint_cases as rpc
import rollout_param_adjoint_model as rpm
import rollout_tree_adjoint_cases as tc
import rollout_tree_adjoint_model as rtm
import test_rollout_adjoint_model as base

L = tc.L
STEP, FLOOR_RATIO, FD_BAR, FD_FLOOR = base.STEP, base.FLOOR_RATIO, base.FD_BAR, base.FD_FLOOR
P_BAR, P_FLOOR = rpc.FD_BAR, rpc.FD_FLOOR
MUTATION_MISS = base.MUTATION_MISS
# A throttle limit's step is a hundredth of the other gains' relative step.  test_rollout_adjoint_edge_cases.py takes a tenth
# for its box of 1 %; on the tree plant the boxed loop has a free throttle 0.08 % from its limit at tick 7 (73.08 against 73),
# and a step of 1e-3 of 73 % moves the limit across it inside the quotient (measured: d/d throttle_min = 1.7962 with the
# relative step 1e-3, 1.85877035431 with 1e-4 and 1.85877035441 with 1e-5; the sweep gives 1.85877035442).  The bar stays.
LIMIT_STEP = 1e-2
UNSOLVED_TICK = 4
# scenario -> (loop, selector, unsolved ticks)
SCENARIOS = {**{tc.NAMES[b]: (b, None, ()) for b in range(tc.B)},
             "selected": (tc.SELECTED[0], tc.SELECTED[1], ()), "tick_unsolved": (0, None, (UNSOLVED_TICK,))}
# the loop whose thrust references are NaN has no difference quotient (the loss reads them in the final state); what a tick
# that is not Solved does to the sweep is checked on tick_unsolved
FD_SCENARIOS = tuple(n for n in SCENARIOS if n != tc.NAMES[tc.UNSOLVED])
PARAM_SCENARIOS = ("posed", "tick2")           # the loops whose parameter and track gradients are checked entry by entry
ENTRY_FIELDS = tuple(f for f in rpm.PARAM_FIELDS if f[0] not in ("INERTIA_B", "AMOM0", "DJ"))
UNREAD = tuple(f for f in rpm.PARAM_FIELDS if f[0] in ("INERTIA_B", "AMOM0", "DJ"))


def _central(name):
    """(grad_state0 [40], grad_cfg [32], grad_params [249] or None, grad_traj row or None) of a scenario by
    Richardson-extrapolated central differences of the whole loop, entry by entry"""
    import vsmpc_ref as ref
    b, sel, unsolved = SCENARIOS[name]
    cfg, s0, p, traj, lb, sb = tc.loop_inputs(ref, b)
    kw = dict(unsolved_ticks=unsolved)
    rtm.set_tree(tc.tree(), sel)
    try:
        gs, gc = np.zeros(ram.NS), np.zeros(am.GRAD_SIZE)
        scale, g0 = ram.state_scale(), ram.gains_of(cfg)
        for i in range(ram.NS):
            gs[i] = ram.central(cfg, s0, p, traj, tc.TICKS, lb, sb, d_state=np.eye(ram.NS)[i], step=STEP * scale[i], **kw)
        for i in range(31):
            gc[i] = ram.central(cfg, s0, p, traj, tc.TICKS, lb, sb, d_gains=np.eye(am.GRAD_SIZE)[i],
                                step=STEP * (g0[i] if g0[i] != 0.0 else 1.0) * (LIMIT_STEP if i in (29, 30) else 1.0), **kw)
        gp = gt = None
        if name in PARAM_SCENARIOS:
            sc = rpm.param_scale()
            gp = np.zeros(rpm.NP)
            for _, off, n in ENTRY_FIELDS + UNREAD[:1]:    # (I_B among them: the quotient of an unread block is zero too)
                for i in range(off, off + n):
                    gp[i] = rpm.central(cfg, s0, p, traj, tc.TICKS, lb, sb, d_params=np.eye(rpm.NP)[i], step=STEP * sc[i], **kw)
            n_traj, n_alpha = len(traj[0]), len(traj[2])
            rs, ra = rpm.reached(cfg, p, traj, tc.TICKS)
            gpos, gvel, galpha = np.zeros((n_traj, 3)), np.zeros((n_traj, 3)), np.zeros(n_alpha)
            for k in np.flatnonzero(rs):
                for c in range(3):
                    d = np.zeros((n_traj, 3))
                    d[k, c] = 1.0
                    gpos[k, c] = rpm.central(cfg, s0, p, traj, tc.TICKS, lb, sb, d_pos=d, step=STEP * rpm.TRACK_SCALE["pos"], **kw)
                    gvel[k, c] = rpm.central(cfg, s0, p, traj, tc.TICKS, lb, sb, d_vel=d, step=STEP * rpm.TRACK_SCALE["vel"], **kw)
            for k in np.flatnonzero(ra):
                galpha[k] = rpm.central(cfg, s0, p, traj, tc.TICKS, lb, sb, d_alpha=np.eye(n_alpha)[k],
                                        step=STEP * rpm.TRACK_SCALE["alpha"], **kw)
            gt = np.concatenate([gpos.reshape(-1), gvel.reshape(-1), galpha])
        return name, gs, gc, gp, gt
    finally:
        rtm.set_tree(None)


@pytest.fixture(scope="module")
def central(ref):
    with concurrent.futures.ProcessPoolExecutor(max_workers=min(len(FD_SCENARIOS), os.cpu_count() or 1)) as pool:
        return {r[0]: r[1:] for r in pool.map(_central, list(FD_SCENARIOS))}


def _sweep(name, mutation=None):
    b, sel, unsolved = SCENARIOS[name]
    return tc.model(b, tc.HORIZONS[0], sel, unsolved, mutation)


def _errors(out, fd):
    es, fs = ram.field_errors(out["grad_state0"], fd[0], ram.STATE_FIELDS, FD_BAR, FD_FLOOR)
    ec, fc = ram.field_errors(out["grad_cfg"], fd[1], am.GRAD_FIELDS, FD_BAR, FD_FLOOR)
    return max(es, ec), (fs if es >= ec else fc)


def test_loops_cross_what_they_are_meant_to(ref):
    st, pa = tc.plants()
    for name, (b, sel, unsolved) in SCENARIOS.items():
        m = _sweep(name)
        status = m["log"][:, 14]
        if b == tc.UNSOLVED:
            assert (status != L.STATUS_SOLVED).all() and all(f == am.UNSOLVED for f in m["tick_flags"])
            assert np.array_equal(m["final"][L.PS_Q:L.PS_Q + 8], st[b, L.PS_Q:L.PS_Q + 8])      # no move was consumed
            # its solves hand nothing back; the plant half of every tick still does
            assert m["flags"] == am.UNSOLVED and (m["grad_cfg"] == 0.0).all() and np.isfinite(m["grad_state0"]).all()
            assert (m["grad_state0"][0:20] != 0.0).all() and m["grad_params"][L.PP_MASS] != 0.0
            continue
        want = [L.STATUS_MAX_ITER if t in unsolved else L.STATUS_SOLVED for t in range(tc.TICKS)]
        assert list(status) == want, (name, status)
        assert all(f == (am.UNSOLVED if t in unsolved else 0) for t, f in enumerate(m["tick_flags"])), (name, m["tick_flags"])
        release = [t for t in range(tc.TICKS) if (t + int(pa[b, L.PP_TICK0])) % tc.rc.RATIO == tc.rc.RATIO - 1]
        assert len(release) == 2, (name, release)
        assert np.abs(m["final"][L.PS_Q:L.PS_Q + 8] - st[b, L.PS_Q:L.PS_Q + 8]).max() > 0.01     # the joints do move
    boxed = _sweep("boxed")
    assert any(boxed["tick_active"]) and boxed["tick_active"][0]                                  # a limit of the box, from tick 0
    # and active-set passes did run: more than the one pass of a QP whose box is idle (the hover loop's every tick)
    assert min(boxed["tick_iters"]) > 1 and max(_sweep("hover")["tick_iters"]) == 1, boxed["tick_iters"]
    print("active-set passes per tick, boxed:", boxed["tick_iters"], "hover:", _sweep("hover")["tick_iters"])
    assert np.abs(st[tc.POSED, L.PS_Q:L.PS_Q + 8]).max() > 0.2 and pa[4, L.PP_TICK0] == 2.0
    t_sub = (np.arange(tc.TICKS)[:, None] + np.arange(5)[None, :] / 5.0) * tc.rc.PERIODS["period_mpc"]
    inside = (t_sub >= pa[tc.POSED, L.PP_DIST_T0]) & (t_sub < pa[tc.POSED, L.PP_DIST_T1])
    assert inside.any() and not inside.all()
    # the selector does change the loop
    assert not np.array_equal(_sweep("selected")["log"], _sweep("posed")["log"])


@pytest.mark.parametrize("name", FD_SCENARIOS)
def test_sweep_matches_central_differences(central, name):
    out, fd = _sweep(name), central[name]
    e, f = _errors(out, fd)
    print(f"{name}: {e:.2e} of the bar ({f}); worst entry "
          f"{np.abs(out['grad_state0'] - fd[0]).max() / np.abs(fd[0]).max():.2e} of the largest state entry")
    assert e <= 1.0, (name, e, f)
    assert (out["grad_state0"] != 0.0).sum() >= 32
    q = slice(L.PS_Q, L.PS_Q + 8)
    assert np.abs(fd[0][q]).max() > FLOOR_RATIO * np.abs(fd[0]).max()          # the joints are above the floor: judged on themselves


@pytest.mark.parametrize("name", PARAM_SCENARIOS)
def test_parameters_and_tracks_match_central_differences(central, name):
    out, (_, _, gp, gt) = _sweep(name), central[name]
    n_traj, n_alpha = len(tc.trajectory()[0]), len(tc.trajectory()[2])
    ep, fp = ram.field_errors(out["grad_params"], gp, ENTRY_FIELDS, P_BAR, P_FLOOR)
    et, ft = ram.field_errors(rpc.traj_row(out), gt, rpc.traj_fields(n_traj, n_alpha), P_BAR, P_FLOOR)
    print(f"{name}: parameters {ep:.2e} of the bar ({fp}), tracks {et:.2e} ({ft})")
    assert ep <= 1.0 and et <= 1.0, (name, ep, fp, et, ft)
    # what the tree plant does not read: exactly +0.0 in the sweep, and nothing in the quotient either
    for _, off, n in UNREAD:
        blk = out["grad_params"][off:off + n]
        assert (blk == 0.0).all() and not np.signbit(blk).any()
    assert (gp[L.PP_INERTIA_B:L.PP_INERTIA_B + 9] == 0.0).all()


@pytest.mark.parametrize("mutation", rtm.MUTATIONS)
def test_planted_defects_miss_the_bar(central, mutation):
    worst, where, row = 0.0, None, []
    for name in FD_SCENARIOS:
        e, f = _errors(_sweep(name, mutation), central[name])
        row.append(f"{name} {e:.1e}")
        if e > worst:
            worst, where = e, (name, f)
    print(f"{mutation}: misses the bar by {worst:.3g} ({where}); " + ", ".join(row))
    assert worst >= MUTATION_MISS, (mutation, worst, where)
