"""The executable model of the rollout adjoint (tests/rollout_adjoint_model.py) on the CPU: the numpy sweep against central
differences of the forward loop model, entry by entry, on the four loops of tests/rollout_adjoint_cases.py at horizon
(6, 2, 3), ratio 4, 9 ticks (two release ticks and the `first` fill of the window are crossed; loop 0 starts at tick 2, loop
1 is pushed, loop 2 sits on the 100 % throttle clamp, loop 3 hovers), and planted defects.

Bar.  Every entry of grad_state0[0:40] and of grad_cfg against a central difference quotient of the whole loop with the
step STEP times the entry's scale (rollout_adjoint_model.state_scale; a gain's own value), Richardson extrapolated with
half the step as adjoint_record_model.kkt_record_adjoint does, under the rule of adjoint_record_model.field_errors:
|err| <= FD_BAR (|field|_inf + FLOOR_RATIO max |gradient|).  The floor is there because the noise of a difference quotient is
absolute, ~1e-16 |L| / h for every entry, while the fields span six decades (dL/dp ~ 6e2, dL/d thrust references ~ 1e-5):
FLOOR_RATIO = 1e-3 lets a field be judged against itself down to a thousandth of the largest entry.  Measured here (seeds of
rollout_adjoint_cases, worst of the four loops and the unsolved scenario): 7.8e-9 of |field|_inf + 1e-3 max |gradient| (loop 1, w_reg_joint_pos; the worst
field is 1.5e-7 off itself, the worst entry 2.5e-10 of the largest); FD_BAR is 10 times that, for the step's dependence on the seed.  No tick of any loop is flagged degenerate by the model, so
no entry is excluded."""
import numpy as np
import pytest

import adjoint_model as am
import rollout_adjoint_cases as rc
import rollout_adjoint_model as ram

HORIZON = rc.HORIZONS[0]
STEP = 1e-2
FLOOR_RATIO = 1e-3
MEASURED = 7.8e-9                       # worst error in units of |field|_inf + FLOOR_RATIO max |gradient|, measured: see above
FD_BAR = 10.0 * MEASURED
FD_FLOOR = FD_BAR * FLOOR_RATIO
MUTATION_MISS = 10.0                   # a planted defect misses the bar by at least this factor on some loop
UNSOLVED_TICK = 4                      # of loop 3, for the scenario with a tick that does not consume its move


def _inputs(ref, b):
    cfg = ram.with_gains(rc.config(ref.Config, HORIZON), rc.gains(ref.Config, HORIZON)[b])
    st, pa = rc.plants()
    lb, sb = rc.loss_weights()
    return cfg, st[b], pa[b], rc.trajectory(), lb[:, b], sb[b]


def _central_gradients(ref, b, unsolved_ticks=()):
    """(grad_state0 [40], grad_cfg [32]) of loop b by Richardson-extrapolated central differences, entry by entry"""
    cfg, s0, p, traj, lb, sb = _inputs(ref, b)
    gs, gc = np.zeros(ram.NS), np.zeros(am.GRAD_SIZE)
    scale = ram.state_scale()
    for i in range(ram.NS):
        d = np.zeros(ram.NS)
        d[i] = 1.0
        gs[i] = ram.central(cfg, s0, p, traj, rc.TICKS, lb, sb, d_state=d, step=STEP * scale[i], unsolved_ticks=unsolved_ticks)
    g0 = ram.gains_of(cfg)
    for i in range(31):
        d = np.zeros(am.GRAD_SIZE)
        d[i] = 1.0
        gc[i] = ram.central(cfg, s0, p, traj, rc.TICKS, lb, sb, d_gains=d, step=STEP * (g0[i] if g0[i] != 0.0 else 1.0),
                            unsolved_ticks=unsolved_ticks)
    return gs, gc


@pytest.fixture(scope="module")
def central(ref):
    """the difference quotients of the four loops, and of loop 3 with one tick that is not Solved: computed once"""
    out = {b: _central_gradients(ref, b) for b in range(rc.B)}
    out["unsolved"] = _central_gradients(ref, 3, unsolved_ticks=(UNSOLVED_TICK,))
    return out


def _sweep(ref, b, mutation=None, unsolved_ticks=()):
    cfg, s0, p, traj, lb, sb = _inputs(ref, b)
    _, _, tape = ram.forward(cfg, s0, p, traj, rc.TICKS, unsolved_ticks=unsolved_ticks)
    return ram.backward(cfg, tape, p, traj, lb, sb, mutation=mutation)


def _errors(out, fd):
    es, fs = ram.field_errors(out["grad_state0"], fd[0], ram.STATE_FIELDS, FD_BAR, FD_FLOOR)
    ec, fc = ram.field_errors(out["grad_cfg"], fd[1], am.GRAD_FIELDS, FD_BAR, FD_FLOOR)
    return max(es, ec), (fs if es >= ec else fc)


def test_loops_cross_what_they_are_meant_to(ref):
    m = rc.model(HORIZON)
    assert (m["log"][:, :, 14] == rc.L.STATUS_SOLVED).all()
    _, pa = rc.plants()
    ticks = np.arange(rc.TICKS)
    for b in range(rc.B):
        release = [t for t in ticks if (t + int(pa[b, rc.L.PP_TICK0])) % rc.RATIO == rc.RATIO - 1]
        assert len(release) == 2, (b, release)
    assert pa[0, rc.L.PP_TICK0] != 0.0
    t_sub = (ticks[:, None] + np.arange(5)[None, :] / 5.0) * rc.PERIODS["period_mpc"]
    inside = (t_sub >= pa[1, rc.L.PP_DIST_T0]) & (t_sub < pa[1, rc.L.PP_DIST_T1])
    assert inside.any() and not inside.all()
    assert (m["log"][3, 2, 10:14] == 100.0).all()                   # the clamp, strictly inside the clamped piece:
    v0 = m["tapes"][2][3][2][rc.L.FM_V0:rc.L.FM_V0 + 4]
    assert (v0 > ref.v_of_throttle(100.0) + 1e-3).all() and (v0 < ref.v_of_throttle(120.0) - 1e-3).all()
    assert (m["log"][:3, 2, 10:14] < 100.0).all()


def test_no_tick_is_degenerate(ref):
    m = rc.model(HORIZON)
    assert all(f == 0 for flags in m["tick_flags"] for f in flags) and (m["flags"] == 0).all()


@pytest.mark.parametrize("b", range(rc.B))
def test_sweep_matches_central_differences(ref, central, b):
    out = rc.model(HORIZON)
    got = {"grad_state0": out["grad_state0"][b], "grad_cfg": out["grad_cfg"][b]}
    gs, gc = central[b]
    e, f = _errors(got, central[b])
    rel_field = max(np.abs(got["grad_state0"][o:o + n] - gs[o:o + n]).max() / np.abs(gs[o:o + n]).max()
                    for _, o, n in ram.STATE_FIELDS if np.abs(gs[o:o + n]).max() > 1e-6 * np.abs(gs).max())
    rel_cfg = max(np.abs(got["grad_cfg"][o:o + n] - gc[o:o + n]).max() / np.abs(gc[o:o + n]).max()
                  for _, o, n in am.GRAD_FIELDS if np.abs(gc[o:o + n]).max() > 1e-6 * np.abs(gc).max())
    print(f"loop {b} ({rc.NAMES[b]}): {e:.2e} of the bar ({f}); worst field {max(rel_field, rel_cfg):.2e} of itself, worst entry "
          f"{max(np.abs(got['grad_state0'] - gs).max() / np.abs(gs).max(), np.abs(got['grad_cfg'] - gc).max() / np.abs(gc).max()):.2e} "
          f"of the largest")
    assert e <= 1.0, (b, e, f)
    assert (got["grad_state0"] != 0.0).sum() >= 32                  # every block but the thrust references is live


def test_unsolved_tick_passes_through(ref, central):
    out = _sweep(ref, 3, unsolved_ticks=(UNSOLVED_TICK,))
    e, f = _errors(out, central["unsolved"])
    print(f"loop 3 with tick {UNSOLVED_TICK} not consumed: {e:.2e} of the bar ({f})")
    assert e <= 1.0, (e, f)
    assert out["tick_flags"][UNSOLVED_TICK] == am.UNSOLVED and out["flags"] == am.UNSOLVED
    # and the scenario does differ from the solved one
    assert _errors(out, central[3])[0] > MUTATION_MISS


@pytest.mark.parametrize("mutation", ram.MUTATIONS)
def test_planted_defects_miss_the_bar(ref, central, mutation):
    worst, where = 0.0, None
    for b in range(rc.B):
        e, f = _errors(_sweep(ref, b, mutation), central[b])
        if e > worst:
            worst, where = e, (b, f)
    # a tick that is not Solved exists only in the scenario built for it
    e, f = _errors(_sweep(ref, 3, mutation, unsolved_ticks=(UNSOLVED_TICK,)), central["unsolved"])
    if e > worst:
        worst, where = e, ("unsolved", f)
    print(f"{mutation}: misses the bar by {worst:.3g} ({where})")
    assert worst >= MUTATION_MISS, (mutation, worst, where)
