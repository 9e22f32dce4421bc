"""The rollout adjoint's numpy model (tests/rollout_adjoint_model.py) on the cases of tests/rollout_adjoint_edge_cases.py, CPU
only: that every case reaches what it is there for, the sweep against Richardson central differences of the forward loop
model under the rule and bar of test_rollout_adjoint_model.py (field_errors with FD_BAR and FD_FLOOR, not widened), and
the planted defects of rollout_adjoint_model.EDGE_MUTATIONS.

Quotients.  Entry by entry at (6, 2, 3), for the loops of FD_LOOPS (a case's other loops run the same lines of the model
under the same timing); along N_DIR random directions in state0 and N_DIR in the gains at (17, 7, 12) and (40, 2, 40), each
set of directional derivatives judged as one field.  A case's step is Case.step times the entry's scale.

`python tests/test_rollout_adjoint_edge_cases.py` writes profiles/rollout_adjoint_cases_mutations.txt: every planted defect
on every case and on the four loops of rollout_adjoint_cases.py."""
import functools
import math
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_root, os.path.join(_root, "oracle"), os.path.join(_root, "tests")]

import adjoint_model as am
import rollout_adjoint_cases as rc
import rollout_adjoint_edge_cases as ec
import rollout_adjoint_model as ram
import sensitivity_model as sm
import test_rollout_adjoint_model as base

L = rc.L
FD_BAR, FD_FLOOR, MUTATION_MISS = base.FD_BAR, base.FD_FLOOR, base.MUTATION_MISS
N_DIR = 6
# ... but 2 + 2 where one forward loop takes 0.4 s (5000 ticks of the tick model in front of the run) and 0.85 s ((40, 2, 40))
N_DIR_OF = {("paper_tuned", 1): 2, ("long_window", 1): 2}
# the loops whose sweep is compared with difference quotients (every loop of a case where the loops differ in what they reach)
FD_LOOPS = {"sub1": (1,), "sub16_ratio2": (0,), "paper_rt": (0,), "paper_tuned": (1, 2), "rounded_ratio": (0,),
            "trajectory_end": (0, 1), "trajectory_one": (0,), "long_window": (1,), "tilted": (0, 1, 2), "boxed": (1,)}
# A throttle limit's step is a tenth of the other gains' relative step: 1e-2 of 73 % would be 0.73 %, most of the way across
# the box of 1 %, and throttles would change their state inside the quotient (measured on the boxed loop: throttle_min is
# 4e-2 off with 1e-2, 3e-12 with 1e-3)
LIMIT_STEP = 0.1
# the cases a planted defect is run on in the test (the table of write_profile runs every defect on every case)
MUTATION_CASES = {"drot_sign": ("tilted",), "drop_winv_pitch": ("tilted",), "inertia_half": ("tilted",),
                  "alpha_per_tick": ("trajectory_end",), "dist_per_tick": ("sub16_ratio2",), "push_unclamped": ("trajectory_end",),
                  "first_clamp_early": ("trajectory_end",), "h_1ms": ("sub16_ratio2",), "limits_last_tick": ("boxed", "paper_tuned"),
                  "shift_first_chunk": ("paper_tuned",)}
# defects that change nothing at all on the four loops of rollout_adjoint_cases.py: the lines they spoil are never run there
INVISIBLE_BEFORE = ("push_unclamped", "first_clamp_early", "h_1ms", "limits_last_tick", "shift_first_chunk")
# a free throttle is at least this far (times 1 + |v|) inside its box: 1000 times VSMPC_SENS_BOUND_TOL, from which on the
# device calls a throttle nearly active, and 100 times the 1e-8 by which the device's throttles may differ from the model's
INSIDE = 1e-6


def _entrywise(case):
    return ec.CASES[case].horizon == (6, 2, 3)


def _directions(case, b):
    import vsmpc_ref as ref
    n = N_DIR_OF.get((case, b), N_DIR)
    rng = np.random.default_rng(ec.SEED + 11 + b)
    ds = rng.normal(size=(n, ram.NS)) * ram.state_scale()
    g0 = ec.gains(ref.Config, case)[b]
    dg = rng.normal(size=(n, am.GRAD_SIZE)) * np.where(g0 != 0.0, g0, 1.0)
    dg[:, 29:31] *= LIMIT_STEP
    dg[:, 31] = 0.0
    return ds, dg


@functools.lru_cache(maxsize=None)
def quotients(case, b):
    """entry-wise: (grad_state0 [40], grad_cfg [32]); else the derivatives along _directions: ([N_DIR], [N_DIR])"""
    import vsmpc_ref as ref
    cfg, s0, p, traj, lb, sb = ec.loop_inputs(ref, case, b)
    c = ec.CASES[case]
    if not _entrywise(case):
        ds, dg = _directions(case, b)
        qs = np.array([ram.central(cfg, s0, p, traj, c.ticks, lb, sb, d_state=d, step=c.step) for d in ds])
        qg = np.array([ram.central(cfg, s0, p, traj, c.ticks, lb, sb, d_gains=d, step=c.step) for d in dg])
        return qs, qg
    gs, gc = np.zeros(ram.NS), np.zeros(am.GRAD_SIZE)
    scale, g0 = ram.state_scale(), ram.gains_of(cfg)
    for i in range(ram.NS):
        d = np.zeros(ram.NS)
        d[i] = 1.0
        gs[i] = ram.central(cfg, s0, p, traj, c.ticks, lb, sb, d_state=d, step=c.step * scale[i])
    for i in range(31):
        d = np.zeros(am.GRAD_SIZE)
        d[i] = 1.0
        gc[i] = ram.central(cfg, s0, p, traj, c.ticks, lb, sb, d_gains=d,
                            step=c.step * (g0[i] if g0[i] != 0.0 else 1.0) * (LIMIT_STEP if i in (29, 30) else 1.0))
    return gs, gc


def errors(case, b, out):
    """the sweep `out` of loop b against its quotients: (worst share of the bar, where)"""
    qs, qg = quotients(case, b)
    if _entrywise(case):
        es, fs = ram.field_errors(out["grad_state0"], qs, ram.STATE_FIELDS, FD_BAR, FD_FLOOR)
        ec_, fc = ram.field_errors(out["grad_cfg"], qg, am.GRAD_FIELDS, FD_BAR, FD_FLOOR)
    else:
        ds, dg = _directions(case, b)
        es, fs = ram.field_errors(ds @ out["grad_state0"], qs, (("state0 directions", 0, len(ds)),), FD_BAR, FD_FLOOR)
        ec_, fc = ram.field_errors(dg @ out["grad_cfg"], qg, (("gains directions", 0, len(dg)),), FD_BAR, FD_FLOOR)
    return max(es, ec_), (fs if es >= ec_ else fc)


def sweep(case, b, mutation=None):
    import vsmpc_ref as ref
    cfg, s0, p, traj, lb, sb = ec.loop_inputs(ref, case, b)
    return ram.backward(cfg, ec.model(case)["tapes"][b], p, traj, lb, sb, mutation=mutation)


# ----------------------------------------------------------------------------------------------------------------------
# the cases reach what they are there for
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(ec.CASES))
def test_every_tick_is_solved_and_none_is_degenerate(ref, case):
    m = ec.model(case)
    assert (m["log"][:, :, 14] == L.STATUS_SOLVED).all()
    assert (m["flags"] == 0).all() and all(f == 0 for flags in m["tick_flags"] for f in flags)
    # the CPU model stands for the device: tick_model's rates are those vsmpc_rollout_create derives
    r = ec.model_rates(ref, case)
    assert r["des_fps"][0] == r["des_fps"][1] and r["ratio"][0] == r["ratio"][1] and r["alpha_up"][0] == r["alpha_up"][1], r
    assert r["des_fps"][1] % r["fps_alpha"] == 0


def test_substep_rule(ref):
    want = {"sub1": 1, "sub16_ratio2": 16, "paper_rt": 10, "paper_tuned": 10, "rounded_ratio": 4, "trajectory_end": 4,
            "trajectory_one": 4, "long_window": 5, "tilted": 5, "boxed": 5}
    for case, n in want.items():
        assert ram.substeps_of(ec.config(ref.Config, case)) == n, case
    cfg = ec.config(ref.Config, "sub16_ratio2")
    assert cfg.period_mpc / ram.substeps_of(cfg) == 1.25e-3            # beyond 16 ms the sub-step is no longer 1 ms
    assert ram.substeps_of(rc.config(ref.Config, rc.HORIZONS[0])) == 5  # what the first tests hard-coded
    for period, n in ((0.0004, 1), (0.0015, 2), (0.0025, 3), (0.0154, 15), (0.0156, 16), (0.1, 16)):   # lround: halves away from 0
        assert ram.substeps_of(ref.Config(period_mpc=period)) == n, period


def test_ratios_and_releases(ref):
    for case, ratio in (("sub16_ratio2", 2), ("paper_rt", 10), ("paper_tuned", 10), ("rounded_ratio", 20), ("long_window", 2)):
        cfg = ec.config(ref.Config, case)
        assert cfg.ratio == ratio, case
        _, pa = ec.plants(case)
        for b in range(len(pa)):
            tk = np.arange(ec.CASES[case].ticks) + int(pa[b, L.PP_TICK0])
            assert (tk % ratio == ratio - 1).any(), (case, b)          # every loop crosses a release
    assert ec.config(ref.Config, "rounded_ratio").period_large / ec.config(ref.Config, "rounded_ratio").period_small != 20.0
    assert ec.plants("paper_tuned")[1][1, L.PP_TICK0] == 5000.0
    assert 12 * ec.config(ref.Config, "long_window").n_ref_cols == 468 == 7 * 64 + 20


def test_pushed_between_sub_steps(ref):
    cfg = ec.config(ref.Config, "sub16_ratio2")
    _, pa = ec.plants("sub16_ratio2")
    n = ram.substeps_of(cfg)
    t = (1 + np.arange(n) / n) * cfg.period_mpc                        # the sub-step times of tick 1
    on = (t >= pa[0, L.PP_DIST_T0]) & (t < pa[0, L.PP_DIST_T1])
    assert on.any() and not on.all() and not on[0]
    assert not np.isin([pa[0, L.PP_DIST_T0], pa[0, L.PP_DIST_T1]], t).any()
    assert t[2] < pa[0, L.PP_DIST_T0] < t[3] and t[9] < pa[0, L.PP_DIST_T1] < t[10]


def test_trajectory_clamps_are_taken(ref):
    c = ec.CASES["trajectory_end"]
    cfg = ec.config(ref.Config, "trajectory_end")
    _, pa = ec.plants("trajectory_end")
    tk = np.arange(c.ticks) + int(pa[0, L.PP_TICK0])
    pushed = [1 + (t + 1) // cfg.ratio for t in tk if t % cfg.ratio == cfg.ratio - 1]
    assert any(i >= c.n_traj for i in pushed) and any(i < c.n_traj for i in pushed), pushed     # release branch, loop 0
    ns0 = 1 + int(pa[1, L.PP_TICK0]) // cfg.ratio
    fill = [ns0 - (cfg.n_ref_cols - 1 - j) for j in range(cfg.n_ref_cols)]
    assert max(fill) >= c.n_traj and min(fill) < 0, fill                                          # `first` fill, loop 1
    assert ec.CASES["trajectory_one"].n_traj == 1 and len(ec.trajectory("trajectory_one")[0]) == 1
    # alpha: every sub-step of the first ticks reads its own value, later ticks lie beyond the track
    _, _, alpha, adt = ec.trajectory("trajectory_end")
    n = ram.substeps_of(cfg)
    pos = (np.arange(c.ticks)[:, None] + np.arange(n)[None, :] / n) * cfg.period_mpc / adt
    a = np.array([[ram.pm.interp_clamped(alpha, x) for x in row] for row in pos])
    assert len(set(a[0])) == n and len(set(a[2])) == n and (pos[-1] > len(alpha) - 1).all() and (a[4:] == alpha[-1]).all()


def test_tilted_loops_cross_pi():
    m = ec.model("tilted")
    st, _ = ec.plants("tilted")
    yaw = np.vstack([st[None, :, L.PS_RPY + 2], m["log"][:, :, 5]])    # [ticks + 1, loops]
    assert yaw[0, 0] < math.pi < yaw[-1, 0] and yaw[0, 1] > -math.pi > yaw[-1, 1], yaw[[0, -1]]
    assert (np.abs(np.diff(yaw, axis=0)) < 0.1).all()                  # the plant integrates it continuously
    assert m["log"][:, 2, 4].min() > 1.15                              # pitch 1.2: 1 / cos^2 > 6
    assert np.abs(st[:2, L.PS_RPY:L.PS_RPY + 2]).min() >= 0.5


def _bounds(ref, case, b):
    cfg = ram.with_gains(ec.config(ref.Config, case), ec.gains(ref.Config, case)[b])
    return ref.throttle_bounds(cfg)


def test_boxed_loops_sit_on_their_limits(ref):
    for case, b in (ec.BOXED, ec.SWITCHING):
        m = ec.model(case)
        vmin, vmax = _bounds(ref, case, b)
        inside = np.inf
        for act, v in zip(m["tick_active"][b], m["tick_v"][b]):
            assert (v[act == sm.LOWER] == vmin).all() and (v[act == sm.UPPER] == vmax).all()
            free = v[act == sm.FREE]
            inside = min([inside] + list((free - vmin) / (1.0 + np.abs(free))) + list((vmax - free) / (1.0 + np.abs(free))))
        print(f"{case} loop {b}: the free throttles stay {inside:.2e} (1 + |v|) inside the box; grad_cfg[29:31] = {m['grad_cfg'][b, 29:31]}")
        assert inside >= INSIDE, (case, b, inside)
    m = ec.model(ec.BOXED[0])
    b = ec.BOXED[1]
    assert (m["grad_cfg"][b, 29:31] != 0.0).all()
    first = m["tick_active"][b][0]
    assert (first == sm.LOWER).any() and (first == sm.UPPER).any()     # both limits, from the first tick
    assert (np.delete(m["grad_cfg"], b, axis=0)[:, 29:31] == 0.0).all()   # and the loops beside it are not boxed in
    m = ec.model(ec.SWITCHING[0])
    b = ec.SWITCHING[1]
    assert m["grad_cfg"][b, 29] != 0.0
    sets = {tuple(np.nonzero((a == sm.LOWER) | (a == sm.UPPER))[0]) for a in m["tick_active"][b]}
    assert len(sets) >= 2 and () in sets, sets                         # free at first, on the limit later


# ----------------------------------------------------------------------------------------------------------------------
# the sweep against difference quotients
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,b", [(c, b) for c, loops in FD_LOOPS.items() for b in loops])
def test_sweep_matches_central_differences(case, b):
    m = ec.model(case)
    got = {"grad_state0": m["grad_state0"][b], "grad_cfg": m["grad_cfg"][b]}
    e, f = errors(case, b, got)
    print(f"{case} loop {b} ({ec.CASES[case].loops[b]}): {e:.2e} of the bar ({f})")
    assert e <= 1.0, (case, b, e, f)
    assert (got["grad_state0"] != 0.0).sum() >= 32


# ----------------------------------------------------------------------------------------------------------------------
# planted defects
# ----------------------------------------------------------------------------------------------------------------------
def _miss(mutation, cases):
    worst, where = 0.0, None
    for case in cases:
        for b in FD_LOOPS[case]:
            e, f = errors(case, b, sweep(case, b, mutation))
            if e > worst:
                worst, where = e, (case, b, f)
    return worst, where


def _miss_before(ref, mutation, central=None):
    """the defect on the four loops of rollout_adjoint_cases.py: against their quotients when given, else against the
    model's own sweep, which test_rollout_adjoint_model.py holds within a tenth of the bar of them"""
    worst = 0.0
    for b in range(rc.B):
        out = base._sweep(ref, b, mutation)
        want = central[b] if central is not None else (rc.model(base.HORIZON)["grad_state0"][b], rc.model(base.HORIZON)["grad_cfg"][b])
        worst = max(worst, base._errors(out, want)[0])
    return worst


@pytest.mark.parametrize("mutation", ram.EDGE_MUTATIONS)
def test_planted_defects_miss_the_bar(ref, mutation):
    worst, where = _miss(mutation, MUTATION_CASES[mutation])
    before = _miss_before(ref, mutation)
    print(f"{mutation}: misses the bar by {worst:.3g} ({where}); on the four loops of rollout_adjoint_cases.py by {before:.3g}")
    assert worst >= MUTATION_MISS, (mutation, worst, where)
    if mutation in INVISIBLE_BEFORE:
        assert before == 0.0, (mutation, before)


def write_profile(root):
    import vsmpc_ref as ref
    central = {b: base._central_gradients(ref, b) for b in range(rc.B)}
    cases = list(FD_LOOPS)
    lines = ["One-line mistakes planted in tests/rollout_adjoint_model.py (mutation=), CPU only (python",
             "tests/test_rollout_adjoint_edge_cases.py).  Figures: by how many bars (field_errors with FD_BAR, FD_FLOOR of",
             "tests/test_rollout_adjoint_model.py, against Richardson central differences of the forward loop model) the",
             "mistaken sweep misses, worst loop per case of tests/rollout_adjoint_edge_cases.py, and the same on the four",
             "loops of tests/rollout_adjoint_cases.py: 'before'.  <= 1 passes; a 'before' figure <= 1 means that the suite let",
             f"the mistake through before these cases.  A defect counts as caught from {MUTATION_MISS:g} bars on.  unsolved_as_solved is",
             "not listed: it needs a tick that is not Solved, which only test_rollout_adjoint_model.py's own scenario has.",
             "", f"{'mutation':22s}" + "".join(f"{c:>15s}" for c in cases) + f"{'before':>12s}"]
    for mutation in [m for m in ram.MUTATIONS if m != "unsolved_as_solved"] + list(ram.EDGE_MUTATIONS):
        row = [_miss(mutation, (c,))[0] for c in cases]
        before = _miss_before(ref, mutation, central)
        lines.append(f"{mutation:22s}" + "".join(f"{v:15.1e}" for v in row) + f"{before:12.1e}"
                     + ("   LET THROUGH" if before <= 1.0 else "") + ("   UNCAUGHT" if max(row) < MUTATION_MISS else ""))
    lines += ["", "the unmutated sweep:", f"{'':22s}" + "".join(f"{_miss(None, (c,))[0]:15.1e}" for c in cases)
              + f"{_miss_before(ref, None, central):12.1e}"]
    with open(os.path.join(root, "profiles", "rollout_adjoint_cases_mutations.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    write_profile(_root)
