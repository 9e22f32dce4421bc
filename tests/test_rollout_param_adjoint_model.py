"""The executable model of the rollout adjoint's parameter and track gradients (tests/rollout_param_adjoint_model.py) on the
CPU: the numpy sweep against central differences of the forward loop model on the loops of
tests/rollout_param_adjoint_cases.py at horizon (6, 2, 3) -- the four loops of rollout_adjoint_cases.py, the push inside one
tick and 16 sub-steps, the 3-sample and 1-sample tracks with the alpha track that ends inside the run, the tilted loops, the
loop that starts at tick 5000, and two loops that make the mass visible through the window and DIST_F visible at all -- and
planted defects.

Entry by entry: MASS, INERTIA_B, QREF0, PINIT, RPYINIT, DIST_F, DIST_TAU and every track sample the run can reach
(rollout_param_adjoint_model.reached).  Along random directions: AMOM0 (8) and each DJ[j] block (1 each), 16 in all.

Bar.  The rule of adjoint_record_model.worst_field with the convention of test_rollout_adjoint_model.py: |err| <= FD_BAR
(|field|_inf + FLOOR_RATIO max |gradient|), the quotients with the step STEP times the entry's scale
(rollout_param_adjoint_model.param_scale, TRACK_SCALE; 1e-4 along the directions), Richardson extrapolated.  The gradient
vectors are: the parameters checked entry by entry (the fields above), one row of grad_traj (pos | vel | alpha), and the 16
directional derivatives (AMOM0 | DJ).  Measured here, worst of all loops and the unsolved scenario: 9.14e-8 of |field|_inf +
1e-3 max |gradient| (loop 0 of `tilted`, RPYINIT; the other loops lie between 4.7e-10 and 8.9e-8, most of them on the track
positions); FD_BAR (rollout_param_adjoint_cases.py) is 10 times that.  The planted defects miss it by factors from 8e3
(qref0_sign, on pushed_long) to 1.6e6.  Every tick of every loop is Solved and not degenerate, except tick 4 of the scenario
that forces it."""
import numpy as np
import pytest

import adjoint_model as am
import rollout_adjoint_model as ram
import rollout_param_adjoint_cases as pc
import rollout_param_adjoint_model as rpm

L = pc.L
STEP = 1e-2
DIR_STEP = 1e-4
FLOOR_RATIO, FD_BAR, FD_FLOOR = pc.FLOOR_RATIO, pc.FD_BAR, pc.FD_FLOOR
MUTATION_MISS = 10.0                   # a planted defect misses the bar by at least this factor on some loop
ENTRY_FIELDS = tuple(f for f in rpm.PARAM_FIELDS if f[0] not in ("AMOM0", "DJ"))
DIR_FIELDS = (("AMOM0 directions", 0, 8), ("DJ directions", 8, 8))
UNSOLVED_KEY, UNSOLVED_TICK = pc.UNSOLVED


def directions():
    """16 directions in the parameters: 8 inside AMOM0, one inside each DJ[j] block"""
    rng = np.random.default_rng(pc.rc.SEED + 31)
    d = np.zeros((16, rpm.NP))
    d[:8, L.PP_AMOM0:L.PP_AMOM0 + 24] = rng.normal(size=(8, 24))
    for j in range(8):
        d[8 + j, L.PP_DJ + 24 * j:L.PP_DJ + 24 * (j + 1)] = rng.normal(size=24)
    return d


def central_gradients(ref, key, unsolved_ticks=()):
    """(parameters [249] with the entry-wise fields filled, grad_traj row with the reached samples filled, the 16
    directional derivatives) of one loop by Richardson-extrapolated central differences"""
    cfg, s0, p, traj, lb, sb, ticks = pc.loop_inputs(ref, key)
    kw = dict(unsolved_ticks=unsolved_ticks)
    sc = rpm.param_scale()
    gp = np.zeros(rpm.NP)
    for _, off, n in ENTRY_FIELDS:
        for i in range(off, off + n):
            d = np.zeros(rpm.NP)
            d[i] = 1.0
            gp[i] = rpm.central(cfg, s0, p, traj, ticks, lb, sb, d_params=d, step=STEP * sc[i], **kw)
    n_traj, n_alpha = len(traj[0]), len(traj[2])
    rs, ra = rpm.reached(cfg, p, traj, ticks)
    gpos, gvel, galpha = np.zeros((n_traj, 3)), np.zeros((n_traj, 3)), np.zeros(n_alpha)
    for k in np.nonzero(rs)[0]:
        for c in range(3):
            d = np.zeros((n_traj, 3))
            d[k, c] = 1.0
            gpos[k, c] = rpm.central(cfg, s0, p, traj, ticks, lb, sb, d_pos=d, step=STEP * rpm.TRACK_SCALE["pos"], **kw)
            gvel[k, c] = rpm.central(cfg, s0, p, traj, ticks, lb, sb, d_vel=d, step=STEP * rpm.TRACK_SCALE["vel"], **kw)
    for k in np.nonzero(ra)[0]:
        d = np.zeros(n_alpha)
        d[k] = 1.0
        galpha[k] = rpm.central(cfg, s0, p, traj, ticks, lb, sb, d_alpha=d, step=STEP * rpm.TRACK_SCALE["alpha"], **kw)
    gdir = np.array([rpm.central(cfg, s0, p, traj, ticks, lb, sb, d_params=d, step=DIR_STEP, **kw) for d in directions()])
    return gp, np.concatenate([gpos.reshape(-1), gvel.reshape(-1), galpha]), gdir


@pytest.fixture(scope="module")
def central(ref):
    """the difference quotients of every loop, and of the hover loop with one tick that is not Solved: computed once"""
    out = {key: central_gradients(ref, key) for key in pc.LOOPS}
    out["unsolved"] = central_gradients(ref, UNSOLVED_KEY, unsolved_ticks=(UNSOLVED_TICK,))
    return out


def sweep(ref, key, mutation=None, unsolved_ticks=()):
    cfg, s0, p, traj, lb, sb, ticks = pc.loop_inputs(ref, key)
    _, _, tape = ram.forward(cfg, s0, p, traj, ticks, unsolved_ticks=unsolved_ticks)
    return rpm.backward(cfg, tape, p, traj, lb, sb, mutation=mutation)


def errors(out, fd):
    """the worst error of a sweep's three gradient vectors in units of the bar, and where"""
    gp, gt, gdir = fd
    row = pc.traj_row(out)
    n_traj, n_alpha = len(out["grad_traj_pos"]), len(out["grad_traj_alpha"])
    got_p = np.zeros(rpm.NP)
    for _, off, n in ENTRY_FIELDS:
        got_p[off:off + n] = out["grad_params"][off:off + n]
    parts = [ram.field_errors(got_p, gp, ENTRY_FIELDS, FD_BAR, FD_FLOOR),
             ram.field_errors(row, gt, pc.traj_fields(n_traj, n_alpha), FD_BAR, FD_FLOOR),
             ram.field_errors(directions() @ out["grad_params"], gdir, DIR_FIELDS, FD_BAR, FD_FLOOR)]
    return max(parts, key=lambda ef: ef[0])


def test_every_tick_is_solved_and_not_degenerate():
    for key in pc.LOOPS:
        m = pc.model(key)
        assert (m["log"][:, 14] == L.STATUS_SOLVED).all(), key
        assert m["flags"] == 0 and all(f == 0 for f in m["tick_flags"]), key


def test_loops_cross_what_they_are_meant_to(ref):
    def inside(key):
        cfg, _, p, _, _, _, ticks = pc.loop_inputs(ref, key)
        ss = ram.substeps_of(cfg)
        t = (np.arange(ticks)[:, None] + int(p[L.PP_TICK0]) + np.arange(ss)[None, :] / ss) * cfg.period_mpc
        return (t >= p[L.PP_DIST_T0]) & (t < p[L.PP_DIST_T1]), ss
    one_tick, ss = inside(("sub16_ratio2", 0))
    assert ss == 16 and one_tick[1].any() and not one_tick[1].all() and not np.delete(one_tick, 1, axis=0).any()
    assert inside(("pushed_long", 0))[0].all()
    for key in pc.PUSH_MISSES:
        assert not inside(key)[0].any()
    cfg, _, p, traj, _, _, ticks = pc.loop_inputs(ref, ("trajectory_end", 0))
    assert len(traj[0]) == 3 and (ticks + 1) * cfg.period_mpc > (len(traj[2]) - 1) * traj[3]      # alpha ends inside the run
    assert len(pc.loop_inputs(ref, ("trajectory_one", 0))[3][0]) == 1
    assert pc.loop_inputs(ref, ("tick5000", 0))[2][L.PP_TICK0] == 5000.0
    assert abs(pc.loop_inputs(ref, ("tilted", 2))[1][L.PS_RPY + 1]) > 1.0


def test_every_field_is_above_the_floor_somewhere():
    """every differentiable parameter field and each of the three tracks is judged against itself, not against the floor, in
    at least one loop; and in one loop the mass is seen through the window columns too"""
    seen_p, seen_t, mass_window = set(), set(), 0.0
    for key in pc.LOOPS:
        m = pc.model(key)
        gp = np.zeros(rpm.NP)
        for _, off, n in ENTRY_FIELDS:
            gp[off:off + n] = m["grad_params"][off:off + n]
        seen_p |= {name for name, off, n in ENTRY_FIELDS if np.abs(gp[off:off + n]).max() > FLOOR_RATIO * np.abs(gp).max()}
        row = pc.traj_row(m)
        seen_t |= {name for name, off, n in pc.traj_fields(len(m["grad_traj_pos"]), len(m["grad_traj_alpha"]))
                   if np.abs(row[off:off + n]).max() > FLOOR_RATIO * np.abs(row).max()}
        gdir = directions() @ m["grad_params"]
        assert all(np.abs(gdir[off:off + n]).max() > FLOOR_RATIO * np.abs(gdir).max() for _, off, n in DIR_FIELDS), key
        mass_window = max(mass_window, abs(m["mass_window"]) / abs(m["grad_params"][L.PP_MASS]))
    assert seen_p == {f[0] for f in ENTRY_FIELDS}, seen_p
    assert seen_t == {"pos", "vel", "alpha"}, seen_t
    print(f"largest share of the window in dL/dmass: {mass_window:.2e}")
    assert mass_window > 100.0 * FD_BAR            # a dropped window share misses the bar on MASS itself


@pytest.mark.parametrize("key", pc.LOOPS, ids=lambda k: f"{k[0]}-{k[1]}")
def test_sweep_matches_central_differences(central, key):
    e, f = errors(pc.model(key), central[key])
    print(f"loop {key}: {e:.2e} of the bar ({f}) = {e * FD_BAR:.2e} of |field|_inf + {FLOOR_RATIO} max |gradient|")
    assert e <= 1.0, (key, e, f)


def test_unsolved_tick_keeps_its_plant_and_window_shares(ref, central):
    out = sweep(ref, UNSOLVED_KEY, unsolved_ticks=(UNSOLVED_TICK,))
    e, f = errors(out, central["unsolved"])
    print(f"loop {UNSOLVED_KEY} with tick {UNSOLVED_TICK} not consumed: {e:.2e} of the bar ({f})")
    assert e <= 1.0, (e, f)
    assert out["tick_flags"][UNSOLVED_TICK] == am.UNSOLVED
    assert errors(out, central[UNSOLVED_KEY])[0] > MUTATION_MISS        # and the scenario does differ from the solved one


def test_exact_identities(ref):
    for key in pc.LOOPS:
        m = pc.model(key)
        cfg, _, p, traj, _, _, ticks = pc.loop_inputs(ref, key)
        gp = m["grad_params"]
        total = m["grad_traj_pos"].sum(axis=0)
        tol = 16 * np.finfo(float).eps * np.abs(m["grad_traj_pos"]).sum(axis=0)
        assert (np.abs(gp[L.PP_PINIT:L.PP_PINIT + 3] - total) <= tol).all(), key      # PINIT enters beside every sample
        rs, ra = rpm.reached(cfg, p, traj, ticks)
        for g in (m["grad_traj_pos"][~rs], m["grad_traj_vel"][~rs], m["grad_traj_alpha"][~ra]):
            assert (g == 0.0).all() and not np.signbit(g).any(), key
        for i in rpm.STRUCTURAL:
            assert gp[i] == 0.0 and not np.signbit(gp[i]), key
    for key in pc.PUSH_MISSES:
        g = pc.model(key)["grad_params"][L.PP_DIST_F:L.PP_DIST_TAU + 3]
        assert (g == 0.0).all() and not np.signbit(g).any(), key


@pytest.mark.parametrize("mutation", rpm.MUTATIONS)
def test_planted_defects_miss_the_bar(ref, central, mutation):
    worst, where = 0.0, None
    for key in pc.LOOPS:
        e, f = errors(sweep(ref, key, mutation), central[key])
        if e > worst:
            worst, where = e, (key, f)
    print(f"{mutation}: misses the bar by {worst:.3g} ({where})")
    assert worst >= MUTATION_MISS, (mutation, worst, where)
