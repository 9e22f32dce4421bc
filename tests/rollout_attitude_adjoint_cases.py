"""The closed loops the attitude-track gradients of the rollout adjoint are tested on
(tests/test_rollout_attitude_adjoint_model.py on the CPU model, tests/test_gpu_rollout_attitude_adjoint.py on the device), built
without a device.  The four loops of rollout_adjoint_cases.py -- starts at tick 2 | pushed | on the throttle clamp | hover --
with loop 3 tilted to rpy (0.5, -0.7, 3.1) rad (RPYINIT with it, as rollout_adjoint_edge_cases.py's tilted loops), its timing
(ratio 4, 5 sub-steps), trajectory, alpha track, gains and loss, under the attitude tracks

    rpy[k]     = 0.05 sin(3 t_k) [1, -0.6, 0.4]              t_k = k period_large
    rpy_dot[k] = 0.15 cos(3 t_k) [1, -0.5, 0.2] + 0.02

so that the h_ang reference R I_B R^T W rpy_dot reaches 1.4 at I_B = diag(8, 7, 2).  A loop is named by a key (case, b):

  base        the four loops over 9 ticks: the `first` fill (samples 0, 1) and two pushes (2, 3).  Loop 0's PP_TICK0 = 2: its fill
              comes from shifted samples, its release ticks are ticks 1 and 5 of the run
  short3      a track of 3 samples: the fill's columns and the pushes share samples (the owner rule)
  late        the run that is taped begins 3 ticks after the reset: 9 taped ticks behind 3 untaped ones
  null_rpyd   no RPYDot track (NULL under the flag): the gradient at the zero track
  null_both   neither track: the loops of rollout_adjoint_cases.py as they fly without attitude tracks, loop 3 tilted
  offdiag     an I_B with nine distinct entries
  unsolved    rollout_adjoint_cases.plants(unsolved_loop=1): loop 1 never solves
  tree        loop POSED of rollout_tree_adjoint_cases.py (the kinematic-tree plant, joints away from zero, pushed) under the
              same tracks, b = 0

All at horizon (6, 2, 3); `base` also at (17, 7, 12), the tuned handle's."""
import functools

import numpy as np

import rollout_adjoint_cases as rc
import rollout_attitude_adjoint_model as atm
import rollout_adjoint_model as ram
import rollout_param_adjoint_cases as pc
import rollout_tree_adjoint_cases as tc
import rollout_tree_adjoint_model as rtm

L = rc.L
B, TICKS = rc.B, rc.TICKS
HORIZONS = rc.HORIZONS
HORIZON = HORIZONS[0]
TILTED, TILT = 3, (0.5, -0.7, 3.1)
LATE_FROM = 3
UNSOLVED_LOOP = 1
TREE_LOOP = tc.POSED
OFFDIAG = np.array([[0.0, 0.31, -0.22], [0.13, 0.0, 0.27], [-0.36, 0.18, 0.0]])
PARAMETRIC = ("base", "short3", "late", "null_rpyd", "null_both", "offdiag")
N_TRAJ = {"short3": 3}
# the bar of both test files: rollout_param_adjoint_cases.py's rule and constants, for the old outputs and for the two new track
# fields (test_rollout_attitude_adjoint_model.py measures the model's worst error on them: within a tenth of FD_BAR)
FLOOR_RATIO, FD_BAR, FD_FLOOR = pc.FLOOR_RATIO, pc.FD_BAR, pc.FD_FLOOR

# the loops of the CPU checks against central differences: `base` whole, of the other parametric cases the loop that starts at
# tick 2 and the tilted one; the device covers every loop of every case
CPU_LOOPS = tuple(("base", b) for b in range(B)) + tuple((c, b) for c in PARAMETRIC[1:] for b in (0, TILTED)) + (("tree", 0),)


def n_traj_of(case):
    return N_TRAJ.get(case, 24)


def ticks_before(case):
    return LATE_FROM if case == "late" else 0


def trajectory(case):
    return tc.trajectory() if case == "tree" else rc.trajectory(n_traj=n_traj_of(case))


def attitude_tracks(case):
    """(rpy, rpy_dot) [n_traj, 3]; rpy_dot is None for null_rpyd, both are for null_both"""
    t = np.arange(n_traj_of(case)) * rc.PERIODS["period_large"]
    rpy = 0.05 * np.sin(3.0 * t)[:, None] * np.array([1.0, -0.6, 0.4])
    rpyd = 0.15 * np.cos(3.0 * t)[:, None] * np.array([1.0, -0.5, 0.2]) + 0.02
    return (None if case == "null_both" else rpy), (None if case in ("null_rpyd", "null_both") else rpyd)


def plants(case):
    """(state [B, PLANT_STATE], params [B, PLANT_PARAMS]) of a case's loops (tree: its one loop, B = 1)"""
    if case == "tree":
        st, pa = tc.plants()
        return st[TREE_LOOP:TREE_LOOP + 1].copy(), pa[TREE_LOOP:TREE_LOOP + 1].copy()
    st, pa = rc.plants(UNSOLVED_LOOP if case == "unsolved" else None)
    st[TILTED, L.PS_RPY:L.PS_RPY + 3] = pa[TILTED, L.PP_RPYINIT:L.PP_RPYINIT + 3] = TILT
    if case == "offdiag":
        pa[:, L.PP_INERTIA_B:L.PP_INERTIA_B + 9] += OFFDIAG.reshape(-1)
    return st, pa


def gains(make, case, horizon=HORIZON):
    if case == "tree":
        return tc.gains(make, horizon)[TREE_LOOP:TREE_LOOP + 1]
    return rc.gains(make, horizon)


def config(make, horizon=HORIZON):
    return rc.config(make, horizon)


def loss_weights(case):
    """(log_bar [TICKS, B, 16], state_bar [B, PLANT_STATE]) on the taped ticks"""
    if case == "tree":
        lb, sb = tc.loss_weights()
        return lb[:, TREE_LOOP:TREE_LOOP + 1].copy(), sb[TREE_LOOP:TREE_LOOP + 1].copy()
    return rc.loss_weights()


def loop_inputs(ref, key, horizon=HORIZON):
    """(cfg, state0, params, trajectory, attitude tracks, log_bar [TICKS, 16], state_bar) of one loop for the numpy model"""
    case, b = key
    cfg = ram.with_gains(config(ref.Config, horizon), gains(ref.Config, case, horizon)[b])
    st, pa = plants(case)
    lb, sb = loss_weights(case)
    return cfg, st[b], pa[b], trajectory(case), attitude_tracks(case), lb[:, b], sb[b]


def forward(ref, key, horizon=HORIZON, att=None):
    """(log, final, tape) of the taped ticks of one loop (`att`: other attitude tracks than the case's)"""
    case, _ = key
    cfg, s0, p, traj, att0, _, _ = loop_inputs(ref, key, horizon)
    n0 = ticks_before(case)
    if case == "tree":
        rtm.set_tree(tc.tree())
    try:
        log, fin, tape = atm.forward(cfg, s0, p, traj, att0 if att is None else att, n0 + TICKS)
    finally:
        rtm.set_tree(None)
    return log[n0:], fin, tape[n0:]


def sweep(ref, key, horizon=HORIZON, mutation=None, tape=None):
    case, _ = key
    cfg, _, p, traj, att, lb, sb = loop_inputs(ref, key, horizon)
    tape = forward(ref, key, horizon)[2] if tape is None else tape
    n0 = ticks_before(case)
    return atm.backward(cfg, tape, p, traj, att, lb, sb, first=n0 == 0, tick_base=n0, mutation=mutation,
                        tree=tc.tree() if case == "tree" else None)


def central(ref, key, **kw):
    """rollout_attitude_adjoint_model.central of one loop (d_rpy=, d_rpy_dot=, step=, ...)"""
    case, _ = key
    cfg, s0, p, traj, att, lb, sb = loop_inputs(ref, key)
    n0 = ticks_before(case)
    if case == "tree":
        rtm.set_tree(tc.tree())
    try:
        return atm.central(cfg, s0, p, traj, att, n0 + TICKS, lb, sb, taped_from=n0, **kw)
    finally:
        rtm.set_tree(None)


@functools.lru_cache(maxsize=None)
def model(key, horizon=HORIZON):
    """One loop on the CPU model, computed once: the sweep's outputs with "log", "final" and "tape" of the taped ticks"""
    import vsmpc_ref as ref
    log, fin, tape = forward(ref, key, horizon)
    out = sweep(ref, key, horizon, tape=tape)
    out.update(log=log, final=fin, tape=tape)
    return out


def att_row(out):
    """grad_att of one loop as the entry lays it out: traj_rpy | traj_rpy_dot"""
    return np.concatenate([out["grad_traj_rpy"].reshape(-1), out["grad_traj_rpy_dot"].reshape(-1)])


def att_fields(n_traj):
    """(field, offset, length) of one row of grad_att"""
    return tuple((name, off, n) for name, (off, n, _) in L.att_grad_blocks(n_traj).items())


def reached(ref, key):
    case, _ = key
    cfg, _, p, traj, _, _, _ = loop_inputs(ref, key)
    n0 = ticks_before(case)
    return atm.reached(cfg, p, len(traj[0]), TICKS, first=n0 == 0, tick_base=n0)
