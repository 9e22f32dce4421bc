"""The closed loops the rollout adjoint is tested on with the KINEMATIC-TREE plant (tests/test_rollout_tree_adjoint_model.py
on the CPU model, tests/test_gpu_rollout_tree_adjoint.py on the device), built without a device.  The default tree
(robot_tree.default_tree), rollout_adjoint_cases.py's timing (periods 0.005 / 0.005 / 0.02: ratio 4), moving trajectory,
falling alpha-gravity and nine ticks, so that two release ticks and the `first` fill of the window are crossed:

  0  hover      rollout.make_plant_tree's hover instance, joints at zero
  1  posed      joints drawn at 0.3 rad standard deviation, one thrust 20 % low with its reference, pushed over ticks 2 .. 5
  2  boxed      under its own row of gains with the throttle box 73 .. 74 % and a cheap throttle (as
                rollout_adjoint_edge_cases.py's boxed loop): a limit is active from the first tick
  3  unsolved   the latched thrust references are NaN (rollout_adjoint_cases.plants): no tick is Solved, no move is consumed
  4  tick2      starts at PP_TICK0 = 2: its release ticks are ticks 1 and 5 of the run

SELECTED = (1, SELECTOR) is loop 1 again under a joint selector (vsmpc_set_kinematics_options) that is not the default: the
MPC then reads Lambda_ang's columns pairwise swapped.  Loops 0 and 1 are also run at (17, 7, 12), the tuned handle's horizon.
The loss is rollout_adjoint_cases.py's, drawn for five loops."""
import functools
import importlib

import numpy as np

import rollout_adjoint_cases as rc
import rollout_adjoint_edge_cases as ec
import rollout_adjoint_model as ram
import rollout_tree_adjoint_model as rtm

PKG = rc.PKG
L = rc.L
B, TICKS = 5, rc.TICKS
HORIZONS = rc.HORIZONS
NAMES = ("hover", "posed", "boxed", "unsolved", "tick2")
TUNED_LOOPS = (0, 1)                           # the loops that are also run at HORIZONS[1]
UNSOLVED, BOXED, POSED = 3, 2, 1
SELECTOR = (4, 3, 6, 5, 8, 7, 10, 9)           # robot joints of Lambda_ang's columns: the default 3 .. 10 swapped in pairs
SELECTED = (POSED, SELECTOR)
SEED = 20253
BOX = (73.0, 74.0)
BOX_W_THROTTLE = ec.BOX_W_THROTTLE


def tree():
    return importlib.import_module(PKG + ".robot_tree").default_tree()


def config(make, horizon):
    return rc.config(make, horizon)


def trajectory():
    return rc.trajectory()


def plants():
    """(state [5, PLANT_STATE], params [5, PLANT_PARAMS]) of the five loops"""
    ro = importlib.import_module(PKG + ".rollout")
    st, pa = ro.make_plant_tree(config(L.MPCConfig, HORIZONS[0]), B, tree(), workload="hover", seed0=SEED)
    rng = np.random.default_rng(SEED)
    pa[:, L.PP_TICK0] = 0.0
    pa[4, L.PP_TICK0] = 2.0
    st[POSED, L.PS_Q:L.PS_Q + 8] = 0.3 * rng.normal(size=8)
    st[POSED, L.PS_T + 1] *= 0.8
    st[POSED, L.PS_TDES + 1] = st[POSED, L.PS_T + 1]
    pa[POSED, L.PP_DIST_F:L.PP_DIST_F + 3] = [12.0, -8.0, 5.0]
    pa[POSED, L.PP_DIST_TAU:L.PP_DIST_TAU + 3] = [1.5, -2.0, 0.8]
    pa[POSED, L.PP_DIST_T0], pa[POSED, L.PP_DIST_T1] = 0.0105, 0.0285
    st[UNSOLVED, L.PS_TDES:L.PS_TDES + 4] = np.nan
    return st, pa


def gains(make, horizon):
    """one row of gains per loop ([5, 32], VSMPC_GRAD_* order): the configuration's, the boxed loop with its own"""
    g = np.tile(ram.gains_of(config(make, horizon)), (B, 1))
    g[BOXED, 29], g[BOXED, 30] = BOX
    g[BOXED, 26] = g[BOXED, 27] = BOX_W_THROTTLE
    return g


def loss_weights():
    """(log_bar [TICKS, 5, 16], state_bar [5, PLANT_STATE])"""
    return ec.loss_weights(TICKS, B)


def loop_inputs(ref, b, horizon=HORIZONS[0]):
    """(cfg, state0, params, trajectory, log_bar [TICKS, 16], state_bar) of loop b for the numpy models"""
    cfg = ram.with_gains(config(ref.Config, horizon), gains(ref.Config, horizon)[b])
    st, pa = plants()
    lb, sb = loss_weights()
    return cfg, st[b], pa[b], trajectory(), lb[:, b], sb[b]


def forward(ref, b, horizon=HORIZONS[0], selector=None, unsolved_ticks=()):
    """(log, final, tape) of loop b on the tree plant; rollout_model is back on the parametric plant afterwards.
    unsolved_ticks: rollout_adjoint_model.forward's (those ticks do not consume their move)"""
    cfg, s0, p, traj, _, _ = loop_inputs(ref, b, horizon)
    rtm.set_tree(tree(), selector)
    try:
        return ram.forward(cfg, s0, p, traj, TICKS, unsolved_ticks=unsolved_ticks)
    finally:
        rtm.set_tree(None)


def qp_iterations(cfg, rec):
    """the pass count of the throttle box QP of one record (runtime_model.box_qp, the kernel's P4): what the device logs in
    column 15.  The same route as rollout_adjoint_model.solve_tick, which drops the count.  0 for a record that does not factor."""
    import adjoint_model as am
    import runtime_model as rm
    import vsmpc_ref as ref
    try:
        M, S, s, gmax, vprev, _ = am._schur(cfg, rec)
    except FloatingPointError:
        return 0
    if not np.isfinite(M).all():
        return 0
    nv = am.NTH * cfg.n_vblocks
    vmin, vmax = ref.throttle_bounds(cfg)
    fixed, lo, hi = np.zeros(nv, dtype=bool), np.full(nv, vmin), np.full(nv, vmax)
    if rec[ref.IN_HOLD] != 0.0:
        fixed[:am.NTH] = True
        lo[:am.NTH] = hi[:am.NTH] = vprev
    return int(rm.box_qp(S, s, lo, hi, fixed, 1e-10 * (1.0 + gmax))[2])


@functools.lru_cache(maxsize=None)
def model(b, horizon=HORIZONS[0], selector=None, unsolved_ticks=(), mutation=None):
    """Loop b on the CPU model, computed once: rollout_tree_adjoint_model.backward's outputs with "log", "final" and "tape"
    of the forward loop beside them"""
    import vsmpc_ref as ref
    cfg, s0, p, traj, lb, sb = loop_inputs(ref, b, horizon)
    log, fin, tape = forward(ref, b, horizon, selector, unsolved_ticks)
    out = rtm.backward(cfg, tape, p, traj, lb, sb, tree(), selector, mutation=mutation)
    out.update(log=log, final=fin, tape=tape, tick_iters=[qp_iterations(cfg, t[1]) for t in tape])
    return out
