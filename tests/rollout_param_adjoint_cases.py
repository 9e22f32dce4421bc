"""The closed loops the parameter and track gradients of the rollout adjoint are tested on
(tests/test_rollout_param_adjoint_model.py on the CPU model, tests/test_gpu_rollout_param_adjoint.py on the device), built
without a device.  All at horizon (6, 2, 3) but the tuned one.  A loop is named by a key:

  ("rc", b)            loop b of rollout_adjoint_cases.py: starts at tick 2 | pushed over ticks 2 .. 5 | on the throttle
                       clamp | hover
  (case, b)            loop b of a case of rollout_adjoint_edge_cases.py:
                         sub16_ratio2     16 sub-steps; loop 0 is pushed inside tick 1 only
                         trajectory_end   a track of 3 samples; the alpha track (4 samples at period_mpc) ends inside the run
                         trajectory_one   a track of 1 sample
                         tilted           rpy far from zero, yaw through +-pi, pitch 1.2
                         tick5000         this module's: the paper's timing (10 sub-steps, ratio 10) from tick 5000 over 12
                                          ticks, trajectory samples 497 .. 502 of 520, alpha beyond its end
                         fast_track       this module's: the hover loop under a track that moves at metres per second, so that
                                          the mass is seen through the window columns' R^T m v_ref and not only through the plant
                         pushed_long      this module's: loop 1 of rollout_adjoint_cases.py pushed from the start to beyond the
                                          end of 21 ticks, so that DIST_F -- which reaches the loss through h_lin / m only --
                                          rises above a thousandth of the largest parameter gradient

The three cases of this module (OWN) are built by rollout_adjoint_edge_cases.py's builders (config, trajectory, plants, gains,
loss weights) like its own: `_ec` enters the case into its table for the length of one call and takes it out again, so that
nothing that walks that table ever sees them.  The loss is rollout_adjoint_cases.py's."""
import functools

import numpy as np

import rollout_adjoint_cases as rc
import rollout_adjoint_edge_cases as ec
import rollout_adjoint_model as ram
import rollout_param_adjoint_model as rpm

L = rc.L
HORIZON = rc.HORIZONS[0]
FAST_VEL = (1.5, -1.0, 2.0)                    # [m/s] of fast_track's track, constant; its positions follow
OWN = {"tick5000": ec.Case(HORIZON, ec.PAPER, 12, "always", ("tick5000",), n_traj=520, bounded=True),
       "fast_track": ec.Case(HORIZON, ec.DEFAULT, 9, "always", ("hover",)),
       "pushed_long": ec.Case(HORIZON, ec.DEFAULT, 21, "always", ("rc1",))}


def case(name):
    """the Case of a name: this module's, or rollout_adjoint_edge_cases.py's"""
    return OWN[name] if name in OWN else ec.CASES[name]


def _ec(fn, name, *args):
    """fn(*args) of rollout_adjoint_edge_cases.py with this module's case `name` in its table while the call lasts"""
    if name not in OWN:
        return fn(*args)
    assert name not in ec.CASES
    ec.CASES[name] = OWN[name]
    try:
        return fn(*args)
    finally:
        del ec.CASES[name]


# The bar of both test files, in the form of adjoint_record_model.worst_field: |err| <= FD_BAR (|field|_inf + FLOOR_RATIO max
# |gradient|).  MEASURED is the worst error of the numpy sweep against the Richardson-extrapolated quotients over LOOPS and the
# unsolved scenario (test_rollout_param_adjoint_model.py, which prints every loop's figure): loop 0 of `tilted`, RPYINIT.
FLOOR_RATIO = 1e-3
MEASURED = 9.2e-8
FD_BAR = 10.0 * MEASURED
FD_FLOOR = FD_BAR * FLOOR_RATIO
TUNED = "paper_tuned"                          # rollout_adjoint_edge_cases.py's, (17, 7, 12) on the tuned handle: device only

# every loop of the CPU checks, the device covers them all
LOOPS = tuple(("rc", b) for b in range(rc.B)) + (("sub16_ratio2", 0), ("sub16_ratio2", 1), ("trajectory_end", 0),
                                                 ("trajectory_end", 1), ("trajectory_one", 0), ("tilted", 0), ("tilted", 1),
                                                 ("tilted", 2), ("tick5000", 0), ("fast_track", 0), ("pushed_long", 0))
PUSH_MISSES = (("rc", 0), ("tilted", 0))       # loops whose push window (empty) misses the run
UNSOLVED = (("rc", 3), 4)                      # the loop and the tick of the scenario with a tick that is not Solved


def case_of(key):
    return None if key[0] == "rc" else key[0]


def trajectory(case):
    """(pos, vel, alpha, alpha_dt) of a case (None: rollout_adjoint_cases.py's)"""
    if case is None:
        return rc.trajectory()
    pos, vel, alpha, adt = _ec(ec.trajectory, case, case)
    if case == "fast_track":
        t = np.arange(len(pos)) * OWN[case].periods[2]
        vel = np.tile(np.array(FAST_VEL), (len(pos), 1))
        pos = t[:, None] * vel
    return pos, vel, alpha, adt


def ticks_of(name):
    return rc.TICKS if name is None else case(name).ticks


def plants(case):
    """(state [B, PLANT_STATE], params [B, PLANT_PARAMS]) of a case's loops (None: rollout_adjoint_cases.py's four)"""
    if case is None:
        return rc.plants()
    st, pa = _ec(ec.plants, case, case)
    if case == "pushed_long":
        pa[0, L.PP_DIST_T0], pa[0, L.PP_DIST_T1] = 0.0, 1.0
    return st, pa


def gains(make, case):
    return rc.gains(make, HORIZON) if case is None else _ec(ec.gains, case, make, case)


def config(make, case):
    return rc.config(make, HORIZON) if case is None else _ec(ec.config, case, make, case)


def loss_weights(case):
    """(log_bar [ticks, B, 16], state_bar [B, PLANT_STATE])"""
    return rc.loss_weights() if case is None else _ec(ec.case_loss_weights, case, case)


def loop_inputs(ref, key):
    """(cfg, state0, params, trajectory, log_bar [ticks, 16], state_bar, ticks) of one loop for the numpy models"""
    case, b = case_of(key), key[1]
    cfg = ram.with_gains(config(ref.Config, case), gains(ref.Config, case)[b])
    st, pa = plants(case)
    lb, sb = loss_weights(case)
    return cfg, st[b], pa[b], trajectory(case), lb[:, b], sb[b], ticks_of(case)


@functools.lru_cache(maxsize=None)
def model(key, unsolved_ticks=()):
    """One loop on the CPU model, computed once: rollout_param_adjoint_model.backward's outputs with "log", "final" and "tape"
    of the forward loop beside them"""
    import vsmpc_ref as ref
    cfg, s0, p, traj, lb, sb, ticks = loop_inputs(ref, key)
    log, fin, tape = ram.forward(cfg, s0, p, traj, ticks, unsolved_ticks=unsolved_ticks)
    out = rpm.backward(cfg, tape, p, traj, lb, sb)
    out.update(log=log, final=fin, tape=tape)
    return out


def traj_row(out):
    """grad_traj of one loop as the entry lays it out: traj_pos | traj_vel | traj_alpha"""
    return np.concatenate([out["grad_traj_pos"].reshape(-1), out["grad_traj_vel"].reshape(-1), out["grad_traj_alpha"]])


def traj_fields(n_traj, n_alpha):
    """(field, offset, length) of one row of grad_traj"""
    return tuple((name, off, n) for name, (off, n, _) in L.traj_grad_blocks(n_traj, n_alpha).items())
