"""Closed loops for the rollout adjoint away from the one timing, attitude and throttle box of rollout_adjoint_cases.py
(tests/test_rollout_adjoint_edge_cases.py on the CPU model, tests/test_gpu_rollout_adjoint_cases.py on the device), built
without a device.  One entry of CASES is one rollout: a horizon, the three periods, a number of ticks, the kind of handle
(runtime-sized "always" | tuned "never"), a trajectory and one to four loops, every loop with its own row of gains.

  sub1             period_mpc = 1 ms: one sub-step per tick, the recomputation loop of the plant half runs zero times
  sub16_ratio2     period_mpc = 20 ms: the cap of 16 sub-steps (h = 1.25 ms, not 1 ms), every LDS row of the sub-steps full;
                   ratio 2; loop 0 is pushed from between sub-steps 2 and 3 to between sub-steps 9 and 10 of tick 1
  paper_rt         the paper's timing 0.01 / 0.01 / 0.1 (10 sub-steps, ratio 10) over 21 ticks at (6, 2, 3); starts at tick 7
  paper_tuned      the same timing at (17, 7, 12) on the tuned handle: a plain loop, a loop with PP_TICK0 = 5000 (trajectory
                   samples 501 .. 503 of 520, alpha beyond its end), and a loop with throttle_min = 71 whose throttles fall
                   from 75 % onto that limit during the run: its active set changes
  rounded_ratio    period_small = 0.0047, period_large = 0.093: ratio lround(19.79) = 20, period_mpc = 0.004 (4 sub-steps);
                   the loops start at ticks 17 and 38, so that each crosses one release
  trajectory_end   a trajectory of 3 samples over 13 ticks: loop 0 pushes samples 2, 3, 4 (the last two clamped), loop 1
                   starts at tick 9, where the `first` fill asks for sample 3.  Alpha has 4 samples at alpha_dt = 0.004 =
                   period_mpc: every sub-step of ticks 0 .. 2 reads another alpha, ticks 3 .. lie beyond the track's end.
                   (A track finer than the controller's rate, with sub-steps of one tick in different segments, cannot be
                   had: vsmpc_rollout_create refuses a track whose rate does not divide 1 / period_mpc.)
  trajectory_one   a trajectory of one sample: every index is 0
  long_window      (40, 2, 40) at ratio 2: n_ref = 39, a window of 468 = 7 * 64 + 20 entries, shifted back twice in 5 ticks
  tilted           rpy (0.5, -0.7, 3.1) with h_ang (3, -2, 4): yaw passes +pi during the run; the opposite signs: yaw passes
                   -pi; pitch 1.2, where 1 / cos^2 is 7.6
  boxed            the hover loop under its own row with throttle_min = 73, throttle_max = 74, both active from the first
                   tick, between two loops of rollout_adjoint_cases.py under the plain box

The loss is rollout_adjoint_cases.py's: a random linear functional of the log and of the final state.  BATCHES describes
the batch sizes the device test runs rollout_adjoint_cases.py's own four loops at."""
import dataclasses
import functools
import math

import numpy as np

import rollout_adjoint_cases as rc
import rollout_adjoint_model as ram

L = rc.L
SEED = rc.SEED + 100
DEFAULT = (0.005, 0.005, 0.02)                # rollout_adjoint_cases.PERIODS: 5 sub-steps, ratio 4
PAPER = (0.01, 0.01, 0.1)
ALPHA = (1.0, 0.9, 0.85, 0.8)
BATCHES = (1, 257)                            # the hover loop alone | more loops than the device has compute units
BOX_W_THROTTLE = 100.0                        # w_throttle and w_initial_throttle of the loop boxed in at 73 .. 74 %


@dataclasses.dataclass(frozen=True)
class Case:
    horizon: tuple
    periods: tuple                            # period_mpc, period_small, period_large
    ticks: int
    runtime: str                              # ClosedLoopRollout(runtime=...): "always" | "never"
    loops: tuple                              # names of _LOOPS
    n_traj: int = 24
    alpha_dt: float = 0.1
    bounded: bool = False                     # a trajectory that stays small however long it is
    step: float = 1e-2                        # of the difference quotients, times the entry's scale


CASES = {
    "sub1": Case((6, 2, 3), (0.001, 0.005, 0.02), 9, "always", ("hover", "tick2")),
    "sub16_ratio2": Case((6, 2, 3), (0.02, 0.005, 0.01), 5, "always", ("pushed_in_tick1", "tick1")),
    "paper_rt": Case((6, 2, 3), PAPER, 21, "always", ("tick7",), n_traj=520, bounded=True),
    # step: the throttles of min71 reach their limit one after the other, some tick always has one within 1e-5 (1 + |v|) of
    # it, and a quotient that crosses the change is off: its gains directions miss the bar by 1.4e4 with the step 1e-2, by
    # 3.2e2 with 1e-3, and are at 7e-3 of it with 1e-4 (the state directions at 8e-3)
    "paper_tuned": Case((17, 7, 12), PAPER, 21, "never", ("hover", "tick5000", "min71"), n_traj=520, bounded=True, step=1e-4),
    "rounded_ratio": Case((6, 2, 3), (0.004, 0.0047, 0.093), 5, "always", ("tick17", "tick38")),
    "trajectory_end": Case((6, 2, 3), (0.004, 0.005, 0.02), 13, "always", ("hover", "tick9"), n_traj=3, alpha_dt=0.004),
    "trajectory_one": Case((6, 2, 3), (0.004, 0.005, 0.02), 5, "always", ("hover",), n_traj=1, alpha_dt=0.004),
    "long_window": Case((40, 2, 40), (0.005, 0.005, 0.01), 5, "always", ("hover", "tick1")),
    "tilted": Case((6, 2, 3), DEFAULT, 9, "always", ("yaw_plus_pi", "yaw_minus_pi", "pitch12")),
    "boxed": Case((6, 2, 3), DEFAULT, 9, "always", ("rc0", "box7374", "rc1")),
}
SWITCHING = ("paper_tuned", 2)                # the loop whose active set changes
BOXED = ("boxed", 1)                          # the loop with both limits active from the first tick

# loop name -> (row of rollout_adjoint_cases.plants() it starts from, PP_TICK0, what else is changed)
_LOOPS = {
    "hover": (3, 0, None), "tick1": (0, 1, None), "tick2": (0, 2, None), "tick7": (0, 7, None), "tick9": (0, 9, None),
    "tick17": (3, 17, None), "tick38": (0, 38, None), "tick5000": (1, 5000, None),
    "pushed_in_tick1": (1, 0, "push"), "yaw_plus_pi": (3, 0, "tilt+"), "yaw_minus_pi": (0, 0, "tilt-"), "pitch12": (1, 0, "pitch"),
    "min71": (3, 0, "min71"), "box7374": (3, 0, "box"), "rc0": (0, 2, None), "rc1": (1, 0, "rc"),
}


def config(make, case):
    """make = layout.MPCConfig or vsmpc_ref.Config"""
    c = CASES[case]
    n, ns, hc = c.horizon
    return make(n_iter=n, n_iter_small=ns, control_horizon=hc, period_mpc=c.periods[0], period_small=c.periods[1],
                period_large=c.periods[2])


def trajectory(case):
    """(pos, vel, alpha, alpha_dt): rollout_adjoint_cases.trajectory's accelerating track at this case's period_large, or
    (bounded) a slow sway of a few centimetres"""
    c = CASES[case]
    t = np.arange(c.n_traj) * c.periods[2]
    if c.bounded:
        pos = np.stack([0.05 * np.sin(0.7 * t), 0.04 * (np.cos(0.5 * t) - 1.0), 0.06 * np.sin(0.3 * t)], axis=1)
        vel = np.stack([0.035 * np.cos(0.7 * t), -0.02 * np.sin(0.5 * t), 0.018 * np.cos(0.3 * t)], axis=1)
    else:
        pos = np.stack([0.3 * t ** 2, -0.2 * t ** 2 + 0.05 * t, 0.5 * t ** 2], axis=1)
        vel = np.stack([0.6 * t, -0.4 * t + 0.05, 1.0 * t], axis=1)
    return pos, vel, np.array(ALPHA), c.alpha_dt


def plants(case):
    """(state [B, PLANT_STATE], params [B, PLANT_PARAMS]) of the case's loops, from rollout_adjoint_cases.plants()"""
    c = CASES[case]
    st0, pa0 = rc.plants()
    st, pa = np.zeros((len(c.loops), L.PLANT_STATE)), np.zeros((len(c.loops), L.PLANT_PARAMS))
    for b, name in enumerate(c.loops):
        row, tick0, what = _LOOPS[name]
        s, p = st0[row].copy(), pa0[row].copy()
        p[L.PP_TICK0] = float(tick0)
        if what != "rc":
            p[L.PP_DIST_F:L.PP_DIST_F + 3] = p[L.PP_DIST_TAU:L.PP_DIST_TAU + 3] = 0.0
            p[L.PP_DIST_T0] = p[L.PP_DIST_T1] = 0.0
        if what == "push":                     # on from between sub-steps 2, 3 to between sub-steps 9, 10 of tick 1
            h = c.periods[0] / ram.substeps_of(config(L.MPCConfig, case))
            p[L.PP_DIST_F:L.PP_DIST_F + 3] = [12.0, -8.0, 5.0]
            p[L.PP_DIST_TAU:L.PP_DIST_TAU + 3] = [1.5, -2.0, 0.8]
            p[L.PP_DIST_T0], p[L.PP_DIST_T1] = c.periods[0] + 2.5 * h, c.periods[0] + 9.5 * h
        if what in ("tilt+", "tilt-", "pitch"):
            rpy, hang = {"tilt+": ((0.5, -0.7, 3.1), (3.0, -2.0, 4.0)), "tilt-": ((-0.5, 0.7, -3.1), (-3.0, 2.0, -4.0)),
                         "pitch": ((0.3, 1.2, -1.0), (2.0, 1.5, -3.0))}[what]
            s[L.PS_RPY:L.PS_RPY + 3] = p[L.PP_RPYINIT:L.PP_RPYINIT + 3] = rpy
            s[L.PS_HANG:L.PS_HANG + 3] = hang
        st[b], pa[b] = s, p
    return st, pa


def gains(make, case):
    """one row of gains per loop (VSMPC_GRAD_* order): the configuration's, the boxed loops with their own limits"""
    c = CASES[case]
    g = np.tile(ram.gains_of(config(make, case)), (len(c.loops), 1))
    for b, name in enumerate(c.loops):
        what = _LOOPS[name][2]
        if what == "min71":
            g[b, 29] = 71.0
        elif what == "box":
            g[b, 29], g[b, 30] = 73.0, 74.0
            # under the configuration's w_throttle = 8e4 a free throttle beside a pinned one that sits on a limit follows it
            # to 7e-7 (1 + |v|): a hundredth of a percent of throttle from changing its state.  Cheap as loop 2 of
            # rollout_adjoint_cases.py it keeps 5.8e-4 (measured), with the same throttles on the same limits.
            g[b, 26] = g[b, 27] = BOX_W_THROTTLE
    return g


def loss_weights(ticks, batch, seed=SEED + 7):
    """rollout_adjoint_cases.loss_weights for any number of ticks and loops"""
    rng = np.random.default_rng(seed)
    log_scale = np.concatenate([np.full(3, 1e2), np.full(3, 1e2), np.full(4, 1.0), np.full(4, 1.0), np.full(2, 1e3)])
    log_bar = rng.normal(size=(ticks, batch, L.ROLLOUT_LOG)) * log_scale
    state_bar = rng.normal(size=(batch, L.PLANT_STATE))
    state_bar[:, :ram.NS] /= ram.state_scale()
    return log_bar, state_bar


def case_loss_weights(case):
    return loss_weights(CASES[case].ticks, len(CASES[case].loops))


def loop_inputs(ref, case, b):
    """(cfg, state0, params, trajectory, log_bar, state_bar) of loop b for rollout_adjoint_model"""
    st, pa = plants(case)
    lb, sb = case_loss_weights(case)
    cfg = ram.with_gains(config(ref.Config, case), gains(ref.Config, case)[b])
    return cfg, st[b], pa[b], trajectory(case), lb[:, b], sb[b]


@functools.lru_cache(maxsize=None)
def model(case, ticks=None):
    """The case's loops on the CPU model, computed once, as rollout_adjoint_cases.model: log [ticks, B, 16], final, tapes and
    the sweep's grad_state0, grad_cfg, flags, tick_flags; tick_active and tick_v are the states (sensitivity_model's) and
    the values of the QP's throttles at every tick.  ticks: another number of ticks than the case's (its first rows of the
    loss weights, or rows of their own beyond them)."""
    import vsmpc_ref as ref
    c = CASES[case]
    B, T = len(c.loops), c.ticks if ticks is None else ticks
    lb_all = loss_weights(T, B)[0] if T > c.ticks else case_loss_weights(case)[0][:T]
    out = {"log": np.zeros((T, B, L.ROLLOUT_LOG)), "final": np.zeros((B, L.PLANT_STATE)), "tapes": [],
           "grad_state0": np.zeros((B, ram.NS)), "grad_cfg": np.zeros((B, 32)), "flags": np.zeros(B, dtype=int), "tick_flags": [],
           "tick_active": [], "tick_v": [], "log_bar": lb_all}
    for b in range(B):
        cfg, s0, p, traj, _, sb = loop_inputs(ref, case, b)
        log, fin, tape = ram.forward(cfg, s0, p, traj, T)
        bw = ram.backward(cfg, tape, p, traj, lb_all[:, b], sb)
        out["log"][:, b], out["final"][b] = log, fin
        out["tapes"].append(tape)
        out["grad_state0"][b], out["grad_cfg"][b], out["flags"][b] = bw["grad_state0"], bw["grad_cfg"], bw["flags"]
        for k in ("tick_flags", "tick_active", "tick_v"):
            out[k].append(bw[k])
    return out


def model_rates(ref, case):
    """the rates tick_model derives from the case's periods and tracks, with those of vsmpc_rollout_create beside them: the
    CPU model stands for the device only where they agree"""
    c = CASES[case]
    cfg = config(ref.Config, case)
    fps_alpha = int(round(1.0 / c.alpha_dt))
    return {"des_fps": (int(1 / cfg.period_mpc), int(1.0 / cfg.period_mpc + 1e-9)),
            "ratio": (cfg.ratio, int(math.floor(cfg.period_large / cfg.period_small + 0.5))),
            "alpha_up": (int(1 / cfg.period_mpc) / fps_alpha, int(1.0 / cfg.period_mpc + 1e-9) // fps_alpha),
            "fps_alpha": fps_alpha}
