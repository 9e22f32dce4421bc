"""Closed-loop batched rollout: host side of vsmpc_rollout_* in include/vsmpc.h.

`ClosedLoopRollout` keeps `batch` plant states resident in HBM and advances them tick by tick entirely on the GPU
(record builder -> MPC solve -> first move + plant integration); only the optional log rows come back to the host.
It exposes the tick state machine the reference hides in its plugins (20-tick throttle hold, reference window cursor,
alpha-gravity cursor: SURVEY.md A.7) and the harness loop of src/variable_sampling_mpc.py:49-152.

`make_plant` synthesises a well-posed jet humanoid for it: four jets (two on the arms, moved by the 8 controlled arm
joints, two on the back), symmetric about the CoM so that equal thrusts hover.  The reference takes these quantities
from a URDF + MuJoCo (out of scope); nothing here is read from the reference's model files.
All numerics run in libvsmpc.so (HIP); there is no CPU path in this module.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np

from . import _lib
from . import layout as L
from .jet_model import JetModel
from .solver import BatchedVSMPC, _ptr, pack_tunables
from .synth import GRAVITY, NOMINAL_MASS, alpha_gravity_profile, takeoff_profile

_JET = JetModel()


def make_plant(cfg: L.MPCConfig, batch: int, *, workload: str = "hover", seed0: int = 4321, first_index: int = 0):
    """(state[batch, PLANT_STATE], params[batch, PLANT_PARAMS]) for `workload`:
    "hover"       start near the hover equilibrium (sigma as configs[1]), trajectory offsets zero
    "takeoff"     start on the reference at a random tick of the flight part (19 s .. 35 s) of the take-off timeline
                  (configs[2]); the plant has no ground contact, so the supported phase before lift-off is left out
    "montecarlo"  hover with 4x wider initial scatter and a disturbance push of up to 50 N / 30 Nm lasting 0.1 s
                  that starts within the first second (configs[3])
    Every instance is drawn from its own generator seeded seed0 + index, so any slice can be rebuilt on any rank."""
    sigma = {"hover": 1.0, "takeoff": 0.2, "montecarlo": 4.0}[workload]
    state = np.zeros((batch, L.PLANT_STATE))
    params = np.zeros((batch, L.PLANT_PARAMS))
    # joint rotation axes of the two 4-dof arms (shoulder pitch / roll / yaw, elbow) in the body frame
    joint_axes = np.array([[0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, 1.0, 0.0]])
    for b in range(batch):
        rng = np.random.default_rng(seed0 + first_index + b)
        mass = float(np.float32(NOMINAL_MASS + rng.normal(0.0, 0.5)))
        inertia_B = np.diag([8.0, 7.0, 2.0]) + 0.05 * np.eye(3) * rng.uniform(0.0, 1.0)
        # jets: arm jets at (+0.10, +-0.30, 0.25), back jets at (-0.10, +-0.10, 0.20) from the CoM; axes ~ +z_B
        arms = np.array([[0.10, 0.30, 0.25], [0.10, -0.30, 0.25], [-0.10, 0.10, 0.20], [-0.10, -0.10, 0.20]])
        arms = arms + rng.normal(0.0, 0.003, size=(4, 3))
        shoulders = np.array([[0.0, 0.18, 0.35], [0.0, -0.18, 0.35]])
        axes = np.zeros((4, 3))
        for i in range(4):
            tilt = math.radians(2.0) * rng.uniform(0.0, 1.0)
            az = rng.uniform(0.0, 2 * math.pi)
            axes[i] = [math.sin(tilt) * math.cos(az), math.sin(tilt) * math.sin(az), math.cos(tilt)]
        A0 = np.zeros((6, 4))
        for i in range(4):
            A0[0:3, i] = axes[i]
            A0[3:6, i] = np.cross(arms[i], axes[i])
        DJ = np.zeros((8, 6, 4))   # dA_mom/dq_j: joint j of arm a rotates jet a's axis and lever arm about n_j
        for j in range(8):
            a, n = j // 4, joint_axes[j % 4]
            da = np.cross(n, axes[a])
            dr = np.cross(n, arms[a] - shoulders[a])
            DJ[j, 0:3, a] = da
            DJ[j, 3:6, a] = np.cross(dr, axes[a]) + np.cross(arms[a], da)
        p_init = np.array([0.0, 0.0, 1.0])
        rpy_init = rng.normal(0.0, 0.01, size=3)

        tick0 = int(rng.integers(3800, 7001)) if workload == "takeoff" else int(rng.integers(0, cfg.ratio))
        t0 = tick0 * cfg.period_mpc
        if workload == "takeoff":
            alpha = alpha_gravity_profile(t0)
            # start ON the reference the loop tracks at that tick: column 0 of the reference's FIFO window, i.e. the
            # trajectory sample pushed one window length (10 columns = 1 s) earlier (costsVSMPC.cpp:121-165)
            col0 = max(0, 1 + tick0 // cfg.ratio - (cfg.n_ref_cols - 1))
            dp, dv = takeoff_profile(col0 * cfg.period_large)
        else:
            alpha, dp, dv = 1.0, np.zeros(3), np.zeros(3)
        rpy = rpy_init + rng.normal(0.0, 0.05 * sigma, size=3)
        p = p_init + dp + rng.normal(0.0, 0.05 * sigma, size=3)
        T = np.maximum(alpha * mass * GRAVITY / 4.0 * (1.0 + rng.normal(0.0, 0.05 * sigma, size=4)), 5.0)
        u = np.clip([float(_JET.steady_state_throttle(Ti)) for Ti in T], 0.0, 100.0)

        s = state[b]
        s[L.PS_P:L.PS_P + 3] = p
        s[L.PS_HLIN:L.PS_HLIN + 3] = mass * (dv + rng.normal(0.0, 0.02 * sigma, size=3))
        s[L.PS_RPY:L.PS_RPY + 3] = rpy
        s[L.PS_HANG:L.PS_HANG + 3] = rng.normal(0.0, 0.2 * sigma, size=3)
        s[L.PS_T:L.PS_T + 4] = T
        s[L.PS_TD:L.PS_TD + 4] = 0.0
        s[L.PS_Q:L.PS_Q + 8] = 0.0
        s[L.PS_U:L.PS_U + 4] = u
        s[L.PS_TDES:L.PS_TDES + 4] = T
        s[L.PS_TDDES:L.PS_TDDES + 4] = 0.0
        # jet plant option (set_jet_plant): the NN thrust and the EKF estimates start on the plant thrust, P = 0.1 I
        # (ironcub_mujoco_simulator.py:54-57); the polynomial jet plant ignores these fields
        s[L.PS_TNN:L.PS_TNN + 4] = np.asarray(T, dtype=np.float32)
        s[L.PS_EST:L.PS_EST + 8:2] = T
        s[L.PS_EKFP:L.PS_EKFP + 16] = np.tile(0.1 * np.eye(2).reshape(-1), 4)

        q = params[b]
        q[L.PP_MASS] = mass
        q[L.PP_INERTIA_B:L.PP_INERTIA_B + 9] = inertia_B.reshape(-1)
        q[L.PP_AMOM0:L.PP_AMOM0 + 24] = A0.reshape(-1)
        q[L.PP_DJ:L.PP_DJ + 192] = DJ.reshape(-1)
        q[L.PP_QREF0:L.PP_QREF0 + 8] = 0.0
        q[L.PP_PINIT:L.PP_PINIT + 3] = p_init
        q[L.PP_RPYINIT:L.PP_RPYINIT + 3] = rpy_init
        if workload == "montecarlo":
            v = rng.normal(size=3)
            w = rng.normal(size=3)
            q[L.PP_DIST_F:L.PP_DIST_F + 3] = rng.uniform(0.0, 50.0) * v / np.linalg.norm(v)
            q[L.PP_DIST_TAU:L.PP_DIST_TAU + 3] = rng.uniform(0.0, 30.0) * w / np.linalg.norm(w)
            ts = t0 + rng.uniform(0.0, 1.0)
            q[L.PP_DIST_T0], q[L.PP_DIST_T1] = ts, ts + 0.1
        q[L.PP_TICK0] = float(tick0)
    return state, params


def make_plant_tree(cfg: L.MPCConfig, batch: int, tree: dict, *, workload: str = "hover", seed0: int = 4321, first_index: int = 0):
    """Plant states / parameters for the KINEMATIC-TREE plant (ClosedLoopRollout.set_tree): make_plant's instances with the
    tree's total mass, joints at zero and initial thrusts that carry that mass; AMOM0 / DJ / INERTIA_B stay in the
    parameter record but are not read in tree mode (A_mom(q), I_B(q), Lambda come from the provider on the plant's joints)."""
    state, params = make_plant(cfg, batch, workload=workload, seed0=seed0, first_index=first_index)
    m_tree = float(np.float32(sum(tree["mass"])))
    for b in range(batch):
        scale = m_tree / params[b, L.PP_MASS]
        params[b, L.PP_MASS] = m_tree
        state[b, L.PS_HLIN:L.PS_HLIN + 3] *= scale
        T = state[b, L.PS_T:L.PS_T + 4] * scale
        u = np.clip([float(_JET.steady_state_throttle(Ti)) for Ti in T], 0.0, 100.0)
        state[b, L.PS_T:L.PS_T + 4] = T
        state[b, L.PS_U:L.PS_U + 4] = u
        state[b, L.PS_TDES:L.PS_TDES + 4] = T
        state[b, L.PS_TNN:L.PS_TNN + 4] = np.asarray(T, dtype=np.float32)
        state[b, L.PS_EST:L.PS_EST + 8:2] = T
    return state, params


def make_trajectory(cfg: L.MPCConfig, workload: str = "hover", horizon_s: float = 60.0):
    """(pos[n,3], vel[n,3], alpha[m], alpha_dt): CoM offsets / velocities sampled every periodMPCLargeSteps and the
    alpha-gravity profile sampled at 10 Hz, the rates of the reference's MAT trajectories."""
    n = int(round(horizon_s / cfg.period_large)) + 1
    pos, vel = np.zeros((n, 3)), np.zeros((n, 3))
    alpha_dt = 0.1
    m = int(round(horizon_s / alpha_dt)) + 1
    alpha = np.ones(m)
    if workload == "takeoff":
        for i in range(n):
            pos[i], vel[i] = takeoff_profile(i * cfg.period_large)
        alpha = np.array([alpha_gravity_profile(i * alpha_dt) for i in range(m)])
    return pos, vel, alpha, alpha_dt


def load_reference_trajectories(npz_path: str):
    """(pos[n,3], vel[n,3], alpha[m], alpha_dt) from an npz holding the reference's own trajectory arrays
    (`positionCoM`, `velocityCoM` [n,3], `alphaGravity` [m], `trajectory_fps`, `alphaGravity_fps`): the content of
    src/trajectories/{minimumJerkTrajectory,alphaGravity}.mat as plain arrays (tools/gen_reference_constants.py writes
    tests/golden/reference_trajectories.npz; MAT-7.3 reading itself stays outside the path)."""
    d = np.load(npz_path)
    pos = np.ascontiguousarray(d["positionCoM"], dtype=np.float64)
    vel = np.ascontiguousarray(d["velocityCoM"], dtype=np.float64)
    alpha = np.ascontiguousarray(d["alphaGravity"], dtype=np.float64).reshape(-1)
    return pos, vel, alpha, 1.0 / float(d["alphaGravity_fps"].reshape(-1)[0])


class ClosedLoopRollout:
    """`batch` closed loops resident on one GPU.  reset() uploads plant states, run(ticks) advances them."""

    def __init__(self, cfg: L.MPCConfig, batch: int, traj_pos, traj_vel, traj_alpha, alpha_dt: float, device: int = 0,
                 runtime: str = "never", adjoint: bool = False):
        """adjoint: create the handle with what backward() needs (VSMPC_CREATE_ADJOINT_RECORD)"""
        self.cfg = cfg
        self.batch = batch
        self.mpc = BatchedVSMPC(cfg, device=device, max_batch=batch, runtime=runtime, adjoint_record=adjoint)   # runtime: see BatchedVSMPC
        self.lib = self.mpc.lib
        pos = np.ascontiguousarray(traj_pos, dtype=np.float64)
        vel = np.ascontiguousarray(traj_vel, dtype=np.float64)
        alpha = np.ascontiguousarray(traj_alpha, dtype=np.float64)
        if pos.shape != vel.shape or pos.ndim != 2 or pos.shape[1] != 3:
            raise ValueError("traj_pos / traj_vel must be [n, 3]")
        self.n_traj = pos.shape[0]
        self.n_alpha = alpha.shape[0]
        self._r = ctypes.c_void_p()
        _lib.check(self.lib.vsmpc_rollout_create(self.mpc._h, batch, _ptr(pos), _ptr(vel), pos.shape[0], _ptr(alpha),
                                                 alpha.shape[0], float(alpha_dt), ctypes.byref(self._r)),
                   "vsmpc_rollout_create")

    def close(self):
        if getattr(self, "_r", None) is not None and self._r:
            self.lib.vsmpc_rollout_destroy(self._r)
            self._r = None
        if getattr(self, "mpc", None) is not None:
            self.mpc.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self, state: np.ndarray, params: np.ndarray):
        state = np.ascontiguousarray(state, dtype=np.float64)
        params = np.ascontiguousarray(params, dtype=np.float64)
        if state.shape != (self.batch, L.PLANT_STATE) or params.shape != (self.batch, L.PLANT_PARAMS):
            raise ValueError("state / params shape does not match the rollout batch")
        _lib.check(self.lib.vsmpc_rollout_reset(self._r, _ptr(state), _ptr(params)), "vsmpc_rollout_reset")

    def set_attitude_tracks(self, traj_rpy=None, traj_rpy_dot=None, adjoint: bool = False):
        """RPY / RPYDot tracks of the position trajectory (vsmpc_rollout_set_attitude_tracks; costsVSMPC.cpp:110-112,
        141-146), [n_traj, 3] each or None (all zero, the shipped files).  Call reset() afterwards.
        adjoint: vsmpc_rollout_set_attitude_tracks_ex with VSMPC_ATTITUDE_ADJOINT -- run(tape=True) and backward() then work
        with an RPYDot track too, and backward(att=True) returns the gradient to both tracks; without it a rollout with an
        RPYDot track refuses them."""
        a = None if traj_rpy is None else np.ascontiguousarray(traj_rpy, dtype=np.float64)
        b = None if traj_rpy_dot is None else np.ascontiguousarray(traj_rpy_dot, dtype=np.float64)
        for t in (a, b):
            if t is not None and t.shape != (self.n_traj, 3):
                raise ValueError(f"attitude tracks must be [{self.n_traj}, 3]")
        if adjoint:
            _lib.check(self.lib.vsmpc_rollout_set_attitude_tracks_ex(self._r, _ptr(a), _ptr(b), L.ATTITUDE_ADJOINT),
                       "vsmpc_rollout_set_attitude_tracks_ex")
        else:
            _lib.check(self.lib.vsmpc_rollout_set_attitude_tracks(self._r, _ptr(a), _ptr(b)), "vsmpc_rollout_set_attitude_tracks")

    def set_tree(self, tree: dict | None, adjoint: bool = False):
        """Kinematic-tree plant (vsmpc_rollout_set_tree): `tree` = a robot_tree dictionary (None = the parametric plant).
        The plant's A_mom(q), I_B(q) and the MPC's Lambda terms then all come from the kinematics provider on the plant's
        own joints.  Call reset() afterwards; params[:, PP_MASS] must be the tree's total mass.
        adjoint: vsmpc_rollout_set_tree_ex with VSMPC_TREE_ADJOINT -- run(tape=True) and backward() then work on the tree
        plant (the rollout allocates the rows of the tree's terms and their Jacobian); without it they are refused."""
        from . import robot_tree as RT
        self._ctree = None if tree is None else RT.to_c(tree)    # (kept alive; the library copies it anyway)
        ctree = None if tree is None else ctypes.byref(self._ctree)
        if adjoint:
            _lib.check(self.lib.vsmpc_rollout_set_tree_ex(self._r, ctree, L.TREE_ADJOINT), "vsmpc_rollout_set_tree_ex")
        else:
            _lib.check(self.lib.vsmpc_rollout_set_tree(self._r, ctree), "vsmpc_rollout_set_tree")

    def set_tunables(self, configs=None, tunables=None):
        """Per-instance weights and throttle box for the loops' solves (vsmpc_rollout_set_tunables): `configs` = one
        MPCConfig per loop, or `tunables` = their packed rows [batch, L.TUNE_SIZE] (solver.pack_tunables); neither = back
        to the shared configuration.  Call reset() afterwards."""
        if configs is not None and tunables is not None:
            raise ValueError("give configs or tunables, not both")
        rows = None
        if configs is not None:
            rows = pack_tunables(self.mpc, configs)
        elif tunables is not None:
            rows = np.ascontiguousarray(tunables, dtype=np.float64)
        if rows is not None and rows.shape != (self.batch, L.TUNE_SIZE):
            raise ValueError(f"one configuration / one row of {L.TUNE_SIZE} tunables per loop ({self.batch})")
        _lib.check(self.lib.vsmpc_rollout_set_tunables(self._r, _ptr(rows)), "vsmpc_rollout_set_tunables")

    def set_noise(self, seed, first_index: int = 0, lin_vel: float = 0.015, ang_vel: float = 0.015, pos: float = 0.0,
                  rpy: float = 0.0, force: float = 0.0, torque: float = 0.0):
        """Seeded sensor noise and gusts (vsmpc_rollout_set_noise), drawn on the device by a counter-based generator: the
        controller is handed p + pos z, h_lin + m R^T (lin_vel z), rpy + rpy z and h_ang + I_B R^T (ang_vel z) in place of the
        plant's state (m, m/s, rad, rad/s), and a constant world force `force` z [N] and body torque `torque` z [Nm] act on
        the plant over every tick.  The defaults are the reference's simulate_noise (ironcub_mujoco_simulator.py:271-288).
        Loop b draws as loop first_index + b of the whole batch (sharding.rank_first_index).  seed=None turns the noise off.
        Call reset() afterwards; run(tape=True) and backward() are refused while noise is set."""
        if seed is None:
            _lib.check(self.lib.vsmpc_rollout_set_noise(self._r, None), "vsmpc_rollout_set_noise")
            return
        n = L.CNoise(int(seed), int(first_index), float(pos), float(lin_vel), float(rpy), float(ang_vel), float(force), float(torque))
        _lib.check(self.lib.vsmpc_rollout_set_noise(self._r, ctypes.byref(n)), "vsmpc_rollout_set_noise")

    def noise_draws(self, tick0: int, ticks: int, words: bool = False):
        """What ticks tick0 .. tick0 + ticks - 1 draw (vsmpc_rollout_noise_draws, the device function the kernels call):
        z [ticks, batch, 18] -- z[..., 0:12] the measurement of the tick, z[..., 12:18] its gust -- and with words=True also
        the generator's words [ticks, batch, 9, 4] (uint32)."""
        z = np.empty((int(ticks), self.batch, L.NOISE_DRAWS))
        w = np.empty((int(ticks), self.batch, L.NOISE_BLOCKS, 4), dtype=np.uint32) if words else None
        _lib.check(self.lib.vsmpc_rollout_noise_draws(self._r, int(tick0), int(ticks), _ptr(z), _ptr(w)), "vsmpc_rollout_noise_draws")
        return (z, w) if words else z

    def set_jet_plant(self, jet_model=None, Q=None, R=None):
        """Jet plant option (vsmpc_rollout_set_jet_plant): `jet_model` = a jet_plant.JetModelTotal (the LSTM thrust model;
        None = back to the polynomial jet plant); Q, R = EKF covariances, default 0.1 I / 0.5 I
        (ironcub_mujoco_simulator.py:54-56).  Call reset() afterwards."""
        Q = np.ascontiguousarray(0.1 * np.eye(2) if Q is None else Q, dtype=np.float64)
        R = np.ascontiguousarray(0.5 * np.eye(2) if R is None else R, dtype=np.float64)
        self._jet_model = jet_model            # keeps the jet handle alive as long as the rollout uses it
        _lib.check(self.lib.vsmpc_rollout_set_jet_plant(self._r, None if jet_model is None else jet_model._h, _ptr(Q), _ptr(R)),
                   "vsmpc_rollout_set_jet_plant")

    def run(self, ticks: int, log: bool = True, stream=None, tape: bool = False):
        """Advances every instance by `ticks` MPC periods.  Returns the log [ticks, batch, ROLLOUT_LOG] or None.
        tape: the taped run (vsmpc_rollout_run_taped): the same results bit for bit, and what backward() sweeps over."""
        out = np.empty((ticks, self.batch, L.ROLLOUT_LOG)) if log else None
        s = None if stream is None else ctypes.c_void_p(stream.cuda_stream)
        entry = "vsmpc_rollout_run_taped" if tape else "vsmpc_rollout_run"
        _lib.check(getattr(self.lib, entry)(self._r, int(ticks), _ptr(out), s), entry)
        self._taped = int(ticks) if tape else 0
        return out

    def set_trajectories(self, traj_pos=None, traj_vel=None, traj_alpha=None):
        """New values for the tracks, of the shapes given at construction (vsmpc_rollout_set_trajectories); None keeps a
        track.  The tape is gone afterwards; call reset() before the next run."""
        pos = None if traj_pos is None else np.ascontiguousarray(traj_pos, dtype=np.float64)
        vel = None if traj_vel is None else np.ascontiguousarray(traj_vel, dtype=np.float64)
        alpha = None if traj_alpha is None else np.ascontiguousarray(traj_alpha, dtype=np.float64)
        for t in (pos, vel):
            if t is not None and t.shape != (self.n_traj, 3):
                raise ValueError(f"traj_pos / traj_vel must be [{self.n_traj}, 3]")
        if alpha is not None and alpha.shape != (self.n_alpha,):
            raise ValueError(f"traj_alpha must be [{self.n_alpha}]")
        self._taped = 0
        _lib.check(self.lib.vsmpc_rollout_set_trajectories(self._r, _ptr(pos), _ptr(vel), _ptr(alpha)),
                   "vsmpc_rollout_set_trajectories")

    @property
    def traj_grad_size(self) -> int:
        """doubles in one row of grad_traj: 6 n_traj + n_alpha (L.traj_grad_blocks names its three blocks)"""
        return int(self.lib.vsmpc_rollout_traj_grad_size(self._r))

    @property
    def att_grad_size(self) -> int:
        """doubles in one row of grad_att: 6 n_traj (L.att_grad_blocks names its two blocks)"""
        return int(self.lib.vsmpc_rollout_att_grad_size(self._r))

    def backward(self, log_bar=None, state_bar=None, params: bool = False, traj: bool = False, att: bool = False) -> dict:
        """vsmpc_rollout_backward over the last run(ticks, tape=True): the gradient of a loss on the flown trajectory, given
        as log_bar [ticks, batch, ROLLOUT_LOG] = dL/d(log rows) (columns 14, 15 ignored) and / or state_bar [batch,
        PLANT_STATE] = dL/d(final plant state).  Returns grad_state0 [batch, PLANT_STATE] (dL/d the plant state at the start
        of that run, entries 0..39), grad_gains [batch, L.GRAD_SIZE] (field values in L.GRAD_* order, summed over the ticks;
        per loop under its own row with set_tunables) and flags [batch] (OR over the ticks of L.ADJ_*).  Needs adjoint=True.
        params / traj (vsmpc_rollout_backward_full): also grad_params [batch, PLANT_PARAMS] (L.PP_* order; the structural
        entries are zero) and / or grad_traj_pos, grad_traj_vel [batch, n_traj, 3] and grad_traj_alpha [batch, n_alpha], each
        per loop: the tracks are shared, their gradient is the sum over the loops.
        att (vsmpc_rollout_backward_attitude; needs set_attitude_tracks(.., adjoint=True)): also grad_traj_rpy and
        grad_traj_rpy_dot [batch, n_traj, 3], per loop like the other tracks."""
        ticks = getattr(self, "_taped", 0)
        lb = None if log_bar is None else np.ascontiguousarray(log_bar, dtype=np.float64)
        sb = None if state_bar is None else np.ascontiguousarray(state_bar, dtype=np.float64)
        if lb is not None and lb.shape != (ticks, self.batch, L.ROLLOUT_LOG):
            raise ValueError(f"log_bar must be [{ticks}, {self.batch}, {L.ROLLOUT_LOG}], the log of the taped run")
        if sb is not None and sb.shape != (self.batch, L.PLANT_STATE):
            raise ValueError(f"state_bar must be [{self.batch}, {L.PLANT_STATE}]")
        out = {"grad_state0": np.empty((self.batch, L.PLANT_STATE)), "grad_gains": np.empty((self.batch, L.GRAD_SIZE)),
               "flags": np.empty(self.batch, dtype=np.int32)}
        if not params and not traj and not att:
            _lib.check(self.lib.vsmpc_rollout_backward(self._r, _ptr(lb), _ptr(sb), _ptr(out["grad_state0"]),
                                                       _ptr(out["grad_gains"]), _ptr(out["flags"]), None), "vsmpc_rollout_backward")
            return out
        gp = np.empty((self.batch, L.PLANT_PARAMS)) if params else None
        gt = np.empty((self.batch, self.traj_grad_size)) if traj else None
        if att:
            ga = np.empty((self.batch, 6 * self.n_traj))
            _lib.check(self.lib.vsmpc_rollout_backward_attitude(self._r, _ptr(lb), _ptr(sb), _ptr(out["grad_state0"]),
                                                                _ptr(out["grad_gains"]), _ptr(gp), _ptr(gt), _ptr(ga),
                                                                _ptr(out["flags"]), None), "vsmpc_rollout_backward_attitude")
            for name, (off, n, shape) in L.att_grad_blocks(self.n_traj).items():
                out["grad_traj_" + name] = ga[:, off:off + n].reshape((self.batch,) + shape).copy()
        else:
            _lib.check(self.lib.vsmpc_rollout_backward_full(self._r, _ptr(lb), _ptr(sb), _ptr(out["grad_state0"]),
                                                            _ptr(out["grad_gains"]), _ptr(gp), _ptr(gt), _ptr(out["flags"]), None),
                       "vsmpc_rollout_backward_full")
        if params:
            out["grad_params"] = gp
        if traj:
            for name, (off, n, shape) in L.traj_grad_blocks(self.n_traj, self.n_alpha).items():
                out["grad_traj_" + name] = gt[:, off:off + n].reshape((self.batch,) + shape).copy()
        return out

    def backward_device(self, d_log_bar, d_state_bar, d_grad_state0, d_grad_gains, d_flags, stream=None, d_grad_params=None,
                        d_grad_traj=None, d_grad_att=None):
        """vsmpc_rollout_backward_device: backward() on contiguous CUDA tensors (None: not given / not wanted); only enqueues,
        on `stream` or torch's current stream.  d_grad_params [batch, PLANT_PARAMS] and / or d_grad_traj [batch,
        traj_grad_size] given: vsmpc_rollout_backward_full_device; d_grad_att [batch, att_grad_size] given:
        vsmpc_rollout_backward_attitude_device."""
        from .solver import _assert_f64_device, _dptr, _stream
        _assert_f64_device(d_log_bar, d_state_bar, d_grad_state0, d_grad_gains, d_grad_params, d_grad_traj, d_grad_att)
        ref_t = d_log_bar if d_log_bar is not None else d_state_bar
        if d_grad_params is None and d_grad_traj is None and d_grad_att is None:
            _lib.check(self.lib.vsmpc_rollout_backward_device(self._r, _dptr(d_log_bar), _dptr(d_state_bar), _dptr(d_grad_state0),
                                                              _dptr(d_grad_gains), _dptr(d_flags), _stream(ref_t, stream)),
                       "vsmpc_rollout_backward_device")
            return
        if d_grad_params is not None and tuple(d_grad_params.shape) != (self.batch, L.PLANT_PARAMS):
            raise ValueError(f"d_grad_params must be [{self.batch}, {L.PLANT_PARAMS}]")
        if d_grad_traj is not None and tuple(d_grad_traj.shape) != (self.batch, self.traj_grad_size):
            raise ValueError(f"d_grad_traj must be [{self.batch}, {self.traj_grad_size}] (6 n_traj + n_alpha)")
        if d_grad_att is not None:
            if tuple(d_grad_att.shape) != (self.batch, 6 * self.n_traj):
                raise ValueError(f"d_grad_att must be [{self.batch}, {6 * self.n_traj}] (6 n_traj)")
            _lib.check(self.lib.vsmpc_rollout_backward_attitude_device(
                self._r, _dptr(d_log_bar), _dptr(d_state_bar), _dptr(d_grad_state0), _dptr(d_grad_gains), _dptr(d_grad_params),
                _dptr(d_grad_traj), _dptr(d_grad_att), _dptr(d_flags), _stream(ref_t, stream)),
                "vsmpc_rollout_backward_attitude_device")
            return
        _lib.check(self.lib.vsmpc_rollout_backward_full_device(self._r, _dptr(d_log_bar), _dptr(d_state_bar), _dptr(d_grad_state0),
                                                               _dptr(d_grad_gains), _dptr(d_grad_params), _dptr(d_grad_traj),
                                                               _dptr(d_flags), _stream(ref_t, stream)),
                   "vsmpc_rollout_backward_full_device")

    def state(self) -> np.ndarray:
        out = np.empty((self.batch, L.PLANT_STATE))
        _lib.check(self.lib.vsmpc_rollout_get_state(self._r, _ptr(out)), "vsmpc_rollout_get_state")
        return out

    def next_records(self) -> np.ndarray:
        """Records the next tick will solve (after reset: tick 0; after run(k): tick k)."""
        out = np.empty((self.batch, self.cfg.n_in))
        _lib.check(self.lib.vsmpc_rollout_get_records(self._r, _ptr(out)), "vsmpc_rollout_get_records")
        return out
