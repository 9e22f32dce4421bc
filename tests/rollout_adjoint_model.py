"""Adjoint of the closed-loop rollout in numpy: the gradient of a scalar loss on the flown trajectory -- a linear functional
of the log rows plus one of the final plant state -- with respect to the plant state at the start of the run and to the
gains, for tests/test_rollout_adjoint_model.py and tests/test_gpu_rollout_adjoint.py.  Mirror of vsmpc_rollout_backward
(csrc/vsmpc_rollout_adjoint.hip + the record adjoint between its launches).

  forward      the loop model: tick_model.ReferenceTickModel builds the records, adjoint_model's condensed route solves
               them, rollout_model.advance flies the plant.  Keeps the tape (s_t, record, first move, status).
  backward     the sweep, last tick to first: transpose of rollout_model.advance (plant_adjoint), the solve's record adjoint
               (adjoint_record_model.condensed_record_adjoint, adjoint_model.condensed_adjoint for the gains), transpose of
               the record assembly and of the window FIFO (record_adjoint).  Written from the formulas, not from `forward`.
  central      central differences of `forward` itself, Richardson extrapolated, along given directions.

The three imported models are not changed.  `mutation` (one of MUTATIONS) plants one defect, for the mutation tests only.
"""
from __future__ import annotations

import dataclasses
import math

import numpy as np

import adjoint_model as am
import adjoint_record_model as arm
import rollout_model as pm
import runtime_model as rm
import sensitivity_model as sm
import tick_model
import vsmpc_ref as ref

L = pm.L
NS = 40                      # live entries of the plant state (the jet-plant slots behind them carry no gradient)
GRAV = 9.81
MUTATIONS = ("window_late", "release_off_by_one", "drop_dv_du", "drop_amom_qbar", "unsolved_as_solved")
# what tests/rollout_adjoint_edge_cases.py is there to catch, one line of the sweep each (kept apart from MUTATIONS, which
# test_rollout_adjoint_model.py requires the four loops of rollout_adjoint_cases.py to catch: they let most of these through)
EDGE_MUTATIONS = (
    "drot_sign",            # d R[1][0] / d pitch = -sy sp, second order at rpy = 0, with the wrong sign
    "drop_winv_pitch",      # the pitch derivative of W^-1(rpy) is dropped
    "inertia_half",         # I_G = R I_B R^T pulled back through dR I_B R^T alone, without R I_B dR^T
    "alpha_per_tick",       # alpha-gravity sampled at the tick's start for every sub-step
    "dist_per_tick",        # the disturbance window tested at the tick's start for every sub-step
    "push_unclamped",       # the pushed column's trajectory sample is not clamped at the end of the track
    "first_clamp_early",    # the `first` fill clamps one sample early
    "h_1ms",                # the sub-step is 1 ms whatever period_mpc / substeps is
    "limits_last_tick",     # grad_cfg's throttle limits are the last tick's, not the sum over the ticks
    "shift_first_chunk")    # the window cotangent shifts back 12 entries within its first 64 entries only
_JET = pm._JET


# (field, offset, length) of the live plant state: VSMPC_PS_*
STATE_FIELDS = (("P", 0, 3), ("HLIN", 3, 3), ("RPY", 6, 3), ("HANG", 9, 3), ("T", 12, 4), ("TD", 16, 4), ("Q", 20, 8), ("U", 28, 4),
                ("TDES", 32, 4), ("TDDES", 36, 4))


field_errors = arm.worst_field   # (got, want, fields, bar, floor) on the fields of a plant-state or a gains gradient


def with_gains(cfg, row):
    """`cfg` with its tunable fields replaced by one row of field values in VSMPC_GRAD_* order"""
    kw = {name: (float(row[off]) if n == 1 else tuple(float(v) for v in row[off:off + n])) for name, off, n in am.GRAD_FIELDS}
    return dataclasses.replace(cfg, **kw)


def gains_of(cfg):
    row = np.zeros(am.GRAD_SIZE)
    for name, off, n in am.GRAD_FIELDS:
        row[off:off + n] = getattr(cfg, name)
    return row


# ----------------------------------------------------------------------------------------------------------------------
# forward loop
# ----------------------------------------------------------------------------------------------------------------------
def solve_tick(cfg, rec):
    """(first move [24], status) of one record: the condensed route of adjoint_model.condensed_adjoint up to the solution"""
    N, HC, nvb = cfg.n_iter, cfg.control_horizon, cfg.n_vblocks
    NX, NJ, NTH = am.NX, am.NJ, am.NTH
    nu, nv = NJ * HC, NTH * nvb
    nz = nu + nv
    try:
        M, S, s, gmax, vprev, (A, Bj, Bt, c, dts) = am._schur(cfg, rec)
    except FloatingPointError:
        return np.zeros(L.FM_SIZE), L.STATUS_NUMERICAL
    if not np.isfinite(M).all():
        return np.zeros(L.FM_SIZE), L.STATUS_NUMERICAL
    vmin, vmax = ref.throttle_bounds(cfg)
    fixed = np.zeros(nv, dtype=bool)
    lo, hi = np.full(nv, vmin), np.full(nv, vmax)
    if rec[ref.IN_HOLD] != 0.0:
        fixed[:NTH] = True
        lo[:NTH] = hi[:NTH] = vprev
    v, status, _ = rm.box_qp(S, s, lo, hi, fixed, 1e-10 * (1.0 + gmax))
    if status != rm.SOLVED:
        return np.zeros(L.FM_SIZE), int(status)
    Ljj, Lvj = np.tril(M[:nu, :nu]), M[nu:nz, :nu]
    u = np.linalg.solve(Ljj.T, -(Lvj.T @ v + M[nz, :nu]))
    X1 = rec[ref.IN_X0:ref.IN_X0 + NX] + dts[0] * (A @ rec[ref.IN_X0:ref.IN_X0 + NX] + Bj @ u[:NJ] + Bt @ v[:NTH] + c)
    fm = np.concatenate([u[:NJ], v[:NTH], ref.destd_throttle(v[:NTH]), X1[12:16], X1[16:20]])
    return fm, L.STATUS_SOLVED


def substeps_of(cfg):
    """the plant's sub-steps per tick as vsmpc_rollout_create derives them: 1 ms each, at least 1 and at most 16 of them
    (min(16, max(1, lround(period_mpc / 1 ms))); beyond 16 ms the sub-step is period_mpc / 16)"""
    return min(16, max(1, int(math.floor(cfg.period_mpc / 1e-3 + 0.5))))


def forward(cfg, s0, p, traj, ticks, substeps=None, unsolved_ticks=()):
    """One instance: (log [ticks, 16], final state, tape).  traj = (pos, vel, alpha, alpha_dt).  `unsolved_ticks`: ticks whose
    solve is reported as STATUS_MAX_ITER whatever it found, so that the move is not consumed (model tests only)."""
    pos, vel, alpha, alpha_dt = traj
    substeps = substeps_of(cfg) if substeps is None else substeps
    model = tick_model.ReferenceTickModel(cfg, s0, p, pos, vel, alpha, fps_traj=int(round(1.0 / cfg.period_large)),
                                          fps_alpha=int(round(1.0 / alpha_dt)), ticks_before=int(p[L.PP_TICK0]),
                                          configured_elsewhere=True)
    s = np.array(s0, dtype=float)
    log = np.zeros((ticks, L.ROLLOUT_LOG))
    tape = []
    for t in range(ticks):
        rec = tick_model.record_from_tick(cfg, model.update(s), pm.kin_record(cfg, s, p))
        fm, status = solve_tick(cfg, rec)
        if t in unsolved_ticks:
            status = L.STATUS_MAX_ITER
        model.consume(fm, status)
        tape.append((s.copy(), rec, fm, status))
        s = pm.advance(cfg, s, p, t, fm, status, alpha, alpha_dt, substeps)
        log[t, 0:3], log[t, 3:6] = s[L.PS_P:L.PS_P + 3], s[L.PS_RPY:L.PS_RPY + 3]
        log[t, 6:10], log[t, 10:14], log[t, 14] = s[L.PS_T:L.PS_T + 4], s[L.PS_U:L.PS_U + 4], status
    return log, s, tape


def loss(log, final, log_bar, state_bar):
    return float((log_bar[:, :14] * log[:, :14]).sum() + state_bar[:NS] @ final[:NS])


# ----------------------------------------------------------------------------------------------------------------------
# the three transposes
# ----------------------------------------------------------------------------------------------------------------------
def drot(rpy, mutation=None):
    """R(rpy) of rollout_model.rot and its partials to roll, pitch, yaw"""
    r, p, y = rpy
    cr, sr, cp, sp, cy, sy = math.cos(r), math.sin(r), math.cos(p), math.sin(p), math.cos(y), math.sin(y)
    dr = np.array([[0.0, cy * sp * cr + sy * sr, -cy * sp * sr + sy * cr],
                   [0.0, sy * sp * cr - cy * sr, -sy * sp * sr - cy * cr],
                   [0.0, cp * cr, -cp * sr]])
    dp = np.array([[-cy * sp, cy * cp * sr, cy * cp * cr],
                   [-sy * sp, sy * cp * sr, sy * cp * cr],
                   [-cp, -sp * sr, -sp * cr]])
    if mutation == "drot_sign":
        dp[1, 0] = sy * sp
    dy = np.array([[-sy * cp, -sy * sp * sr - cy * cr, -sy * sp * cr + cy * sr],
                   [cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr],
                   [0.0, 0.0, 0.0]])
    return pm.rot(rpy), (dr, dp, dy)


def _dv_du(u):
    """derivative of Jet::v_of_throttle"""
    return am.dv_dthrottle(u)


def plant_adjoint(cfg, s, p, tick, fm, status, alpha_track, alpha_dt, sbar_next, substeps=None, mutation=None, trace=None):
    """Transpose of rollout_model.advance at (s, fm, status): sbar_next [40] = dL/d s_{t+1} -> (direct part of dL/d s_t [40],
    fmbar [24]).  The sub-steps are recomputed and kept, then run backwards.  This is the only copy of that recursion: `trace`
    (a dict, or None) receives what a caller builds further shares of the sub-steps from (rollout_param_adjoint_model) --
    "steps": one (x, lam, R, dR, om, ombar, alpha, dist, t) per sub-step, in the order the recursion takes them (the last
    sub-step first), lam the cotangent behind the sub-step; "h", "Abar" [6, 4], and "q", "DJ": the joints after the move and
    d A_mom / dq there."""
    substeps = substeps_of(cfg) if substeps is None else substeps
    solved = status == L.STATUS_SOLVED or mutation == "unsolved_as_solved"
    s = np.array(s, dtype=float)
    if status == L.STATUS_SOLVED:                              # (the forward pass is never mutated)
        s[L.PS_Q:L.PS_Q + 8] += fm[L.FM_DQ:L.FM_DQ + 8]
        s[L.PS_U:L.PS_U + 4] = fm[L.FM_THROTTLE:L.FM_THROTTLE + 4]
    tk = tick + int(p[L.PP_TICK0])
    m = p[L.PP_MASS]
    IB = p[L.PP_INERTIA_B:L.PP_INERTIA_B + 9].reshape(3, 3)
    IBi = np.linalg.inv(IB)
    A, DJ = pm.amom_of_q(s, p)
    u = s[L.PS_U:L.PS_U + 4]
    vthr = np.array([_JET.compute_v(_JET.standardizeThrottle_u2T(v)) for v in u])
    co, (muT, sgT, _, _) = ref.JET_COEFF, ref.JET_NORM
    h = 1e-3 if mutation == "h_1ms" else cfg.period_mpc / substeps
    xs, x = [], s[0:20].copy()
    for ss in range(substeps):                                 # the forward sub-steps, as rollout_model.advance takes them
        xs.append(x.copy())
        x = pm.substep(cfg, x, p, tk, ss, substeps, A, IB, vthr, alpha_track, alpha_dt)
    lam = np.array(sbar_next[0:20], dtype=float)
    Abar, vbar, steps = np.zeros((6, 4)), np.zeros(4), []
    for ss in range(substeps - 1, -1, -1):
        x = xs[ss]
        t = (tk + ss / substeps) * cfg.period_mpc
        t_tick = tk * cfg.period_mpc
        alpha = pm.interp_clamped(alpha_track, (t_tick if mutation == "alpha_per_tick" else t) / alpha_dt)
        dist = p[L.PP_DIST_T0] <= (t_tick if mutation == "dist_per_tick" else t) < p[L.PP_DIST_T1]
        R, dR = drot(x[6:9], mutation)
        om = IBi @ x[9:12]
        lp, ll, lr, la = lam[0:3], lam[3:6], lam[6:9], lam[9:12]
        hl, ha, T = x[3:6], x[9:12], x[12:16]
        sr, cr, sp, cp = math.sin(x[6]), math.cos(x[6]), math.sin(x[7]), math.cos(x[7])
        tp = sp / cp
        E = np.array([[1.0, sr * tp, cr * tp], [0.0, cr, -sr], [0.0, sr / cp, cr / cp]])
        dEr = np.array([[0.0, cr * tp, -sr * tp], [0.0, -sr, -cr], [0.0, cr / cp, -sr / cp]])
        dEp = np.array([[0.0, sr / cp ** 2, cr / cp ** 2], [0.0, 0.0, 0.0], [0.0, sr * tp / cp, cr * tp / cp]])
        ombar = np.cross(ll, hl) + np.cross(la, ha) + E.T @ lr
        steps.append((x, lam, R, dR, om, ombar, alpha, dist, t))
        fw = alpha * m * np.array([0.0, 0.0, -GRAV])           # world-frame force that enters through R^T
        if dist:
            fw = fw + p[L.PP_DIST_F:L.PP_DIST_F + 3]
        g = np.zeros(20)
        g[3:6] = R.T @ lp / m + np.cross(om, ll)
        g[9:12] = np.cross(om, la) + IBi.T @ ombar
        for a in range(3):
            g[6 + a] = lp @ (dR[a] @ hl) / m + (dR[a] @ ll) @ fw
        g[6] += lr @ (dEr @ om)
        if mutation != "drop_winv_pitch":
            g[7] += lr @ (dEp @ om)
        g[12:16] = A[0:3].T @ ll + A[3:6].T @ la
        for j in range(4):
            Tb, Tdb = (x[12 + j] - muT) / sgT, x[16 + j] / sgT
            dfT, dfTd = co[1] + co[3] * Tdb + 2 * co[4] * Tb, co[2] + co[3] * Tb + 2 * co[5] * Tdb
            dgT, dgTd = co[7] + co[9] * Tdb + 2 * co[10] * Tb, co[8] + co[9] * Tb + 2 * co[11] * Tdb
            g[12 + j] += lam[16 + j] * (dfT + dgT * vthr[j])
            g[16 + j] = lam[12 + j] + lam[16 + j] * (dfTd + dgTd * vthr[j])
            vbar[j] += h * lam[16 + j] * sgT * _JET.compute_g(Tb, Tdb)
        Abar[0:3] += h * np.outer(ll, T)
        Abar[3:6] += h * np.outer(la, T)
        lam = lam + h * g
    if trace is not None:
        trace.update(steps=steps, h=h, Abar=Abar, q=s[L.PS_Q:L.PS_Q + 8], DJ=DJ)
    qbar = np.array(sbar_next[L.PS_Q:L.PS_Q + 8], dtype=float)
    if mutation != "drop_amom_qbar":
        qbar += np.einsum("jrc,rc->j", DJ, Abar)
    ubar = sbar_next[L.PS_U:L.PS_U + 4] + vbar * (1.0 if mutation == "drop_dv_du" else _dv_du(u))
    out, fmbar = np.zeros(NS), np.zeros(L.FM_SIZE)
    out[0:20] = lam
    out[L.PS_Q:L.PS_Q + 8] = qbar
    if solved:
        fmbar[L.FM_DQ:L.FM_DQ + 8] = qbar
        fmbar[L.FM_THROTTLE:L.FM_THROTTLE + 4] = ubar
        fmbar[L.FM_THRUST:L.FM_THRUST + 4] = sbar_next[L.PS_TDES:L.PS_TDES + 4]
        fmbar[L.FM_THRUSTDOT:L.FM_THRUSTDOT + 4] = sbar_next[L.PS_TDDES:L.PS_TDDES + 4]
    else:
        out[L.PS_U:L.PS_U + 4] = ubar
        out[L.PS_TDES:L.PS_TDES + 4] = sbar_next[L.PS_TDES:L.PS_TDES + 4]
        out[L.PS_TDDES:L.PS_TDDES + 4] = sbar_next[L.PS_TDDES:L.PS_TDDES + 4]
    return out, fmbar


def _sample(cfg, n_traj, idx):
    return min(max(idx, 0), n_traj - 1)


def record_adjoint(cfg, s, p, tk, first, traj_vel, gin, sbar, wbar, mutation=None):
    """Transpose of the record assembly of tick tk (vsmpc_rollout.hip: assemble_record) at plant state s: adds the pull-back
    of gin [n_in] to sbar [40] in place and returns the window cotangent in front of this tick's update.  wbar [n_ref, 12] is
    the cotangent of the window this tick's record read, as later ticks left it."""
    nref, ratio = cfg.n_ref_cols, cfg.ratio
    m = p[L.PP_MASS]
    IB = p[L.PP_INERTIA_B:L.PP_INERTIA_B + 9].reshape(3, 3)
    IBi = np.linalg.inv(IB)
    DJ = p[L.PP_DJ:L.PP_DJ + 192].reshape(8, 6, 4)
    R, dR = drot(s[L.PS_RPY:L.PS_RPY + 3], mutation)
    w = wbar + gin[ref.IN_XREF:ref.IN_XREF + 12 * nref].reshape(nref, 12)
    x0b = gin[ref.IN_X0:ref.IN_X0 + 26]
    sbar[0:20] += x0b[0:20]                                    # X0: identity (the unwrapped RPY has derivative 1)
    sbar[0:3] += x0b[20:23]                                    # errors against column 0 of the window
    sbar[6:9] += x0b[23:26]
    w[0, 0:3] += gin[ref.IN_PREF:ref.IN_PREF + 3] - x0b[20:23]
    w[0, 6:9] -= x0b[23:26]
    Gw = gin[ref.IN_WRB:ref.IN_WRB + 9].reshape(3, 3)
    Gi = gin[ref.IN_INERTIA:ref.IN_INERTIA + 9].reshape(3, 3)
    for a in range(3):
        partner = 0.0 if mutation == "inertia_half" else R @ IB @ dR[a].T
        sbar[6 + a] += (Gw * dR[a]).sum() + (Gi * (dR[a] @ IB @ R.T + partner)).sum()
    sbar[6:9] += gin[ref.IN_RPY:ref.IN_RPY + 3]
    sbar[9:12] += IBi.T @ gin[ref.IN_OMEGA:ref.IN_OMEGA + 3]
    sbar[L.PS_Q:L.PS_Q + 8] += np.einsum("jl,l->j", DJ.reshape(8, 24), gin[ref.IN_AMOM:ref.IN_AMOM + 24]) \
        + gin[ref.IN_QERR:ref.IN_QERR + 8]
    GL = np.vstack([gin[ref.IN_LLIN:ref.IN_LLIN + 24].reshape(3, 8), gin[ref.IN_LANG:ref.IN_LANG + 24].reshape(3, 8)])   # [row][j]
    sbar[L.PS_T:L.PS_T + 4] += np.einsum("jrc,rj->c", DJ, GL) + gin[ref.IN_T0:ref.IN_T0 + 4]
    sbar[L.PS_TD:L.PS_TD + 4] += gin[ref.IN_TD0:ref.IN_TD0 + 4]
    sbar[L.PS_U:L.PS_U + 4] += gin[ref.IN_UPREV:ref.IN_UPREV + 4]
    sbar[L.PS_TDES:L.PS_TDES + 4] += gin[ref.IN_TDES:ref.IN_TDES + 4]
    sbar[L.PS_TDDES:L.PS_TDDES + 4] += gin[ref.IN_TDDES:ref.IN_TDDES + 4]
    # the window FIFO: a release tick pushed a column whose h_lin entry is R^T m v_ref at this tick's R
    n_traj = len(traj_vel)
    release = ((tk + 1) % ratio == ratio - 1) if mutation == "release_off_by_one" else (tk % ratio == ratio - 1)
    if release:
        idx = 1 + (tk + 1) // ratio
        if mutation == "push_unclamped" and idx >= n_traj:     # reads behind the track: whatever lies there, zeros here
            v = np.zeros(3)
        else:
            v = traj_vel[_sample(cfg, n_traj, idx)]
        pushed = nref - 2 if mutation == "window_late" and nref > 1 else nref - 1
        for a in range(3):
            sbar[6 + a] += (dR[a] @ w[pushed, 3:6]) @ (m * v)
        prev = np.zeros_like(w)
        prev[1:] = w[:-1]
        if mutation == "shift_first_chunk":                    # entries 64 .. stay where they were
            prev.reshape(-1)[64:] = w.reshape(-1)[64:]
        w = prev
    if first:                                                  # every column was frozen with the R of this tick
        ns0 = 1 + tk // ratio
        for j in range(nref):
            v = traj_vel[_sample(cfg, n_traj - 1 if mutation == "first_clamp_early" and n_traj > 1 else n_traj,
                                 ns0 - (nref - 1 - j))]
            for a in range(3):
                sbar[6 + a] += (dR[a] @ w[j, 3:6]) @ (m * v)
        w = np.zeros_like(w)
    return w


# ----------------------------------------------------------------------------------------------------------------------
# the sweep
# ----------------------------------------------------------------------------------------------------------------------
def backward(cfg, tape, p, traj, log_bar, state_bar, substeps=None, first=True, tick_base=0, mutation=None):
    """One instance: grad_state0 [40], grad_cfg [32], flags, the per-tick flags and the per-tick states of the QP's throttles
    (sensitivity_model.FREE / LOWER / UPPER / pinned; None for a tick that is not Solved) with the throttles themselves and
    their limits.  tape = forward()'s; log_bar [ticks, 16] (columns 14, 15 ignored) or None, state_bar [>= 40] or None."""
    substeps = substeps_of(cfg) if substeps is None else substeps
    _, vel, alpha, alpha_dt = traj
    ticks = len(tape)
    sbar = np.zeros(NS) if state_bar is None else np.array(state_bar[:NS], dtype=float)
    wbar = np.zeros((cfg.n_ref_cols, 12))
    gcfg, flags, tick_flags, tick_active, tick_v = np.zeros(am.GRAD_SIZE), 0, [], [], []
    xbar0 = np.zeros(cfg.n_var)
    for t in range(ticks - 1, -1, -1):
        s, rec, fm, status = tape[t]
        if log_bar is not None:
            sbar[0:3] += log_bar[t, 0:3]
            sbar[6:9] += log_bar[t, 3:6]
            sbar[12:16] += log_bar[t, 6:10]
            sbar[L.PS_U:L.PS_U + 4] += log_bar[t, 10:14]
        sbar, fmbar = plant_adjoint(cfg, s, p, tick_base + t, fm, status, alpha, alpha_dt, sbar, substeps, mutation)
        if status == L.STATUS_SOLVED:
            adj = am.condensed_adjoint(cfg, rec, xbar0, fmbar)
            gin = arm.condensed_record_adjoint(cfg, rec, xbar0, fmbar)["grad_in"]
            gt = adj["grad_cfg"].copy()
            if mutation == "limits_last_tick" and t != ticks - 1:
                gt[29:31] = 0.0
            gcfg += gt
            f = int(adj["flags"])
            tick_active.append(adj["active"])
            tick_v.append(adj["x"][cfg.off_throttle:])
        else:
            gin, f = np.zeros(cfg.n_in), am.UNSOLVED
            tick_active.append(None)
            tick_v.append(None)
        flags |= f
        tick_flags.append(f)
        wbar = record_adjoint(cfg, s, p, tick_base + t + int(p[L.PP_TICK0]), first and tick_base + t == 0, vel, gin, sbar, wbar,
                              mutation)
    return {"grad_state0": sbar, "grad_cfg": gcfg, "flags": flags, "tick_flags": tick_flags[::-1],
            "tick_active": tick_active[::-1], "tick_v": tick_v[::-1]}


# ----------------------------------------------------------------------------------------------------------------------
# central differences of the forward loop
# ----------------------------------------------------------------------------------------------------------------------
def central(cfg, s0, p, traj, ticks, log_bar, state_bar, d_state=None, d_gains=None, step=1e-4, substeps=None,
            unsolved_ticks=(), richardson=True):
    """Directional derivative of the loss of `forward` along (d_state [40], d_gains [32]) (either may be None): central
    differences with the step `step`, Richardson extrapolated with step / 2 (O(h^4))."""
    g0 = gains_of(cfg)

    def at(e):
        s = np.array(s0, dtype=float)
        c = cfg
        if d_state is not None:
            s[:NS] += e * np.asarray(d_state)
        if d_gains is not None:
            c = with_gains(cfg, g0 + e * np.asarray(d_gains))
        log, fin, _ = forward(c, s, p, traj, ticks, substeps, unsolved_ticks)
        return loss(log, fin, log_bar, state_bar)

    def quotient(h):
        return (at(h) - at(-h)) / (2.0 * h)

    q = quotient(step)
    return (4.0 * quotient(0.5 * step) - q) / 3.0 if richardson else q


def state_scale():
    """step scale of every live state entry for the difference quotients: positions [m], momenta, angles [rad], thrusts [N],
    thrust rates, joints [rad], throttle [%], thrust references"""
    sc = np.ones(NS)
    sc[0:3], sc[3:6], sc[6:9], sc[9:12] = 1e-2, 1e-1, 1e-2, 1e-2
    sc[12:16], sc[16:20], sc[20:28], sc[28:32], sc[32:36], sc[36:40] = 1.0, 1.0, 1e-2, 1.0, 1.0, 1.0
    return sc
