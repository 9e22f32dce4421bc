"""Adjoint of the closed-loop rollout in numpy, the part behind rollout_param_adjoint_model.py and
rollout_tree_adjoint_model.py: a rollout whose reference carries an RPY and an RPYDot track, and the gradient of the same loss
with respect to both tracks, for tests/test_rollout_attitude_adjoint_model.py and tests/test_gpu_rollout_attitude_adjoint.py.
Mirror of vsmpc_rollout_backward_attitude (the ATT instantiations of advance_adjoint_body,
csrc/vsmpc_rollout_adjoint_device.hpp).

  forward      rollout_adjoint_model.forward with the two attitude tracks handed to tick_model.ReferenceTickModel (which has
               taken them all along).  On the tree plant the locked inertia the window columns are frozen with is the tree's
               I_B(q) of the tick that pushes them, as the device has it, not the parameter block.
  backward     the sweep of rollout_param_adjoint_model.backward (tree: of rollout_tree_adjoint_model.backward), whose
               transposes are imported and not changed, with one pull-back added at the record half of a tick
               (record_att_adjoint): rows 6..11 of a window column at the moment its cotangent is complete -- the pushed
               column at a release tick, every column at the `first` fill.  Written from the formulas:

                   rows 6..8   RPYINIT + rpy[idx]                  their cotangent goes to sample idx of the RPY track
                   rows 9..11  h = R y, y = I_B v, v = R^T u, u = W(roll, pitch) d, d = rpy_dot[idx]; with their cotangent w
                               ybar = R^T w, vbar = I_B^T ybar, ubar = R vbar
                               dbar = W^T ubar                     to sample idx of the RPYDot track
                               I_B_bar = ybar v^T                  to INERTIA_B, or on the tree through J to the joints
                               Rbar = w y^T + u vbar^T             rpy_a += <dR_a, Rbar>
                               roll += ubar . (dW/droll d), pitch += ubar . (dW/dpitch d)

  central      central differences of `forward`, Richardson extrapolated, along directions of both attitude tracks; for a run
               that does not begin at a reset the tracks are perturbed from the first taped tick on, the window the earlier
               ticks built held fixed (the derivative the sweep defines there).

`mutation` (one of MUTATIONS) plants one defect, for the mutation tests only."""
from __future__ import annotations

import math

import numpy as np

import adjoint_model as am
import adjoint_record_model as arm
import rollout_adjoint_model as ram
import rollout_model as pm
import rollout_param_adjoint_model as rpm
import rollout_tree_adjoint_model as rtm
import tick_model
import tree_jacobian_model as tj
import vsmpc_ref as ref

L = pm.L
NS, NP = ram.NS, rpm.NP
MUTATIONS = (
    "drop_dw_droll",          # the roll derivative of W dropped
    "drop_dw_dpitch",         # the pitch derivative of W dropped
    "rbar_without_u_vbar",    # Rbar = w y^T alone: R^T in v = R^T u not differentiated
    "ib_bar_transposed",      # I_B_bar = v ybar^T
    "w_not_transposed",       # dbar = W ubar
    "fill_takes_push_sample",  # every column of the `first` fill is given the sample a push at that tick would take
    "rpy_share_push_only",    # the RPY track gets its share at the pushes, not at the `first` fill
    "shared_sample_once",     # of the columns of one tick that hold the same sample only the first is counted
    "tree_ib_not_through_j")  # tree plant: the h_ang entries' cotangent of I_B is not sent through J to the joints
TREE_MUTATIONS = ("tree_ib_not_through_j",)
# Step scales of the difference quotients [rad], [rad/s].  With the tests' STEP = 1e-2 the steps are 1e-3: 2 % and 0.7 % of the
# tracks' amplitudes (0.05, 0.15).  The tracks enter the records linearly and the loss is smooth in them, so the Richardson
# quotient's truncation error (O(h^4)) stays below its roundoff eps |L| / h, which at |L| ~ 1e3 .. 1e4 is 2e-10 .. 2e-9 here and
# ten times that at a step of 1e-4 -- more than the smallest gradients of the cases (the run that does not begin at a reset:
# 0.06) bear at rollout_param_adjoint_cases.FD_BAR.
ATT_SCALE = {"rpy": 1e-1, "rpy_dot": 1e-1}


def tracks_of(att, n_traj):
    """(rpy, rpy_dot) [n_traj, 3] of att = (rpy or None, rpy_dot or None): a missing track reads as zeros"""
    rpy, rpyd = att
    return (np.zeros((n_traj, 3)) if rpy is None else np.asarray(rpy, float),
            np.zeros((n_traj, 3)) if rpyd is None else np.asarray(rpyd, float))


# ----------------------------------------------------------------------------------------------------------------------
# forward loop
# ----------------------------------------------------------------------------------------------------------------------
def _tick_params(s, p):
    """the parameter record tick_model's Robot reads: on the tree plant its locked inertia is the tree's I_B(q)"""
    if pm._TREE is None:
        return p
    pl = np.array(p, dtype=float)
    pl[L.PP_INERTIA_B:L.PP_INERTIA_B + 9] = pm.inertia_body(s, p).reshape(-1)
    return pl


def forward(cfg, s0, p, traj, att, ticks, substeps=None, unsolved_ticks=(), switch=None):
    """rollout_adjoint_model.forward with the attitude tracks att = (rpy, rpy_dot) ([n_traj, 3] or None each): (log, final
    state, tape).  switch = (tick, att2): from that tick of the run on the window is fed from att2 (central, for a run that
    does not begin at a reset).  Under rollout_tree_adjoint_model.set_tree the plant is the tree's."""
    pos, vel, alpha, alpha_dt = traj
    substeps = ram.substeps_of(cfg) if substeps is None else substeps
    rpy, rpyd = tracks_of(att, len(pos))
    model = tick_model.ReferenceTickModel(cfg, s0, _tick_params(s0, p), pos, vel, alpha, fps_traj=int(round(1.0 / cfg.period_large)),
                                          fps_alpha=int(round(1.0 / alpha_dt)), ticks_before=int(p[L.PP_TICK0]),
                                          configured_elsewhere=True, traj_rpy=rpy, traj_rpy_dot=rpyd)
    s = np.array(s0, dtype=float)
    log = np.zeros((ticks, L.ROLLOUT_LOG))
    tape = []
    for t in range(ticks):
        if switch is not None and t == switch[0]:
            for name, track in zip(("RPY", "RPYDot"), tracks_of(switch[1], len(pos))):
                tr = model.cost.m_trajManager.trajectories_map[name]
                assert len(tr.values) == len(track)
                tr.values = [np.array(v, dtype=float) for v in track]
        model.p = _tick_params(s, p)
        rec = tick_model.record_from_tick(cfg, model.update(s), pm.kin_record(cfg, s, p))
        fm, status = ram.solve_tick(cfg, rec)
        if t in unsolved_ticks:
            status = L.STATUS_MAX_ITER
        model.consume(fm, status)
        tape.append((s.copy(), rec, fm, status))
        s = pm.advance(cfg, s, p, t, fm, status, alpha, alpha_dt, substeps)
        log[t, 0:3], log[t, 3:6] = s[L.PS_P:L.PS_P + 3], s[L.PS_RPY:L.PS_RPY + 3]
        log[t, 6:10], log[t, 10:14], log[t, 14] = s[L.PS_T:L.PS_T + 4], s[L.PS_U:L.PS_U + 4], status
    return log, s, tape


# ----------------------------------------------------------------------------------------------------------------------
# the pull-back of a window column's attitude rows
# ----------------------------------------------------------------------------------------------------------------------
def w_matrix(roll, pitch):
    """W(roll, pitch) of costsVSMPC.cpp:266-286 and its partials to roll and pitch"""
    sr, cr, sp, cp = math.sin(roll), math.cos(roll), math.sin(pitch), math.cos(pitch)
    W = np.array([[1.0, 0.0, -sp], [0.0, cr, cp * sr], [0.0, -sr, cr * cp]])
    dWr = np.array([[0.0, 0.0, 0.0], [0.0, -sr, cp * cr], [0.0, -cr, -sr * cp]])
    dWp = np.array([[0.0, 0.0, -cp], [0.0, 0.0, -sp * sr], [0.0, 0.0, -cr * sp]])
    return W, dWr, dWp


def hang_pullback(rpy, IB, w, d, mutation=None):
    """rows 9..11 of a column, h = R I_B R^T W d at the attitude rpy, with cotangent w: (dbar [3], the shares of roll, pitch,
    yaw [3], I_B_bar [3, 3])"""
    R, dR = ram.drot(rpy)
    W, dWr, dWp = w_matrix(rpy[0], rpy[1])
    u = W @ d
    v = R.T @ u
    y = IB @ v
    ybar = R.T @ w
    vbar = IB.T @ ybar
    ubar = R @ vbar
    ib_bar = np.outer(v, ybar) if mutation == "ib_bar_transposed" else np.outer(ybar, v)
    Rbar = np.outer(w, y)
    if mutation != "rbar_without_u_vbar":
        Rbar = Rbar + np.outer(u, vbar)
    dbar = (W if mutation == "w_not_transposed" else W.T) @ ubar
    share = np.array([(dR[a] * Rbar).sum() for a in range(3)])
    if mutation != "drop_dw_droll":
        share[0] += ubar @ (dWr @ d)
    if mutation != "drop_dw_dpitch":
        share[1] += ubar @ (dWp @ d)
    return dbar, share, ib_bar


def record_att_adjoint(cfg, s, IB, tk, first, att_tracks, gin, wbar, sbar, gib, grpy, grpyd, mutation=None):
    """The attitude rows' shares of the record assembly of tick tk at plant state s: added in place to sbar [40] (rpy), gib
    [3, 3] (the cotangent of the I_B the columns were frozen with), grpy and grpyd [n_traj, 3].  gin and wbar as
    rollout_param_adjoint_model.record_param_adjoint is given them; nothing else is touched."""
    _, rpyd = att_tracks
    nref, ratio, n_traj = cfg.n_ref_cols, cfg.ratio, len(rpyd)
    rpy_s = s[L.PS_RPY:L.PS_RPY + 3]
    x0b = gin[ref.IN_X0:ref.IN_X0 + 26]
    w = wbar + gin[ref.IN_XREF:ref.IN_XREF + 12 * nref].reshape(nref, 12)
    w[0, 6:9] -= x0b[23:26]
    seen = set()

    def column(cw, idx, rpy_share=True):
        dbar, share, ib_bar = hang_pullback(rpy_s, IB, cw[9:12], rpyd[idx], mutation)
        sbar[6:9] += share
        gib[:] += ib_bar
        if mutation == "shared_sample_once" and idx in seen:
            return
        seen.add(idx)
        if rpy_share:
            grpy[idx] += cw[6:9]
        grpyd[idx] += dbar

    if tk % ratio == ratio - 1:
        column(w[nref - 1], rpm.push_sample(cfg, n_traj, tk))
        prev = np.zeros_like(w)
        prev[1:] = w[:-1]
        w = prev
    if first:
        for j in range(nref):
            idx = rpm.push_sample(cfg, n_traj, tk) if mutation == "fill_takes_push_sample" else rpm.fill_sample(cfg, n_traj, tk, j)
            column(w[j], idx, rpy_share=mutation != "rpy_share_push_only")


# ----------------------------------------------------------------------------------------------------------------------
# the sweep
# ----------------------------------------------------------------------------------------------------------------------
def backward(cfg, tape, p, traj, att, log_bar, state_bar, substeps=None, first=True, tick_base=0, mutation=None, tree=None,
             selector=None):
    """One instance: rollout_param_adjoint_model.backward's outputs (tree given: rollout_tree_adjoint_model.backward's) and
    grad_traj_rpy, grad_traj_rpy_dot [n_traj, 3].  tape = forward()'s (tree: under rollout_tree_adjoint_model.set_tree)."""
    substeps = ram.substeps_of(cfg) if substeps is None else substeps
    pos, vel, alpha, alpha_dt = traj
    tracks = tracks_of(att, len(pos))
    ticks = len(tape)
    sbar = np.zeros(NS) if state_bar is None else np.array(state_bar[:NS], dtype=float)
    wbar = np.zeros((cfg.n_ref_cols, 12))
    gcfg, flags, tick_flags = np.zeros(am.GRAD_SIZE), 0, []
    gp, gpos, gvel, galpha = np.zeros(NP), np.zeros((len(pos), 3)), np.zeros((len(vel), 3)), np.zeros(len(alpha))
    grpy, grpyd = np.zeros((len(pos), 3)), np.zeros((len(pos), 3))
    xbar0 = np.zeros(cfg.n_var)
    keep = [e for name, o, n in rpm.PARAM_FIELDS if name not in ("INERTIA_B", "AMOM0", "DJ") for e in range(o, o + n)]
    for t in range(ticks - 1, -1, -1):
        s, rec, fm, status = tape[t]
        solved = status == L.STATUS_SOLVED
        if log_bar is not None:
            sbar[0:3] += log_bar[t, 0:3]
            sbar[6:9] += log_bar[t, 3:6]
            sbar[12:16] += log_bar[t, 6:10]
            sbar[L.PS_U:L.PS_U + 4] += log_bar[t, 10:14]
        # ---- plant half
        if tree is None:
            sbar, fmbar = rpm.plant_param_adjoint(cfg, s, p, tick_base + t, fm, status, alpha, alpha_dt, sbar, substeps, gp, galpha)
        else:                                                  # as rollout_tree_adjoint_model.backward
            q_next = s[L.PS_Q:L.PS_Q + 8] + (fm[L.FM_DQ:L.FM_DQ + 8] if solved else 0.0)
            tau, J = tj.jacobian(tree, q_next, s[L.PS_T:L.PS_T + 4], selector)
            gl = np.zeros(NP)
            with rtm._parametric():
                sbar, fmbar = rpm.plant_param_adjoint(cfg, s, rtm._local(p, tau), tick_base + t, fm, status, alpha, alpha_dt, sbar,
                                                      substeps, gl, galpha)
            gp[keep] += gl[keep]
            tbar = np.zeros(tj.TT_SIZE)
            tbar[tj.TT_AMOM:tj.TT_AMOM + 24] = gl[L.PP_AMOM0:L.PP_AMOM0 + 24]
            tbar[tj.TT_IB:tj.TT_IB + 9] = gl[L.PP_INERTIA_B:L.PP_INERTIA_B + 9]
            qbar = J[:, 0:8].T @ tbar
            sbar[L.PS_Q:L.PS_Q + 8] += qbar
            if solved:
                fmbar[L.FM_DQ:L.FM_DQ + 8] += qbar
        # ---- the solve
        if solved:
            adj = am.condensed_adjoint(cfg, rec, xbar0, fmbar)
            gin = arm.condensed_record_adjoint(cfg, rec, xbar0, fmbar)["grad_in"]
            gcfg += adj["grad_cfg"]
            f = int(adj["flags"])
        else:
            gin, f = np.zeros(cfg.n_in), am.UNSOLVED
        flags |= f
        tick_flags.append(f)
        # ---- record half
        tk = tick_base + t + int(p[L.PP_TICK0])
        is_first = first and tick_base + t == 0
        gib = np.zeros((3, 3))
        if tree is None:
            IB = p[L.PP_INERTIA_B:L.PP_INERTIA_B + 9].reshape(3, 3)
            record_att_adjoint(cfg, s, IB, tk, is_first, tracks, gin, wbar, sbar, gib, grpy, grpyd, mutation)
            gp[L.PP_INERTIA_B:L.PP_INERTIA_B + 9] += gib.reshape(-1)
            rpm.record_param_adjoint(cfg, s, p, tk, is_first, traj, gin, wbar, gp, gpos, gvel, galpha)
            wbar = ram.record_adjoint(cfg, s, p, tk, is_first, vel, gin, sbar, wbar)
        else:
            tau, J = tj.jacobian(tree, s[L.PS_Q:L.PS_Q + 8], s[L.PS_T:L.PS_T + 4], selector)
            pl = rtm._local(p, tau)
            record_att_adjoint(cfg, s, tau[tj.TT_IB:tj.TT_IB + 9].reshape(3, 3), tk, is_first, tracks, gin, wbar, sbar, gib, grpy,
                               grpyd, mutation)
            gl = np.zeros(NP)
            with rtm._parametric():
                rpm.record_param_adjoint(cfg, s, pl, tk, is_first, traj, gin, wbar, gl, gpos, gvel, galpha)
                wbar = ram.record_adjoint(cfg, s, pl, tk, is_first, vel, gin, sbar, wbar)
            gp[keep] += gl[keep]
            tbar = np.zeros(tj.TT_SIZE)
            tbar[tj.TT_AMOM:tj.TT_AMOM + 24] = gl[L.PP_AMOM0:L.PP_AMOM0 + 24]
            tbar[tj.TT_LLIN:tj.TT_LLIN + 24] = gin[ref.IN_LLIN:ref.IN_LLIN + 24]
            tbar[tj.TT_LANG:tj.TT_LANG + 24] = gin[ref.IN_LANG:ref.IN_LANG + 24]
            tbar[tj.TT_IB:tj.TT_IB + 9] = gl[L.PP_INERTIA_B:L.PP_INERTIA_B + 9]
            if mutation != "tree_ib_not_through_j":
                tbar[tj.TT_IB:tj.TT_IB + 9] += gib.reshape(-1)
            sbar[L.PS_T:L.PS_T + 4] += J[:, 8:12].T @ tbar
            sbar[L.PS_Q:L.PS_Q + 8] += J[:, 0:8].T @ tbar
    return {"grad_state0": sbar, "grad_cfg": gcfg, "flags": flags, "tick_flags": tick_flags[::-1], "grad_params": gp,
            "grad_traj_pos": gpos, "grad_traj_vel": gvel, "grad_traj_alpha": galpha, "grad_traj_rpy": grpy,
            "grad_traj_rpy_dot": grpyd}


# ----------------------------------------------------------------------------------------------------------------------
# central differences of the forward loop
# ----------------------------------------------------------------------------------------------------------------------
def central(cfg, s0, p, traj, att, ticks, log_bar, state_bar, d_rpy=None, d_rpy_dot=None, d_state=None, d_params=None, step=1e-4,
            substeps=None, unsolved_ticks=(), taped_from=0, richardson=True, both_steps=False):
    """Directional derivative of the loss of `forward` along (d_rpy, d_rpy_dot [n_traj, 3], d_state [40], d_params [249]) (any
    may be None): central differences, Richardson extrapolated with step / 2 (O(h^4)).  taped_from > 0: the loss is on the
    ticks from there on (log_bar's rows) and the tracks are perturbed from that tick on only; the state and the parameters
    cannot be perturbed then.  both_steps: returns (the extrapolated value, the quotient at `step`, the quotient at step / 2)."""
    n = len(traj[0])
    rpy, rpyd = tracks_of(att, n)
    assert taped_from == 0 or (d_state is None and d_params is None)

    def at(e):
        a2 = (rpy if d_rpy is None else rpy + e * np.asarray(d_rpy), rpyd if d_rpy_dot is None else rpyd + e * np.asarray(d_rpy_dot))
        s = np.array(s0, dtype=float)
        if d_state is not None:
            s[:NS] += e * np.asarray(d_state)
        pp = np.array(p, dtype=float) if d_params is None else p + e * np.asarray(d_params)
        if taped_from:
            log, fin, _ = forward(cfg, s, pp, traj, (rpy, rpyd), ticks, substeps, unsolved_ticks, switch=(taped_from, a2))
        else:
            log, fin, _ = forward(cfg, s, pp, traj, a2, ticks, substeps, unsolved_ticks)
        return ram.loss(log[taped_from:], fin, log_bar, state_bar)

    def quotient(h):
        return (at(h) - at(-h)) / (2.0 * h)

    q1, q2 = quotient(step), quotient(0.5 * step)
    val = (4.0 * q2 - q1) / 3.0 if richardson else q1
    return (val, q1, q2) if both_steps else val


def reached(cfg, p, n_traj, ticks, first=True, tick_base=0):
    """samples [n_traj] bool that a window column of the taped run holds"""
    rs = np.zeros(n_traj, dtype=bool)
    for t in range(ticks):
        tk = tick_base + t + int(p[L.PP_TICK0])
        if first and tick_base + t == 0:
            for j in range(cfg.n_ref_cols):
                rs[rpm.fill_sample(cfg, n_traj, tk, j)] = True
        if tk % cfg.ratio == cfg.ratio - 1:
            rs[rpm.push_sample(cfg, n_traj, tk)] = True
    return rs
