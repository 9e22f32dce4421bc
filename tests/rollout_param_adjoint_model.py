"""Adjoint of the closed-loop rollout in numpy, the part behind rollout_adjoint_model.py: the gradient of the same loss with
respect to the plant parameters (VSMPC_PP_*) and to the three reference tracks (traj_pos | traj_vel | traj_alpha), for
tests/test_rollout_param_adjoint_model.py and tests/test_gpu_rollout_param_adjoint.py.  Mirror of
vsmpc_rollout_backward_full (the PT instantiation of advance_adjoint_kernel in csrc/vsmpc_rollout_adjoint.hip).

  backward     rollout_adjoint_model.backward's sweep with the last step of the chain rule added at both halves of a tick:
               record_param_adjoint at the taped state (the record's entries that are parameters or are built from them, the
               window columns at the moment their cotangent is complete, alpha of the tick), plant_param_adjoint in place of
               plant_adjoint (every sub-step: mass, I_B^-1, the jet map, the push, alpha of the sub-step).  Written from the
               formulas.
  central      central differences of rollout_adjoint_model.forward along directions in the parameters and the tracks,
               Richardson extrapolated as rollout_adjoint_model.central.

The derivative is taken with the tick state at the start of the taped run held fixed, except at a reset (`first`), where the
window is built from the tracks and is differentiated.  DIST_T0, DIST_T1 and TICK0 are structural: +0.0.
rollout_model, tick_model and adjoint_record_model are imported and not changed.  The state recursion of the sub-steps is
rollout_adjoint_model.plant_adjoint's, the one copy: plant_param_adjoint calls it and builds its shares from the per-sub-step
quantities it hands over, so a defect planted in the recursion reaches the state and the parameter gradients alike.
`mutation` (one of MUTATIONS) plants one defect, for the mutation tests only.
"""
from __future__ import annotations

import numpy as np

import adjoint_model as am
import adjoint_record_model as arm
import rollout_adjoint_model as ram
import rollout_model as pm
import vsmpc_ref as ref

L = pm.L
NS = ram.NS
GRAV = ram.GRAV
NP = L.PLANT_PARAMS
# (field, offset, length) of the differentiable plant parameters: VSMPC_PP_*
PARAM_FIELDS = (("MASS", L.PP_MASS, 1), ("INERTIA_B", L.PP_INERTIA_B, 9), ("AMOM0", L.PP_AMOM0, 24), ("DJ", L.PP_DJ, 192),
                ("QREF0", L.PP_QREF0, 8), ("PINIT", L.PP_PINIT, 3), ("RPYINIT", L.PP_RPYINIT, 3), ("DIST_F", L.PP_DIST_F, 3),
                ("DIST_TAU", L.PP_DIST_TAU, 3))
STRUCTURAL = (L.PP_DIST_T0, L.PP_DIST_T1, L.PP_TICK0)
MUTATIONS = (
    "push_after_shift",       # the pushed column's share is taken from the last column after the shift, not before
    "fill_clamp_off_by_one",  # the `first` fill clamps one sample early
    "drop_mass_window",       # the mass share of the window columns' R^T m v_ref is dropped
    "ibi_record_only",        # the cotangent of I_B^-1 is taken in the record half only
    "dist_outside_window",    # DIST_F is counted in every sub-step, inside the push window or not
    "alpha_one_sample",       # an alpha share goes to the lower of its two samples, undivided
    "qref0_sign",             # the posture error hands +gi[QERR] to QREF0
    "dj_without_lambda")      # DJ gets the A_mom(q) parts only, not Lambda column j = DJ[j] T


def alpha_up_of(cfg, alpha_dt):
    """up-sampling factor of the alpha track as vsmpc_rollout_create derives it"""
    return int(1.0 / cfg.period_mpc + 1e-9) // int(round(1.0 / alpha_dt))


def alpha_tick_samples(n, up, tk, mutation=None):
    """[(sample, weight)] of alpha_of_tick (vsmpc_rollout.hip): tick tk reads sample tk + 1 of the up-sampled track, whose
    last original sample is dropped unless the track is at the rate already"""
    last = n - 1 if up == 1 else up * (n - 1) - 1
    idx = max(min(tk + 1, last), 0)
    i = idx // up
    f = (idx - up * i) / up
    if mutation == "alpha_one_sample":
        return [(i, 1.0)]
    return [(i, 1.0 - f), (min(i + 1, n - 1), f)]


def interp_samples(n, pos, mutation=None):
    """[(sample, weight)] of rollout_model.interp_clamped"""
    if pos <= 0:
        return [(0, 1.0)]
    if pos >= n - 1:
        return [(n - 1, 1.0)]
    i = int(pos)
    f = pos - i
    if mutation == "alpha_one_sample":
        return [(i, 1.0)]
    return [(i, 1.0 - f), (i + 1, f)]


def fill_sample(cfg, n_traj, tk, j, mutation=None):
    """window_fill_sample (vsmpc_rollout_device.hpp)"""
    idx = 1 + tk // cfg.ratio - (cfg.n_ref_cols - 1 - j)
    top = n_traj - 2 if mutation == "fill_clamp_off_by_one" and n_traj > 1 else n_traj - 1
    return min(max(idx, 0), top)


def push_sample(cfg, n_traj, tk):
    """window_push_sample"""
    return min(1 + (tk + 1) // cfg.ratio, n_traj - 1)


def plant_param_adjoint(cfg, s, p, tick, fm, status, alpha_track, alpha_dt, sbar_next, substeps, gp, galpha, mutation=None):
    """rollout_adjoint_model.plant_adjoint at (s, fm, status) -- its arguments, its result (direct part of dL/d s_t [40],
    fmbar [24]) -- with the parameter and alpha shares of rollout_model.advance added to gp [249] and galpha [n_alpha] in
    place.  The shares are built from the quantities the one state recursion hands over, sub-step by sub-step."""
    trace = {}
    out = ram.plant_adjoint(cfg, s, p, tick, fm, status, alpha_track, alpha_dt, sbar_next, substeps, mutation, trace)
    m = p[L.PP_MASS]
    IBi = np.linalg.inv(p[L.PP_INERTIA_B:L.PP_INERTIA_B + 9].reshape(3, 3))
    h, Abar = trace["h"], trace["Abar"]
    gw = np.array([0.0, 0.0, -GRAV])
    n_alpha = len(alpha_track)
    for x, lam, R, _, om, ombar, alpha, dist, t in trace["steps"]:   # the parameters of a sub-step, at the cotangent behind it
        lp, ll, la, hl = lam[0:3], lam[3:6], lam[9:12], x[3:6]
        gp[L.PP_MASS] += h * (alpha * (ll @ (R.T @ gw)) - lp @ (R @ hl) / m ** 2)        # alpha m R^T g; p' = R h_lin / m
        if mutation != "ibi_record_only":                                               # omega = I_B^-1 h_ang
            gp[L.PP_INERTIA_B:L.PP_INERTIA_B + 9] -= h * np.outer(IBi.T @ ombar, om).reshape(-1)
        if dist or (mutation == "dist_outside_window" and p[L.PP_DIST_T1] > p[L.PP_DIST_T0]):
            gp[L.PP_DIST_F:L.PP_DIST_F + 3] += h * (R @ ll)                              # R^T F
        if dist:
            gp[L.PP_DIST_TAU:L.PP_DIST_TAU + 3] += h * la
        for i, wgt in interp_samples(n_alpha, t / alpha_dt, mutation):
            galpha[i] += wgt * h * m * (ll @ (R.T @ gw))
    # A_mom(q) = A_mom0 + sum_j DJ[j] (q_j - q_ref0_j), q the joints after the move
    dq = trace["q"] - p[L.PP_QREF0:L.PP_QREF0 + 8]
    gp[L.PP_AMOM0:L.PP_AMOM0 + 24] += Abar.reshape(-1)
    gp[L.PP_DJ:L.PP_DJ + 192] += np.outer(dq, Abar.reshape(-1)).reshape(-1)
    gp[L.PP_QREF0:L.PP_QREF0 + 8] -= trace["DJ"].reshape(8, 24) @ Abar.reshape(-1)
    return out


def record_param_adjoint(cfg, s, p, tk, first, traj, gin, wbar, gp, gpos, gvel, galpha, mutation=None, diag=None):
    """The parameter and track shares of the record assembly of tick tk at plant state s, added in place to gp [249], gpos,
    gvel [n_traj, 3] and galpha [n_alpha].  gin [n_in] is the record adjoint's grad_in of the tick, wbar [n_ref, 12] the
    window cotangent as later ticks left it (what rollout_adjoint_model.record_adjoint is given).  diag (a dict, or None):
    "mass_window" receives the mass's share through the window columns alone."""
    pos, vel, alpha, alpha_dt = traj
    nref, ratio, n_traj = cfg.n_ref_cols, cfg.ratio, len(vel)
    m = p[L.PP_MASS]
    IB = p[L.PP_INERTIA_B:L.PP_INERTIA_B + 9].reshape(3, 3)
    IBi = np.linalg.inv(IB)
    DJ = p[L.PP_DJ:L.PP_DJ + 192].reshape(8, 24)
    R = pm.rot(s[L.PS_RPY:L.PS_RPY + 3])
    x0b = gin[ref.IN_X0:ref.IN_X0 + 26]
    w = wbar + gin[ref.IN_XREF:ref.IN_XREF + 12 * nref].reshape(nref, 12)
    w[0, 0:3] += gin[ref.IN_PREF:ref.IN_PREF + 3] - x0b[20:23]
    w[0, 6:9] -= x0b[23:26]
    gp[L.PP_MASS] += gin[ref.IN_MASS]
    Gi = gin[ref.IN_INERTIA:ref.IN_INERTIA + 9].reshape(3, 3)
    gom = gin[ref.IN_OMEGA:ref.IN_OMEGA + 3]
    om = IBi @ s[L.PS_HANG:L.PS_HANG + 3]
    gp[L.PP_INERTIA_B:L.PP_INERTIA_B + 9] += (R.T @ Gi @ R - np.outer(IBi.T @ gom, om)).reshape(-1)   # I_G = R I_B R^T; omega
    GA = gin[ref.IN_AMOM:ref.IN_AMOM + 24]
    dq = s[L.PS_Q:L.PS_Q + 8] - p[L.PP_QREF0:L.PP_QREF0 + 8]
    gp[L.PP_AMOM0:L.PP_AMOM0 + 24] += GA
    gdj = np.outer(dq, GA).reshape(8, 6, 4)
    if mutation != "dj_without_lambda":                            # Lambda[row][j] = sum_c DJ[j][row][c] T_c
        GL = np.vstack([gin[ref.IN_LLIN:ref.IN_LLIN + 24].reshape(3, 8), gin[ref.IN_LANG:ref.IN_LANG + 24].reshape(3, 8)])
        gdj = gdj + np.einsum("rj,c->jrc", GL, s[L.PS_T:L.PS_T + 4])
    gp[L.PP_DJ:L.PP_DJ + 192] += gdj.reshape(-1)
    sign = 1.0 if mutation == "qref0_sign" else -1.0
    gp[L.PP_QREF0:L.PP_QREF0 + 8] += sign * gin[ref.IN_QERR:ref.IN_QERR + 8] - DJ @ GA
    gp[L.PP_RPYINIT:L.PP_RPYINIT + 3] += gin[ref.IN_RPYINIT:ref.IN_RPYINIT + 3]
    for i, wgt in alpha_tick_samples(len(alpha), alpha_up_of(cfg, alpha_dt), tk, mutation):
        galpha[i] += wgt * gin[ref.IN_ALPHA]

    def column(cw, idx):
        """a window column built from trajectory sample idx, its cotangent cw [12] complete"""
        gp[L.PP_PINIT:L.PP_PINIT + 3] += cw[0:3]
        gpos[idx] += cw[0:3]
        gp[L.PP_RPYINIT:L.PP_RPYINIT + 3] += cw[6:9]
        if mutation != "drop_mass_window":
            gp[L.PP_MASS] += cw[3:6] @ (R.T @ vel[idx])            # h_lin entry R^T m v_ref
            if diag is not None:
                diag["mass_window"] = diag.get("mass_window", 0.0) + cw[3:6] @ (R.T @ vel[idx])
        gvel[idx] += m * (R @ cw[3:6])

    if tk % ratio == ratio - 1:
        prev = np.zeros_like(w)
        prev[1:] = w[:-1]
        column(prev[nref - 1] if mutation == "push_after_shift" else w[nref - 1], push_sample(cfg, n_traj, tk))
        w = prev
    if first:
        for j in range(nref):
            column(w[j], fill_sample(cfg, n_traj, tk, j, mutation))


def backward(cfg, tape, p, traj, log_bar, state_bar, substeps=None, first=True, tick_base=0, mutation=None):
    """One instance: rollout_adjoint_model.backward's outputs (grad_state0, grad_cfg, flags, tick_flags) and grad_params
    [249], grad_traj_pos, grad_traj_vel [n_traj, 3], grad_traj_alpha [n_alpha]."""
    substeps = ram.substeps_of(cfg) if substeps is None else substeps
    pos, vel, alpha, alpha_dt = traj
    ticks = len(tape)
    sbar = np.zeros(NS) if state_bar is None else np.array(state_bar[:NS], dtype=float)
    wbar = np.zeros((cfg.n_ref_cols, 12))
    gcfg, flags, tick_flags = np.zeros(am.GRAD_SIZE), 0, []
    gp, gpos, gvel, galpha = np.zeros(NP), np.zeros((len(pos), 3)), np.zeros((len(vel), 3)), np.zeros(len(alpha))
    xbar0 = np.zeros(cfg.n_var)
    diag = {"mass_window": 0.0}
    for t in range(ticks - 1, -1, -1):
        s, rec, fm, status = tape[t]
        if log_bar is not None:
            sbar[0:3] += log_bar[t, 0:3]
            sbar[6:9] += log_bar[t, 3:6]
            sbar[12:16] += log_bar[t, 6:10]
            sbar[L.PS_U:L.PS_U + 4] += log_bar[t, 10:14]
        sbar, fmbar = plant_param_adjoint(cfg, s, p, tick_base + t, fm, status, alpha, alpha_dt, sbar, substeps, gp, galpha, mutation)
        if status == L.STATUS_SOLVED:
            adj = am.condensed_adjoint(cfg, rec, xbar0, fmbar)
            gin = arm.condensed_record_adjoint(cfg, rec, xbar0, fmbar)["grad_in"]
            gcfg += adj["grad_cfg"]
            f = int(adj["flags"])
        else:
            gin, f = np.zeros(cfg.n_in), am.UNSOLVED
        flags |= f
        tick_flags.append(f)
        tk = tick_base + t + int(p[L.PP_TICK0])
        is_first = first and tick_base + t == 0
        record_param_adjoint(cfg, s, p, tk, is_first, traj, gin, wbar, gp, gpos, gvel, galpha, mutation, diag)
        wbar = ram.record_adjoint(cfg, s, p, tk, is_first, vel, gin, sbar, wbar)
    return {"grad_state0": sbar, "grad_cfg": gcfg, "flags": flags, "tick_flags": tick_flags[::-1], "grad_params": gp,
            "grad_traj_pos": gpos, "grad_traj_vel": gvel, "grad_traj_alpha": galpha, "mass_window": diag["mass_window"]}


def central(cfg, s0, p, traj, ticks, log_bar, state_bar, d_params=None, d_pos=None, d_vel=None, d_alpha=None, step=1e-4,
            substeps=None, unsolved_ticks=(), richardson=True):
    """Directional derivative of the loss of rollout_adjoint_model.forward along (d_params [249], d_pos, d_vel [n_traj, 3],
    d_alpha [n_alpha]) (any may be None): central differences, Richardson extrapolated with step / 2 (O(h^4))."""
    pos, vel, alpha, alpha_dt = traj

    def at(e):
        pp = np.array(p, dtype=float) if d_params is None else p + e * np.asarray(d_params)
        tr = (pos if d_pos is None else pos + e * np.asarray(d_pos), vel if d_vel is None else vel + e * np.asarray(d_vel),
              alpha if d_alpha is None else alpha + e * np.asarray(d_alpha), alpha_dt)
        log, fin, _ = ram.forward(cfg, s0, pp, tr, ticks, substeps, unsolved_ticks)
        return ram.loss(log, fin, log_bar, state_bar)

    def quotient(h):
        return (at(h) - at(-h)) / (2.0 * h)

    q = quotient(step)
    return (4.0 * quotient(0.5 * step) - q) / 3.0 if richardson else q


def param_scale():
    """step scale of every plant parameter for the difference quotients: mass [kg], inertia, the jet map and its joint
    derivatives, joints and angles [rad], position [m], force [N], torque [Nm]"""
    sc = np.ones(NP)
    sc[L.PP_INERTIA_B:L.PP_INERTIA_B + 9] = 1e-1
    sc[L.PP_AMOM0:L.PP_AMOM0 + 24] = 1e-2
    sc[L.PP_DJ:L.PP_DJ + 192] = 1e-2
    sc[L.PP_QREF0:L.PP_QREF0 + 8] = 1e-2
    sc[L.PP_PINIT:L.PP_PINIT + 3] = 1e-2
    sc[L.PP_RPYINIT:L.PP_RPYINIT + 3] = 1e-2
    sc[L.PP_DIST_TAU:L.PP_DIST_TAU + 3] = 1e-1
    return sc


TRACK_SCALE = {"pos": 1e-2, "vel": 1e-2, "alpha": 1e-2}


def reached(cfg, p, traj, ticks, first=True, tick_base=0, substeps=None):
    """(pos/vel samples [n_traj] bool, alpha samples [n_alpha] bool) that the taped run can reach: a window column of the
    run holds the sample; a tick or a sub-step reads the alpha sample with a weight that is not zero"""
    substeps = ram.substeps_of(cfg) if substeps is None else substeps
    pos, _, alpha, alpha_dt = traj
    n_traj, n_alpha = len(pos), len(alpha)
    rs, ra = np.zeros(n_traj, dtype=bool), np.zeros(n_alpha, dtype=bool)
    up = alpha_up_of(cfg, alpha_dt)
    for t in range(ticks):
        tk = tick_base + t + int(p[L.PP_TICK0])
        if first and tick_base + t == 0:
            for j in range(cfg.n_ref_cols):
                rs[fill_sample(cfg, n_traj, tk, j)] = True
        if tk % cfg.ratio == cfg.ratio - 1:
            rs[push_sample(cfg, n_traj, tk)] = True
        for i, wgt in alpha_tick_samples(n_alpha, up, tk):
            ra[i] |= wgt != 0.0
        for ss in range(substeps):
            for i, wgt in interp_samples(n_alpha, (tk + ss / substeps) * cfg.period_mpc / alpha_dt):
                ra[i] |= wgt != 0.0
    return rs, ra
