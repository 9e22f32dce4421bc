"""Adjoint of the closed-loop rollout on the KINEMATIC-TREE plant in numpy (rollout_model.set_tree): the sweep of
rollout_adjoint_model / rollout_param_adjoint_model with the tree's one smooth map per tick,

    tau(q, T) = A_mom,body | Lambda_lin,B | Lambda_ang,B | I_B      (tree_jacobian_model.terms, 81 numbers),

in place of the parametric plant's A_mom0 + DJ (q - q_ref0), DJ T and constant I_B.  Mirror of the tree instantiations of
advance_adjoint_kernel (csrc/vsmpc_rollout_adjoint.hip) behind tree_jacobian_kernel.

How it is built on the two models, which are imported and not changed (they share one state recursion,
rollout_adjoint_model.plant_adjoint, which rollout_param_adjoint_model.plant_param_adjoint calls).  At the state between two ticks the tree plant IS a
parametric plant whose record holds A_mom0 = A_mom(q), I_B = I_B(q) and DJ = 0 -- for everything but the dependence of
those numbers on (q, T).  So both halves of a tick run the imported transposes on that local record, with the parametric
branch of rollout_model selected for the length of the call; rollout_param_adjoint_model's parameter shares of A_mom0 and
I_B are then exactly the cotangents of tau's A_mom and I_B rows, and the record adjoint's grad_in carries Lambda's.  What
this module adds is the last step: tau_bar is pulled back through J = d tau / d(q | T) (tree_jacobian_model.jacobian),

    record half of tick k    (A_mom, Lambda, I_B through I_G and omega) at (q_k, T_k): to the joints, and -- Lambda being
                             linear in T -- to the thrusts, in front of the sub-steps of tick k - 1;
    plant half of tick k-1   (A_mom, I_B through omega) of the sub-steps, at q_k = q_{k-1} + dq: to the joints, and to the
                             joint block of the first move's cotangent when the tick was Solved.

In grad_params the blocks the tree plant does not read (INERTIA_B, AMOM0, DJ) are +0.0, QREF0 keeps the posture error's
share, everything else is the parametric plant's.  `mutation` (one of MUTATIONS) plants one defect, for the mutation tests."""
from __future__ import annotations

import contextlib

import numpy as np

import adjoint_model as am
import adjoint_record_model as arm
import rollout_adjoint_model as ram
import rollout_model as pm
import rollout_param_adjoint_model as rpm
import sensitivity_model as sm
import tree_jacobian_model as tj
import vsmpc_ref as ref

L = pm.L
NS, NP = ram.NS, rpm.NP
TT = tj
MUTATIONS = (
    "drop_dib_dq",            # d I_B / dq dropped, both halves
    "drop_damom_dq_plant",    # d A_mom / dq dropped from the plant half only
    "drop_lambda_thrust",     # Lambda's pull-back to the thrusts dropped
    "lambda_const_in_q",      # Lambda's dependence on q dropped (the Jacobians behind it held constant)
    "tau_at_previous_q",      # the plant half's tau evaluated at q_{k-1} instead of q_k = q_{k-1} + dq
    "qbar_not_to_move",       # the plant half's joint pull-back not shared with the joint block of fmbar
    "qbar_to_unsolved_move",  # ... or shared with it, and handed to the solve's adjoint, on a tick that was not Solved
    "default_selector")       # the default joint selector used under another one
_ORIG_TREE_TERMS = pm.tree_terms


def set_tree(tree, selector=None):
    """rollout_model.set_tree, with the handle's joint selector (vsmpc_set_kinematics_options) for Lambda_ang's columns: the
    forward model's tree_terms is replaced by this module's while a selector is set (rollout_model knows the default only)."""
    pm.set_tree(tree)
    if tree is None or selector is None:
        pm.tree_terms = _ORIG_TREE_TERMS
        return
    sel = [int(v) for v in selector]

    def tree_terms(q, T):
        t = tj.oracle_terms(tree, q, T, sel)
        return t[0:24].reshape(6, 4), t[24:72].reshape(6, 8), t[72:81].reshape(3, 3)

    pm.tree_terms = tree_terms


@contextlib.contextmanager
def _parametric():
    """the parametric branch of rollout_model while the imported transposes run on a local record"""
    keep = pm._TREE
    pm._TREE = None
    try:
        yield
    finally:
        pm._TREE = keep


def _local(p, tau):
    """the parameter record of the parametric plant that has tau's A_mom and I_B and no dependence on q"""
    pl = np.array(p, dtype=float)
    pl[L.PP_AMOM0:L.PP_AMOM0 + 24] = tau[TT.TT_AMOM:TT.TT_AMOM + 24]
    pl[L.PP_DJ:L.PP_DJ + 192] = 0.0
    pl[L.PP_INERTIA_B:L.PP_INERTIA_B + 9] = tau[TT.TT_IB:TT.TT_IB + 9]
    return pl


def backward(cfg, tape, p, traj, log_bar, state_bar, tree, selector=None, substeps=None, first=True, tick_base=0, mutation=None):
    """One instance on the tree plant: rollout_param_adjoint_model.backward's outputs (grad_state0 [40], grad_cfg [32], flags,
    tick_flags, grad_params [249], grad_traj_pos / _vel [n_traj, 3], grad_traj_alpha [n_alpha]) and tick_active (is any throttle of the
    tick's QP at a limit of its box).  tape = rollout_adjoint_model.forward's under set_tree(tree, selector)."""
    substeps = ram.substeps_of(cfg) if substeps is None else substeps
    pos, vel, alpha, alpha_dt = traj
    ticks = len(tape)
    sbar = np.zeros(NS) if state_bar is None else np.array(state_bar[:NS], dtype=float)
    wbar = np.zeros((cfg.n_ref_cols, 12))
    gcfg, flags, tick_flags, tick_active = np.zeros(am.GRAD_SIZE), 0, [], []
    gp, gpos, gvel, galpha = np.zeros(NP), np.zeros((len(pos), 3)), np.zeros((len(vel), 3)), np.zeros(len(alpha))
    xbar0 = np.zeros(cfg.n_var)
    sel = None if mutation == "default_selector" else selector
    keep = [e for name, o, n in rpm.PARAM_FIELDS if name not in ("INERTIA_B", "AMOM0", "DJ") for e in range(o, o + n)]

    def jac(q, T):
        return tj.jacobian(tree, q, T, sel)

    for t in range(ticks - 1, -1, -1):
        s, rec, fm, status = tape[t]
        solved = status == L.STATUS_SOLVED
        if log_bar is not None:
            sbar[0:3] += log_bar[t, 0:3]
            sbar[6:9] += log_bar[t, 3:6]
            sbar[12:16] += log_bar[t, 6:10]
            sbar[L.PS_U:L.PS_U + 4] += log_bar[t, 10:14]
        # ---- plant half: tau at the joints after the move (A_mom and I_B do not read the thrusts)
        q_next = s[L.PS_Q:L.PS_Q + 8] + (fm[L.FM_DQ:L.FM_DQ + 8] if solved and mutation != "tau_at_previous_q" else 0.0)
        tau, J = jac(q_next, s[L.PS_T:L.PS_T + 4])
        pl = _local(p, tau)
        gl = np.zeros(NP)
        with _parametric():
            sbar, fmbar = rpm.plant_param_adjoint(cfg, s, pl, tick_base + t, fm, status, alpha, alpha_dt, sbar, substeps, gl, galpha)
        gp[keep] += gl[keep]
        tbar = np.zeros(TT.TT_SIZE)
        if mutation != "drop_damom_dq_plant":
            tbar[TT.TT_AMOM:TT.TT_AMOM + 24] = gl[L.PP_AMOM0:L.PP_AMOM0 + 24]
        if mutation != "drop_dib_dq":
            tbar[TT.TT_IB:TT.TT_IB + 9] = gl[L.PP_INERTIA_B:L.PP_INERTIA_B + 9]
        qbar = J[:, 0:8].T @ tbar
        sbar[L.PS_Q:L.PS_Q + 8] += qbar
        if (solved and mutation != "qbar_not_to_move") or (not solved and mutation == "qbar_to_unsolved_move"):
            fmbar[L.FM_DQ:L.FM_DQ + 8] += qbar
        # ---- the solve
        if solved or (mutation == "qbar_to_unsolved_move" and np.isfinite(rec).all()):   # (the defect lets the solve see it)
            adj = am.condensed_adjoint(cfg, rec, xbar0, fmbar)
            gin = arm.condensed_record_adjoint(cfg, rec, xbar0, fmbar)["grad_in"]
            gcfg += adj["grad_cfg"]
            f = int(adj["flags"])
            tick_active.append(bool(np.isin(np.asarray(adj["active"]), (sm.LOWER, sm.UPPER)).any()))
        else:
            gin, f = np.zeros(cfg.n_in), am.UNSOLVED
            tick_active.append(False)
        flags |= f
        tick_flags.append(f)
        # ---- record half: tau at the taped state
        tk = tick_base + t + int(p[L.PP_TICK0])
        is_first = first and tick_base + t == 0
        tau, J = jac(s[L.PS_Q:L.PS_Q + 8], s[L.PS_T:L.PS_T + 4])
        pl = _local(p, tau)
        gl = np.zeros(NP)
        with _parametric():
            rpm.record_param_adjoint(cfg, s, pl, tk, is_first, traj, gin, wbar, gl, gpos, gvel, galpha)
            wbar = ram.record_adjoint(cfg, s, pl, tk, is_first, vel, gin, sbar, wbar)
        gp[keep] += gl[keep]
        tbar = np.zeros(TT.TT_SIZE)
        tbar[TT.TT_AMOM:TT.TT_AMOM + 24] = gl[L.PP_AMOM0:L.PP_AMOM0 + 24]          # = grad_in's A_mom
        tbar[TT.TT_LLIN:TT.TT_LLIN + 24] = gin[ref.IN_LLIN:ref.IN_LLIN + 24]
        tbar[TT.TT_LANG:TT.TT_LANG + 24] = gin[ref.IN_LANG:ref.IN_LANG + 24]
        if mutation != "drop_dib_dq":
            tbar[TT.TT_IB:TT.TT_IB + 9] = gl[L.PP_INERTIA_B:L.PP_INERTIA_B + 9]    # I_G = R I_B R^T, omega = I_B^-1 h_ang
        if mutation != "drop_lambda_thrust":
            sbar[L.PS_T:L.PS_T + 4] += J[:, 8:12].T @ tbar
        if mutation == "lambda_const_in_q":
            tbar[TT.TT_LLIN:TT.TT_IB] = 0.0
        sbar[L.PS_Q:L.PS_Q + 8] += J[:, 0:8].T @ tbar
    return {"grad_state0": sbar, "grad_cfg": gcfg, "flags": flags, "tick_flags": tick_flags[::-1], "grad_params": gp,
            "grad_traj_pos": gpos, "grad_traj_vel": gvel, "grad_traj_alpha": galpha, "tick_active": tick_active[::-1]}
