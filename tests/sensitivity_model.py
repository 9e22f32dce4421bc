"""Jacobian of the MPC solution with respect to the measured state X0 (record[0:26]), two ways, for
tests/test_sensitivity_model.py and tests/test_gpu_sensitivity.py:

  kkt_jacobian        the oracle's dense reference-ordered QP (vsmpc_ref.assemble_dense / solve_exact) with its final active
                      set: [H Ae^T; Ae 0] [J; dy] = [0; E], Ae = the equality rows (dynamics, initial state) and the active
                      throttle rows, E = I_26 on the initial-state rows
  condensed_jacobian  numpy mirror of sens_kernel_rt (csrc/vsmpc_rt_sens.hpp), the way tests/runtime_model.py mirrors
                      solve_kernel_rt: condensing with 26 parameter columns (X_0 = e_i, no input, no c, no reference), the
                      joint-column Cholesky, the box QP, then S_FF dv_F = -F~_F, L_jj^T du = -(L_vj^T dv + l~) and
                      dX_{k+1} = dX_k + dt_k (A dX_k + Bj dU + Bt dV)

X0 enters the QP only through the initial-state rows lo = hi (the linearisation reads other record fields), so both are
the total derivative of the map record -> x*, one-sided where the active set is about to change (`flags`).
"""
from __future__ import annotations

import numpy as np

import runtime_model as rm
import vsmpc_ref as ref

NX, NJ, NTH = ref.N_STATES, ref.N_JOINTS, ref.N_THRUSTS
NPAR = NX
GRAD_TOL, BOUND_TOL = 1e-8, 1e-9        # VSMPC_SENS_GRAD_TOL, VSMPC_SENS_BOUND_TOL (include/vsmpc.h)
DEGENERATE, UNSOLVED = 0x1, 0x2         # VSMPC_SENS_*
FREE, LOWER, UPPER, PINNED = 0, -1, 1, 2


def dthrottle_dv(v):
    """derivative of vsmpc_ref.destd_throttle: sigma_u / sqrt(1 + 4 c12 v), 0 where the clamp to [0, 100] is active"""
    c12, mu, sg = ref.JET_COEFF[12], ref.JET_NORM[2], ref.JET_NORM[3]
    r = np.sqrt(1.0 + 4.0 * c12 * np.asarray(v, dtype=float))
    u = (-1.0 + r) / (2.0 * c12) * sg + mu
    return np.where((u < 0.0) | (u > 100.0), 0.0, sg / r)


def first_move_jacobian(cfg: ref.Config, v0, J):
    """d(first-move block)/dX0 (24 x 26) from the first throttle block v0 and J = dx/dX0 (reference order)"""
    offJ, offV = cfg.off_joints, cfg.off_throttle
    D = np.zeros((24, NPAR))
    D[0:8] = J[offJ:offJ + 8]
    D[8:12] = J[offV:offV + 4]
    D[12:16] = dthrottle_dv(v0)[:, None] * J[offV:offV + 4]
    D[16:24] = J[NX + 12:NX + 20]            # thrust and thrust rate of node 1
    return D


def throttle_states(v, lo, hi, fixed):
    return np.where(fixed, PINNED, np.where(v == lo, LOWER, np.where(v == hi, UPPER, FREE)))


def kkt_jacobian(cfg: ref.Config, inp: np.ndarray):
    """(x, J, active): the oracle's optimum, dx/dX0 (nVar x 26) and the final throttle states"""
    H, g, Ac, lo, hi = ref.assemble_dense(cfg, inp)
    x, _, _ = ref.solve_exact(cfg, H, g, Ac, lo, hi)
    nxs, nv = NX * (cfg.n_iter + 1), NTH * cfg.n_vblocks
    tlo, thi = lo[nxs:nxs + nv], hi[nxs:nxs + nv]
    active = throttle_states(x[cfg.off_throttle:cfg.off_throttle + nv], tlo, thi, tlo == thi)
    rows = np.concatenate([np.arange(nxs), nxs + np.nonzero(active != FREE)[0]])
    n, m = H.shape[0], rows.size
    K = np.zeros((n + m, n + m))
    K[:n, :n] = H
    K[:n, n:] = Ac[rows].T
    K[n:, :n] = Ac[rows]
    rhs = np.zeros((n + m, NPAR))
    r0 = NX * cfg.n_iter                     # initial-state rows (IQPUtilsMPC.cpp:71-92)
    rhs[n + r0:n + r0 + NX] = np.eye(NX)
    return x, np.linalg.solve(K, rhs)[:n], active


def condense(cfg: ref.Config, inp: np.ndarray):
    """runtime_model.condense with the 26 parameter columns after the affine one: rows NZ + 1 .. NZ + 26 of the lower
    triangle hold F = d(condensed gradient)/dX0; the input costs (P2) touch [U | v | 1] only."""
    C0, gmax, vprev, lin = rm.condense(cfg, inp)
    A, Bj, Bt, c, dts = lin
    nz = C0.shape[0] - 1
    nu = NJ * cfg.control_horizon
    n = nz + 1 + NPAR
    sq = np.sqrt(ref.state_weight(cfg))[rm.WROWS]
    X = np.zeros((NX, n))
    X[:, nz] = inp[ref.IN_X0:ref.IN_X0 + NX]
    X[:, nz + 1:] = np.eye(NX)
    xref = inp[ref.IN_XREF:ref.IN_XREF + 12 * cfg.n_ref_cols].reshape(cfg.n_ref_cols, 12)
    C = np.zeros((n, n))
    for k in range(cfg.n_iter):
        Bk = np.zeros((NX, n))
        jb, tb = ref.joint_block_of_stage(cfg, k), ref.throttle_block_of_stage(cfg, k)
        Bk[:, NJ * jb:NJ * (jb + 1)] = Bj
        Bk[:, nu + NTH * tb:nu + NTH * (tb + 1)] = Bt
        Bk[:, nz] = c
        X = X + dts[k] * (A @ X + Bk)
        col = 0 if k < cfg.n_iter_small else k - cfg.n_iter_small
        R = X[rm.WROWS, :].copy()
        R[:12, nz] -= xref[col]
        Y = sq[:, None] * R
        C += Y.T @ Y
    C = np.tril(C)
    C[:nz + 1, :nz + 1] = C0
    return C, gmax, vprev, lin


def condensed_jacobian(cfg: ref.Config, inp: np.ndarray) -> dict:
    """status, active, flags, v (throttles) and J = dx/dX0 (zero unless Solved), as sens_kernel_rt computes them"""
    nu, nv = NJ * cfg.control_horizon, NTH * cfg.n_vblocks
    nz = nu + nv
    M, gmax, vprev, (A, Bj, Bt, c, dts) = condense(cfg, inp)
    if not rm._chol_partial(M, nu):
        raise FloatingPointError("non-positive joint pivot")
    S = M[nu:nz, nu:nz]
    S = np.tril(S) + np.tril(S, -1).T
    s = M[nz, nu:nz].copy()
    Ft, lt = M[nz + 1:, nu:nz], M[nz + 1:, :nu]      # reduced parameter rows: throttle and joint columns
    vmin, vmax = ref.throttle_bounds(cfg)
    fixed = np.zeros(nv, dtype=bool)
    lo, hi = np.full(nv, vmin), np.full(nv, vmax)
    if inp[ref.IN_HOLD] != 0.0:
        fixed[:NTH] = True
        lo[:NTH] = hi[:NTH] = vprev
    v, status, _ = rm.box_qp(S, s, lo, hi, fixed, 1e-10 * (1.0 + gmax))
    active = throttle_states(v, lo, hi, fixed)
    J = np.zeros((NX * (cfg.n_iter + 1) + nz, NPAR))
    if status != rm.SOLVED:
        return {"status": status, "active": active, "flags": UNSOLVED, "v": v, "J": J}
    grad = S @ v + s
    gt = GRAD_TOL * (1.0 + np.abs(s).max())
    bt = BOUND_TOL * (1.0 + np.abs(v))
    weak = (active == LOWER) | (active == UPPER)
    weak &= np.abs(grad) <= gt
    near = (active == FREE) & ((v - vmin <= bt) | (vmax - v <= bt))
    flags = DEGENERATE if (weak | near).any() else 0
    F = active == FREE
    dv = np.zeros((nv, NPAR))
    if F.any():
        dv[F] = np.linalg.solve(S[np.ix_(F, F)], -Ft[:, F].T)
    du = np.linalg.solve(np.tril(M[:nu, :nu]).T, -(M[nu:nz, :nu].T @ dv + lt.T))
    dX = np.zeros((cfg.n_iter + 1, NX, NPAR))
    dX[0] = np.eye(NX)
    for k in range(cfg.n_iter):
        jb, tb = ref.joint_block_of_stage(cfg, k), ref.throttle_block_of_stage(cfg, k)
        dX[k + 1] = dX[k] + dts[k] * (A @ dX[k] + Bj @ du[NJ * jb:NJ * (jb + 1)] + Bt @ dv[NTH * tb:NTH * (tb + 1)])
    J = np.concatenate([dX.reshape(-1, NPAR), du, dv])
    return {"status": status, "active": active, "flags": flags, "v": v, "J": J}
