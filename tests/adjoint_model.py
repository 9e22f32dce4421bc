"""Adjoint of the MPC solve -- the gradient of a scalar loss on the plan with respect to the measured state X0 and to the
tunable configuration fields -- two ways, for tests/test_adjoint_model.py and tests/test_gpu_adjoint.py:

  kkt_adjoint        the oracle's dense reference-ordered QP (vsmpc_ref.assemble_dense / solve_exact) with its final active
                     set, like sensitivity_model.kkt_jacobian: K [a; b] = [xbar; 0] with K = [H E^T; E 0], E the equality
                     rows (dynamics, initial state) and the active throttle rows.  Then dL/dX0 = b on the initial-state rows,
                     dL/d(throttle limit) = the sum of b over the non-pinned throttles on that limit, and
                     dL/dw = -a^T (dH/dw x + dg/dw) for every weight w
  condensed_adjoint  numpy mirror of adjoint_kernel_rt (csrc/vsmpc_rt_adjoint.hpp: rt_adj_rhs, rt_adj_solve, rt_adj_states,
                     rt_adj_costates, rt_adj_reduce_write) on runtime_model.condense / _chol_partial / box_qp: the
                     right-hand side Z^T xbar by a costate recursion, one right-hand side through the joint factor and the
                     factor of S_FF, a forward recursion for the state part of a, certify's costate recursion for b

Gradient rows follow include/vsmpc.h VSMPC_GRAD_*: the order of the vsmpc_config fields, derivatives with respect to the
field values (weights, not their square roots; throttle limits in percent, not warped).  An optional first-move cotangent
fmbar [24] is folded into xbar first (fold_first_move).  Both routes return the flags by sensitivity_model's rule.
"""
from __future__ import annotations

import numpy as np

import runtime_model as rm
import sensitivity_model as sm
import vsmpc_ref as ref

NX, NJ, NTH = ref.N_STATES, ref.N_JOINTS, ref.N_THRUSTS
GRAD_SIZE = 32
# (config field, offset, length): VSMPC_GRAD_*
GRAD_FIELDS = (("w_com_pos", 0, 3), ("w_com_pos_err", 3, 3), ("w_lin_mom", 6, 3), ("w_rpy", 9, 3), ("w_rpy_err", 12, 3),
               ("w_ang_mom", 15, 3), ("w_delta_joint", 18, 8), ("w_throttle", 26, 1), ("w_initial_throttle", 27, 1),
               ("w_reg_joint_pos", 28, 1), ("throttle_min", 29, 1), ("throttle_max", 30, 1))
# state row of every state-weight entry of a gradient row (entries 0..17)
STATE_ROW = [0, 1, 2, 20, 21, 22, 3, 4, 5, 6, 7, 8, 23, 24, 25, 9, 10, 11]
DEGENERATE, UNSOLVED = sm.DEGENERATE, sm.UNSOLVED


def dv_dthrottle(u_percent):
    """derivative of vsmpc_ref.v_of_throttle: (1 + 2 c12 u_bar) / sigma_u"""
    c12, mu, sg = ref.JET_COEFF[12], ref.JET_NORM[2], ref.JET_NORM[3]
    return (1.0 + 2.0 * c12 * (u_percent - mu) / sg) / sg


def fold_first_move(cfg: ref.Config, v0, xbar, fmbar):
    """xbar + the first-move cotangent: DQ -> U_0, V0 and THROTTLE (through d throttle / dv at v0) -> V_0, THRUST and
    THRUSTDOT -> rows 12..19 of X_1"""
    xb = np.array(xbar, dtype=float)
    if fmbar is None:
        return xb
    fmbar = np.asarray(fmbar, dtype=float)
    offJ, offV = cfg.off_joints, cfg.off_throttle
    xb[offJ:offJ + NJ] += fmbar[0:8]
    xb[offV:offV + NTH] += fmbar[8:12] + sm.dthrottle_dv(v0) * fmbar[12:16]
    xb[NX + 12:NX + 20] += fmbar[16:24]
    return xb


def _contractions(cfg: ref.Config, inp, x, a, b_lower, b_upper):
    """the gradient row from the solution x, the primal part a of the adjoint and the sums of b over the lower- and the
    upper-active non-pinned throttles"""
    N, HC, nvb = cfg.n_iter, cfg.control_horizon, cfg.n_vblocks
    offJ, offV = cfg.off_joints, cfg.off_throttle
    X, aX = x[:NX * (N + 1)].reshape(N + 1, NX), a[:NX * (N + 1)].reshape(N + 1, NX)
    U, aU = x[offJ:offV].reshape(HC, NJ), a[offJ:offV].reshape(HC, NJ)
    V, aV = x[offV:].reshape(nvb, NTH), a[offV:].reshape(nvb, NTH)
    win = inp[ref.IN_XREF:ref.IN_XREF + 12 * cfg.n_ref_cols].reshape(cfg.n_ref_cols, 12)
    xr = np.zeros((N + 1, NX))
    for i in range(1, N + 1):
        xr[i, :12] = win[0 if i - 1 < cfg.n_iter_small else i - 1 - cfg.n_iter_small]
    qerr = inp[ref.IN_QERR:ref.IN_QERR + NJ]
    vprev = np.array([ref.v_of_throttle(inp[ref.IN_UPREV + k]) for k in range(NTH)])
    g = np.zeros(GRAD_SIZE)
    for e, r in enumerate(STATE_ROW):
        g[e] = -float(aX[1:, r] @ (X[1:, r] - xr[1:, r]))
    for j in range(NJ):
        g[18 + j] = -float(aU[:, j] @ U[:, j])
    g[26] = -float(((aV[:-1] - aV[1:]) * (V[:-1] - V[1:])).sum())
    g[27] = -float(aV[0] @ (V[0] - vprev))
    g[28] = -float((aU * (U + qerr)).sum())
    g[29] = b_lower * dv_dthrottle(cfg.throttle_min)
    g[30] = b_upper * dv_dthrottle(cfg.throttle_max)
    return g


def degeneracy_flags(S, s, v, active, vmin, vmax) -> int:
    """sensitivity_model's rule on the throttle Schur complement S, its reduced gradient s, the throttles v and their states:
    DEGENERATE when a non-pinned throttle is weakly active (bound, |S v + s| <= GRAD_TOL (1 + max |s|)) or nearly active
    (free, within BOUND_TOL (1 + |v|) of a limit)"""
    grad = S @ v + s
    weak = ((active == sm.LOWER) | (active == sm.UPPER)) & (np.abs(grad) <= sm.GRAD_TOL * (1.0 + np.abs(s).max()))
    bt = sm.BOUND_TOL * (1.0 + np.abs(v))
    near = (active == sm.FREE) & ((v - vmin <= bt) | (vmax - v <= bt))
    return DEGENERATE if (weak | near).any() else 0


def _schur(cfg: ref.Config, inp: np.ndarray):
    """the condensed matrix after the joint-column Cholesky, the throttle Schur complement S (symmetric) and its reduced
    gradient s, with what runtime_model.condense returns beside the matrix"""
    nu = NJ * cfg.control_horizon
    nz = nu + NTH * cfg.n_vblocks
    M, gmax, vprev, lin = rm.condense(cfg, inp)
    if not rm._chol_partial(M, nu):
        raise FloatingPointError("non-positive joint pivot")
    S = M[nu:nz, nu:nz]
    return M, np.tril(S) + np.tril(S, -1).T, M[nz, nu:nz].copy(), gmax, vprev, lin


def kkt_adjoint(cfg: ref.Config, inp: np.ndarray, xbar, fmbar=None) -> dict:
    """x, active, flags (sensitivity_model's rule, on the condensed route's Schur complement at the oracle's throttles),
    grad_x0 [26], grad_cfg [32]"""
    H, g, Ac, lo, hi = ref.assemble_dense(cfg, inp)
    x, _, _ = ref.solve_exact(cfg, H, g, Ac, lo, hi)
    nxs, nv = NX * (cfg.n_iter + 1), NTH * cfg.n_vblocks
    offV = cfg.off_throttle
    tlo, thi = lo[nxs:nxs + nv], hi[nxs:nxs + nv]
    active = sm.throttle_states(x[offV:offV + nv], tlo, thi, tlo == thi)
    act = np.nonzero(active != sm.FREE)[0]
    rows = np.concatenate([np.arange(nxs), nxs + act])
    n, m = H.shape[0], rows.size
    K = np.zeros((n + m, n + m))
    K[:n, :n] = H
    K[:n, n:] = Ac[rows].T
    K[n:, :n] = Ac[rows]
    rhs = np.zeros(n + m)
    rhs[:n] = fold_first_move(cfg, x[offV:offV + NTH], xbar, fmbar)
    sol = np.linalg.solve(K, rhs)
    a, b = sol[:n], sol[n:]
    r0 = NX * cfg.n_iter
    bt = b[nxs:]
    b_lower = float(bt[active[act] == sm.LOWER].sum())
    b_upper = float(bt[active[act] == sm.UPPER].sum())
    _, S, s, _, _, _ = _schur(cfg, inp)
    vmin, vmax = ref.throttle_bounds(cfg)
    return {"x": x, "active": active, "flags": degeneracy_flags(S, s, x[offV:offV + nv], active, vmin, vmax),
            "grad_x0": b[r0:r0 + NX].copy(), "grad_cfg": _contractions(cfg, inp, x, a, b_lower, b_upper)}


def condensed_adjoint(cfg: ref.Config, inp: np.ndarray, xbar, fmbar=None) -> dict:
    """status, active, flags, x and the gradients (zero unless Solved), as adjoint_kernel_rt computes them"""
    N, HC, nvb = cfg.n_iter, cfg.control_horizon, cfg.n_vblocks
    nu, nv = NJ * HC, NTH * nvb
    nz, nxs = nu + nv, NX * (N + 1)
    M, S, s, gmax, vprev, (A, Bj, Bt, c, dts) = _schur(cfg, inp)
    Ljj, Lvj = np.tril(M[:nu, :nu]), M[nu:nz, :nu]
    vmin, vmax = ref.throttle_bounds(cfg)
    fixed = np.zeros(nv, dtype=bool)
    lo, hi = np.full(nv, vmin), np.full(nv, vmax)
    if inp[ref.IN_HOLD] != 0.0:
        fixed[:NTH] = True
        lo[:NTH] = hi[:NTH] = vprev
    v, status, _ = rm.box_qp(S, s, lo, hi, fixed, 1e-10 * (1.0 + gmax))
    active = sm.throttle_states(v, lo, hi, fixed)
    out = {"status": status, "active": active, "flags": UNSOLVED, "grad_x0": np.zeros(NX), "grad_cfg": np.zeros(GRAD_SIZE)}
    if status != rm.SOLVED:
        return out
    out["flags"] = degeneracy_flags(S, s, v, active, vmin, vmax)
    # the solution (P5, P6)
    u = np.linalg.solve(Ljj.T, -(Lvj.T @ v + M[nz, :nu]))
    jb = [ref.joint_block_of_stage(cfg, k) for k in range(N)]
    tb = [ref.throttle_block_of_stage(cfg, k) for k in range(N)]
    X = np.zeros((N + 1, NX))
    X[0] = inp[ref.IN_X0:ref.IN_X0 + NX]
    for k in range(N):
        X[k + 1] = X[k] + dts[k] * (A @ X[k] + Bj @ u[NJ * jb[k]:NJ * (jb[k] + 1)] + Bt @ v[NTH * tb[k]:NTH * (tb[k] + 1)] + c)
    x = np.concatenate([X.ravel(), u, v])
    out["x"] = x
    xb = fold_first_move(cfg, v[:NTH], xbar, fmbar)
    xbX, xbU, xbV = xb[:nxs].reshape(N + 1, NX), xb[nxs:nxs + nu].copy(), xb[nxs + nu:].copy()
    # 1: r = Z^T xbar, costate form
    rU, rV = xbU, xbV
    lam = xbX[N].copy()
    for k in range(N - 1, -1, -1):
        rU[NJ * jb[k]:NJ * (jb[k] + 1)] += dts[k] * (Bj.T @ lam)
        rV[NTH * tb[k]:NTH * (tb[k] + 1)] += dts[k] * (Bt.T @ lam)
        if k > 0:
            lam = xbX[k] + (lam + dts[k] * (A.T @ lam))
    # 2: one right-hand side through the factors
    w = np.linalg.solve(Ljj, rU)
    t = rV - Lvj @ w
    F = active == sm.FREE
    dv = np.zeros(nv)
    if F.any():
        K = S[np.ix_(F, F)].copy()
        assert rm._chol_partial(K, int(F.sum()))
        Lf = np.tril(K)
        dv[F] = np.linalg.solve(Lf.T, np.linalg.solve(Lf, t[F]))
    du = np.linalg.solve(Ljj.T, w - Lvj.T @ dv)
    # 3: state part of a
    aX = np.zeros((N + 1, NX))
    for k in range(N):
        aX[k + 1] = aX[k] + dts[k] * (A @ aX[k] + Bj @ du[NJ * jb[k]:NJ * (jb[k] + 1)] + Bt @ dv[NTH * tb[k]:NTH * (tb[k] + 1)])
    # 4: costates
    q = ref.state_weight(cfg)
    b = np.zeros((N, NX))
    b[N - 1] = q * aX[N] - xbX[N]
    for i in range(N - 1, 0, -1):
        b[i - 1] = q * aX[i] - xbX[i] + (b[i] + dts[i] * (A.T @ b[i]))
    out["grad_x0"] = xbX[0] - (b[0] + dts[0] * (A.T @ b[0]))
    aV = dv.reshape(nvb, NTH)
    hxV = np.zeros((nvb, NTH))
    for tt in range(nvb):
        if tt > 0:
            hxV[tt] += cfg.w_throttle * (aV[tt] - aV[tt - 1])
        if tt < nvb - 1:
            hxV[tt] += cfg.w_throttle * (aV[tt] - aV[tt + 1])
    hxV[0] += cfg.w_initial_throttle * aV[0]
    bt = np.zeros((nvb, NTH))
    for tt in range(nvb):
        ssum = sum((dts[i] * (Bt.T @ b[i]) for i in range(N) if tb[i] == tt), np.zeros(NTH))
        bt[tt] = xb[nxs + nu + NTH * tt:nxs + nu + NTH * (tt + 1)] - hxV[tt] - ssum
    bt = bt.ravel()
    # 5: contractions
    a = np.concatenate([aX.ravel(), du, dv])
    out["grad_cfg"] = _contractions(cfg, inp, x, a, float(bt[active == sm.LOWER].sum()), float(bt[active == sm.UPPER].sum()))
    return out
