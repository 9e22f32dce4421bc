"""Executable numpy model of the runtime-sized solve kernel (csrc/vsmpc_rt_core.hpp, driver in csrc/vsmpc_runtime.hip), step for step:

  P1  sensitivity recursion of every condensed column (joints 8 per block, throttles in the reference order, then the
      affine column), Y_k = sqrt(Q) (X_k - xref_k) on the 18 weighted rows, C = sum_k Y_k^T Y_k
  P2  input costs and gradient row
  P3  Cholesky of the joint columns only -> throttle Schur complement S and reduced gradient s in the trailing block
  P4  block principal pivoting on (S, s): each iteration factors S_FF of the free throttles and solves
  P5  joints from L_jj^T u = -(L_vj^T v + l_j)
  P6  state trajectory by forward simulation, primal in the reference order

Checked against oracle/vsmpc_ref.solve_instance by tests/test_runtime_model.py (CPU).
"""
from __future__ import annotations

import numpy as np

import vsmpc_ref as ref

NX, NJ, NTH = ref.N_STATES, ref.N_JOINTS, ref.N_THRUSTS
WROWS = list(range(12)) + list(range(20, 26))
PATIENCE = 10
MAX_ITER = 64          # DevCfg::max_as_iter
SOLVED, MAX_ITER_STATUS, NUMERICAL = 1, 2, 3


def _chol_partial(M: np.ndarray, ncols: int) -> bool:
    """Right-looking Cholesky of the first `ncols` columns of the symmetric M (lower triangle used), in place."""
    n = M.shape[0]
    for j in range(ncols):
        piv = M[j, j]
        if not piv > 0.0:
            return False
        l = np.sqrt(piv)
        M[j + 1:, j] /= l
        M[j, j] = l
        col = M[j + 1:, j]
        M[j + 1:, j + 1:] -= np.tril(np.outer(col, col))
    return True


def condense(cfg: ref.Config, inp: np.ndarray):
    """Augmented condensed matrix (lower triangle) and max |gradient|; unknowns [U | v | 1]."""
    N, nS, HC = cfg.n_iter, cfg.n_iter_small, cfg.control_horizon
    A, Bj, Bt, c = ref.linearize(cfg, inp)
    dts = ref.dt_schedule(cfg)
    sq = np.sqrt(ref.state_weight(cfg))[WROWS]
    nu, nv = NJ * HC, NTH * cfg.n_vblocks
    nz = nu + nv
    X = np.zeros((NX, nz + 1))
    X[:, nz] = inp[ref.IN_X0:ref.IN_X0 + NX]
    xref = inp[ref.IN_XREF:ref.IN_XREF + 12 * cfg.n_ref_cols].reshape(cfg.n_ref_cols, 12)
    C = np.zeros((nz + 1, nz + 1))
    for k in range(N):
        Bk = np.zeros((NX, nz + 1))
        jb, tb = ref.joint_block_of_stage(cfg, k), ref.throttle_block_of_stage(cfg, k)
        Bk[:, NJ * jb:NJ * (jb + 1)] = Bj
        Bk[:, nu + NTH * tb:nu + NTH * (tb + 1)] = Bt
        Bk[:, nz] = c
        X = X + dts[k] * (A @ X + Bk)
        i = k + 1
        col = 0 if (i - 1) < nS else (i - 1) - nS
        R = X[WROWS, :].copy()
        R[:12, nz] -= xref[col]
        Y = sq[:, None] * R
        C += Y.T @ Y
    # input costs (costsVSMPC.cpp:375-409,468-487,558-592)
    wj = np.asarray(cfg.w_delta_joint, dtype=float) + cfg.w_reg_joint_pos
    qerr = inp[ref.IN_QERR:ref.IN_QERR + NJ]
    vprev = np.array([ref.v_of_throttle(inp[ref.IN_UPREV + r]) for r in range(NTH)])
    for j in range(nu):
        C[j, j] += wj[j % NJ]
        C[nz, j] += cfg.w_reg_joint_pos * qerr[j % NJ]
    nvb = cfg.n_vblocks
    for q in range(nv):
        p, b, r = nu + q, q // NTH, q % NTH
        C[p, p] += cfg.w_throttle * ((b < nvb - 1) + (b > 0))
        if b == 0:
            C[p, p] += cfg.w_initial_throttle
            C[nz, p] += -cfg.w_initial_throttle * vprev[r]
        if b > 0:
            C[p, p - NTH] -= cfg.w_throttle
    gmax = float(np.abs(C[nz, :nz]).max())
    return np.tril(C), gmax, vprev, (A, Bj, Bt, c, dts)


def box_qp(S, s, lo, hi, fixed, gtol, max_iter=MAX_ITER):
    """Block principal pivoting on min 1/2 v'Sv + s'v, lo <= v <= hi (the kernel's P4). Returns v, status, iterations."""
    n = s.size
    state = np.where(fixed, -1, 0)
    v = np.zeros(n)
    best, patience = n + 1, PATIENCE
    for it in range(max_iter):
        B = state != 0
        v[state == -1] = lo[state == -1]
        v[state == 1] = hi[state == 1]
        F = np.nonzero(~B)[0]
        if F.size:
            rhs = -(s[F] + S[np.ix_(F, np.nonzero(B)[0])] @ v[B])
            K = S[np.ix_(F, F)].copy()
            if not _chol_partial(K, F.size):
                return v, NUMERICAL, it + 1
            L = np.tril(K)
            y = np.linalg.solve(L, rhs)
            v[F] = np.linalg.solve(L.T, y)
        grad = S @ v + s
        tol = 1e-12 * (1.0 + np.abs(v))
        vlo = (state == 0) & (v < lo - tol)
        vhi = (state == 0) & (v > hi + tol)
        rel = ~fixed & (((state == -1) & (grad < -gtol)) | ((state == 1) & (grad > gtol)))
        inf = vlo | vhi | rel
        ninf = int(inf.sum())
        if ninf == 0:
            return v, SOLVED, it + 1
        if ninf < best:
            best, patience = ninf, PATIENCE
            pick = inf
        elif patience > 0:
            patience -= 1
            pick = inf
        else:
            pick = np.zeros(n, dtype=bool)
            pick[np.nonzero(inf)[0].max()] = True
        state[pick & vlo] = -1
        state[pick & vhi] = 1
        state[pick & rel] = 0
    v[state == -1] = lo[state == -1]
    v[state == 1] = hi[state == 1]
    return v, MAX_ITER_STATUS, max_iter


def solve(cfg: ref.Config, inp: np.ndarray):
    """x (reference order), first-move block, status, active-set iterations."""
    HC = cfg.control_horizon
    nu, nv = NJ * HC, NTH * cfg.n_vblocks
    nz = nu + nv
    M, gmax, vprev, (A, Bj, Bt, c, dts) = condense(cfg, inp)
    if not _chol_partial(M, nu):
        raise FloatingPointError("non-positive joint pivot")
    S = M[nu:nz, nu:nz]
    S = np.tril(S) + np.tril(S, -1).T
    s = M[nz, nu:nz].copy()
    vmin, vmax = ref.throttle_bounds(cfg)
    hold = inp[ref.IN_HOLD] != 0.0
    fixed = np.zeros(nv, dtype=bool)
    lo, hi = np.full(nv, vmin), np.full(nv, vmax)
    if hold:
        fixed[:NTH] = True
        lo[:NTH] = hi[:NTH] = vprev
    v, status, iters = box_qp(S, s, lo, hi, fixed, 1e-10 * (1.0 + gmax))
    Ljj = np.tril(M[:nu, :nu])
    u = np.linalg.solve(Ljj.T, -(M[nu:nz, :nu].T @ v + M[nz, :nu]))
    X = np.zeros((cfg.n_iter + 1, NX))
    X[0] = inp[ref.IN_X0:ref.IN_X0 + NX]
    for k in range(cfg.n_iter):
        jb, tb = ref.joint_block_of_stage(cfg, k), ref.throttle_block_of_stage(cfg, k)
        X[k + 1] = X[k] + dts[k] * (A @ X[k] + Bj @ u[NJ * jb:NJ * (jb + 1)] + Bt @ v[NTH * tb:NTH * (tb + 1)] + c)
    x = np.concatenate([X.ravel(), u, v])
    return x, ref.first_move_vector(cfg, x), status, iters
