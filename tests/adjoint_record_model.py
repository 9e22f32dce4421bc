"""Adjoint of the MPC solve with respect to EVERY entry of the input record -- the gradient of a scalar loss on the plan to
the reference window, the previous throttle, the linearisation point, the posture error and the model data -- two ways, for
tests/test_adjoint_record_model.py and tests/test_gpu_adjoint_record.py (adjoint_model.py has the gradients to X0 and the
gains and is imported, not changed):

  kkt_record_adjoint        the dense route.  K [a; b] = [xbar; 0] as in adjoint_model.kkt_adjoint, nu = the multipliers of
                            the equality and active rows (solve_exact's y), and for every record entry p
                                dL/dp = -a^T (dH/dp x + dg/dp + dE^T/dp nu) + b^T (de/dp - dE/dp x)
                            with dH, dg, dE, de from central differences of vsmpc_ref.assemble_dense ALONE (Richardson
                            extrapolated: the assembly is smooth, no active set is involved); e takes lo or hi by the
                            throttle's state.  grad_model: the same formula with A, Bj, Bt, c perturbed directly (the
                            assembly is affine in them: one difference is exact).  Owes nothing to the transposes below.
  condensed_record_adjoint  numpy mirror of adjoint_record_kernel_rt (csrc/vsmpc_rt_adjoint_record.hpp: rt_adj_model,
                            rt_adj_record) on the recursions of adjoint_model.condensed_adjoint: the solve's costates nu by
                            certify's recursion, G_A | G_Bj | G_Bt | G_c = dL/d(A, Bj, Bt, c) as sums of rank-one terms over
                            the stages, then the transpose of vsmpc_ref.linearize and the entries that reach the QP directly

Sign convention (assemble_dense's rows): (I + dt_k A) X_k - X_{k+1} + dt_k Bj U_jb(k) + dt_k Bt V_tb(k) = -dt_k c, so
    G_A = -sum_k dt_k (nu_k a_Xk^T + b_k X_k^T),   G_Bj, G_Bt likewise with (a_U, U), (a_V, V),   G_c = -sum_k dt_k b_k
grad_model is [1014]: A [26][26] | Bj [26][8] | Bt [26][4] | c [26], the layout of vsmpc_linearize_batch.
"""
from __future__ import annotations

import math

import numpy as np

import adjoint_model as am
import runtime_model as rm
import sensitivity_model as sm
import vsmpc_ref as ref

NX, NJ, NTH = ref.N_STATES, ref.N_JOINTS, ref.N_THRUSTS
GM_A, GM_BJ, GM_BT, GM_C = 0, NX * NX, NX * NX + NX * NJ, NX * NX + NX * NJ + NX * NTH
GRAD_MODEL_SIZE = GM_C + NX                                   # 1014
# (field, offset, length) of the record; XREF's length depends on the horizon (fields())
_FIXED = (("X0", 0, 26), ("MASS", 26, 1), ("WRB", 27, 9), ("OMEGA", 36, 3), ("ALPHA", 39, 1), ("GRAV", 40, 3), ("AMOM", 43, 24),
          ("LLIN", 67, 24), ("LANG", 91, 24), ("INERTIA", 115, 9), ("RPY", 124, 3), ("PREF", 127, 3), ("RPYINIT", 130, 3),
          ("T0", 133, 4), ("TD0", 137, 4), ("UPREV", 141, 4), ("TDES", 145, 4), ("TDDES", 149, 4), ("QERR", 153, 8),
          ("HOLD", 161, 1))
JET_FIELDS = ("T0", "TD0", "TDES", "TDDES")                   # zero gradient with use_jet_dynamic = False
MUTATIONS = ("drop_nu", "window_late", "drop_pin", "transpose_GA", "drop_dhT_T0")


def fields(cfg):
    """(name, offset, length) of every field of the record of this horizon"""
    return _FIXED + (("XREF", ref.IN_XREF, 12 * cfg.n_ref_cols),)


def dead(cfg):
    """entries no kernel reads: the yaw of IN_RPY and the last column of the window (record_cases.dead) -- where the window
    has more than one column: with n_iter == n_iter_small its only column is tracked by every node"""
    last = ref.IN_XREF + 12 * (cfg.n_ref_cols - 1)
    return [ref.IN_RPY + 2] + (list(range(last, last + 12)) if cfg.n_ref_cols > 1 else [])


def worst_field(got, want, fields, bar=1e-6, floor=1e-12):
    """the project's bar form on (name, offset, length) fields of a gradient: the worst |err| / (bar |field|_inf + floor
    max |want|) and the field it was found in"""
    gall = np.abs(want).max()
    worst, where = 0.0, None
    for name, off, n in fields:
        f = want[off:off + n]
        e = float(np.abs(got[off:off + n] - f).max() / (bar * np.abs(f).max() + floor * gall))
        if e > worst or where is None:
            worst, where = max(worst, e), name if e >= worst else where
    return worst, where


def field_errors(cfg, got_in, want_in, bar=1e-6, floor=1e-12):
    """worst_field over the fields of the record"""
    return worst_field(got_in, want_in, fields(cfg), bar, floor)[0]


# --------------------------------------------------------------------------------------------------------------------
# dense route
# --------------------------------------------------------------------------------------------------------------------
def _kkt(cfg, inp, xbar, fmbar):
    """x, nu, a, b, which rows take hi for e, the states of the throttles: nu and b over all rows of Ac, zero off E"""
    H, g, Ac, lo, hi = ref.assemble_dense(cfg, inp)
    x, y, _ = ref.solve_exact(cfg, H, g, Ac, lo, hi)
    nxs, nv = NX * (cfg.n_iter + 1), NTH * cfg.n_vblocks
    offV = cfg.off_throttle
    tlo, thi = lo[nxs:nxs + nv], hi[nxs:nxs + nv]
    active = sm.throttle_states(x[offV:offV + nv], tlo, thi, tlo == thi)
    act = np.nonzero(active != sm.FREE)[0]
    rows = np.concatenate([np.arange(nxs), nxs + act])
    upper = np.concatenate([np.zeros(nxs, dtype=bool), active[act] == sm.UPPER])
    n, m = H.shape[0], rows.size
    K = np.zeros((n + m, n + m))
    K[:n, :n] = H
    K[:n, n:] = Ac[rows].T
    K[n:, :n] = Ac[rows]
    rhs = np.zeros(n + m)
    rhs[:n] = am.fold_first_move(cfg, x[offV:offV + NTH], xbar, fmbar)
    sol = np.linalg.solve(K, rhs)
    nu, b, up = np.zeros(Ac.shape[0]), np.zeros(Ac.shape[0]), np.zeros(Ac.shape[0], dtype=bool)
    nu[rows], b[rows], up[rows] = y[rows], sol[n:], upper
    return x, nu, sol[:n], b, up, active


def _term(asm, x, k):
    """the formula on one difference quotient (dH, dg, dAc, dlo, dhi) of the assembly; k = _kkt()'s tuple, whose nu and b
    are spread over all rows of Ac (zero on the rows of free throttles)"""
    dH, dg, dAc, dlo, dhi = asm
    _, nu, a, b, upper, _ = k
    return float(-a @ (dH @ x + dg + dAc.T @ nu) + b @ (np.where(upper, dhi, dlo) - dAc @ x))


def _central(cfg, inp, i, h):
    p, m = inp.copy(), inp.copy()
    p[i] += h
    m[i] -= h
    return [(u - v) / (2.0 * h) for u, v in zip(ref.assemble_dense(cfg, p), ref.assemble_dense(cfg, m))]


# the fields the assembly is neither affine nor quadratic in, entry by entry: 1 / m, I^-1, sin / cos / tan.  For every
# other entry one central difference is exact up to rounding (test_adjoint_record_model.py checks that on a record).
NONLINEAR = ("MASS", "INERTIA", "RPY")


def kkt_record_adjoint(cfg: ref.Config, inp: np.ndarray, xbar, fmbar=None, model=False, step=1e-3, richardson=None) -> dict:
    """grad_in [n_in] (and grad_model [1014] with model=True), x, active.  Every entry's difference quotient is central with
    h = step max(1, |p|); for the NONLINEAR fields (or every field with richardson=True) a second one with h / 2 is
    Richardson extrapolated with it, O(h^4).  The hold flag is a switch: 0."""
    inp = np.asarray(inp, dtype=float)
    k = _kkt(cfg, inp, xbar, fmbar)
    x = k[0]
    grad = np.zeros(cfg.n_in)
    for name, off, n in fields(cfg):
        if name == "HOLD":
            continue
        twice = name in NONLINEAR if richardson is None else richardson
        for i in range(off, off + n):
            h = step * max(1.0, abs(inp[i]))
            grad[i] = _term(_central(cfg, inp, i, h), x, k)
            if twice:
                grad[i] = (4.0 * _term(_central(cfg, inp, i, 0.5 * h), x, k) - grad[i]) / 3.0
    out = {"x": x, "active": k[5], "grad_in": grad}
    if model:
        out["grad_model"] = _dense_model(cfg, inp, x, k)
    return out


def _dense_model(cfg, inp, x, k):
    """dL/d(A, Bj, Bt, c): assemble_dense with vsmpc_ref.linearize's result moved by one in one entry"""
    lin0 = ref.linearize(cfg, inp)
    base = ref.assemble_dense(cfg, inp)
    keep = ref.linearize
    g = np.zeros(GRAD_MODEL_SIZE)
    try:
        for e in range(GRAD_MODEL_SIZE):
            mats = [m.copy() for m in lin0]
            which = 0 if e < GM_BJ else 1 if e < GM_BT else 2 if e < GM_C else 3
            mats[which].reshape(-1)[e - (GM_A, GM_BJ, GM_BT, GM_C)[which]] += 1.0
            ref.linearize = lambda c_, i_, _m=tuple(mats): _m
            moved = ref.assemble_dense(cfg, inp)
            g[e] = _term([u - v for u, v in zip(moved, base)], x, k)
    finally:
        ref.linearize = keep
    return g


# --------------------------------------------------------------------------------------------------------------------
# mirror of the kernel
# --------------------------------------------------------------------------------------------------------------------
def _intermediates(cfg, inp, xbar, fmbar):
    """adjoint_model.condensed_adjoint's recursions with what they leave behind: X, U, V, a_X, a_U, a_V, b, b_init, b_t"""
    N, HC, nvb = cfg.n_iter, cfg.control_horizon, cfg.n_vblocks
    nu_, nv = NJ * HC, NTH * nvb
    nz, nxs = nu_ + nv, NX * (N + 1)
    M, S, s, gmax, vprev, (A, Bj, Bt, c, dts) = am._schur(cfg, inp)
    Ljj, Lvj = np.tril(M[:nu_, :nu_]), M[nu_:nz, :nu_]
    vmin, vmax = ref.throttle_bounds(cfg)
    fixed = np.zeros(nv, dtype=bool)
    lo, hi = np.full(nv, vmin), np.full(nv, vmax)
    hold = inp[ref.IN_HOLD] != 0.0
    if hold:
        fixed[:NTH] = True
        lo[:NTH] = hi[:NTH] = vprev
    v, status, _ = rm.box_qp(S, s, lo, hi, fixed, 1e-10 * (1.0 + gmax))
    active = sm.throttle_states(v, lo, hi, fixed)
    if status != rm.SOLVED:
        return None
    u = np.linalg.solve(Ljj.T, -(Lvj.T @ v + M[nz, :nu_]))
    jb = [ref.joint_block_of_stage(cfg, k) for k in range(N)]
    tb = [ref.throttle_block_of_stage(cfg, k) for k in range(N)]
    X = np.zeros((N + 1, NX))
    X[0] = inp[ref.IN_X0:ref.IN_X0 + NX]
    for k in range(N):
        X[k + 1] = X[k] + dts[k] * (A @ X[k] + Bj @ u[NJ * jb[k]:NJ * (jb[k] + 1)] + Bt @ v[NTH * tb[k]:NTH * (tb[k] + 1)] + c)
    xb = am.fold_first_move(cfg, v[:NTH], xbar, fmbar)
    xbX, rU, rV = xb[:nxs].reshape(N + 1, NX), xb[nxs:nxs + nu_].copy(), xb[nxs + nu_:].copy()
    lam = xbX[N].copy()
    for k in range(N - 1, -1, -1):
        rU[NJ * jb[k]:NJ * (jb[k] + 1)] += dts[k] * (Bj.T @ lam)
        rV[NTH * tb[k]:NTH * (tb[k] + 1)] += dts[k] * (Bt.T @ lam)
        if k > 0:
            lam = xbX[k] + (lam + dts[k] * (A.T @ lam))
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
    aX = np.zeros((N + 1, NX))
    for k in range(N):
        aX[k + 1] = aX[k] + dts[k] * (A @ aX[k] + Bj @ du[NJ * jb[k]:NJ * (jb[k] + 1)] + Bt @ dv[NTH * tb[k]:NTH * (tb[k] + 1)])
    q = ref.state_weight(cfg)
    b = np.zeros((N, NX))
    b[N - 1] = q * aX[N] - xbX[N]
    for i in range(N - 1, 0, -1):
        b[i - 1] = q * aX[i] - xbX[i] + (b[i] + dts[i] * (A.T @ b[i]))
    b_init = xbX[0] - (b[0] + dts[0] * (A.T @ b[0]))
    aV = dv.reshape(nvb, NTH)
    bt = np.zeros((nvb, NTH))
    for tt in range(nvb):
        hx = np.zeros(NTH)
        if tt > 0:
            hx += cfg.w_throttle * (aV[tt] - aV[tt - 1])
        if tt < nvb - 1:
            hx += cfg.w_throttle * (aV[tt] - aV[tt + 1])
        if tt == 0:
            hx += cfg.w_initial_throttle * aV[0]
        ssum = sum((dts[i] * (Bt.T @ b[i]) for i in range(N) if tb[i] == tt), np.zeros(NTH))
        bt[tt] = xb[nxs + nu_ + NTH * tt:nxs + nu_ + NTH * (tt + 1)] - hx - ssum
    return {"A": A, "dts": dts, "jb": jb, "tb": tb, "q": q, "hold": hold, "active": active, "X": X, "U": u.reshape(HC, NJ),
            "V": v.reshape(nvb, NTH), "aX": aX, "aU": du.reshape(HC, NJ), "aV": aV, "b": b, "b_init": b_init, "bt": bt}


def _dw_inverse(rpy):
    """d W^-1 / d roll, d W^-1 / d pitch of vsmpc_ref.w_inverse"""
    r, p = rpy[0], rpy[1]
    sr, cr, cp, tp = math.sin(r), math.cos(r), math.cos(p), math.tan(p)
    dr = np.array([[0.0, cr * tp, -sr * tp], [0.0, -sr, -cr], [0.0, cr / cp, -sr / cp]])
    dp = np.array([[0.0, sr / cp ** 2, cr / cp ** 2], [0.0, 0.0, 0.0], [0.0, sr * tp / cp, cr * tp / cp]])
    return dr, dp


def condensed_record_adjoint(cfg: ref.Config, inp: np.ndarray, xbar, fmbar=None, mutation=None) -> dict:
    """status-free mirror of the record phases: grad_in [n_in], grad_model [1014] (zeros unless Solved), active, solved.
    `mutation` (one of MUTATIONS) plants one defect, for the mutation tests only."""
    assert mutation is None or mutation in MUTATIONS
    inp = np.asarray(inp, dtype=float)
    out = {"solved": False, "grad_in": np.zeros(cfg.n_in), "grad_model": np.zeros(GRAD_MODEL_SIZE)}
    m = _intermediates(cfg, inp, xbar, fmbar)
    if m is None:
        return out
    N, nS, HC = cfg.n_iter, cfg.n_iter_small, cfg.control_horizon
    A, dts, jb, tb, q = m["A"], m["dts"], m["jb"], m["tb"], m["q"]
    X, U, V, aX, aU, aV, b = m["X"], m["U"], m["V"], m["aX"], m["aU"], m["aV"], m["b"]
    win = inp[ref.IN_XREF:ref.IN_XREF + 12 * cfg.n_ref_cols].reshape(cfg.n_ref_cols, 12)

    def column(i):                                             # window column of node i >= 1
        col = 0 if i - 1 < nS else i - 1 - nS
        return min(col + 1, cfg.n_ref_cols - 1) if mutation == "window_late" else col

    xr = np.zeros((N + 1, NX))
    for i in range(1, N + 1):
        xr[i, :12] = win[column(i)]
    # rt_adj_model: the solve's costates (certify's recursion) fused with the rank-one sums, stages N - 1 .. 0
    GA, GBj, GBt, Gc = np.zeros((NX, NX)), np.zeros((NX, NJ)), np.zeros((NX, NTH)), np.zeros(NX)
    nu = q * (X[N] - xr[N])
    for k in range(N - 1, -1, -1):
        nk = np.zeros(NX) if mutation == "drop_nu" else nu
        GA -= dts[k] * (np.outer(nk, aX[k]) + np.outer(b[k], X[k]))
        GBj -= dts[k] * (np.outer(nk, aU[jb[k]]) + np.outer(b[k], U[jb[k]]))
        GBt -= dts[k] * (np.outer(nk, aV[tb[k]]) + np.outer(b[k], V[tb[k]]))
        Gc -= dts[k] * b[k]
        if k > 0:
            nu = q * (X[k] - xr[k]) + (nu + dts[k] * (A.T @ nu))
    out["grad_model"] = np.concatenate([GA.ravel(), GBj.ravel(), GBt.ravel(), Gc])
    if mutation == "transpose_GA":
        GA = GA.T
    # rt_adj_record: direct entries, then the transpose of linearize
    g = out["grad_in"]
    g[ref.IN_X0:ref.IN_X0 + NX] = m["b_init"]
    for i in range(1, N + 1):
        col = column(i)
        g[ref.IN_XREF + 12 * col:ref.IN_XREF + 12 * col + 12] += q[:12] * aX[i, :12]
    g[ref.IN_QERR:ref.IN_QERR + NJ] = -cfg.w_reg_joint_pos * aU.sum(axis=0)
    c12, muT, sgT, muU, sgU = ref.JET_COEFF[12], *ref.JET_NORM
    up = inp[ref.IN_UPREV:ref.IN_UPREV + NTH]
    ub = (up - muU) / sgU
    dvdu = (1.0 + 2.0 * c12 * ub) / sgU
    pin = m["bt"][0] if (m["hold"] and mutation != "drop_pin") else np.zeros(NTH)
    g[ref.IN_UPREV:ref.IN_UPREV + NTH] = dvdu * (cfg.w_initial_throttle * aV[0] + pin)
    g[ref.IN_AMOM:ref.IN_AMOM + 24] = np.concatenate([GA[3:6, 12:16].ravel(), GA[9:12, 12:16].ravel()])
    g[ref.IN_LLIN:ref.IN_LLIN + 24] = GBj[3:6].ravel()
    g[ref.IN_LANG:ref.IN_LANG + 24] = GBj[9:12].ravel()
    g[ref.IN_PREF:ref.IN_PREF + 3] = -Gc[20:23]
    g[ref.IN_RPYINIT:ref.IN_RPYINIT + 3] = -Gc[23:26]
    mass, alpha = inp[ref.IN_MASS], inp[ref.IN_ALPHA]
    R = inp[ref.IN_WRB:ref.IN_WRB + 9].reshape(3, 3)
    grav = inp[ref.IN_GRAV:ref.IN_GRAV + 3]
    Gcom, Gcl = GA[0:3, 3:6], Gc[3:6]
    g[ref.IN_MASS] = -(Gcom * R).sum() / mass ** 2 + alpha * (Gcl @ (R.T @ grav))
    g[ref.IN_WRB:ref.IN_WRB + 9] = (Gcom / mass + alpha * mass * np.outer(grav, Gcl)).ravel()
    g[ref.IN_ALPHA] = mass * (Gcl @ (R.T @ grav))
    g[ref.IN_GRAV:ref.IN_GRAV + 3] = alpha * mass * (R @ Gcl)
    P = GA[3:6, 3:6] + GA[9:12, 9:12]                          # the two -S(omega) blocks
    g[ref.IN_OMEGA:ref.IN_OMEGA + 3] = [P[1, 2] - P[2, 1], P[2, 0] - P[0, 2], P[0, 1] - P[1, 0]]
    Gm = GA[6:9, 9:12]                                         # A[rpy, angMom] = W^-1(rpy) I^-1
    Iinv = np.linalg.inv(inp[ref.IN_INERTIA:ref.IN_INERTIA + 9].reshape(3, 3))
    Mm = ref.w_inverse(inp[ref.IN_RPY:ref.IN_RPY + 3]) @ Iinv
    Nm = Gm @ Iinv.T
    g[ref.IN_INERTIA:ref.IN_INERTIA + 9] = -(Mm.T @ Nm).ravel()
    dWr, dWp = _dw_inverse(inp[ref.IN_RPY:ref.IN_RPY + 3])
    g[ref.IN_RPY], g[ref.IN_RPY + 1] = (dWr * Nm).sum(), (dWp * Nm).sum()
    if cfg.use_jet_dynamic:
        co = ref.JET_COEFF
        for i in range(NTH):
            T0, Td0 = inp[ref.IN_T0 + i], inp[ref.IN_TD0 + i]
            ta, tb_ = (T0 - muT) / sgT, Td0 / sgT
            vv = ub[i] + c12 * ub[i] ** 2
            dfT, dfTd = co[1] + co[3] * tb_ + 2 * co[4] * ta, co[2] + co[3] * ta + 2 * co[5] * tb_
            dgT, dgTd = co[7] + co[9] * tb_ + 2 * co[10] * ta, co[8] + co[9] * ta + 2 * co[11] * tb_
            dhT, dhTd = dfT + dgT * vv, dfTd + dgTd * vv
            gc = Gc[16 + i]
            wT = GA[16 + i, 12 + i] - (0.0 if mutation == "drop_dhT_T0" else gc * T0)   # on dh/dT, through A and c
            wTd = GA[16 + i, 16 + i] - gc * Td0                                           # on dh/dTdot
            hTT, hTTd, hTdTd = (2 * co[4] + 2 * co[10] * vv) / sgT, (co[3] + co[9] * vv) / sgT, (2 * co[5] + 2 * co[11] * vv) / sgT
            g[ref.IN_T0 + i] = wT * hTT + wTd * hTTd + gc * (dfT - (0.0 if mutation == "drop_dhT_T0" else dhT))
            g[ref.IN_TD0 + i] = wT * hTTd + wTd * hTdTd + gc * (dfTd - dhTd)
            g[ref.IN_UPREV + i] += (wT * dgT + wTd * dgTd) * dvdu[i]
            da, db = (inp[ref.IN_TDES + i] - muT) / sgT, inp[ref.IN_TDDES + i] / sgT
            g[ref.IN_TDES + i] = GBt[16 + i, i] * (co[7] + co[9] * db + 2 * co[10] * da)
            g[ref.IN_TDDES + i] = GBt[16 + i, i] * (co[8] + co[9] * da + 2 * co[11] * db)
    out["solved"], out["active"] = True, m["active"]
    return out
