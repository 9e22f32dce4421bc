"""Executable model of certify_kernel (csrc/vsmpc_certify.hip): duals and KKT certificate of a given primal by the
structured route -- one backward costate recursion through A, the box multipliers as the leftover throttle gradient, the
joint gradient as the stationarity residual -- in numpy, written from the formulas of DESIGN.md ("Duals and certificate"),
not from oracle/vsmpc_ref.py solve_exact.  It uses the oracle's linearisation, time grid, weights and move-blocking maps
(the definitions of the QP) and nothing of its solver or of its dense matrices.

    y_{N-1} = Q (X_N - xr_N),   y_{i-1} = Q (X_i - xr_i) + (I + dt_i A)^T y_i,   y_init = -(I + dt_0 A)^T y_0
    mu_t    = -(gV_t + sum_{i: tb(i) = t} dt_i Bt^T y_i)
    stat_j  = (W_dq + w_reg I) U_j + w_reg q_err + sum_{i: jb(i) = j} dt_i Bj^T y_i
"""
import numpy as np

CERT_STATIONARITY, CERT_STAT_SCALE, CERT_PRIMAL, CERT_COMPLEMENTARITY, CERT_OBJECTIVE, CERT_DUAL_MAX = range(6)
CERT_SIZE = 8


HORIZONS = {"paper": (17, 7, 12), "h2x": (34, 14, 24), "odd": (21, 9, 15), "unlisted": (20, 5, 9)}
_cache = {}


def case_configs(ref, layout, name):
    """(MPCConfig, oracle Config) of a horizon of HORIZONS, paper weights (h2x: BASELINE.json's halved fast period)"""
    n, ns, hc = HORIZONS[name]
    extra = dict(period_small=0.0025) if name == "h2x" else {}
    return (layout.MPCConfig(n_iter=n, n_iter_small=ns, control_horizon=hc, **extra),
            ref.Config(n_iter=n, n_iter_small=ns, control_horizon=hc, **extra))


def oracle_cases(ref, synth, layout, name, workload, count):
    """[(record, x, y)] of oracle/vsmpc_ref.py solve_instance on the first `count` synthetic records of a workload:
    computed once per session and shared by the CPU and the GPU tests (left unchanged by both)"""
    key = (name, workload, count)
    if key not in _cache:
        cfg, rcfg = case_configs(ref, layout, name)
        out = []
        for rec in synth.make_batch(cfg, count, workload=workload):
            x, y, _, _ = ref.solve_instance(rcfg, rec)
            out.append((rec, x, y))
        _cache[key] = out
    return _cache[key]


def certify(ref, cfg, rec, x):
    """(y [n_con], cert [CERT_SIZE]) of the primal x for the record rec under the oracle configuration cfg"""
    N, nS, Hc, nvb = cfg.n_iter, cfg.n_iter_small, cfg.control_horizon, cfg.n_vblocks
    nx, nj, nt = ref.N_STATES, ref.N_JOINTS, ref.N_THRUSTS
    A, Bj, Bt, c = ref.linearize(cfg, rec)
    dt = ref.dt_schedule(cfg)
    q = ref.state_weight(cfg)
    X = x[:nx * (N + 1)].reshape(N + 1, nx)
    U = x[cfg.off_joints:cfg.off_joints + nj * Hc].reshape(Hc, nj)
    V = x[cfg.off_throttle:cfg.off_throttle + nt * nvb].reshape(nvb, nt)
    jb = [ref.joint_block_of_stage(cfg, i) for i in range(N)]
    tb = [ref.throttle_block_of_stage(cfg, i) for i in range(N)]
    xr = np.zeros((N + 1, nx))
    win = rec[ref.IN_XREF:ref.IN_XREF + 12 * cfg.n_ref_cols].reshape(cfg.n_ref_cols, 12)
    for i in range(1, N + 1):
        xr[i, :12] = win[0 if i - 1 < nS else i - 1 - nS]
    vprev = np.array([ref.v_of_throttle(rec[ref.IN_UPREV + k]) for k in range(nt)])
    vmin, vmax = ref.throttle_bounds(cfg)
    w_dq = np.asarray(cfg.w_delta_joint, dtype=float)
    w_reg, w_thr, w_init = cfg.w_reg_joint_pos, cfg.w_throttle, cfg.w_initial_throttle
    qerr = rec[ref.IN_QERR:ref.IN_QERR + nj]
    hold = rec[ref.IN_HOLD] != 0.0

    y = np.zeros(cfg.n_con)
    Y = y[:nx * N].reshape(N, nx)                 # views into y
    # costates
    Y[N - 1] = q * (X[N] - xr[N])
    for i in range(N - 1, 0, -1):
        Y[i - 1] = q * (X[i] - xr[i]) + (Y[i] + dt[i] * (A.T @ Y[i]))
    y[nx * N:nx * (N + 1)] = -(Y[0] + dt[0] * (A.T @ Y[0]))
    # throttle multipliers
    hxV = np.zeros((nvb, nt))
    gV = np.zeros((nvb, nt))
    for t in range(nvb):
        if t > 0:
            hxV[t] += w_thr * (V[t] - V[t - 1])
        if t < nvb - 1:
            hxV[t] += w_thr * (V[t] - V[t + 1])
    hxV[0] += w_init * V[0]
    gV[0] = -w_init * vprev
    mu = np.zeros((nvb, nt))
    for t in range(nvb):
        s = sum((dt[i] * (Bt.T @ Y[i]) for i in range(N) if tb[i] == t), np.zeros(nt))
        mu[t] = -(hxV[t] + gV[t] + s)
    r1 = nx * (N + 1)
    y[r1:r1 + nt * nvb] = mu.reshape(-1)

    # certificate
    stat, scale, prim, comp = 0.0, 1.0, 0.0, 0.0
    obj = 0.0
    for j in range(Hc):
        s = sum((dt[i] * (Bj.T @ Y[i]) for i in range(N) if jb[i] == j), np.zeros(nj))
        hx, g = (w_dq + w_reg) * U[j], w_reg * qerr
        stat = max(stat, np.abs(hx + g + s).max())
        scale = max(scale, np.abs(hx).max(), np.abs(g).max())
        obj += float(U[j] @ (0.5 * hx + g))
    for i in range(1, N + 1):
        hx, g = q * X[i], -q * xr[i]
        scale = max(scale, np.abs(hx).max(), np.abs(g).max())
        obj += float(X[i] @ (0.5 * hx + g))
    scale = max(scale, np.abs(hxV).max(), np.abs(gV).max())
    for t in range(nvb - 1):
        obj += 0.5 * w_thr * float((V[t] - V[t + 1]) @ (V[t] - V[t + 1]))
    obj += float(V[0] @ (0.5 * w_init * V[0] + gV[0]))
    for i in range(N):
        res = X[i] + dt[i] * (A @ X[i] + Bj @ U[jb[i]] + Bt @ V[tb[i]] + c) - X[i + 1]
        prim = max(prim, np.abs(res).max())
    prim = max(prim, np.abs(X[0] - rec[ref.IN_X0:ref.IN_X0 + nx]).max())
    for t in range(nvb):
        if hold and t == 0:
            prim = max(prim, np.abs(V[0] - vprev).max())
            continue
        prim = max(prim, np.maximum(0.0, np.maximum(vmin - V[t], V[t] - vmax)).max())
        comp = max(comp, np.maximum(np.maximum(mu[t], 0.0) * (vmax - V[t]), np.maximum(-mu[t], 0.0) * (V[t] - vmin)).max())
    cert = np.zeros(CERT_SIZE)
    cert[CERT_STATIONARITY], cert[CERT_STAT_SCALE], cert[CERT_PRIMAL] = stat, scale, prim
    cert[CERT_COMPLEMENTARITY], cert[CERT_OBJECTIVE], cert[CERT_DUAL_MAX] = comp, obj, np.abs(y).max()
    if not (np.isfinite(rec).all() and np.isfinite(x).all()):
        cert[CERT_STATIONARITY] = cert[CERT_PRIMAL] = np.nan
    return y, cert


def field_tolerances(H, g, Ac, x, y):
    """Absolute tolerances for comparing a certificate with oracle/vsmpc_ref.py kkt_certificate on the same (x, y), from the
    arithmetic alone (eps = 2^-52): two correctly rounded evaluations of the same real quantity by different routes.

    stationarity  every entry of Hx + g + Ac'y is a sum of at most 256 terms (26 rows x at most nIter - controlHorizon + 1
                  stages of the last joint block, plus the cost terms), each at most max(scale, |Ac|_max |y|_inf) in
                  magnitude: 256 eps of that per route.  The oracle's maximum also runs over the state and throttle
                  entries, which the structured route makes zero by construction and the dense one leaves at this same
                  rounding level -- covered by the same bound.
    primal        a row of Ac x has at most 26 + 26 + 8 + 4 = 64 terms of magnitude at most |Ac|_max |x|_inf; the oracle's
                  previous-throttle and limit warps differ from the device's by one fused multiply-add (2 ulp of a value
                  below |x|_inf, inside the same bound).
    complementarity  the product y (hi - v): y is the same number on both sides; the slack differs by the rounding of the
                  warped limits, at most 4 ulp of max(1, |x|_inf).
    objective     relative to max(1, |obj|, x'Hx / 2): both are sums of at most 2 n_var terms whose magnitudes add up to
                  at most 4 times that scale (g'x cancels against the quadratic term): 8 n_var eps.
    """
    eps = np.finfo(float).eps
    amax = max(1.0, float(np.abs(Ac).max()))
    xmax = max(1.0, float(np.abs(x).max()))
    ymax = max(1.0, float(np.abs(y).max()))
    scale = max(1.0, float(np.abs(g).max()), float(np.abs(H @ x).max()))
    return {
        "stationarity": 2 * 256 * eps * max(scale, amax * ymax),
        "primal": 2 * 64 * eps * amax * xmax,
        "complementarity": 8 * eps * xmax * ymax,
        "objective_rel": 8 * x.size * eps,
    }
