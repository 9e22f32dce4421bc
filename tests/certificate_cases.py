"""Primals for certify_kernel (csrc/vsmpc_certify.hip) away from the optimum (plain helper module, imported by tests).

At an optimum STATIONARITY, PRIMAL and COMPLEMENTARITY are rounding noise and four of the six certificate fields are maxima,
which see their largest entry only: a kernel that skips rows, blocks or a second pass of a strided loop reports too little
and nothing notices.  The cases here put a known value on a chosen row.  Everything is built from the definitions of the QP
(oracle/vsmpc_ref.py linearize, dt_schedule, the move-blocking maps, the weights) and from tests/certificate_model.py; the
device is never read.

  offopt        random primals: states X0 (1 + 0.3 N) per node, joints 0.05 N, throttles uniform over the box widened by 20 %
                on each side, and three variants with the states, the joints, the throttles times 1e3 (STAT_SCALE's maximum
                sits in each class in turn).  Pins OBJECTIVE (a sum), STAT_SCALE, DUAL_MAX and the whole of y.
  spotlights    one row or entry carries the maximum and the value is known in closed form:
                  primal_dyn (i, r)     X simulated exactly, a defect delta put into X_{i+1}[r]
                  primal_init r         X_0 = x0 - delta e_r
                  primal_box (t, k, +-) V_t[k] = vmax + delta or vmin - delta (filled, non-pinned blocks)
                  primal_pin k          a held record with V_0[k] = vprev + delta
                  stat (j, k)           any X; U chosen so that every joint gradient is rounding, then d / (w_dq[k] + w_reg)
                                        added at (j, k): STATIONARITY = d = 1e-3 |sum dt Bj^T y|_max
                  comp (t, k, +-)       any X; mu is affine in V (probed through the model), V solved so that mu = m e_(t,k)
                                        on the non-pinned entries: COMPLEMENTARITY = |m| (vmax - v) or |m| (v - vmin)
  pinned        a held record with V_0 != vprev, mu = m e_(t,k) on the non-pinned entries and large multipliers on the
                pinned block: COMPLEMENTARITY must leave that block out
  optimum       x, y of the oracle's solve_instance on the tie-broken records of tests/record_cases.py
"""
import numpy as np

import certificate_model as cm
import config_cases as cc
import record_cases as rc

S, SC, P, C, O, D = range(6)
FIELD = {S: "stationarity", P: "primal", C: "complementarity"}
TUNED = [(17, 7, 12), (21, 9, 15), (34, 14, 24)]
RUNTIME = [(20, 5, 9), (6, 2, 3), (2, 2, 2), (12, 12, 12), (40, 2, 2), (40, 2, 40)]
HORIZONS = TUNED + RUNTIME
EXHAUSTIVE = [(6, 2, 3), (2, 2, 2)]
DELTA = 1e-3               # primal defects (the exactly simulated rows are at 1e-13)
M_COMP = 50.0              # the spotlighted multiplier
EDGE_RECORDS = ("hold_-1", "hold_1e-300", "hold_-0.0", "pitch_1.45_roll_0.7", "lateral_30m")
TUNABLE_SETTINGS = [{}, dict(throttle_min=10.0, throttle_max=90.0), dict(w_delta_joint=cc.JOINT_SPREAD),
                    {k: v for k, v in cc.ALL_DISTINCT.items() if not k.startswith("period")},
                    {k: v for k, v in cc.NON_DEFAULT.items() if not k.startswith("period")}]
_cache = {}


def settings_of(horizon, config):
    return {"default": {}, "non_default": cc.NON_DEFAULT, "all_distinct": cc.all_distinct(horizon)}[config]


def config_names(horizon):
    return ["default", "non_default"] + (["all_distinct"] if tuple(horizon) in TUNED else [])


class Problem:
    """the definitions of the QP of one (configuration, record) pair"""

    def __init__(self, ref, cfg, rec):
        self.ref, self.cfg, self.rec = ref, cfg, rec
        self.N, self.Hc, self.nvb = cfg.n_iter, cfg.control_horizon, cfg.n_vblocks
        self.A, self.Bj, self.Bt, self.c = ref.linearize(cfg, rec)
        self.dt = ref.dt_schedule(cfg)
        self.jb = [ref.joint_block_of_stage(cfg, i) for i in range(self.N)]
        self.tb = [ref.throttle_block_of_stage(cfg, i) for i in range(self.N)]
        self.vprev = np.array([ref.v_of_throttle(rec[ref.IN_UPREV + k]) for k in range(4)])
        self.vmin, self.vmax = ref.throttle_bounds(cfg)
        self.hold = bool(rec[ref.IN_HOLD] != 0.0)
        self.x0 = rec[:26].copy()
        self.w = np.asarray(cfg.w_delta_joint, dtype=float) + cfg.w_reg_joint_pos
        self.qerr = rec[ref.IN_QERR:ref.IN_QERR + 8]
        self.r1 = 26 * (self.N + 1)

    def simulate(self, U, V, X0=None, defect=None):
        X = np.empty((self.N + 1, 26))
        X[0] = self.x0 if X0 is None else X0
        for i in range(self.N):
            X[i + 1] = X[i] + self.dt[i] * (self.A @ X[i] + self.Bj @ U[self.jb[i]] + self.Bt @ V[self.tb[i]] + self.c)
            if defect is not None and defect[0] == i:
                X[i + 1, defect[1]] += defect[2]
        return X

    def pack(self, X, U, V):
        return np.concatenate([X.reshape(-1), U.reshape(-1), V.reshape(-1)])

    def inside(self, rng):
        """(U, V): joints 0.05 N, throttles strictly inside the box, V_0 = vprev on a held record"""
        U = 0.05 * rng.normal(size=(self.Hc, 8))
        V = rng.uniform(self.vmin + 0.1 * (self.vmax - self.vmin), self.vmax - 0.1 * (self.vmax - self.vmin), size=(self.nvb, 4))
        if self.hold:
            V[0] = self.vprev
        return U, V

    def states(self, rng):
        return self.x0[None, :] * (1.0 + 0.3 * rng.normal(size=(self.N + 1, 26)))

    def model(self, x):
        return cm.certify(self.ref, self.cfg, self.rec, x)


def _case(family, name, rec_name, pb, x, closed=None, row=None, y_ref=None):
    return dict(family=family, name=name, rec_name=rec_name, rec=pb.rec, x=x, closed=closed or {}, row=row, y_ref=y_ref)


def offopt(pb, rec_name, rng, scaled=False):
    out = []
    for variant in (("plain",) + (("states", "joints", "throttles") if scaled else ())):
        X = pb.states(rng)
        U = 0.05 * rng.normal(size=(pb.Hc, 8))
        w = pb.vmax - pb.vmin
        V = rng.uniform(pb.vmin - 0.2 * w, pb.vmax + 0.2 * w, size=(pb.nvb, 4))
        X, U, V = (X * 1e3 if variant == "states" else X, U * 1e3 if variant == "joints" else U,
                   V * 1e3 if variant == "throttles" else V)
        out.append(_case("offopt", variant, rec_name, pb, pb.pack(X, U, V)))
    return out


def primal_dyn(pb, rec_name, rng, i, r):
    U, V = pb.inside(rng)
    x = pb.pack(pb.simulate(U, V, defect=(i, r, DELTA)), U, V)
    return _case("primal_dyn", f"stage {i} row {r}", rec_name, pb, x, {P: DELTA}, (P, 26 * i + r))


def primal_init(pb, rec_name, rng, r):
    U, V = pb.inside(rng)
    X0 = pb.x0.copy()
    X0[r] -= DELTA
    return _case("primal_init", f"row {r}", rec_name, pb, pb.pack(pb.simulate(U, V, X0=X0), U, V), {P: DELTA}, (P, 26 * pb.N + r))


def primal_box(pb, rec_name, rng, t, k, side):
    assert not (pb.hold and t == 0)
    U, V = pb.inside(rng)
    V[t, k] = pb.vmax + DELTA if side > 0 else pb.vmin - DELTA
    want = V[t, k] - pb.vmax if side > 0 else pb.vmin - V[t, k]
    return _case("primal_box", f"block {t} jet {k} side {side:+d}", rec_name, pb, pb.pack(pb.simulate(U, V), U, V), {P: want},
                 (P, pb.r1 + 4 * t + k))


def primal_pin(pb, rec_name, rng, k):
    assert pb.hold
    U, V = pb.inside(rng)
    V[0, k] = pb.vprev[k] + DELTA
    return _case("primal_pin", f"jet {k}", rec_name, pb, pb.pack(pb.simulate(U, V), U, V), {P: V[0, k] - pb.vprev[k]},
                 (P, pb.r1 + k))


def _stat_base(pb, rng):
    """(X, V, U0, d): with U0 every joint gradient is rounding; d = 1e-3 |s|_max"""
    X = pb.states(rng)
    _, V = pb.inside(rng)
    y, _ = pb.model(pb.pack(X, np.zeros((pb.Hc, 8)), V))               # y depends on the states alone
    Y = y[:26 * pb.N].reshape(pb.N, 26)
    s = np.zeros((pb.Hc, 8))
    for i in range(pb.N):
        s[pb.jb[i]] += pb.dt[i] * (pb.Bj.T @ Y[i])
    U0 = -(pb.cfg.w_reg_joint_pos * pb.qerr[None, :] + s) / pb.w[None, :]
    return X, V, U0, 1e-3 * float(np.abs(s).max())


def stat(pb, rec_name, base, j, k):
    X, V, U0, d = base
    U = U0.copy()
    U[j, k] += d / pb.w[k]
    return _case("stat", f"block {j} joint {k}", rec_name, pb, pb.pack(X, U, V), {S: d}, (S, pb.cfg.off_joints + 8 * j + k))


def _comp_base(pb, rng):
    """(X, U, mu0, T): mu = mu0 - T V on the throttle entries, probed through the model at V = 0 and V = e_j.  The throttles
    that make mu = 0 must lie well inside the box for the spotlights to be solvable there, and the costates push them by
    sum dt Bt^T y / w_throttle: the weighted state rows are the node's reference (1 + sigma N) + sigma N with the largest
    sigma of 0.3, 0.03, ... that keeps them inside (the rows without a weight, which y does not see, stay X0 (1 + 0.3 N))."""
    U = 0.05 * rng.normal(size=(pb.Hc, 8))
    n = 4 * pb.nvb
    X0 = pb.states(rng)
    noise = rng.normal(size=(2, pb.N + 1, 26))
    xr = np.zeros((pb.N + 1, 26))
    win = pb.rec[pb.ref.IN_XREF:pb.ref.IN_XREF + 12 * pb.cfg.n_ref_cols].reshape(pb.cfg.n_ref_cols, 12)
    for i in range(1, pb.N + 1):
        xr[i, :12] = win[0 if i - 1 < pb.cfg.n_iter_small else i - 1 - pb.cfg.n_iter_small]
    weighted = list(range(12)) + list(range(20, 26))
    for sigma in (0.3, 0.03, 3e-3, 3e-4, 3e-5, 3e-6):
        X = X0.copy()
        X[1:, weighted] = (xr * (1.0 + sigma * noise[0]) + sigma * noise[1])[1:, weighted]

        def mu(V):
            return pb.model(pb.pack(X, U, V.reshape(pb.nvb, 4)))[0][pb.r1:pb.r1 + n]
        mu0 = mu(np.zeros(n))
        T = np.column_stack([mu0 - mu(np.eye(n)[j]) for j in range(n)])
        base = (X, U, mu0, T)
        V, _ = _solve_v(pb, base, pb.nvb - 1, 0, 0.0, check=False)
        margin = 0.05 * (pb.vmax - pb.vmin)
        free = V[1:] if pb.hold else V
        if (free > pb.vmin + margin).all() and (free < pb.vmax - margin).all():
            return base
    raise AssertionError("no states keep the throttles of mu = 0 inside the box")


def _solve_v(pb, base, t, k, m, v0=None, check=True):
    X, U, mu0, T = base
    n = 4 * pb.nvb
    free = np.ones(n, dtype=bool)
    V = np.zeros(n)
    if pb.hold:
        free[:4] = False
        V[:4] = pb.vprev if v0 is None else v0
    e = np.zeros(n)
    e[4 * t + k] = m
    V[free] = np.linalg.solve(T[np.ix_(free, free)], (mu0 - e - T[:, ~free] @ V[~free])[free])
    v = V[4 * t + k]
    lo, hi = pb.vmin, pb.vmax
    assert not check or ((V[free] > lo).all() and (V[free] < hi).all()), "the solved throttles left the box"
    return V.reshape(pb.nvb, 4), abs(m) * (hi - v if m > 0 else v - lo)


def comp(pb, rec_name, base, t, k, side):
    assert not (pb.hold and t == 0)
    V, want = _solve_v(pb, base, t, k, side * M_COMP)
    return _case("comp", f"block {t} jet {k} side {side:+d}", rec_name, pb, pb.pack(base[0], base[1], V), {C: want},
                 (C, pb.r1 + 4 * t + k))


def pinned(pb, rec_name, base, t, k, side, kp, delta=0.05):
    """V_0[kp] = vprev + delta on a held record: counts in PRIMAL, not in COMPLEMENTARITY"""
    assert pb.hold and t > 0
    v0 = pb.vprev.copy()
    v0[kp] += delta
    V, want = _solve_v(pb, base, t, k, side * M_COMP, v0=v0)
    return _case("pinned", f"block {t} jet {k} side {side:+d}, V_0[{kp}] off", rec_name, pb, pb.pack(base[0], base[1], V),
                 {C: want}, (C, pb.r1 + 4 * t + k))


def positions(cfg):
    """(stages, joint blocks, throttle blocks) of the by-class coverage"""
    N, nS, Hc, nvb = cfg.n_iter, cfg.n_iter_small, cfg.control_horizon, cfg.n_vblocks
    stages = sorted({i for i in (0, nS - 1, nS, Hc - 1, Hc, N - 1) if 0 <= i < N})
    joints = sorted({0, Hc // 2, Hc - 1})
    throttles = sorted({t for t in (0, 1, nvb // 2, nvb - 1) if 0 <= t < nvb})
    return stages, joints, throttles


def spotlights(ref, rcfg, recs, rng, exhaustive, thin=False):
    """recs: {name: record}, one free and one held.  exhaustive: every row and entry; otherwise by class at positions(),
    all 26 state rows, 8 joints and 4 jets at each (thin: a few of them)"""
    N, Hc, nvb = rcfg.n_iter, rcfg.control_horizon, rcfg.n_vblocks
    stages, joints, throttles = (range(N), range(Hc), range(nvb)) if exhaustive else positions(rcfg)
    rows, jn, jets = ((0, 5, 11, 12, 19, 20, 25), (0, 7), (0, 3)) if thin else (range(26), range(8), range(4))
    out = []
    for name, rec in recs.items():
        pb = Problem(ref, rcfg, rec)
        primary = not pb.hold or exhaustive           # by class, the held record takes what the hold changes
        if primary:
            out += [primal_dyn(pb, name, rng, i, r) for i in stages for r in rows]
            out += [primal_init(pb, name, rng, r) for r in rows]
            base = _stat_base(pb, rng)
            out += [stat(pb, name, base, j, k) for j in joints for k in jn]
        else:
            out += [primal_dyn(pb, name, rng, i, r) for i in (stages[0], stages[-1]) for r in (12, 16, 19)]
        free_blocks = [t for t in throttles if not (pb.hold and t == 0)]
        out += [primal_box(pb, name, rng, t, k, s) for t in free_blocks for k in jets for s in (1, -1)]
        if pb.hold:
            out += [primal_pin(pb, name, rng, k) for k in range(4)]
        if free_blocks:
            base = _comp_base(pb, rng)
            out += [comp(pb, name, base, t, k, s) for t in free_blocks for k in jets for s in (1, -1)]
            if pb.hold:
                out += [pinned(pb, name, base, free_blocks[-1], 2, 1, kp) for kp in (0, 3)]
                out += [pinned(pb, name, base, free_blocks[0], 1, -1, 2)]
    return out


def optima(ref, rcfg, names, recs):
    out = []
    for name, rec in zip(names, recs):
        x, y, _, _ = ref.solve_instance(rcfg, rec)
        out.append(_case("optimum", "oracle", name, Problem(ref, rcfg, rec), x, y_ref=y))
    return out


def cases(ref, horizon, config):
    """[case] of a horizon under a configuration of config_names(): computed once per session, left unchanged by the tests.
    A case is a dict: family, name, rec_name, rec, x, closed {field: closed-form value}, row (field, the oracle row or entry
    that must carry the maximum) and, for an optimum, y_ref."""
    key = (tuple(horizon), config)
    if key in _cache:
        return _cache[key]
    horizon = tuple(horizon)
    cfg, rcfg = cc.configs(ref, horizon, settings_of(horizon, config))
    names, recs = rc.records(cfg)
    by_name = dict(zip(names, recs))
    rng = np.random.default_rng(1000 * horizon[0] + 10 * horizon[2] + len(config))
    out = []
    chosen = [f"all_distinct_{i}" for i in range(6)] + list(EDGE_RECORDS)
    for n in chosen:
        out += offopt(Problem(ref, rcfg, by_name[n]), n, rng, scaled=n in ("all_distinct_0", "all_distinct_1"))
    pair = {n: by_name[n] for n in ("all_distinct_0", "all_distinct_1")}
    out += spotlights(ref, rcfg, pair, rng, horizon in EXHAUSTIVE, thin=config != "default" and horizon not in EXHAUSTIVE)
    if config == "default":
        out += optima(ref, rcfg, names, recs)
    else:
        out += optima(ref, rcfg, chosen[:6], [by_name[n] for n in chosen[:6]])
    _cache[key] = out
    return out


def boxqp_cases(ref):
    """(cfg, rcfg, [case]): table H34 of tests/boxqp_pass_cases.py at (34, 14, 24), 44 throttles with lower and upper bounds
    active at the optimum; the oracle's optimum and one off-optimum primal per record"""
    import boxqp_pass_cases as bp
    if "H34" not in _cache:
        cfg, rcfg, recs = bp.batch(ref, "H34")
        rng = np.random.default_rng(34)
        names = [f"H34_{w}_{i}" for w, i, _, _ in bp.TABLES["H34"][2]]
        out = optima(ref, rcfg, names, recs)
        for n, rec in zip(names, recs):
            out += offopt(Problem(ref, rcfg, rec), n, rng)
        _cache["H34"] = (cfg, rcfg, out)
    return _cache["H34"]


def tunable_cases(ref, horizon=cc.PAPER):
    """[(MPCConfig, oracle Config, case)]: one batch for per-instance rows, len(TUNABLE_SETTINGS) distinct rows in it"""
    key = ("tunables", tuple(horizon))
    if key in _cache:
        return _cache[key]
    rng = np.random.default_rng(5150)
    out = []
    base_cfg, _ = cc.configs(ref, horizon, {})
    names, recs = rc.records(base_cfg)
    by_name = dict(zip(names, recs))
    for w, s in enumerate(TUNABLE_SETTINGS):
        cfg, rcfg = cc.configs(ref, horizon, s)
        pair = {n: by_name[n] for n in ("all_distinct_0", "all_distinct_1")}
        group = spotlights(ref, rcfg, pair, rng, False, thin=True)
        for n in ("all_distinct_2", "all_distinct_3", "hold_-0.0"):
            group += offopt(Problem(ref, rcfg, by_name[n]), n, rng, scaled=n == "all_distinct_2")
        group += optima(ref, rcfg, ["all_distinct_4", "all_distinct_5"], [by_name["all_distinct_4"], by_name["all_distinct_5"]])
        out += [(cfg, rcfg, c) for c in group]
    _cache[key] = out
    return out


# ---- the reference values of a case

ROW_CLASSES = [f"costate row {r}" for r in range(26)] + ["initial rows", "throttle rows"]
# Off the optimum y has no oracle value; the float64 model is measured per row class against the same recursion in
# np.longdouble (duals_longdouble), relative to max(1, |y|_max of the class).  Ceilings on the worst figure over every case of
# this module (tests/test_certificate_cases.py asserts them; measured 1.44e-14 and 1.65e-11, profiles/certificate_cases.txt),
# for the 27 classes of costate and initial rows and for the throttle rows, whose multiplier is what is left of terms of size
# w_throttle |v| (the spotlights make it 50 out of 1e5).  Y_BAR, the device's bars: 100 times the ceilings (the kernel uses
# fused multiply-adds and two partial chains per sum: a small factor, not orders of magnitude), never looser than 1e-8.
Y_WORST_COSTATE, Y_WORST_THROTTLE = 1.5e-14, 1.7e-11
Y_MODEL_WORST = np.array([Y_WORST_COSTATE] * 27 + [Y_WORST_THROTTLE])
Y_BAR = np.minimum(1e-8, 100 * Y_MODEL_WORST)


def certified_margins(cert, x):
    """the three relative tests of solver.certified, each as a multiple of its right-hand side at tol = 1"""
    return np.array([cert[S] / cert[SC], cert[P] / max(1.0, float(np.abs(x).max())), cert[C] / max(1.0, cert[D])])


def class_errors(rcfg, y, y_want):
    """|y - y_want|_inf / max(1, |y_want|_inf of the class) per row class of ROW_CLASSES"""
    N = rcfg.n_iter
    Y, Yw = y[:26 * N].reshape(N, 26), y_want[:26 * N].reshape(N, 26)
    out = [float(np.abs(Y[:, r] - Yw[:, r]).max() / max(1.0, np.abs(Yw[:, r]).max())) for r in range(26)]
    for a, b in ((26 * N, 26 * (N + 1)), (26 * (N + 1), 26 * (N + 1) + 4 * rcfg.n_vblocks)):
        out.append(float(np.abs(y[a:b] - y_want[a:b]).max() / max(1.0, np.abs(y_want[a:b]).max())))
    return np.array(out)


def duals_longdouble(ref, cfg, rec, x):
    """y of tests/certificate_model.py certify, the recursion restated in np.longdouble (the linearisation, the time grid and
    the weights are the float64 data both sides read)"""
    ld = np.longdouble
    N, nS, nvb = cfg.n_iter, cfg.n_iter_small, cfg.n_vblocks
    A, _, Bt, _ = (a.astype(ld) for a in ref.linearize(cfg, rec))
    dt = ref.dt_schedule(cfg).astype(ld)
    q = ref.state_weight(cfg).astype(ld)
    xl = x.astype(ld)
    X = xl[:26 * (N + 1)].reshape(N + 1, 26)
    V = xl[cfg.off_throttle:cfg.off_throttle + 4 * nvb].reshape(nvb, 4)
    win = rec[ref.IN_XREF:ref.IN_XREF + 12 * cfg.n_ref_cols].reshape(cfg.n_ref_cols, 12).astype(ld)
    xr = np.zeros((N + 1, 26), dtype=ld)
    for i in range(1, N + 1):
        xr[i, :12] = win[0 if i - 1 < nS else i - 1 - nS]
    Y = np.zeros((N, 26), dtype=ld)
    Y[N - 1] = q * (X[N] - xr[N])
    for i in range(N - 1, 0, -1):
        Y[i - 1] = q * (X[i] - xr[i]) + (Y[i] + dt[i] * (A.T @ Y[i]))
    yinit = -(Y[0] + dt[0] * (A.T @ Y[0]))
    vprev = np.array([ref.v_of_throttle(rec[ref.IN_UPREV + k]) for k in range(4)]).astype(ld)
    w_thr, w_init = ld(cfg.w_throttle), ld(cfg.w_initial_throttle)
    mu = np.zeros((nvb, 4), dtype=ld)
    for t in range(nvb):
        h = np.zeros(4, dtype=ld)
        if t > 0:
            h += w_thr * (V[t] - V[t - 1])
        if t < nvb - 1:
            h += w_thr * (V[t] - V[t + 1])
        if t == 0:
            h += w_init * V[0] - w_init * vprev
        for i in range(N):
            if ref.throttle_block_of_stage(cfg, i) == t:
                h += dt[i] * (Bt.T @ Y[i])
        mu[t] = -h
    y = np.zeros(cfg.n_con, dtype=ld)
    y[:26 * N] = Y.reshape(-1)
    y[26 * N:26 * (N + 1)] = yinit
    y[26 * (N + 1):26 * (N + 1) + 4 * nvb] = mu.reshape(-1)
    return y


_dense = {}


def dense(ref, rcfg, rec):
    """assemble_dense, once per (configuration, record)"""
    key = (repr(rcfg), rec.tobytes())
    if key not in _dense:
        _dense[key] = ref.assemble_dense(rcfg, rec)
    return _dense[key]


def field_figures(ref, rcfg, case, y, cert):
    """A certificate (model's or device's) for a case against oracle/vsmpc_ref.py kkt_certificate on the same (x, y) and
    against the case's closed-form values, each as a fraction of its bound of certificate_model.field_tolerances.  Returns
    ({name: fraction}, the oracle's row or entry that carries the maximum of the case's spotlighted field or None)."""
    H, g, Ac, lo, hi = dense(ref, rcfg, case["rec"])
    x = case["x"]
    want = ref.kkt_certificate(H, g, Ac, lo, hi, x, y)
    tol = cm.field_tolerances(H, g, Ac, x, y)
    scale = max(1.0, float(np.abs(g).max()), float(np.abs(H @ x).max()))
    oscale = max(1.0, abs(want["objective"]), 0.5 * float(x @ H @ x))
    fig = {"stationarity": abs(cert[S] - want["stationarity"]) / tol["stationarity"],
           "primal": abs(cert[P] - want["primal"]) / tol["primal"],
           "complementarity": abs(cert[C] - want["complementarity"]) / tol["complementarity"],
           "objective": abs(cert[O] - want["objective"]) / oscale / tol["objective_rel"],
           "scale": abs(cert[SC] - scale) / scale / (4 * np.finfo(float).eps)}
    for f, v in case["closed"].items():
        fig["closed " + FIELD[f]] = abs(cert[f] - v) / tol[FIELD[f]]
    arg = None
    if case["row"] is not None:
        f = case["row"][0]
        Ax = Ac @ x
        if f == S:
            arg = int(np.abs(H @ x + g + Ac.T @ y).argmax())
        elif f == P:
            arg = int(np.maximum(0.0, np.maximum(lo - Ax, Ax - hi)).argmax())
        else:
            arg = int(np.where(lo < hi, np.maximum(np.maximum(y, 0.0) * (hi - Ax), np.maximum(-y, 0.0) * (Ax - lo)), 0.0).argmax())
    return fig, arg
