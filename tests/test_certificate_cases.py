"""The cases of tests/certificate_cases.py on the CPU: the reference side of tests/test_gpu_certificate_cases.py.  No GPU.

1. On every case the numpy model of certify_kernel (tests/certificate_model.py) agrees with oracle/vsmpc_ref.py
   kkt_certificate on the model's own (x, y) inside a FIFTH of the bounds of certificate_model.field_tolerances (the
   reference alone uses a fifth of the bar), the oracle's maximum sits on the row or entry the spotlight was aimed at, and
   every closed-form value is met inside the same fifth.
2. Off the optimum y has no oracle value (solve_exact's y exists at an optimum only): the float64 model is measured against
   the same recursion in np.longdouble (certificate_cases.duals_longdouble), per row class and relative to
   max(1, |y|_max of the class).  The device's bar is 100 times the worst class figure (the kernel uses fused multiply-adds
   and two partial chains per sum: its rounding differs from numpy's by a small factor), and never looser than the
   project's 1e-8: certificate_cases.Y_BAR, whose ceilings are asserted here.
3. One-line mistakes put into a copy of the model (MUTATIONS): each must move a case of certificate_cases by at least ten
   bars, and what the inputs of tests/test_gpu_certificate.py see of it is recorded next to it.

`python tests/test_certificate_cases.py` writes profiles/certificate_cases.txt and profiles/certificate_cases_mutations.txt.
"""
import os
import sys

import numpy as np
import pytest

import certificate_cases as ccs
import certificate_model as cm
import config_cases as cc

S, SC, P, C, O, D = range(6)
Y_WORST_COSTATE, Y_WORST_THROTTLE, Y_MODEL_WORST, Y_BAR = ccs.Y_WORST_COSTATE, ccs.Y_WORST_THROTTLE, ccs.Y_MODEL_WORST, ccs.Y_BAR
FIFTH = 0.2


def _groups():
    return [(h, c) for h in ccs.HORIZONS for c in ccs.config_names(h)]


def _check_reference_side(ref, rcfg, cases, worst):
    for case in cases:
        y, cert = cm.certify(ref, rcfg, case["rec"], case["x"])
        fig, arg = ccs.field_figures(ref, rcfg, case, y, cert)
        for k, v in fig.items():
            worst[k] = max(worst.get(k, 0.0), v)
            assert v <= (1.0 if k == "scale" else FIFTH), (case["family"], case["name"], case["rec_name"], k, v)
        if case["row"] is not None:
            assert arg == case["row"][1], (case["family"], case["name"], case["rec_name"], arg, case["row"])
        assert cert[D] == np.abs(y).max() and (cert[6:] == 0.0).all()
        # solver.certified at 1e-9: true at the oracle's optima (the edge records among them), false everywhere else, each
        # with a margin the device's rounding cannot cross
        margin = float(ccs.certified_margins(cert, case["x"]).max())
        if case["family"] == "optimum":
            worst["certified, optima"] = max(worst.get("certified, optima", 0.0), margin)
            assert margin <= 0.5e-9, (case["rec_name"], margin)
        else:
            worst["certified, others (least)"] = min(worst.get("certified, others (least)", np.inf), margin)
            assert margin >= 1e-7, (case["family"], case["name"], margin)
        err = ccs.class_errors(rcfg, y, ccs.duals_longdouble(ref, rcfg, case["rec"], case["x"]).astype(np.float64))
        worst["y costate"] = max(worst.get("y costate", 0.0), float(err[:27].max()))
        worst["y throttle"] = max(worst.get("y throttle", 0.0), float(err[27]))
        assert (err <= Y_MODEL_WORST).all(), (case["family"], case["name"], err.max())
        if case["y_ref"] is not None:
            e = float(np.abs(y - case["y_ref"]).max() / max(1.0, np.abs(case["y_ref"]).max()))
            worst["y optimum"] = max(worst.get("y optimum", 0.0), e)
            assert e <= 1e-8


@pytest.mark.parametrize("horizon, config", _groups(), ids=lambda v: str(v).replace(" ", ""))
def test_reference_side(ref, horizon, config):
    _, rcfg = cc.configs(ref, horizon, ccs.settings_of(horizon, config))
    worst = {}
    cases = ccs.cases(ref, horizon, config)
    _check_reference_side(ref, rcfg, cases, worst)
    print(horizon, config, len(cases), "cases; worst fraction of the bound:", {k: f"{v:.2e}" for k, v in worst.items()})


def test_reference_side_tunables_and_boxqp(ref):
    worst = {}
    for _, rcfg, case in ccs.tunable_cases(ref):
        _check_reference_side(ref, rcfg, [case], worst)
    _, rcfg, cases = ccs.boxqp_cases(ref)
    _check_reference_side(ref, rcfg, cases, worst)
    vmin, vmax = ref.throttle_bounds(rcfg)
    v = np.array([c["x"][rcfg.off_throttle:] for c in cases if c["family"] == "optimum"])
    assert v.shape[1] == 44 and (v == vmin).any() and (v == vmax).any()
    print({k: f"{v:.2e}" for k, v in worst.items()})


def test_coverage(ref):
    """what the module must reach (the conditions of the module docstring, counted)"""
    for h in ccs.HORIZONS:
        _, rcfg = cc.configs(ref, h, {})
        N, nS, Hc, nvb = h[0], h[1], h[2], h[2] - h[1] + 1
        cases = ccs.cases(ref, h, "default")
        seen = {}
        for c in cases:
            seen.setdefault(c["family"], set()).add((c["rec_name"], c["name"]))
        names = lambda fam, rec: {n for r, n in seen.get(fam, ()) if r == rec}
        free, held = "all_distinct_0", "all_distinct_1"
        if h in ccs.EXHAUSTIVE:
            for rec in (free, held):
                assert names("primal_dyn", rec) == {f"stage {i} row {r}" for i in range(N) for r in range(26)}
                assert names("primal_init", rec) == {f"row {r}" for r in range(26)}
                assert names("stat", rec) == {f"block {j} joint {k}" for j in range(Hc) for k in range(8)}
                blocks = range(1 if rec == held else 0, nvb)
                want = {f"block {t} jet {k} side {s:+d}" for t in blocks for k in range(4) for s in (1, -1)}
                assert names("primal_box", rec) == want and names("comp", rec) == want
            assert names("primal_pin", held) == {f"jet {k}" for k in range(4)}
        else:
            stages, joints, throttles = ccs.positions(rcfg)
            assert {0, nS - 1, Hc - 1, N - 1} <= set(stages) and {0, Hc - 1} <= set(joints) and {0, nvb - 1} <= set(throttles)
            assert names("primal_dyn", free) == {f"stage {i} row {r}" for i in stages for r in range(26)}
            assert names("stat", free) == {f"block {j} joint {k}" for j in joints for k in range(8)}
            want = {f"block {t} jet {k} side {s:+d}" for t in throttles for k in range(4) for s in (1, -1)}
            assert names("primal_box", free) == want and names("comp", free) == want
        if nvb > 1:
            assert seen["pinned"]
        recs = {c["rec_name"] for c in cases if c["family"] == "optimum"}
        assert len(recs) == 20 and set(ccs.EDGE_RECORDS) <= recs
        assert set(ccs.EDGE_RECORDS) <= {c["rec_name"] for c in cases if c["family"] == "offopt"}
    # phase B's second pass at (40, 2, 40): joint entries 256..319 are blocks 32.., every throttle entry is behind 320
    cases = ccs.cases(ref, (40, 2, 40), "default")
    assert any(c["family"] == "stat" and c["name"].startswith("block 39 ") for c in cases)
    for fam in ("primal_box", "comp", "pinned"):
        assert any(c["family"] == fam for c in cases)
    assert len({repr(s) for s in ccs.TUNABLE_SETTINGS}) >= 4


# ---- mutations: certificate_model.certify with one mistake in it

MUTATIONS = ["window column off by one in the costate recursion", "window column off by one in the objective and scale",
             "last joint block sums stage HC - 1 alone", "throttle_block off by one at k = nS",
             "primal skips state rows 20 to 25", "primal skips the initial rows", "primal skips the last stage",
             "phase B drops entries >= 256", "hold read as == 1.0", "the pinned block counted in complementarity",
             "upper and lower slack swapped", "w_init on the wrong block", "vp of the last block reads beyond it",
             "q_diag of rows >= 20 reads sq[r]", "one joint weight for all joints", "padding rows not zeroed"]


def mutant(ref, cfg, rec, x, mut):
    """certificate_model.certify with the mistake MUTATIONS[mut] (None: none; the copy is then checked against the model)"""
    m = None if mut is None else MUTATIONS[mut]
    N, nS, Hc, nvb = cfg.n_iter, cfg.n_iter_small, cfg.control_horizon, cfg.n_vblocks
    nx, nj, nt = 26, 8, 4
    A, Bj, Bt, c = ref.linearize(cfg, rec)
    dt = ref.dt_schedule(cfg)
    q = ref.state_weight(cfg)
    w_dq = np.asarray(cfg.w_delta_joint, dtype=float)
    w_reg, w_thr, w_init = cfg.w_reg_joint_pos, cfg.w_throttle, cfg.w_initial_throttle
    if m == "q_diag of rows >= 20 reads sq[r]":
        q = q.copy()
        q[20:26] = (w_dq + w_reg)[2:8] ** 2              # CFG_WJ follows the 18 square roots of CFG_SQ
    if m == "one joint weight for all joints":
        w_dq = np.full(8, w_dq[0])
    X = x[:nx * (N + 1)].reshape(N + 1, nx)
    U = x[cfg.off_joints:cfg.off_joints + nj * Hc].reshape(Hc, nj)
    V = x[cfg.off_throttle:cfg.off_throttle + nt * nvb].reshape(nvb, nt)
    jb = [ref.joint_block_of_stage(cfg, i) for i in range(N)]
    tb = [ref.throttle_block_of_stage(cfg, i) for i in range(N)]
    if m == "throttle_block off by one at k = nS" and nS < N:
        tb[nS] = max(tb[nS] - 1, 0)
    win = rec[ref.IN_XREF:ref.IN_XREF + 12 * cfg.n_ref_cols].reshape(cfg.n_ref_cols, 12)
    xr, xr1 = np.zeros((N + 1, nx)), np.zeros((N + 1, nx))
    for i in range(1, N + 1):
        col = 0 if i - 1 < nS else i - 1 - nS
        xr[i, :12] = win[col]
        xr1[i, :12] = win[min(col + 1, cfg.n_ref_cols - 1)]
    xr_y = xr1 if m == "window column off by one in the costate recursion" else xr
    xr_o = xr1 if m == "window column off by one in the objective and scale" else xr
    vprev = np.array([ref.v_of_throttle(rec[ref.IN_UPREV + k]) for k in range(nt)])
    vmin, vmax = ref.throttle_bounds(cfg)
    qerr = rec[ref.IN_QERR:ref.IN_QERR + nj]
    hold = rec[ref.IN_HOLD] == 1.0 if m == "hold read as == 1.0" else rec[ref.IN_HOLD] != 0.0
    y = np.zeros(cfg.n_con)
    Y = y[:nx * N].reshape(N, nx)
    Y[N - 1] = q * (X[N] - xr_y[N])
    for i in range(N - 1, 0, -1):
        Y[i - 1] = q * (X[i] - xr_y[i]) + (Y[i] + dt[i] * (A.T @ Y[i]))
    y[nx * N:nx * (N + 1)] = -(Y[0] + dt[0] * (A.T @ Y[0]))
    hxV, gV = np.zeros((nvb, nt)), np.zeros((nvb, nt))
    for t in range(nvb):
        if t > 0:
            hxV[t] += w_thr * (V[t] - V[t - 1])
        if t < nvb - 1:
            hxV[t] += w_thr * (V[t] - V[t + 1])
    if m == "vp of the last block reads beyond it":
        hxV[nvb - 1] += w_thr * (V[nvb - 1] - 0.0)       # whatever lies behind x in LDS; 0 here
    t0 = nvb - 1 if m == "w_init on the wrong block" else 0
    hxV[t0] += w_init * V[t0]
    gV[t0] = -w_init * vprev
    drop = m == "phase B drops entries >= 256"
    mu = np.zeros((nvb, nt))
    for t in range(nvb):
        s = sum((dt[i] * (Bt.T @ Y[i]) for i in range(N) if tb[i] == t), np.zeros(nt))
        mu[t] = -(hxV[t] + gV[t] + s)
    done_v = np.ones((nvb, nt), dtype=bool)
    done_u = np.ones((Hc, nj), dtype=bool)
    if drop:
        done_u.reshape(-1)[256:] = False
        done_v.reshape(-1)[max(0, 256 - nj * Hc):] = False
        mu[~done_v] = 0.0                                  # (never written: whatever LDS held)
    r1 = nx * (N + 1)
    y[r1:r1 + nt * nvb] = mu.reshape(-1)
    if m == "padding rows not zeroed":
        y[r1 + nt * nvb:] = -7.0
    stat, scale, prim, comp, obj = 0.0, 1.0, 0.0, 0.0, 0.0
    for j in range(Hc):
        stages = [i for i in range(N) if jb[i] == j]
        if m == "last joint block sums stage HC - 1 alone" and j == Hc - 1:
            stages = [Hc - 1]
        s = sum((dt[i] * (Bj.T @ Y[i]) for i in stages), np.zeros(nj))
        hx, g = (w_dq + w_reg) * U[j], w_reg * qerr
        k = done_u[j]
        if k.any():
            stat = max(stat, np.abs(hx + g + s)[k].max())
            scale = max(scale, np.abs(hx)[k].max(), np.abs(g)[k].max())
            obj += float(U[j][k] @ (0.5 * hx + g)[k])
    for i in range(1, N + 1):
        hx, g = q * X[i], -q * xr_o[i]
        scale = max(scale, np.abs(hx).max(), np.abs(g).max())
        obj += float(X[i] @ (0.5 * hx + g))
    scale = max(scale, np.abs(hxV[done_v]).max(initial=0.0), np.abs(gV[done_v]).max(initial=0.0))
    for t in range(nvb - 1):
        obj += 0.5 * w_thr * float(((V[t] - V[t + 1]) ** 2)[done_v[t]].sum())
    obj += float((V[t0] * (0.5 * w_init * V[t0] + gV[t0]))[done_v[t0]].sum())
    rows = slice(0, 20) if m == "primal skips state rows 20 to 25" else slice(0, 26)
    for i in range(N - 1 if m == "primal skips the last stage" else N):
        res = X[i] + dt[i] * (A @ X[i] + Bj @ U[jb[i]] + Bt @ V[tb[i]] + c) - X[i + 1]
        prim = max(prim, np.abs(res[rows]).max())
    if m != "primal skips the initial rows":
        prim = max(prim, np.abs(X[0] - rec[ref.IN_X0:ref.IN_X0 + nx]).max())
    for t in range(nvb):
        k = done_v[t]
        if not k.any():
            continue
        if hold and t == 0:
            prim = max(prim, np.abs(V[0] - vprev)[k].max())
            if m == "the pinned block counted in complementarity":
                comp = max(comp, np.maximum(np.maximum(mu[0], 0.0) * (vprev - V[0]), np.maximum(-mu[0], 0.0) * (V[0] - vprev))[k].max())
            continue
        prim = max(prim, np.maximum(0.0, np.maximum(vmin - V[t], V[t] - vmax))[k].max())
        up, dn = (V[t] - vmin, vmax - V[t]) if m == "upper and lower slack swapped" else (vmax - V[t], V[t] - vmin)
        comp = max(comp, np.maximum(np.maximum(mu[t], 0.0) * up, np.maximum(-mu[t], 0.0) * dn)[k].max())
    cert = np.zeros(cm.CERT_SIZE)
    cert[:6] = stat, scale, prim, comp, obj, np.abs(y).max()
    return y, cert


def bars(ref, rcfg, case, y, cert, y_bar=Y_BAR):
    """how far (y, cert) is from what tests/test_gpu_certificate_cases.py accepts for a case, in bars (<= 1 passes)"""
    y_true, _ = cm.certify(ref, rcfg, case["rec"], case["x"])
    fig, _ = ccs.field_figures(ref, rcfg, case, y, cert)
    worst = max(fig.values())
    worst = max(worst, float((ccs.class_errors(rcfg, y, y_true) / y_bar).max()))
    r1 = 26 * (rcfg.n_iter + 1) + 4 * rcfg.n_vblocks
    if (y[r1:] != 0.0).any() or cert[D] != np.abs(y).max():
        worst = np.inf
    return worst


def old_inputs(ref, synth, layout):
    """(rcfg, case) of what tests/test_gpu_certificate.py feeds: oracle optima of synthetic records at its four horizons
    (a sample of its batches), two of them under the JOINT_SPREAD row of its second test, and the joint and state
    perturbations of its third test"""
    out = []
    for name, workload, count in (("paper", "takeoff", 8), ("paper", "montecarlo", 8), ("h2x", "takeoff", 4),
                                  ("odd", "takeoff", 4), ("unlisted", "takeoff", 4)):
        _, rcfg = cm.case_configs(ref, layout, name)
        for rec, x, y in cm.oracle_cases(ref, synth, layout, name, workload, 48 if name == "paper" else 4)[:count]:
            out.append((rcfg, dict(family="old optimum", name=name, rec_name=workload, rec=rec, x=x, closed={}, row=None, y_ref=y)))
    cfg, rcfg = cc.configs(ref, cc.PAPER, dict(w_delta_joint=cc.JOINT_SPREAD))      # its per-instance rows
    for rec in synth.make_batch(cfg, 2, workload="takeoff"):
        x, y, _, _ = ref.solve_instance(rcfg, rec)
        out.append((rcfg, dict(family="old optimum", name="joint spread", rec_name="takeoff", rec=rec, x=x, closed={}, row=None, y_ref=y)))
    rcfg, first = out[0]
    for off in (rcfg.off_joints + 5, 5 * 26 + 1):
        x = first["x"].copy()
        x[off] += 1e-3
        out.append((rcfg, dict(first, family="old perturbed", x=x, y_ref=None)))
    return out


def old_bars(ref, rcfg, case, y, cert):
    """the checks of tests/test_gpu_certificate.py: y globally at 1e-8 against the true y, the fields inside
    field_tolerances of the oracle's on the same (x, y)"""
    y_true, _ = cm.certify(ref, rcfg, case["rec"], case["x"])
    fig, _ = ccs.field_figures(ref, rcfg, case, y, cert)
    worst = max(v for k, v in fig.items() if not k.startswith("closed"))
    worst = max(worst, float(np.abs(y - y_true).max() / max(1.0, np.abs(y_true).max())) / 1e-8)
    r1 = 26 * (rcfg.n_iter + 1) + 4 * rcfg.n_vblocks
    if (y[r1:] != 0.0).any() or cert[D] != np.abs(y).max():
        worst = np.inf
    return worst


MUTATION_GROUPS = [((6, 2, 3), "default"), ((2, 2, 2), "default"), ((6, 2, 3), "non_default"), ((17, 7, 12), "default"),
                   ((17, 7, 12), "all_distinct"), ((12, 12, 12), "default"), ((40, 2, 2), "default"), ((40, 2, 40), "default")]


def mutation_table(ref, synth, layout, stride=1):
    """{mutation: ({family: worst bars over the new cases}, worst bars over the old inputs)}"""
    groups = []
    for h, config in MUTATION_GROUPS:
        _, rcfg = cc.configs(ref, h, ccs.settings_of(h, config))
        groups.append((rcfg, ccs.cases(ref, h, config)[::stride]))
    old = old_inputs(ref, synth, layout)
    table = {}
    for k, name in enumerate(MUTATIONS):
        fam = {}
        for rcfg, cases in groups:
            for case in cases:
                y, cert = mutant(ref, rcfg, case["rec"], case["x"], k)
                fam[case["family"]] = max(fam.get(case["family"], 0.0), bars(ref, rcfg, case, y, cert))
        worst_old = max(old_bars(ref, rcfg, case, *mutant(ref, rcfg, case["rec"], case["x"], k)) for rcfg, case in old)
        table[name] = (fam, worst_old)
    return table


def test_the_copy_is_the_model(ref):
    _, rcfg = cc.configs(ref, (6, 2, 3), cc.NON_DEFAULT)
    for case in ccs.cases(ref, (6, 2, 3), "non_default")[::7]:
        y, cert = cm.certify(ref, rcfg, case["rec"], case["x"])
        y2, cert2 = mutant(ref, rcfg, case["rec"], case["x"], None)
        assert np.array_equal(y, y2) and np.allclose(cert, cert2, rtol=1e-15, atol=0)
        assert bars(ref, rcfg, case, y2, cert2) <= 1.0


def test_every_mutation_is_caught(ref, synth, layout):
    """each mistake moves a new case by at least ten bars (a thinned set of the cases: every fifth, which can only miss)"""
    table = mutation_table(ref, synth, layout, stride=5)
    for name, (fam, old) in table.items():
        print(f"{name}: new {max(fam.values()):.1e} bars ({max(fam, key=fam.get)}), old inputs {old:.1e}")
        assert max(fam.values()) >= 10.0, name


def write_profiles(root):
    import importlib
    import vsmpc_ref as ref
    from conftest import PKG
    synth, layout = importlib.import_module(PKG + ".synth"), importlib.import_module(PKG + ".layout")
    lines = ["Reference side of tests/test_gpu_certificate_cases.py (python tests/test_certificate_cases.py), CPU only.",
             "Per horizon and configuration: number of cases, and the worst figure of the numpy model of certify_kernel",
             "(tests/certificate_model.py) as a fraction of its bound: the fields against oracle/vsmpc_ref.py kkt_certificate",
             "and the closed-form values against certificate_model.field_tolerances (asserted <= 0.2), y per row class",
             "against the np.longdouble recursion relative to max(1, |y|_max of the class), y at the optima against",
             "solve_exact relative to max(1, |y|_inf).  certified: the largest of the three relative tests of solver.certified",
             "(STATIONARITY / STAT_SCALE, PRIMAL / max(1, |x|), COMPLEMENTARITY / max(1, DUAL_MAX)) on the model's certificate:",
             "the worst over the oracle's optima, the edge records among them (asserted <= 0.5e-9: the oracle's own optimum",
             "passes 1e-9 on every record, so the device is asked for the same), and the least over all other cases",
             "(asserted >= 1e-7).", ""]
    overall = {}
    groups = [(h, c, None) for h, c in _groups()] + [("tunables", "", None), ("boxqp H34", "", None)]
    for h, config, _ in groups:
        worst = {}
        if h == "tunables":
            items = ccs.tunable_cases(ref)
            for _, rcfg, case in items:
                _check_reference_side(ref, rcfg, [case], worst)
            n = len(items)
        elif h == "boxqp H34":
            _, rcfg, cases = ccs.boxqp_cases(ref)
            _check_reference_side(ref, rcfg, cases, worst)
            n = len(cases)
        else:
            _, rcfg = cc.configs(ref, h, ccs.settings_of(h, config))
            cases = ccs.cases(ref, h, config)
            _check_reference_side(ref, rcfg, cases, worst)
            n = len(cases)
        for k, v in worst.items():
            overall[k] = (min if "least" in k else max)(overall.get(k, v), v)
        lines.append(f"{str(h):14s} {config:13s} {n:5d} cases  " + "  ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    lines += ["", "worst over all: " + "  ".join(f"{k} {v:.1e}" for k, v in overall.items()),
              f"y: worst class figure {overall['y costate']:.2e} over the costate and initial rows, {overall['y throttle']:.2e} over the",
              f"throttle rows; the ceilings {Y_WORST_COSTATE:.1e} and {Y_WORST_THROTTLE:.1e} are asserted, the device's bars per row class",
              f"are 100 times the ceilings, {Y_BAR[0]:.1e} and {Y_BAR[27]:.1e} (the project's 1e-8 would be the looser one)."]
    with open(os.path.join(root, "profiles", "certificate_cases.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    table = mutation_table(ref, synth, layout)
    fams = ["offopt", "primal_dyn", "primal_init", "primal_box", "primal_pin", "stat", "comp", "pinned", "optimum"]
    lines = ["One-line mistakes in a copy of tests/certificate_model.py certify (tests/test_certificate_cases.py mutant), CPU only.",
             "Figures: by how many bars of tests/test_gpu_certificate_cases.py the mistaken output misses, worst case per family of",
             "tests/certificate_cases.py (horizons and configurations: MUTATION_GROUPS; <= 1 passes, inf = an exact check fails),",
             "and the same for the inputs of tests/test_gpu_certificate.py with its own checks (oracle optima of synthetic",
             "records at its four horizons, its joint and state perturbations): 'old'.  An old figure <= 1 means that the",
             "suite let the mistake through before these cases.", "",
             f"{'mutation':58s}" + "".join(f"{f:>12s}" for f in fams) + f"{'old':>12s}"]
    for name, (fam, old) in table.items():
        lines.append(f"{name:58s}" + "".join(f"{fam.get(f, 0.0):12.1e}" for f in fams) + f"{old:12.1e}" + ("   LET THROUGH" if old <= 1.0 else ""))
    with open(os.path.join(root, "profiles", "certificate_cases_mutations.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "oracle"), os.path.join(root, "tests")):
        sys.path.insert(0, p)
    write_profiles(root)
