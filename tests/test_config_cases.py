"""CPU side of the configuration sweep (tests/config_cases.py): the judges first.

  * known answers per configuration field: for every one_at_a_time() case the oracle's dense assembly differs from the
    default assembly in exactly the entries the reference's sources name, by the stated amount -- so the oracle is an
    independent judge of two keys read into each other's field, not a second copy of such a mix-up;
  * the C oracle against the numpy oracle at ALL_DISTINCT for the three tabled horizons;
  * the numpy models of the tuned kernel's algorithm (algo_model: SYRK and structured condensing behind the joint
    reduction; reduced_condensed) and of the runtime kernel (runtime_model) against the oracle at ALL_DISTINCT and the
    edge configurations: solution at the models' bar (1e-10), equal active-set iteration counts;
  * the small-w_throttle end of the parity range (config_cases.W_THROTTLE_PARITY_MIN).

Measured here (float64 model against the oracle, worst over 13 records per configuration, paper horizon):
ALL_DISTINCT 1.5e-14 ((21, 9, 15): 1.5e-14, (34, 14, 24): 2.1e-13), w_reg = 0 with non-uniform joint weights 7.3e-14,
w_lin_mom = 0 4.7e-14, joint weights 1..1e6 3.1e-14, throttle box 45..55 1.3e-14, periods 0.0047 / 0.093 1.8e-14, hold
outside the box 2.2e-14, w_throttle = 100: 2.6e-13, 10: 1.6e-13 (iteration counts equal everywhere); w_throttle = 1:
0.5 with 4 of 13 iteration counts different -- not a parity case.

Against mpmath (test_oracle_accuracy_against_mpmath; relative error of x against a 40+ digit solve of the final active
set's KKT system, worst of four instances, oracle / float64 model): ALL_DISTINCT 1.1e-14 / 1.8e-14, joint weights 1..1e6
2.0e-14 / 3.0e-14, w_throttle = 10: 9.2e-14 / 2.8e-14, throttle box 45..55 1.3e-14 / 1.3e-15.

File:line citations are relative to the reference's momentum-based-linear-mpc-lib/src/variableSamplingMPC/."""
import dataclasses
import os
import re

import numpy as np
import pytest

from conftest import relerr
import config_cases as cc

STATE_INDEX = {"w_com_pos": 0, "w_lin_mom": 3, "w_rpy": 6, "w_ang_mom": 9, "w_com_pos_err": 20, "w_rpy_err": 23}  # VSconstant.h:6-40


def test_tables_are_what_they_claim(layout):
    d = layout.MPCConfig()
    for k, v in cc.ALL_DISTINCT.items():
        same = np.atleast_1d(np.asarray(v, float) == np.asarray(getattr(d, k), float))
        assert same.sum() == (1 if k == "w_delta_joint" else 0), k     # (the first joint weight keeps the paper's value)
    groups = [[x for f in cc.STATE_FIELDS for x in cc.ALL_DISTINCT[f]], list(cc.ALL_DISTINCT["w_delta_joint"]),
              [cc.ALL_DISTINCT[k] for k in ("w_throttle", "w_initial_throttle", "w_reg_joint_pos")],
              [cc.ALL_DISTINCT[k] for k in ("period_mpc", "period_small", "period_large")]]
    assert [len(g) for g in groups] == [18, 8, 3, 3]
    for g in groups:                                                   # no two values equal where one array holds them
        assert len(set(g)) == len(g), g
    assert set(cc.ALL_DISTINCT) == {f.name for f in dataclasses.fields(d)} - {
        "n_iter", "n_iter_small", "control_horizon", "use_jet_dynamic"}
    names = [n for n, _, _ in cc.one_at_a_time()]
    assert len(names) == len(set(names)) == 18 + 8 + 7
    for name, s, recs in cc.one_at_a_time():
        assert len(s) == 1 and len(recs) >= 3
        (k, v), = s.items()
        diff = np.atleast_1d(np.asarray(v, float) != np.asarray(getattr(d, k), float))
        assert diff.sum() == 1, name                                                   # exactly one component moved
    assert layout.MPCConfig(**cc.all_distinct((17, 7, 12))).ratio == 15
    assert layout.MPCConfig(n_iter=34, n_iter_small=14, control_horizon=24, **cc.all_distinct((34, 14, 24))).ratio == 30


def test_oracle_known_answer_per_field(ref, layout):
    """Each field lands where the reference puts it and nowhere else."""
    dcfg = ref.Config()
    N, nS, Hc, nvb = dcfg.n_iter, dcfg.n_iter_small, dcfg.control_horizon, dcfg.n_vblocks
    offJ, offV, r1 = dcfg.off_joints, dcfg.off_throttle, 26 * (N + 1)
    for name, s, recs in cc.one_at_a_time():
        _, rcfg = cc.configs(ref, cc.PAPER, s)
        (key, val), = s.items()
        for rec in recs[:3]:
            H0, g0, A0, lo0, hi0 = ref.assemble_dense(dcfg, rec)
            H, g, Ac, lo, hi = ref.assemble_dense(rcfg, rec)
            He, ge, Ae, loe, hie = H0.copy(), g0.copy(), A0.copy(), lo0.copy(), hi0.copy()
            xref = rec[layout.IN_XREF:].reshape(dcfg.n_ref_cols, 12)
            vprev = ref.v_of_throttle(rec[layout.IN_UPREV:layout.IN_UPREV + 4])
            if key in STATE_INDEX:            # costsVSMPC.cpp:78-93 (Q), :166-178 (nodes 1..N, gradient -Q x_ref), :191-200
                i = int(np.nonzero(np.asarray(val) != np.asarray(getattr(dcfg, key)))[0][0])
                st = STATE_INDEX[key] + i
                for k in range(1, N + 1):
                    He[26 * k + st, 26 * k + st] = val[i]
                    col = 0 if k - 1 < nS else k - 1 - nS
                    ge[26 * k + st] = -val[i] * xref[col, st] if st < 12 else 0.0     # error states have no reference
            elif key == "w_delta_joint":      # costsVSMPC.cpp:358-359,375-381 + :564-570 (the position regulariser adds)
                j = int(np.nonzero(np.asarray(val) != 65000.0)[0][0])
                for k in range(Hc):
                    He[offJ + 8 * k + j, offJ + 8 * k + j] = val[j] + dcfg.w_reg_joint_pos
            elif key == "w_throttle":         # costsVSMPC.cpp:360-361,383-409: w (v_{b+1} - v_b)^2 over the nvb - 1 differences
                D = np.zeros((nvb - 1, nvb))
                for b in range(nvb - 1):
                    D[b, b], D[b, b + 1] = -1.0, 1.0
                T = val * np.kron(D.T @ D, np.eye(4))
                T[:4, :4] += dcfg.w_initial_throttle * np.eye(4)                       # :468-476, unchanged
                He[offV:, offV:] = T
            elif key == "w_initial_throttle":  # costsVSMPC.cpp:450 (read into m_weightThrottle of its own class), :468-487
                for r in range(4):
                    He[offV + r, offV + r] = dcfg.w_throttle + val
                    ge[offV + r] = -val * vprev[r]
            elif key == "w_reg_joint_pos":    # costsVSMPC.cpp:521,564-591
                for k in range(Hc):
                    for j in range(8):
                        He[offJ + 8 * k + j, offJ + 8 * k + j] = 65000.0 + val
                        ge[offJ + 8 * k + j] = val * rec[layout.IN_QERR + j]
            elif key in ("throttle_min", "throttle_max"):   # constraintsVSMPC.cpp:329-332,338-365
                b = ref.jet_v(ref.std_throttle(val))
                first = 1 if rec[layout.IN_HOLD] != 0.0 else 0
                (loe if key == "throttle_min" else hie)[r1 + 4 * first:r1 + 4 * nvb] = b
            else:                             # periods: constraintsVSMPC.cpp:45-51 (beta1, beta2), :78-84, :156-159
                ps, pl = rcfg.period_small, rcfg.period_large
                beta2 = (pl - nS * ps) / (nS * (nS - 1))
                dts = np.array([ps + 2 * k * beta2 if k < nS else pl for k in range(N)])
                np.testing.assert_allclose(ref.dt_schedule(rcfg), dts, rtol=1e-13, atol=0)
                assert abs(dts[:nS].sum() - pl) < 1e-15                                # the fast steps span one slow step
                A, Bj, Bt, c = ref.linearize(dcfg, rec)
                for k in range(N):
                    r = 26 * k
                    jb, tb = min(k, Hc - 1), (0 if k < nS else min(k, Hc - 1) - (nS - 1))
                    Ae[r:r + 26, r:r + 26] = np.eye(26) + dts[k] * A
                    Ae[r:r + 26, offJ + 8 * jb:offJ + 8 * jb + 8] = dts[k] * Bj
                    Ae[r:r + 26, offV + 4 * tb:offV + 4 * tb + 4] = dts[k] * Bt
                    loe[r:r + 26] = hie[r:r + 26] = -dts[k] * c
                np.testing.assert_allclose(Ac, Ae, rtol=1e-13, atol=1e-15)
                np.testing.assert_allclose(lo, loe, rtol=1e-13, atol=1e-15)
                np.testing.assert_allclose(hi, hie, rtol=1e-13, atol=1e-15)
                Ae, loe, hie = Ac, lo, hi          # (compared to rounding above; the exact comparisons below then cover H and g)
                assert key == "period_large" or np.array_equal(Ac[26 * nS:], A0[26 * nS:])   # slow rows: period_large only
            np.testing.assert_array_equal(H, He, err_msg=name)
            np.testing.assert_array_equal(g, ge, err_msg=name)
            np.testing.assert_array_equal(Ac, Ae, err_msg=name)
            np.testing.assert_array_equal(lo, loe, err_msg=name)
            np.testing.assert_array_equal(hi, hie, err_msg=name)
            changed = (H != H0).sum() + (g != g0).sum() + (Ac != A0).sum() + (lo != lo0).sum() + (hi != hi0).sum()
            assert changed > 0, name                                                   # the field acts on these records


def test_one_at_a_time_cases_move_the_oracles_solution(ref):
    """A case whose field does not move the optimum proves nothing: at least 1e-5 relative (three orders above the
    parity bar) on the case's records, established with the oracle alone."""
    dcfg = ref.Config()
    base = {}
    for name, s, recs in cc.one_at_a_time():
        _, rcfg = cc.configs(ref, cc.PAPER, s)
        for b, rec in enumerate(recs):                    # every record, so that one that proves nothing fails loudly
            key = rec.tobytes()
            if key not in base:
                base[key] = ref.solve_instance(dcfg, rec)[0]
            moved = relerr(ref.solve_instance(rcfg, rec)[0], base[key])
            assert moved >= 1e-5, (name, b, moved)


def test_dual_form_thresholds_match_the_kernel_source():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), cc.PKG, "csrc", "vsmpc_p4.hpp")).read()
    assert int(re.search(r"constexpr int DUAL_MAX_ACTIVE = (\d+);", src).group(1)) == cc.DUAL_FORM_MAX[(17, 7, 12)]
    assert int(re.search(r"constexpr int DUAL3_MAX = (\d+);", src).group(1)) == cc.DUAL_FORM_MAX[(34, 14, 24)]
    assert "n_violated <= (DUAL3 ? DUAL3_MAX : DUAL_MAX_ACTIVE)" in src


@pytest.mark.parametrize("horizon", cc.HORIZONS)
def test_c_oracle_equals_numpy_oracle_at_all_distinct(ref, horizon):
    import oracle_c
    oracle_c.load()
    cfg, rcfg = cc.configs(ref, horizon, cc.all_distinct(horizon))
    recs = cc.records(cfg, n=1)
    for rec in recs:
        H, g, Ac, lo, hi = oracle_c.assemble_dense(rcfg, rec)
        Hr, gr, Acr, lor, hir = ref.assemble_dense(rcfg, rec)
        np.testing.assert_array_equal(H, Hr)
        np.testing.assert_array_equal(Ac == 0, Acr == 0)
        np.testing.assert_allclose(g, gr, rtol=1e-14, atol=1e-12)
        np.testing.assert_allclose(Ac, Acr, rtol=1e-13, atol=1e-14)
        np.testing.assert_allclose(lo, lor, rtol=1e-13, atol=1e-12)
        np.testing.assert_allclose(hi, hir, rtol=1e-13, atol=1e-12)
    A, Bj, Bt, c, dt = oracle_c.linearize(rcfg, recs[0])
    Ar, Bjr, Btr, cr = ref.linearize(rcfg, recs[0])
    np.testing.assert_allclose(A, Ar, rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(c, cr, rtol=1e-13, atol=1e-12)
    # dt_k = warp(k + 1) - warp(k) (constraintsVSMPC.cpp:78-84,156-159): each warp value up to period_large carries half
    # an ulp of it, and C contracts beta1 t + beta2 t^2 into fused multiply-adds where numpy does not.  The default
    # configurations meet 1e-17 because their warp values are short binary fractions; here the bar is cc.dt_atol().
    np.testing.assert_allclose(dt, ref.dt_schedule(rcfg), rtol=0, atol=cc.dt_atol(rcfg))


MODEL_CASES = [(h, "ALL_DISTINCT") for h in cc.HORIZONS] + [(cc.PAPER, name) for name in cc.EDGE]


@pytest.mark.parametrize("horizon, name", MODEL_CASES)
def test_models_match_oracle(ref, horizon, name):
    import algo_model
    import condense_model
    import runtime_model
    cfg, rcfg = cc.configs(ref, horizon, cc.all_distinct(horizon) if name == "ALL_DISTINCT" else cc.EDGE[name])
    recs = cc.records(cfg) if name == "ALL_DISTINCT" else cc.edge_records(name, cfg)
    for b, rec in enumerate(recs):
        xr, _, itr, _ = ref.solve_instance(rcfg, rec)
        out = {}
        xm, st, it = algo_model.solve_model(rcfg, ref, rec, reduce=True, out=out)
        assert st == 1 and it == itr, (b, st, it, itr)
        assert relerr(xm, xr) < 1e-10, (b, relerr(xm, xr))
        if b % 4 == 0:                                    # the other two models on every fourth record
            xs, st, it = algo_model.solve_model(rcfg, ref, rec, reduce=True, condense=condense_model.condense_structured)
            assert st == 1 and it == itr and relerr(xs, xr) < 1e-10, (b, st, it, itr, relerr(xs, xr))
            x2, fm, st, it = runtime_model.solve(rcfg, rec)
            assert st == runtime_model.SOLVED and it == itr and relerr(x2, xr) < 1e-10, (b, st, it, itr)
            assert relerr(fm, ref.first_move_vector(rcfg, xr)) < 1e-10
        if b == 3:                                        # a take-off record: the condensed problem of the dense QP
            Me, ge, Le = algo_model.reduced_condensed(rcfg, ref, rec)
            nz = Me.shape[0]
            assert np.abs(out["M"][:nz, :nz] - Me).max() < 1e-12 * np.abs(Me).max()
            assert np.abs(out["M"][nz, :nz] - ge).max() < 1e-11 * np.abs(ge).max()
            assert np.abs(np.tril(out["L"][:nz, :nz]) - Le).max() < 1e-11 * np.abs(Le).max()


def test_narrow_throttle_box_iterates_and_uses_both_formulations(ref):
    """45..55 %: every record needs more than one active-set pass, and first violated sets on both sides of the size at
    which the tuned kernel switches from the dual to the primal box-QP form occur (16 of 24 throttles at the paper
    horizon).  Sets of at most 4 do not occur with this box: 6 is the smallest over 160 take-off records, hover demands
    75 % throttle; the small sets are covered by ALL_DISTINCT's 8..88 box and test_gpu_parity's default-box test."""
    cfg, rcfg = cc.configs(ref, cc.PAPER, cc.EDGE["throttle_box_45_55"])
    recs = cc.edge_records("throttle_box_45_55", cfg)
    fv = [cc.first_violated(ref, rcfg, rec) for rec in recs]
    its = [ref.solve_instance(rcfg, rec)[2] for rec in recs]
    assert min(its) > 1, its
    assert min(fv) <= cc.DUAL_FORM_MAX[cc.PAPER] < max(fv), fv


def test_small_w_throttle_end_of_the_parity_range(ref):
    """W_THROTTLE_PARITY_MIN is the smallest power of ten at which the oracle and the model of the tuned kernel agree to
    1e-10 with equal iteration counts on records(); one decade below they no longer do (nearly singular reduced Hessian:
    same objective, different minimisers)."""
    import algo_model

    def agree(w):
        cfg, rcfg = cc.configs(ref, cc.PAPER, dict(w_throttle=w))
        ok = True
        for rec in cc.records(cfg):
            xr, _, itr, _ = ref.solve_instance(rcfg, rec)
            xm, st, it = algo_model.solve_model(rcfg, ref, rec, reduce=True)
            ok = ok and st == 1 and it == itr and relerr(xm, xr) < 1e-10
        return ok
    assert agree(cc.W_THROTTLE_PARITY_MIN)
    assert not agree(cc.W_THROTTLE_PARITY_MIN / 10.0)
    assert np.log10(cc.W_THROTTLE_PARITY_MIN) % 1 == 0


@pytest.mark.parametrize("name", ["ALL_DISTINCT", "joint_spread_1_1e6", "w_throttle_parity_min", "throttle_box_45_55"])
def test_oracle_accuracy_against_mpmath(ref, name, capsys):
    """How exact the judges are, measured once: the oracle's x and the float64 model's x against a 50-digit solve of the
    KKT system of the oracle's final active set (same float64 problem data H, g, A, l, u).  The measured values are in the module docstring; the assertion is that the judge sits at least two orders inside the 1e-8
    parity bar, the printed figures are what DESIGN.md quotes."""
    mpmath = pytest.importorskip("mpmath")
    import scipy.linalg
    import algo_model
    mpmath.mp.dps = 50
    mpf = mpmath.mpf
    cfg, rcfg = cc.configs(ref, cc.PAPER, cc.all_distinct(cc.PAPER) if name == "ALL_DISTINCT" else cc.EDGE[name])
    recs = cc.records(cfg) if name == "ALL_DISTINCT" else cc.edge_records(name, cfg)
    nxs, nthr, n = 26 * (rcfg.n_iter + 1), 4 * rcfg.n_vblocks, rcfg.n_var
    worst_o = worst_m = 0.0
    for rec in recs[[1, 3, 9, 12]]:                      # hover (held), take-off, saturated up, saturated down
        xo, _, _, (H, g, Ac, lo, hi) = ref.solve_instance(rcfg, rec)
        xm, st, _ = algo_model.solve_model(rcfg, ref, rec, reduce=True)
        v = xo[rcfg.off_throttle:]
        rows = list(range(nxs)) + [nxs + i for i in range(nthr) if v[i] == lo[nxs + i] or v[i] == hi[nxs + i]]
        bnd = np.concatenate([lo[:nxs], v[[i - nxs for i in rows[nxs:]]]])       # active rows sit on the bound they hit
        Aa = Ac[rows]
        m = len(rows)
        K = np.zeros((n + m, n + m))
        K[:n, :n], K[:n, n:], K[n:, :n] = H, Aa.T, Aa
        rhs = np.concatenate([-g, bnd])
        lu = scipy.linalg.lu_factor(K)
        ii, jj = np.nonzero(K)
        kv = [mpf(float(K[i, j])) for i, j in zip(ii, jj)]
        b = [mpf(float(t)) for t in rhs]
        z = [mpf(float(t)) for t in scipy.linalg.lu_solve(lu, rhs)]
        for _ in range(25):
            res = list(b)
            for i, j, a in zip(ii, jj, kv):
                res[i] -= a * z[j]
            scale = max(abs(t) for t in res)
            if scale == 0:
                break
            d = scipy.linalg.lu_solve(lu, np.array([float(t / scale) for t in res]))
            z = [zi + scale * mpf(float(di)) for zi, di in zip(z, d)]
            if scale < mpf(10) ** -42:
                break
        assert scale < mpf(10) ** -38, scale             # the refinement converged to ~40 digits or better
        xe = np.array([float(t) for t in z[:n]])
        den = max(1.0, np.abs(xe).max())
        eo = max(float(abs(mpf(float(xo[i])) - z[i])) for i in range(n)) / den
        em = max(float(abs(mpf(float(xm[i])) - z[i])) for i in range(n)) / den
        worst_o, worst_m = max(worst_o, eo), max(worst_m, em)
    with capsys.disabled():
        print(f"\n[mpmath] {name}: oracle {worst_o:.2e}  float64 model {worst_m:.2e}")
    assert worst_o < 1e-10 and worst_m < 1e-10, (worst_o, worst_m)
