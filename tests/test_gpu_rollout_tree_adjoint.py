"""The adjoint of the rollout on the KINEMATIC-TREE plant on the device (vsmpc_rollout_set_tree_ex with VSMPC_TREE_ADJOINT,
tree_jacobian_kernel, the tree instantiations of advance_adjoint_kernel, autograd.rollout) on the five loops of
tests/rollout_tree_adjoint_cases.py over 9 ticks at ratio 4, on a runtime handle at (6, 2, 3) and -- loops 0 and 1 -- on the
tuned handle at (17, 7, 12):

  against tests/rollout_tree_adjoint_model.py (itself checked against central differences of the whole loop in
      test_rollout_tree_adjoint_model.py): the log under test_gpu_rollout_adjoint.py's 1e-8, grad_state0 and grad_gains under
      its derivative bar (per field 1e-6 |field|_inf + 1e-12 max |gradient|), grad_params and grad_traj under
      rollout_param_adjoint_cases.FD_BAR's rule; the blocks the tree plant does not read are exactly +0.0;
  against a central difference of the device's OWN forward rollout along one random direction in (state0, gains) on the posed
      loop, judged as test_gpu_rollout_adjoint.py judges it: ten times the CPU model's own quotient error;
  bitwise: the taped run against the untaped one; backward against backward_full; batches of 1 and 257 and a permuted batch;
      a joint selector changed between the run and the sweep; autograd.rollout; set_tree(None) after set_tree(adjoint=True)
      against a rollout that never saw a tree;
  the loop that is never Solved; a joint selector that is not the default; the refusals that stay.

Measured on an MI355X, in units of each bar: state0 at most 1.6e-9, gains 1.3e-6 at (6, 2, 3) and 4.8e-7 at (17, 7, 12),
parameters and tracks at most 9.6e-10; the device's quotient 6.27e-7 off its adjoint, the CPU model's 6.27e-7.
"""
import importlib
import os

import numpy as np
import pytest

import adjoint_model as am
import rollout_adjoint_cases as rc
import rollout_adjoint_model as ram
import rollout_param_adjoint_cases as pc
import rollout_param_adjoint_model as rpm
import rollout_tree_adjoint_cases as tc
import rollout_tree_adjoint_model as rtm
from conftest import PKG, ROOT

pytestmark = pytest.mark.gpu

L = tc.L
T, B = tc.TICKS, tc.B
HANDLES = {(6, 2, 3): "always", (17, 7, 12): "never"}      # the runtime-sized kernel | the tuned instantiation
LOOPS = {(6, 2, 3): tuple(range(B)), (17, 7, 12): tc.TUNED_LOOPS}
KEYS = ("grad_state0", "grad_gains", "flags")
NEW_KEYS = ("grad_params", "grad_traj_pos", "grad_traj_vel", "grad_traj_alpha")
UNREAD = tuple(f for f in rpm.PARAM_FIELDS if f[0] in ("INERTIA_B", "AMOM0", "DJ"))


@pytest.fixture(scope="module")
def ro(solver_mod):
    return importlib.import_module(PKG + ".rollout")


@pytest.fixture(scope="module")
def ag(solver_mod):
    return importlib.import_module(PKG + ".autograd")


def _inputs(horizon, idx=None):
    idx = np.asarray(LOOPS[tuple(horizon)] if idx is None else idx)
    st, pa = tc.plants()
    lb, sb = tc.loss_weights()
    return st[idx], pa[idx], tc.gains(L.MPCConfig, horizon)[idx], lb[:, idx], sb[idx]


def _rollout(ro, ag, horizon, st, pa, gains, tree=True, adjoint=True, selector=None):
    """a rollout of len(st) loops on the tree plant (tree=False: the parametric one), under their own rows of gains, reset"""
    cfg = tc.config(L.MPCConfig, horizon)
    pos, vel, alpha, adt = tc.trajectory()
    r = ro.ClosedLoopRollout(cfg, len(st), pos, vel, alpha, adt, device=0, runtime=HANDLES[tuple(horizon)], adjoint=True)
    try:
        if selector is not None:
            r.mpc.set_kinematics_options(selector)
        if tree:
            r.set_tree(tc.tree(), adjoint=adjoint)
        r.set_tunables(configs=ag.configs_of(cfg, gains))
        r.reset(st, pa)
    except Exception:
        r.close()
        raise
    return r


def _sweep(ro, ag, horizon, idx=None, selector=None):
    """(log, final state, backward_full, backward) of the horizon's loops (or loops idx)"""
    st, pa, g, lb, sb = _inputs(horizon, idx)
    r = _rollout(ro, ag, horizon, st, pa, g, selector=selector)
    try:
        log = r.run(T, tape=True)
        final = r.state()
        return log, final, r.backward(lb, sb, params=True, traj=True), r.backward(lb, sb)
    finally:
        r.close()


@pytest.fixture(scope="module")
def sweeps(ro, ag):
    return {hz: _sweep(ro, ag, hz) for hz in tc.HORIZONS}


def _against_model(full, i, m):
    """loop row i of the device against the model m: the worst error of each group of outputs in units of its bar"""
    es, fs = ram.field_errors(full["grad_state0"][i, :ram.NS], m["grad_state0"], ram.STATE_FIELDS)
    ec, fc = ram.field_errors(full["grad_gains"][i], m["grad_cfg"], am.GRAD_FIELDS)
    n_traj, n_alpha = full["grad_traj_pos"].shape[1], full["grad_traj_alpha"].shape[1]
    row = np.concatenate([full[k][i].reshape(-1) for k in NEW_KEYS[1:]])
    ep, fp = ram.field_errors(full["grad_params"][i], m["grad_params"], rpm.PARAM_FIELDS, pc.FD_BAR, pc.FD_FLOOR)
    et, ft = ram.field_errors(row, pc.traj_row(m), pc.traj_fields(n_traj, n_alpha), pc.FD_BAR, pc.FD_FLOOR)
    return {"state0": (es, fs), "gains": (ec, fc), "params": (ep, fp), "tracks": (et, ft)}


@pytest.mark.parametrize("horizon", tc.HORIZONS)
def test_sweep_matches_model(sweeps, horizon):
    log, final, full, plain = sweeps[horizon]
    worst = 0.0
    for i, b in enumerate(LOOPS[horizon]):
        m = tc.model(b, horizon)
        assert np.array_equal(log[:, i, 14], m["log"][:, 14]), (b, log[:, i, 14])
        assert ((log[:, i, 14] == L.STATUS_SOLVED).all()) == (b != tc.UNSOLVED)
        assert np.abs(log[:, i, :14] - m["log"][:, :14]).max() <= 1e-8 * np.abs(m["log"][:, :14]).max(), b
        if b == tc.UNSOLVED:           # NaN thrust references in, NaN out where the final state's cotangent meets them
            continue
        errs = _against_model(full, i, m)
        print(f"{horizon} loop {b} ({tc.NAMES[b]}): " + ", ".join(f"{k} {e:.2e} of the bar ({f})" for k, (e, f) in errs.items()))
        worst = max(worst, max(e for e, _ in errs.values()))
        assert all(e <= 1.0 for e, _ in errs.values()), (horizon, b, errs)
        assert full["flags"][i] == m["flags"] == 0
        # what the tree plant does not read, the structural entries, samples no tick touches: +0.0 where the model has +0.0
        for _, off, n in UNREAD:
            blk = full["grad_params"][i, off:off + n]
            assert (blk == 0.0).all() and not np.signbit(blk).any(), (b, off)
        zero = m["grad_params"] == 0.0
        assert (full["grad_params"][i][zero] == 0.0).all() and not np.signbit(full["grad_params"][i][zero]).any()
    print(f"{horizon}: worst {worst:.2e} of its bar")
    for k in KEYS:                                                   # the plain outputs, bit for bit, from both entries
        assert np.array_equal(full[k], plain[k], equal_nan=True), (horizon, k)
    tail = full["grad_state0"][:, ram.NS:]
    assert (tail == 0.0).all() and not np.signbit(tail).any()
    if horizon == tc.HORIZONS[0]:
        assert (log[:, tc.BOXED, 15] > 0).any()                      # the boxed loop's active-set passes did run


def test_taped_run_is_the_untaped_run_bit_for_bit(ro, ag, sweeps):
    for hz in tc.HORIZONS:
        st, pa, g, lb, sb = _inputs(hz)
        r = _rollout(ro, ag, hz, st, pa, g)
        try:
            plain_log, plain_state = r.run(T), r.state()
            with pytest.raises(Exception, match="invalid argument"):      # an untaped run leaves no tape
                r.backward(None, sb)
        finally:
            r.close()
        assert np.array_equal(plain_log, sweeps[hz][0], equal_nan=True) and np.array_equal(plain_state, sweeps[hz][1], equal_nan=True)


def test_never_solved_loop_keeps_its_plant_share(sweeps, ref):
    hz = tc.HORIZONS[0]
    log, final, full, _ = sweeps[hz]
    b = tc.UNSOLVED
    assert (log[:, b, 14] != L.STATUS_SOLVED).all() and full["flags"][b] == L.ADJ_UNSOLVED
    assert (full["flags"][[i for i in range(B) if i != b]] == 0).all()
    m = tc.model(b, hz)
    live = np.r_[0:L.PS_TDES]                                        # the thrust references are NaN, and stay where they are
    assert np.isfinite(full["grad_state0"][b, live]).all() and (full["grad_gains"][b] == 0.0).all()
    es, fs = ram.field_errors(full["grad_state0"][b, live], m["grad_state0"][live], tuple(f for f in ram.STATE_FIELDS if f[1] < L.PS_TDES))
    print(f"never solved: state0 {es:.2e} of the bar ({fs})")
    assert es <= 1.0, (es, fs)
    gp = full["grad_params"][b]
    assert gp[L.PP_MASS] != 0.0 and abs(gp[L.PP_MASS] - m["grad_params"][L.PP_MASS]) <= pc.FD_BAR * abs(m["grad_params"][L.PP_MASS])
    assert (full["grad_traj_alpha"][b] != 0.0).any() and (full["grad_traj_pos"][b] == 0.0).all()
    # the joints' cotangent is the final joints' plus what A_mom(q) and I_B(q) hand back through J at every tick
    _, sb = tc.loss_weights()
    assert (full["grad_state0"][b, L.PS_Q:L.PS_Q + 8] != sb[b, L.PS_Q:L.PS_Q + 8]).all()


def test_batches_and_permutations_are_bit_identical(ro, ag, sweeps):
    hz = tc.HORIZONS[0]
    base = sweeps[hz][2]
    solved = np.array([i for i in range(B) if i != tc.UNSOLVED])
    for idx in (np.array([tc.POSED]), solved[np.arange(257) % len(solved)], np.array([4, 2, 0, 1, 1, 0, 2, 4])):
        _, _, full, plain = _sweep(ro, ag, hz, idx)
        for k in KEYS + NEW_KEYS:
            assert np.array_equal(full[k], base[k][idx]), (len(idx), k)
        for k in KEYS:
            assert np.array_equal(full[k], plain[k]), (len(idx), k)


def test_selector_is_kept_with_the_tape(ro, ag, sweeps, ref):
    """Loop 1 under a joint selector that is not the default, against the model under that selector; then the selector is
    changed between the taped run and the sweep: nothing changes."""
    hz = tc.HORIZONS[0]
    b, sel = tc.SELECTED
    st, pa, g, lb, sb = _inputs(hz, [b])
    r = _rollout(ro, ag, hz, st, pa, g, selector=sel)
    try:
        log = r.run(T, tape=True)
        first = r.backward(lb, sb, params=True, traj=True)
        r.mpc.set_kinematics_options(range(3, 11))
        second = r.backward(lb, sb, params=True, traj=True)
    finally:
        r.close()
    for k in KEYS + NEW_KEYS:
        assert np.array_equal(first[k], second[k]), k
    m = tc.model(b, hz, sel)
    assert (log[:, 0, 14] == L.STATUS_SOLVED).all()
    assert np.abs(log[:, 0, :14] - m["log"][:, :14]).max() <= 1e-8 * np.abs(m["log"][:, :14]).max()
    errs = _against_model(first, 0, m)
    print("selected: " + ", ".join(f"{k} {e:.2e} of the bar ({f})" for k, (e, f) in errs.items()))
    assert all(e <= 1.0 for e, _ in errs.values()), errs
    assert not np.array_equal(first["grad_state0"][0], sweeps[hz][2]["grad_state0"][b])      # the selector does matter


def test_central_difference_of_the_device_rollout(ro, ag, sweeps, ref):
    """the posed loop, +-h along one random direction in (state0, gains) on the device's own forward run; the same quotient of
    the CPU model shows the step's truncation error: the bar is 10 times its error"""
    hz, b, h = tc.HORIZONS[0], tc.POSED, 1e-3
    st, pa, g, lb, sb = _inputs(hz, [b])
    rng = np.random.default_rng(tc.SEED + 11)
    ds = rng.normal(size=ram.NS) * ram.state_scale() * h
    dg = rng.normal(size=32) * g[0] * h
    dg[29:] = 0.0
    S = np.concatenate([st, st])
    S[0, :ram.NS] += ds
    S[1, :ram.NS] -= ds
    r = _rollout(ro, ag, hz, S, np.concatenate([pa, pa]), np.concatenate([g + dg, g - dg]), adjoint=False)
    try:
        log = r.run(T)
        final = r.state()
    finally:
        r.close()
    assert (log[:, :, 14] == L.STATUS_SOLVED).all()
    fd_dev = (ram.loss(log[:, 0], final[0], lb[:, 0], sb[0]) - ram.loss(log[:, 1], final[1], lb[:, 0], sb[0])) / 2.0
    full = sweeps[hz][2]
    m = tc.model(b, hz)
    an_dev = full["grad_state0"][b, :ram.NS] @ ds + full["grad_gains"][b] @ dg
    an_cpu = m["grad_state0"] @ ds + m["grad_cfg"] @ dg
    cfg, s0, p, traj, _, _ = tc.loop_inputs(ref, b, hz)
    rtm.set_tree(tc.tree())
    try:
        fd_cpu = ram.central(cfg, s0, p, traj, T, lb[:, 0], sb[0], d_state=ds, d_gains=dg, step=1.0, richardson=False)
    finally:
        rtm.set_tree(None)
    e_dev, e_cpu = abs(fd_dev - an_dev) / abs(an_cpu), abs(fd_cpu - an_cpu) / abs(an_cpu)
    print(f"quotient against adjoint: device {e_dev:.2e}, CPU model {e_cpu:.2e}")
    assert e_dev <= 10.0 * e_cpu, (e_dev, e_cpu)


def test_autograd_rollout(ro, ag, sweeps):
    import torch
    hz = tc.HORIZONS[0]
    idx = [i for i in range(B) if i != tc.UNSOLVED]
    st, pa, g, lb, sb = _inputs(hz, idx)
    _, _, base, _ = _sweep(ro, ag, hz, idx)
    pos, vel, alpha, adt = tc.trajectory()
    r = ro.ClosedLoopRollout(tc.config(L.MPCConfig, hz), len(idx), pos, vel, alpha, adt, device=0, runtime="always", adjoint=True)
    try:
        r.set_tree(tc.tree(), adjoint=True)
        t = lambda a, grad=True: torch.tensor(a, dtype=torch.float64, device="cuda", requires_grad=grad)
        weights = (t(lb[:, :, :14], False), t(sb[:, :ram.NS], False))
        state0, gains, params = t(st[:, :ram.NS]), t(g), t(pa)
        tlog, tfinal = ag.rollout(r, state0, gains, params, T, None)
        assert np.array_equal(tlog.detach().cpu().numpy(), sweeps[hz][0][:, idx, :14])
        ((tlog * weights[0]).sum() + (tfinal * weights[1]).sum()).backward()
        assert np.array_equal(state0.grad.cpu().numpy(), base["grad_state0"][:, :ram.NS])
        assert np.array_equal(gains.grad.cpu().numpy(), base["grad_gains"])
        assert np.array_equal(params.grad.cpu().numpy(), base["grad_params"])
    finally:
        r.close()


def test_set_tree_none_returns_to_the_parametric_plant(ro, ag):
    hz = tc.HORIZONS[0]
    st, pa = rc.plants()
    g = rc.gains(L.MPCConfig, hz)
    lb, sb = rc.loss_weights()
    r = _rollout(ro, ag, hz, st, pa, g, tree=False)
    try:
        want_log = r.run(T, tape=True)
        want = r.backward(lb, sb, params=True, traj=True)
    finally:
        r.close()
    r = _rollout(ro, ag, hz, st, pa, g, tree=True)
    try:
        tree_log = r.run(T, tape=True)
        r.backward(lb, sb, params=True, traj=True)
        r.set_tree(None)
        r.reset(st, pa)
        got_log = r.run(T, tape=True)
        got = r.backward(lb, sb, params=True, traj=True)
        # and the flag is not sticky: a tree set without it refuses as it always did
        r.set_tree(tc.tree())
        r.reset(st, pa)
        with pytest.raises(Exception, match="(?i)run_taped.*tree"):
            r.run(T, tape=True)
    finally:
        r.close()
    assert np.array_equal(got_log, want_log) and not np.array_equal(tree_log, want_log)
    for k in KEYS + NEW_KEYS:
        assert np.array_equal(got[k], want[k]), k


def test_refusals_that_stay(ro, ag):
    hz = tc.HORIZONS[0]
    st, pa, g, lb, sb = _inputs(hz)
    pos = tc.trajectory()[0]
    jp = importlib.import_module(PKG + ".jet_plant")
    gold = np.load(os.path.join(ROOT, "tests", "golden", "jet_lstm.npz"))
    jm = jp.JetModelTotal(gold["w_ih"], gold["w_hh"], gold["b_ih"], gold["b_hh"], gold["fc_w"], gold["fc_b"], gold["norm"],
                          device=0, max_series=64)
    r = _rollout(ro, ag, hz, st, pa, g)
    try:
        for name, on, off in (("jet plant", lambda: r.set_jet_plant(jm), lambda: r.set_jet_plant(None)),
                              ("RPYDot", lambda: r.set_attitude_tracks(None, np.zeros((len(pos), 3))),
                               lambda: r.set_attitude_tracks(None, None))):
            on()
            r.reset(st, pa)
            with pytest.raises(Exception, match="(?i)run_taped.*" + name.split()[0]):
                r.run(T, tape=True)
            r._taped = T
            with pytest.raises(Exception, match="(?i)backward_full.*" + name.split()[0]):
                r.backward(lb, sb, params=True, traj=True)
            off()
        # unknown flag bits; jointsLambdaOption "constant" with the flag
        ctree = importlib.import_module(PKG + ".robot_tree").to_c(tc.tree())
        import ctypes
        assert r.lib.vsmpc_rollout_set_tree_ex(r._r, ctypes.byref(ctree), 2) == -1
        r.mpc.set_kinematics_options(None, constant_lambda=True)
        assert r.lib.vsmpc_rollout_set_tree_ex(r._r, ctypes.byref(ctree), 1) == -2
        r.mpc.set_kinematics_options(None, constant_lambda=False)
        # the refused calls left the rollout as it was: still the tree plant with its adjoint
        r.reset(st, pa)
        r.run(T, tape=True)
        solved = [i for i in range(B) if i != tc.UNSOLVED]
        assert np.isfinite(r.backward(lb, sb)["grad_state0"][solved]).all()
    finally:
        r.close()
