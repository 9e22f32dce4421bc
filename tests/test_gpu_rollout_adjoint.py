"""The adjoint of the rollout on the device (vsmpc_rollout_run_taped, vsmpc_rollout_backward[_device], advance_adjoint_kernel,
autograd.rollout) on the four loops of tests/rollout_adjoint_cases.py over 9 ticks at ratio 4:

  against tests/rollout_adjoint_model.py (itself checked against central differences in test_rollout_adjoint_model.py) at the
      project's derivative bar, per field 1e-6 |field|_inf + 1e-12 max |gradient|, on a runtime handle at (6, 2, 3) and on a
      tuned handle at (17, 7, 12);
  against central differences of the device's OWN forward rollout: the perturbed copies ride as extra loops of one batch,
      +-h along six random directions in state0 and six in the gains (through set_tunables).  One quotient with the same h has
      a truncation error that the CPU model's quotient shows too: the bar is 10 times the CPU model's worst error on the same
      inputs (measured on an MI355X: device worst 6.7e-10 of the directional derivative against the model's 7.4e-10 for state0,
      2.4e-5 against 2.4e-5 for the gains, both quotients' own truncation; against the model the sweep's worst field is at
      2.2e-7 of the bar at (6, 2, 3) and 3.1e-6 at (17, 7, 12));
  bitwise: the taped run against the untaped one, the sweep on a repeated and on a permuted batch, per-loop rows against
      single-loop rollouts; unsolved ticks; the refusals.
"""
import importlib
import os

import numpy as np
import pytest

import adjoint_model as am
import rollout_adjoint_cases as rc
import rollout_adjoint_model as ram
from conftest import PKG, ROOT

pytestmark = pytest.mark.gpu

L = rc.L
T, B = rc.TICKS, rc.B
HANDLES = {(6, 2, 3): "always", (17, 7, 12): "never"}      # the runtime-sized kernel | the tuned instantiation


@pytest.fixture(scope="module")
def ro(solver_mod):
    return importlib.import_module(PKG + ".rollout")


@pytest.fixture(scope="module")
def ag(solver_mod):
    return importlib.import_module(PKG + ".autograd")


def _configs(ag, cfg, gains):
    return ag.configs_of(cfg, gains)


def _loops(ro, ag, horizon, st, pa, gains=None, adjoint=True):
    """a rollout of len(st) loops at `horizon`, reset: per-loop rows when `gains` is given"""
    cfg = rc.config(L.MPCConfig, horizon)
    pos, vel, alpha, adt = rc.trajectory()
    r = ro.ClosedLoopRollout(cfg, len(st), pos, vel, alpha, adt, device=0, runtime=HANDLES[tuple(horizon)], adjoint=adjoint)
    try:
        if gains is not None:
            r.set_tunables(configs=_configs(ag, cfg, gains))
        r.reset(st, pa)
    except Exception:
        r.close()
        raise
    return r


def _sweep(ro, ag, horizon, st, pa, gains, lb, sb):
    r = _loops(ro, ag, horizon, st, pa, gains)
    try:
        log = r.run(T, tape=True)
        return log, r.state(), r.backward(lb, sb)
    finally:
        r.close()


@pytest.fixture(scope="module")
def device_sweeps(ro, ag):
    """horizon -> (log, final state, backward()) of the four loops, computed once"""
    st, pa = rc.plants()
    lb, sb = rc.loss_weights()
    return {hz: _sweep(ro, ag, hz, st, pa, rc.gains(L.MPCConfig, hz), lb, sb) for hz in rc.HORIZONS}


@pytest.mark.parametrize("horizon", rc.HORIZONS)
def test_sweep_matches_model(device_sweeps, horizon):
    log, final, out = device_sweeps[horizon]
    m = rc.model(horizon)
    assert (log[:, :, 14] == L.STATUS_SOLVED).all() and np.array_equal(log[:, :, 14], m["log"][:, :, 14])
    assert np.abs(log[:, :, :14] - m["log"][:, :, :14]).max() <= 1e-8 * np.abs(m["log"][:, :, :14]).max()
    # loop 2 sits on the 100 % clamp from its first release tick on (the pinned ticks in between return the throttle
    # through v(u) and back: 100 to rounding)
    assert (log[3, 2, 10:14] == 100.0).all() and (log[7, 2, 10:14] == 100.0).all() and (log[3:, 2, 10:14] > 100.0 - 1e-9).all()
    worst = 0.0
    for b in range(B):
        es, fs = ram.field_errors(out["grad_state0"][b, :ram.NS], m["grad_state0"][b], ram.STATE_FIELDS)
        ec, fc = ram.field_errors(out["grad_gains"][b], m["grad_cfg"][b], am.GRAD_FIELDS)
        print(f"{horizon} loop {b} ({rc.NAMES[b]}): state0 {es:.2e} of the bar ({fs}), gains {ec:.2e} ({fc})")
        worst = max(worst, es, ec)
        assert es <= 1.0 and ec <= 1.0, (horizon, b, es, fs, ec, fc)
    print(f"{horizon}: worst {worst:.2e} of the bar")
    assert np.array_equal(out["flags"], m["flags"]) and (out["flags"] == 0).all()
    # the jet-plant slots carry nothing: +0.0
    tail = out["grad_state0"][:, ram.NS:]
    assert (tail == 0.0).all() and not np.signbit(tail).any()


N_DIR, STEP = 6, 1e-3


def _directions():
    rng = np.random.default_rng(rc.SEED + 11)
    ds = rng.normal(size=(N_DIR, ram.NS)) * ram.state_scale() * STEP
    g0 = rc.gains(L.MPCConfig, rc.HORIZONS[0])
    dg = rng.normal(size=(N_DIR, B, 32)) * g0 * STEP
    dg[:, :, 29:] = 0.0
    dg[:, :, 29] = rng.normal(size=(N_DIR, B)) * STEP * 10.0         # throttle_min is 0: an absolute step, in percent
    dg[:, :, 30] = rng.normal(size=(N_DIR, B)) * STEP * 100.0
    return ds, dg


def test_central_differences_of_the_device_rollout(ro, ag, device_sweeps, ref):
    hz = rc.HORIZONS[0]
    st, pa = rc.plants()
    g = rc.gains(L.MPCConfig, hz)
    lb, sb = rc.loss_weights()
    ds, dg = _directions()
    # one batch: the four loops, then +d and -d of every state direction, then of every gains direction
    S, P, G = [st], [pa], [g]
    for k in range(N_DIR):
        for sign in (1.0, -1.0):
            s = st.copy()
            s[:, :ram.NS] += sign * ds[k]
            S.append(s), P.append(pa), G.append(g)
    for k in range(N_DIR):
        for sign in (1.0, -1.0):
            S.append(st), P.append(pa), G.append(g + sign * dg[k])
    S, P, G = np.concatenate(S), np.concatenate(P), np.concatenate(G)
    r = _loops(ro, ag, hz, S, P, G, adjoint=False)
    try:
        log = r.run(T)
        final = r.state()
    finally:
        r.close()
    assert (log[:, :, 14] == L.STATUS_SOLVED).all()
    loss = np.array([ram.loss(log[:, i], final[i], lb[:, i % B], sb[i % B]) for i in range(len(S))])
    out = device_sweeps[hz][2]
    m = rc.model(hz)
    cfg0 = rc.config(ref.Config, hz)
    traj = rc.trajectory()
    worst = {"state0": [0.0, 0.0], "gains": [0.0, 0.0]}               # [device, CPU model]
    for b in range(B):
        cfg = ram.with_gains(cfg0, g[b])
        for k in range(N_DIR):
            for kind, d_state, d_gains, base in (("state0", ds[k], None, B), ("gains", None, dg[k, b], B + 2 * N_DIR * B)):
                fd_dev = (loss[base + 2 * k * B + b] - loss[base + (2 * k + 1) * B + b]) / 2.0
                fd_cpu = ram.central(cfg, st[b], pa[b], traj, T, lb[:, b], sb[b], d_state=d_state, d_gains=d_gains, step=1.0,
                                     richardson=False)
                if kind == "state0":
                    an_dev, an_cpu = out["grad_state0"][b, :ram.NS] @ d_state, m["grad_state0"][b] @ d_state
                else:
                    an_dev, an_cpu = out["grad_gains"][b] @ d_gains, m["grad_cfg"][b] @ d_gains
                worst[kind][0] = max(worst[kind][0], abs(fd_dev - an_dev) / abs(an_cpu))
                worst[kind][1] = max(worst[kind][1], abs(fd_cpu - an_cpu) / abs(an_cpu))
    for kind, (dev, cpu) in worst.items():
        print(f"{kind}: quotient against adjoint, worst relative error: device {dev:.2e}, CPU model {cpu:.2e}")
        assert dev <= 10.0 * cpu, (kind, dev, cpu)


def test_taped_run_is_the_untaped_run_bit_for_bit(ro, ag):
    st, pa = rc.plants()
    for hz in rc.HORIZONS:
        g = rc.gains(L.MPCConfig, hz)
        r = _loops(ro, ag, hz, st, pa, g)
        try:
            plain_log, plain_state = r.run(T), r.state()
            r.reset(st, pa)
            taped_log, taped_state = r.run(T, tape=True), r.state()
            assert np.array_equal(plain_log, taped_log) and np.array_equal(plain_state, taped_state)
            # an untaped run invalidates the tape
            r.run(1)
            with pytest.raises(Exception):
                r.backward(None, np.ones((B, L.PLANT_STATE)))
        finally:
            r.close()


def test_tape_of_a_run_that_did_not_begin_at_the_reset(ro, ag, ref):
    """two untaped ticks, then seven taped ones: the sweep ends at the state in front of tick 2, counts the release ticks from
    the rollout's own tick counter and treats the window it found as a constant"""
    hz = rc.HORIZONS[0]
    st, pa = rc.plants()
    g = rc.gains(L.MPCConfig, hz)
    lb, sb = rc.loss_weights()
    r = _loops(ro, ag, hz, st, pa, g)
    try:
        r.run(2)
        r.run(T - 2, tape=True)
        out = r.backward(lb[2:], sb)
    finally:
        r.close()
    m = rc.model(hz)
    for b in range(B):
        cfg = ram.with_gains(rc.config(ref.Config, hz), g[b])
        want = ram.backward(cfg, m["tapes"][b][2:], pa[b], rc.trajectory(), lb[2:, b], sb[b], first=False, tick_base=2)
        es, fs = ram.field_errors(out["grad_state0"][b, :ram.NS], want["grad_state0"], ram.STATE_FIELDS)
        ec, fc = ram.field_errors(out["grad_gains"][b], want["grad_cfg"], am.GRAD_FIELDS)
        assert es <= 1.0 and ec <= 1.0, (b, es, fs, ec, fc)
        assert not np.array_equal(want["grad_cfg"], m["grad_cfg"][b])


def test_sweep_is_bit_identical_on_repeated_and_permuted_batches(ro, ag, device_sweeps):
    hz = rc.HORIZONS[0]
    st, pa = rc.plants()
    g = rc.gains(L.MPCConfig, hz)
    lb, sb = rc.loss_weights()
    base = device_sweeps[hz][2]
    perm = np.array([2, 0, 3, 1, 1, 3, 0, 2])                        # every loop twice, permuted
    _, _, out = _sweep(ro, ag, hz, st[perm], pa[perm], g[perm], lb[:, perm], sb[perm])
    for k in ("grad_state0", "grad_gains", "flags"):
        assert np.array_equal(out[k], base[k][perm]), k
    # and a second sweep over the same tape gives the same bits
    r = _loops(ro, ag, hz, st, pa, g)
    try:
        r.run(T, tape=True)
        one, two = r.backward(lb, sb), r.backward(lb, sb)
        for k in one:
            assert np.array_equal(one[k], two[k]) and np.array_equal(one[k], base[k]), k
        # either cotangent alone; both missing is refused
        only_state = r.backward(None, sb)
        only_log = r.backward(lb, None)
        assert np.isfinite(only_state["grad_state0"]).all() and np.isfinite(only_log["grad_state0"]).all()
        with pytest.raises(Exception, match="invalid argument"):
            r.backward(None, None)
    finally:
        r.close()


def test_per_loop_rows_match_single_loop_rollouts(ro, ag, device_sweeps):
    hz = rc.HORIZONS[0]
    st, pa = rc.plants()
    g = rc.gains(L.MPCConfig, hz)
    lb, sb = rc.loss_weights()
    base = device_sweeps[hz][2]
    for b in range(B):
        own = _configs(ag, rc.config(L.MPCConfig, hz), g[b:b + 1])[0]
        pos, vel, alpha, adt = rc.trajectory()
        r = ro.ClosedLoopRollout(own, 1, pos, vel, alpha, adt, device=0, runtime=HANDLES[hz], adjoint=True)
        try:
            r.reset(st[b:b + 1], pa[b:b + 1])
            r.run(T, tape=True)
            out = r.backward(lb[:, b:b + 1], sb[b:b + 1])
        finally:
            r.close()
        assert np.array_equal(out["grad_gains"][0], base["grad_gains"][b]), b
        assert np.array_equal(out["grad_state0"][0], base["grad_state0"][b]), b


def test_unsolved_ticks_pass_through(ro, ag):
    """Loop 3 starts with NaN thrust references (rollout_adjoint_cases.plants): IN_TDES is NaN in every record of it, every
    factorisation fails, no tick is Solved and no move is consumed, while the plant, which does not read those entries, flies
    on with its latched commands.  The sweep flags the loop, passes the latched entries' cotangents straight through and
    leaves the other loops' gradients as they were.  (A NaN that reaches only the gradient of the QP -- a window entry, alpha
    -- does not serve: the solve kernels report such a tick as Solved, with a NaN move.)"""
    hz = rc.HORIZONS[0]
    st, pa = rc.plants(unsolved_loop=3)
    g = rc.gains(L.MPCConfig, hz)
    lb, sb = rc.loss_weights()
    log, final, out = _sweep(ro, ag, hz, st, pa, g, lb, sb)
    m = rc.model(hz, unsolved_loop=3)
    print("status on the device:", log[:, :, 14].T.astype(int).tolist())
    assert (log[:, 3, 14] != L.STATUS_SOLVED).all() and (log[:, :3, 14] == L.STATUS_SOLVED).all()
    assert np.isfinite(final[:, :L.PS_TDES]).all()
    assert out["flags"].tolist() == [0, 0, 0, L.ADJ_UNSOLVED] == m["flags"].tolist()
    assert np.isfinite(out["grad_state0"]).all() and np.isfinite(out["grad_gains"]).all()
    for b in range(B):
        es, fs = ram.field_errors(out["grad_state0"][b, :ram.NS], m["grad_state0"][b], ram.STATE_FIELDS)
        print(f"loop {b}: state0 {es:.2e} of the bar ({fs})")
        assert es <= 1.0, (b, es, fs)
    for b in range(3):
        ec, fc = ram.field_errors(out["grad_gains"][b], m["grad_cfg"][b], am.GRAD_FIELDS)
        assert ec <= 1.0, (b, ec, fc)
    assert (out["grad_gains"][3] == 0.0).all() and (m["grad_cfg"][3] == 0.0).all()
    # pass-through, bit for bit: nothing but the final-state cotangent reaches the thrust references, the joints' cotangent
    # is that of the final joints plus what A_mom(q) hands back at every tick
    assert np.array_equal(out["grad_state0"][3, L.PS_TDES:L.PS_TDES + 8], sb[3, L.PS_TDES:L.PS_TDES + 8])
    assert (out["grad_state0"][3, L.PS_Q:L.PS_Q + 8] != sb[3, L.PS_Q:L.PS_Q + 8]).all()


def test_refusals(ro, ag):
    hz = (17, 7, 12)
    st, pa = rc.plants()
    pos, vel, alpha, adt = rc.trajectory()
    cfg = rc.config(L.MPCConfig, hz)
    RT = importlib.import_module(PKG + ".robot_tree")
    jp = importlib.import_module(PKG + ".jet_plant")
    gold = np.load(os.path.join(ROOT, "tests", "golden", "jet_lstm.npz"))
    jm = jp.JetModelTotal(gold["w_ih"], gold["w_hh"], gold["b_ih"], gold["b_hh"], gold["fc_w"], gold["fc_b"], gold["norm"],
                          device=0, max_series=64)
    r = ro.ClosedLoopRollout(cfg, B, pos, vel, alpha, adt, device=0, adjoint=True)
    try:
        for name, on, off in (("tree", lambda: r.set_tree(RT.default_tree()), lambda: r.set_tree(None)),
                              ("jet plant", lambda: r.set_jet_plant(jm), lambda: r.set_jet_plant(None)),
                              ("RPYDot", lambda: r.set_attitude_tracks(None, np.zeros((len(pos), 3))),
                               lambda: r.set_attitude_tracks(None, None))):
            on()
            r.reset(st, pa)
            with pytest.raises(Exception, match="(?i)" + name.split()[0]):
                r.run(2, tape=True)
            assert r.run(2).shape == (2, B, L.ROLLOUT_LOG)            # still runs untaped
            off()
        r.reset(st, pa)
        r.run(2, tape=True)                                          # and taped again once the option is gone
        assert np.isfinite(r.backward(None, np.ones((B, L.PLANT_STATE)))["grad_state0"]).all()
    finally:
        r.close()
    # a handle without VSMPC_CREATE_ADJOINT_RECORD: the tape is taken, the sweep is refused and names the flag
    r = ro.ClosedLoopRollout(cfg, B, pos, vel, alpha, adt, device=0)
    try:
        r.reset(st, pa)
        r.run(2, tape=True)
        with pytest.raises(Exception, match="VSMPC_CREATE_ADJOINT_RECORD"):
            r.backward(None, np.ones((B, L.PLANT_STATE)))
    finally:
        r.close()


def test_autograd_rollout(ro, ag, device_sweeps):
    import torch
    hz = rc.HORIZONS[0]
    st, pa = rc.plants()
    g = rc.gains(L.MPCConfig, hz)
    lb, sb = rc.loss_weights()
    log, final, base = device_sweeps[hz]
    pos, vel, alpha, adt = rc.trajectory()
    r = ro.ClosedLoopRollout(rc.config(L.MPCConfig, hz), B, pos, vel, alpha, adt, device=0, runtime=HANDLES[hz], adjoint=True)
    try:
        state0 = torch.tensor(st[:, :ram.NS], dtype=torch.float64, device="cuda", requires_grad=True)
        gains = torch.tensor(g, dtype=torch.float64, device="cuda", requires_grad=True)
        info = {}
        tlog, tfinal = ag.rollout(r, state0, gains, pa, T, info)
        assert np.array_equal(tlog.detach().cpu().numpy(), log[:, :, :14])
        assert np.array_equal(tfinal.detach().cpu().numpy(), final[:, :ram.NS])
        loss = (tlog * torch.tensor(lb[:, :, :14], device="cuda")).sum() + (tfinal * torch.tensor(sb[:, :ram.NS], device="cuda")).sum()
        loss.backward()
        assert np.array_equal(state0.grad.cpu().numpy(), base["grad_state0"][:, :ram.NS])
        assert np.array_equal(gains.grad.cpu().numpy(), base["grad_gains"])
        assert np.array_equal(info["flags"].cpu().numpy(), base["flags"])
    finally:
        r.close()
