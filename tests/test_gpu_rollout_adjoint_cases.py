"""The adjoint of the rollout on the device (vsmpc_rollout_run_taped, vsmpc_rollout_backward, advance_adjoint_kernel; with them
the first runs of advance_kernel and assemble_record at 1 and 16 sub-steps and at ratios 2, 10 and a rounded 20) on the cases
of tests/rollout_adjoint_edge_cases.py: one rollout per case, the runtime-sized handle at (6, 2, 3) and (40, 2, 40), the tuned
one at (17, 7, 12).  Per case:

  the device log against tests/rollout_adjoint_model.py's forward loop (statuses equal, columns 0 .. 13 within 1e-8 of the
      largest), the taped run against the untaped one bit for bit;
  backward against the model's sweep (itself held to central differences in test_rollout_adjoint_edge_cases.py) at the
      project's derivative bar, per field 1e-6 |field|_inf + 1e-12 max |gradient|; flags equal; the jet-plant tail +0.0;
  boxed: the loop under its own row against a single-loop rollout created under that configuration, and the loops beside it
      against a batch without it, bit for bit;
  batches of 1 and of 257 loops (rollout_adjoint_cases.py's four, permuted) against the four-loop sweep bit for bit; a second,
      longer taped run on the same rollout (the tape grows, the run does not begin at the reset) against the model;
  tilted and boxed: central differences of the device's OWN forward rollout along six directions in state0 and six in the
      gains, the perturbed loops as extra loops of one batch; the bar is 10 times the CPU model's quotient error on the same
      inputs.

Measured on an MI355X, worst share of the derivative bar per case (state0 | gains): sub1 1.2e-9 | 2.5e-6, sub16_ratio2
2.0e-9 | 1.1e-6, paper_rt 3.5e-9 | 2.6e-8, paper_tuned 6.4e-9 | 4.4e-8, rounded_ratio 9.6e-10 | 1.7e-6, trajectory_end 2.3e-9 |
9.3e-8, trajectory_one 6.6e-10 | 1.7e-7, long_window 4.2e-9 | 7.1e-7, tilted 8.4e-10 | 1.0e-7, boxed 9.0e-10 | 1.9e-6; the
second, longer run 2.1e-9 | 4.6e-7; every log within 2.6e-15 of its largest entry.  The device's quotient against its adjoint,
relative to the directional derivative, with the CPU model's figure behind it: tilted 3.5e-9 (3.5e-9) in state0 and 4.4e-6
(4.4e-6) in the gains, boxed 1.4e-9 (1.7e-9) and 6.6e-6 (6.6e-6).  Nothing had to be fixed."""
import importlib

import numpy as np
import pytest

import adjoint_model as am
import rollout_adjoint_cases as rc
import rollout_adjoint_edge_cases as ec
import rollout_adjoint_model as ram
from conftest import PKG

pytestmark = pytest.mark.gpu

L = rc.L


@pytest.fixture(scope="module")
def ro(solver_mod):
    return importlib.import_module(PKG + ".rollout")


@pytest.fixture(scope="module")
def ag(solver_mod):
    return importlib.import_module(PKG + ".autograd")


def _rollout(ro, ag, case, st, pa, gains, adjoint=True, own_config=False):
    """a rollout of the loops (st, pa) under the case's configuration, reset: every loop under its own row of `gains`, or
    (own_config, one loop) created under that row's configuration"""
    c = ec.CASES[case]
    cfg = ec.config(L.MPCConfig, case)
    rows = ag.configs_of(cfg, gains)
    pos, vel, alpha, adt = ec.trajectory(case)
    r = ro.ClosedLoopRollout(rows[0] if own_config else cfg, len(st), pos, vel, alpha, adt, device=0, runtime=c.runtime,
                             adjoint=adjoint)
    try:
        if not own_config:
            r.set_tunables(configs=rows)
        r.reset(st, pa)
    except Exception:
        r.close()
        raise
    return r


def _sweep(ro, ag, case, loops=None, own_config=False):
    """(log, final state, backward()) of the case's loops, or of the listed ones"""
    st, pa = ec.plants(case)
    g = ec.gains(L.MPCConfig, case)
    lb, sb = ec.case_loss_weights(case)
    idx = list(range(len(st))) if loops is None else list(loops)
    r = _rollout(ro, ag, case, st[idx], pa[idx], g[idx], own_config=own_config)
    try:
        log = r.run(ec.CASES[case].ticks, tape=True)
        return log, r.state(), r.backward(lb[:, idx], sb[idx])
    finally:
        r.close()


@pytest.fixture(scope="module")
def sweeps(ro, ag):
    """case -> _sweep of all its loops, computed when first asked for"""
    cache = {}

    def get(case):
        if case not in cache:
            cache[case] = _sweep(ro, ag, case)
        return cache[case]
    return get


def _against_model(got, want_state0, want_cfg):
    es, fs = ram.field_errors(got["grad_state0"][:ram.NS], want_state0, ram.STATE_FIELDS)
    eg, fg = ram.field_errors(got["grad_gains"], want_cfg, am.GRAD_FIELDS)
    return es, fs, eg, fg


@pytest.mark.parametrize("case", list(ec.CASES))
def test_case_matches_model(ro, ag, sweeps, case):
    c = ec.CASES[case]
    m = ec.model(case)
    st, pa = ec.plants(case)
    # the untaped run on a rollout of its own, then the taped one with its sweep
    r = _rollout(ro, ag, case, st, pa, ec.gains(L.MPCConfig, case))
    try:
        plain_log, plain_state = r.run(c.ticks), r.state()
    finally:
        r.close()
    log, final, out = sweeps(case)
    assert np.array_equal(plain_log, log) and np.array_equal(plain_state, final)
    assert (log[:, :, 14] == L.STATUS_SOLVED).all() and np.array_equal(log[:, :, 14], m["log"][:, :, 14])
    err = np.abs(log[:, :, :14] - m["log"][:, :, :14]).max() / np.abs(m["log"][:, :, :14]).max()
    print(f"{case}: log {err:.2e} of the largest entry")
    assert err <= 1e-8
    worst = [0.0, 0.0]
    for b in range(len(st)):
        es, fs, eg, fg = _against_model({k: v[b] for k, v in out.items()}, m["grad_state0"][b], m["grad_cfg"][b])
        print(f"{case} loop {b} ({c.loops[b]}): state0 {es:.2e} of the bar ({fs}), gains {eg:.2e} ({fg})")
        worst = [max(worst[0], es), max(worst[1], eg)]
        assert es <= 1.0 and eg <= 1.0, (case, b, es, fs, eg, fg)
    print(f"{case}: worst share of the bar: state0 {worst[0]:.2e}, gains {worst[1]:.2e}")
    assert np.array_equal(out["flags"], m["flags"]) and (out["flags"] == 0).all()
    tail = out["grad_state0"][:, ram.NS:]
    assert (tail == 0.0).all() and not np.signbit(tail).any()
    if case == "boxed":                                                # the limits' entries, live on the boxed loop alone
        b = ec.BOXED[1]
        assert (out["grad_gains"][b, 29:31] != 0.0).all() and (np.delete(out["grad_gains"], b, axis=0)[:, 29:31] == 0.0).all()
    if case == ec.SWITCHING[0]:
        assert out["grad_gains"][ec.SWITCHING[1], 29] != 0.0


def test_boxed_row_matches_a_single_loop_rollout(ro, ag, sweeps):
    case, b = ec.BOXED
    base = sweeps(case)[2]
    _, _, out = _sweep(ro, ag, case, loops=[b], own_config=True)
    for k in ("grad_state0", "grad_gains", "flags"):
        assert np.array_equal(out[k][0], base[k][b]), k


def test_loops_beside_the_boxed_one_do_not_see_it(ro, ag, sweeps):
    case, b = ec.BOXED
    base = sweeps(case)[2]
    others = [i for i in range(len(ec.CASES[case].loops)) if i != b]
    log, _, out = _sweep(ro, ag, case, loops=others)
    assert np.array_equal(log, sweeps(case)[0][:, others])
    for k in ("grad_state0", "grad_gains", "flags"):
        assert np.array_equal(out[k], base[k][others]), k


def _rc_rollout(ro, ag, idx):
    """rollout_adjoint_cases.py's loops `idx` at (6, 2, 3) on the runtime-sized handle, every loop under its own row"""
    hz = rc.HORIZONS[0]
    st, pa = rc.plants()
    cfg = rc.config(L.MPCConfig, hz)
    pos, vel, alpha, adt = rc.trajectory()
    r = ro.ClosedLoopRollout(cfg, len(idx), pos, vel, alpha, adt, device=0, runtime="always", adjoint=True)
    try:
        r.set_tunables(configs=ag.configs_of(cfg, rc.gains(L.MPCConfig, hz)[idx]))
        r.reset(st[idx], pa[idx])
    except Exception:
        r.close()
        raise
    return r


def _rc_sweep(ro, ag, idx):
    lb, sb = rc.loss_weights()
    r = _rc_rollout(ro, ag, idx)
    try:
        r.run(rc.TICKS, tape=True)
        return r.backward(lb[:, idx], sb[idx])
    finally:
        r.close()


def test_batches_of_1_and_257(ro, ag):
    base = _rc_sweep(ro, ag, np.arange(rc.B))
    assert ec.BATCHES == (1, 257)
    one = _rc_sweep(ro, ag, np.array([3]))                             # the hover loop alone: grid = 1
    perm = np.concatenate([np.arange(rc.B), np.random.default_rng(ec.SEED).integers(0, rc.B, size=257 - rc.B)])
    perm = np.random.default_rng(ec.SEED + 1).permutation(perm)
    many = _rc_sweep(ro, ag, perm)                                     # more workgroups than compute units
    for k in ("grad_state0", "grad_gains", "flags"):
        assert np.array_equal(one[k][0], base[k][3]), k
        assert np.array_equal(many[k], base[k][perm]), k
    assert np.isfinite(base["grad_state0"]).all() and (base["grad_gains"] != 0.0).any()


def test_tape_grows_on_a_second_longer_run(ro, ag, ref):
    """9 taped ticks and their sweep, then 12 more on the same rollout: the tape is reallocated, the second run begins at
    tick 9 with the window the first one left, and its sweep is that of the model over ticks 9 .. 20"""
    hz = rc.HORIZONS[0]
    first, second = rc.TICKS, rc.TICKS + 3
    st, pa = rc.plants()
    g = rc.gains(L.MPCConfig, hz)
    lb, sb = ec.loss_weights(second, rc.B)
    idx = np.arange(rc.B)
    r = _rc_rollout(ro, ag, idx)
    try:
        r.run(first, tape=True)
        r.backward(*rc.loss_weights())
        log = r.run(second, tape=True)
        out = r.backward(lb, sb)
    finally:
        r.close()
    assert (log[:, :, 14] == L.STATUS_SOLVED).all()
    for b in range(rc.B):
        cfg = ram.with_gains(rc.config(ref.Config, hz), g[b])
        mlog, _, tape = ram.forward(cfg, st[b], pa[b], rc.trajectory(), first + second)
        assert np.abs(log[:, b, :14] - mlog[first:, :14]).max() <= 1e-8 * np.abs(mlog[:, :14]).max()
        want = ram.backward(cfg, tape[first:], pa[b], rc.trajectory(), lb[:, b], sb[b], first=False, tick_base=first)
        es, fs, eg, fg = _against_model({k: v[b] for k, v in out.items()}, want["grad_state0"], want["grad_cfg"])
        print(f"loop {b}: second run, state0 {es:.2e} of the bar ({fs}), gains {eg:.2e} ({fg})")
        assert es <= 1.0 and eg <= 1.0, (b, es, fs, eg, fg)
        assert out["flags"][b] == want["flags"]


N_DIR, STEP = 6, 1e-3
LIMIT_STEP = 0.1        # of a throttle limit against the other gains, as in test_rollout_adjoint_edge_cases.py: the box is 1 % wide


def _directions(case):
    B = len(ec.CASES[case].loops)
    rng = np.random.default_rng(ec.SEED + 23)
    ds = rng.normal(size=(N_DIR, B, ram.NS)) * ram.state_scale() * STEP
    g0 = ec.gains(L.MPCConfig, case)
    dg = rng.normal(size=(N_DIR, B, 32)) * np.where(g0 != 0.0, g0, 10.0) * STEP
    dg[:, :, 29:31] *= LIMIT_STEP
    dg[:, :, 31] = 0.0
    return ds, dg


@pytest.mark.parametrize("case", ["tilted", "boxed"])
def test_central_differences_of_the_device_rollout(ro, ag, sweeps, ref, case):
    c = ec.CASES[case]
    B, T = len(c.loops), c.ticks
    st, pa = ec.plants(case)
    g = ec.gains(L.MPCConfig, case)
    lb, sb = ec.case_loss_weights(case)
    ds, dg = _directions(case)
    # one batch: the loops, then +d and -d of every state direction, then of every gains direction
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
    r = _rollout(ro, ag, case, S, P, G, adjoint=False)
    try:
        log = r.run(T)
        final = r.state()
    finally:
        r.close()
    assert (log[:, :, 14] == L.STATUS_SOLVED).all()
    loss = np.array([ram.loss(log[:, i], final[i], lb[:, i % B], sb[i % B]) for i in range(len(S))])
    out = sweeps(case)[2]
    m = ec.model(case)
    traj = ec.trajectory(case)
    worst = {"state0": [0.0, 0.0], "gains": [0.0, 0.0]}               # [device, CPU model]
    for b in range(B):
        cfg = ram.with_gains(ec.config(ref.Config, case), g[b])
        for k in range(N_DIR):
            for kind, d_state, d_gains, base in (("state0", ds[k, b], None, B), ("gains", None, dg[k, b], B + 2 * N_DIR * B)):
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
        print(f"{case} {kind}: quotient against adjoint, worst relative error: device {dev:.2e}, CPU model {cpu:.2e}")
        assert dev <= 10.0 * cpu, (case, kind, dev, cpu)
