"""The parameter and track gradients of the rollout adjoint on the device (vsmpc_rollout_backward_full[_device], the PT
instantiation of advance_adjoint_kernel, vsmpc_rollout_set_trajectories, autograd.rollout) on the loops of
tests/rollout_param_adjoint_cases.py, 5 to 21 ticks:

  against tests/rollout_param_adjoint_model.py (itself checked against central differences in
      test_rollout_param_adjoint_model.py), every entry of grad_params and of grad_traj, under that test's rule and bar
      (rollout_param_adjoint_cases.FD_BAR, FLOOR_RATIO), on runtime handles at (6, 2, 3) and on the tuned handle at (17, 7, 12)
      with the paper's timing;
  bitwise: grad_state0, grad_cfg and flags against vsmpc_rollout_backward, with the new outputs requested and with them NULL;
      two sweeps of one tape; a permuted batch; the host and `_device` entries; batches of 1 and 257 against the four-loop
      rows; every loop against its single-loop run under its own row of tunables;
  a loop no tick of which is Solved: the solve's share is absent, the plant's is there;
  set_trajectories against a rollout created with the other track; central differences of the device's own forward run
      along one random direction in the parameters and one in the tracks; autograd; the refusals.
"""
import importlib
import os

import numpy as np
import pytest

import rollout_adjoint_cases as rc
import rollout_adjoint_edge_cases as ec
import rollout_adjoint_model as ram
import rollout_param_adjoint_cases as pc
import rollout_param_adjoint_model as rpm
from conftest import PKG, ROOT

pytestmark = pytest.mark.gpu

L = pc.L
CASES = (None, "sub16_ratio2", "trajectory_end", "trajectory_one", "tilted", "tick5000", "fast_track", "pushed_long")
KEYS = ("grad_state0", "grad_gains", "flags")
NEW_KEYS = ("grad_params", "grad_traj_pos", "grad_traj_vel", "grad_traj_alpha")


@pytest.fixture(scope="module")
def ro(solver_mod):
    return importlib.import_module(PKG + ".rollout")


@pytest.fixture(scope="module")
def ag(solver_mod):
    return importlib.import_module(PKG + ".autograd")


def _rollout(ro, ag, case, st, pa, gains, traj=None, adjoint=True):
    """a rollout of len(st) loops of `case`, under their own rows of gains, reset"""
    cfg = pc.config(L.MPCConfig, case)
    pos, vel, alpha, adt = pc.trajectory(case) if traj is None else traj
    runtime = "always" if case is None else pc.case(case).runtime
    r = ro.ClosedLoopRollout(cfg, len(st), pos, vel, alpha, adt, device=0, runtime=runtime, adjoint=adjoint)
    try:
        r.set_tunables(configs=ag.configs_of(cfg, gains))
        r.reset(st, pa)
    except Exception:
        r.close()
        raise
    return r


def _inputs(case):
    st, pa = pc.plants(case)
    lb, sb = pc.loss_weights(case)
    return st, pa, pc.gains(L.MPCConfig, case), lb, sb


def _sweep(ro, ag, case, idx=None):
    """(log, full backward, plain backward, full backward with the new outputs NULL) of the case's loops (or loops idx)"""
    st, pa, g, lb, sb = _inputs(case)
    if idx is not None:
        st, pa, g, lb, sb = st[idx], pa[idx], g[idx], lb[:, idx], sb[idx]
    r = _rollout(ro, ag, case, st, pa, g)
    try:
        log = r.run(pc.ticks_of(case), tape=True)
        full = r.backward(lb, sb, params=True, traj=True)
        plain = r.backward(lb, sb)
        null = {"grad_state0": np.empty((len(st), L.PLANT_STATE)), "grad_gains": np.empty((len(st), L.GRAD_SIZE)),
                "flags": np.empty(len(st), dtype=np.int32)}
        from ctypes import c_void_p
        p = lambda a: c_void_p(a.ctypes.data)
        assert r.lib.vsmpc_rollout_backward_full(r._r, p(np.ascontiguousarray(lb)), p(np.ascontiguousarray(sb)), p(null["grad_state0"]),
                                                 p(null["grad_gains"]), None, None, p(null["flags"]), None) == 0
        return log, full, plain, null
    finally:
        r.close()


@pytest.fixture(scope="module")
def sweeps(ro, ag):
    return {case: _sweep(ro, ag, case) for case in CASES}


def _against_model(out, b, m):
    """the worst error of loop b's new rows against the model's, in units of the bar, and where"""
    row = np.concatenate([out[k][b].reshape(-1) for k in NEW_KEYS[1:]])
    n_traj, n_alpha = out["grad_traj_pos"].shape[1], out["grad_traj_alpha"].shape[1]
    parts = [ram.field_errors(out["grad_params"][b], m["grad_params"], rpm.PARAM_FIELDS, pc.FD_BAR, pc.FD_FLOOR),
             ram.field_errors(row, pc.traj_row(m), pc.traj_fields(n_traj, n_alpha), pc.FD_BAR, pc.FD_FLOOR)]
    return max(parts, key=lambda ef: ef[0])


@pytest.mark.parametrize("case", CASES, ids=lambda c: c or "rc")
def test_sweep_matches_model(sweeps, case):
    log, full, plain, null = sweeps[case]
    for b in range(log.shape[1]):
        m = pc.model(((case or "rc"), b))
        assert np.array_equal(log[:, b, 14], m["log"][:, 14]) and (log[:, b, 14] == L.STATUS_SOLVED).all()
        e, f = _against_model(full, b, m)
        print(f"{case or 'rc'} loop {b}: {e:.2e} of the bar ({f})")
        assert e <= 1.0, (case, b, e, f)
        # what the model leaves at +0.0 is +0.0 here: the structural parameters, samples and alpha samples the run never touches
        for k in NEW_KEYS:
            zero = m[k] == 0.0
            assert (full[k][b][zero] == 0.0).all() and not np.signbit(full[k][b][zero]).any(), (case, b, k)
    # the old outputs, bit for bit, with the new outputs requested and with them NULL
    for k in KEYS:
        assert np.array_equal(full[k], plain[k]) and np.array_equal(null[k], plain[k]), (case, k)


def test_batches_permutations_and_repeated_sweeps_are_bit_identical(ro, ag, sweeps):
    base = sweeps[None][1]
    for idx in (np.array([3]), np.arange(257) % rc.B, np.array([2, 0, 3, 1, 1, 3, 0, 2])):     # 1 | more loops than CUs | permuted
        _, full, plain, _ = _sweep(ro, ag, None, idx)
        for k in KEYS + NEW_KEYS:
            assert np.array_equal(full[k], base[k][idx]), (len(idx), k)
        for k in KEYS:
            assert np.array_equal(full[k], plain[k]), (len(idx), k)


def test_host_and_device_entries_and_two_sweeps_agree(ro, ag, sweeps):
    import torch
    st, pa, g, lb, sb = _inputs(None)
    base = sweeps[None][1]
    r = _rollout(ro, ag, None, st, pa, g)
    try:
        r.run(rc.TICKS, tape=True)
        one, two = r.backward(lb, sb, params=True, traj=True), r.backward(lb, sb, params=True, traj=True)
        for k in KEYS + NEW_KEYS:
            assert np.array_equal(one[k], two[k]) and np.array_equal(one[k], base[k]), k
        dev = "cuda"
        t = lambda a: torch.tensor(a, dtype=torch.float64, device=dev).contiguous()
        g0, gg = torch.empty((rc.B, L.PLANT_STATE), dtype=torch.float64, device=dev), torch.empty((rc.B, L.GRAD_SIZE), dtype=torch.float64, device=dev)
        gp = torch.empty((rc.B, L.PLANT_PARAMS), dtype=torch.float64, device=dev)
        gt = torch.empty((rc.B, r.traj_grad_size), dtype=torch.float64, device=dev)
        fl = torch.empty(rc.B, dtype=torch.int32, device=dev)
        r.backward_device(t(lb), t(sb), g0, gg, fl, d_grad_params=gp, d_grad_traj=gt)
        torch.cuda.synchronize()
        assert np.array_equal(g0.cpu().numpy(), base["grad_state0"]) and np.array_equal(gg.cpu().numpy(), base["grad_gains"])
        assert np.array_equal(gp.cpu().numpy(), base["grad_params"]) and np.array_equal(fl.cpu().numpy(), base["flags"])
        row = np.concatenate([base[k].reshape(rc.B, -1) for k in NEW_KEYS[1:]], axis=1)
        assert r.traj_grad_size == row.shape[1] == 6 * r.n_traj + r.n_alpha
        assert np.array_equal(gt.cpu().numpy(), row)
        # a buffer of the wrong shape is refused before the call
        with pytest.raises(ValueError, match="d_grad_traj"):
            r.backward_device(t(lb), t(sb), g0, gg, fl, d_grad_traj=gt[:, :-1].contiguous())
        # only one of the two new outputs
        only = r.backward(lb, sb, params=True)
        assert np.array_equal(only["grad_params"], base["grad_params"]) and "grad_traj_pos" not in only
    finally:
        r.close()


def test_per_loop_rows_match_single_loop_rollouts(ro, ag, sweeps):
    base = sweeps[None][1]
    for b in range(rc.B):
        _, full, _, _ = _sweep(ro, ag, None, np.array([b]))
        for k in KEYS + NEW_KEYS:
            assert np.array_equal(full[k][0], base[k][b]), (b, k)


def test_tuned_handle_at_the_papers_timing(ro, ag, ref):
    """(17, 7, 12) on the tuned instantiation, periods 0.01 / 0.01 / 0.1, 21 ticks: the plain loop and the loop from tick 5000"""
    case = pc.TUNED
    log, full, plain, null = _sweep(ro, ag, case, np.array([0, 1]))
    for b in range(2):
        cfg, s0, p, traj, lb, sb = ec.loop_inputs(ref, case, b)
        tape = ec.model(case)["tapes"][b]
        m = rpm.backward(cfg, tape, p, traj, lb, sb)
        e, f = _against_model(full, b, m)
        print(f"{case} loop {b}: {e:.2e} of the bar ({f})")
        assert e <= 1.0, (b, e, f)
    for k in KEYS:
        assert np.array_equal(full[k], plain[k]) and np.array_equal(null[k], plain[k]), k


def test_a_loop_that_is_never_solved_keeps_its_plant_share(ro, ag, ref):
    """Loop 3 with NaN thrust references (rollout_adjoint_cases.plants): no tick of it is Solved on the device.  Its solves
    hand nothing back -- no record cotangent, so no window cotangent either -- and the plant half of every tick still does:
    mass, I_B, the jet map, alpha."""
    st, pa = rc.plants(unsolved_loop=3)
    _, _, g, lb, sb = _inputs(None)
    r = _rollout(ro, ag, None, st, pa, g)
    try:
        log = r.run(rc.TICKS, tape=True)
        out = r.backward(lb, sb, params=True, traj=True)
    finally:
        r.close()
    assert (log[:, 3, 14] != L.STATUS_SOLVED).all() and (log[:, :3, 14] == L.STATUS_SOLVED).all()
    cfg = ram.with_gains(rc.config(ref.Config, pc.HORIZON), rc.gains(ref.Config, pc.HORIZON)[3])
    tape = rc.model(pc.HORIZON, unsolved_loop=3)["tapes"][3]
    m = rpm.backward(cfg, tape, pa[3], rc.trajectory(), lb[:, 3], sb[3])
    assert all(np.isfinite(out[k]).all() for k in NEW_KEYS)
    e, f = _against_model(out, 3, m)
    print(f"never solved: {e:.2e} of the bar ({f})")
    assert e <= 1.0, (e, f)
    gp = out["grad_params"][3]
    assert gp[L.PP_MASS] != 0.0 and (gp[L.PP_AMOM0:L.PP_AMOM0 + 24] != 0.0).any() and (out["grad_traj_alpha"][3] != 0.0).any()
    for k in ("grad_traj_pos", "grad_traj_vel"):
        assert (out[k][3] == 0.0).all()
    assert (gp[L.PP_PINIT:L.PP_RPYINIT + 3] == 0.0).all()


def test_set_trajectories(ro, ag):
    st, pa, g, lb, sb = _inputs(None)
    first, second = pc.trajectory(None), pc.trajectory("fast_track")
    second = (second[0], second[1], np.array([0.95, 0.9, 0.7, 0.6]), second[3])
    made = _rollout(ro, ag, None, st, pa, g, traj=second)
    try:
        want = made.run(rc.TICKS)
    finally:
        made.close()
    r = _rollout(ro, ag, None, st, pa, g, traj=first)
    try:
        other = r.run(rc.TICKS, tape=True)
        r.set_trajectories(second[0], second[1], second[2])
        with pytest.raises(Exception, match="invalid argument"):          # the tape is gone
            r.backward(None, sb, params=True)
        with pytest.raises(Exception, match="invalid argument"):          # and a reset is required
            r.run(1)
        r.reset(st, pa)
        got = r.run(rc.TICKS)
        assert np.array_equal(got, want) and not np.array_equal(got, other)
        r.set_trajectories(None, None, first[2])                           # NULL keeps a track
        r.reset(st, pa)
        assert not np.array_equal(r.run(rc.TICKS), want)
        with pytest.raises(ValueError):
            r.set_trajectories(second[0][:-1])
    finally:
        r.close()


def test_central_differences_of_the_device_rollout(ro, ag, sweeps, ref):
    """the tilted and the pushed loop, +-h along one random direction in the parameters and one in the tracks, on the device's
    own forward run; the same quotient of the CPU model shows the step's truncation error: the bar is 10 times its error"""
    rng = np.random.default_rng(rc.SEED + 41)
    for case, b in (("tilted", 2), (None, 1)):
        st, pa, g, lb, sb = _inputs(case)
        pos, vel, alpha, adt = pc.trajectory(case)
        ticks = pc.ticks_of(case)
        h = 1e-3
        dp = np.zeros(L.PLANT_PARAMS)
        for name, off, n in rpm.PARAM_FIELDS:
            dp[off:off + n] = rng.normal(size=n) * rpm.param_scale()[off:off + n]
        dtr = (rng.normal(size=pos.shape) * 1e-2, rng.normal(size=vel.shape) * 1e-2, rng.normal(size=alpha.shape) * 1e-2)
        out = sweeps[case][1]
        m = pc.model(((case or "rc"), b))
        cfg = pc.loop_inputs(ref, ((case or "rc"), b))[0]

        def loss_of(p_row, traj):
            r = _rollout(ro, ag, case, st[b:b + 1], p_row[None], g[b:b + 1], traj=traj, adjoint=False)
            try:
                log = r.run(ticks)
                return ram.loss(log[:, 0], r.state()[0], lb[:, b], sb[b])
            finally:
                r.close()
        base_traj = (pos, vel, alpha, adt)
        fd_p = (loss_of(pa[b] + h * dp, base_traj) - loss_of(pa[b] - h * dp, base_traj)) / (2 * h)
        tr = lambda s: (pos + s * h * dtr[0], vel + s * h * dtr[1], alpha + s * h * dtr[2], adt)
        fd_t = (loss_of(pa[b], tr(1.0)) - loss_of(pa[b], tr(-1.0))) / (2 * h)
        an_t = lambda o: sum((o[k] * d).sum() for k, d in zip(("grad_traj_pos", "grad_traj_vel", "grad_traj_alpha"), dtr))
        dev_p, dev_t = out["grad_params"][b] @ dp, an_t({k: out[k][b] for k in NEW_KEYS})
        cpu_p = rpm.central(cfg, st[b], pa[b], base_traj, ticks, lb[:, b], sb[b], d_params=dp, step=h, richardson=False)
        cpu_t = rpm.central(cfg, st[b], pa[b], base_traj, ticks, lb[:, b], sb[b], d_pos=dtr[0], d_vel=dtr[1], d_alpha=dtr[2], step=h,
                            richardson=False)
        mod_p, mod_t = m["grad_params"] @ dp, an_t(m)
        for kind, fd, dev, cpu, mod in (("parameters", fd_p, dev_p, cpu_p, mod_p), ("tracks", fd_t, dev_t, cpu_t, mod_t)):
            e_dev, e_cpu = abs(fd - dev) / abs(mod), abs(cpu - mod) / abs(mod)
            print(f"{case or 'rc'} loop {b}, {kind}: quotient against adjoint: device {e_dev:.2e}, CPU model {e_cpu:.2e}")
            assert e_dev <= max(10.0 * e_cpu, pc.FD_BAR), (case, kind, e_dev, e_cpu)


def test_autograd_rollout(ro, ag, sweeps):
    import torch
    st, pa, g, lb, sb = _inputs(None)
    log, base, _, _ = sweeps[None]
    pos, vel, alpha, adt = pc.trajectory(None)
    r = ro.ClosedLoopRollout(pc.config(L.MPCConfig, None), rc.B, pos, vel, alpha, adt, device=0, runtime="always", adjoint=True)
    try:
        T = rc.TICKS
        t = lambda a, grad=True: torch.tensor(a, dtype=torch.float64, device="cuda", requires_grad=grad)
        weights = (t(lb[:, :, :14], False), t(sb[:, :ram.NS], False))
        state0, gains, params = t(st[:, :ram.NS]), t(g), t(pa)
        tracks = (t(pos), t(vel), t(alpha))
        tlog, tfinal = ag.rollout(r, state0, gains, params, T, None, traj=tracks)
        assert np.array_equal(tlog.detach().cpu().numpy(), log[:, :, :14])
        ((tlog * weights[0]).sum() + (tfinal * weights[1]).sum()).backward()
        assert np.array_equal(state0.grad.cpu().numpy(), base["grad_state0"][:, :ram.NS])
        assert np.array_equal(gains.grad.cpu().numpy(), base["grad_gains"])
        assert np.array_equal(params.grad.cpu().numpy(), base["grad_params"])
        assert (params.grad[:, [L.PP_DIST_T0, L.PP_DIST_T1, L.PP_TICK0]] == 0.0).all()
        for tr, k in zip(tracks, NEW_KEYS[1:]):                      # summed over the loops
            want = torch.tensor(base[k], device="cuda").sum(dim=0).cpu().numpy()
            assert np.array_equal(tr.grad.cpu().numpy(), want), k
            assert np.abs(tr.grad.cpu().numpy() - base[k].sum(axis=0)).max() <= 1e-12 * np.abs(base[k]).sum(axis=0).max(), k
        # the old call forms: no traj, params as numpy; same results, nothing new computed
        s2, g2 = t(st[:, :ram.NS]), t(g)
        info = {}
        tlog2, tfinal2 = ag.rollout(r, s2, g2, pa, T, info)
        ((tlog2 * weights[0]).sum() + (tfinal2 * weights[1]).sum()).backward()
        assert np.array_equal(s2.grad.cpu().numpy(), base["grad_state0"][:, :ram.NS])
        assert np.array_equal(g2.grad.cpu().numpy(), base["grad_gains"])
        assert np.array_equal(info["flags"].cpu().numpy(), base["flags"])
    finally:
        r.close()


def test_refusals(ro, ag):
    st, pa, g, lb, sb = _inputs(None)
    pos, vel, alpha, adt = pc.trajectory(None)
    cfg = pc.config(L.MPCConfig, None)
    RT = importlib.import_module(PKG + ".robot_tree")
    jp = importlib.import_module(PKG + ".jet_plant")
    gold = np.load(os.path.join(ROOT, "tests", "golden", "jet_lstm.npz"))
    jm = jp.JetModelTotal(gold["w_ih"], gold["w_hh"], gold["b_ih"], gold["b_hh"], gold["fc_w"], gold["fc_b"], gold["norm"],
                          device=0, max_series=64)
    r = ro.ClosedLoopRollout(cfg, rc.B, pos, vel, alpha, adt, device=0, runtime="always", adjoint=True)
    try:
        for name, on, off in (("tree", lambda: r.set_tree(RT.default_tree()), lambda: r.set_tree(None)),
                              ("jet plant", lambda: r.set_jet_plant(jm), lambda: r.set_jet_plant(None)),
                              ("RPYDot", lambda: r.set_attitude_tracks(None, np.zeros((len(pos), 3))),
                               lambda: r.set_attitude_tracks(None, None))):
            on()
            r.reset(st, pa)
            r._taped = rc.TICKS
            with pytest.raises(Exception, match="(?i)backward_full.*" + name.split()[0]):
                r.backward(lb, sb, params=True, traj=True)
            off()
        r.reset(st, pa)
        r.run(rc.TICKS, tape=True)
        assert np.isfinite(r.backward(lb, sb, params=True, traj=True)["grad_params"]).all()
    finally:
        r.close()
    r = ro.ClosedLoopRollout(cfg, rc.B, pos, vel, alpha, adt, device=0, runtime="always")     # a handle without the flag
    try:
        r.reset(st, pa)
        r.run(rc.TICKS, tape=True)
        with pytest.raises(Exception, match="VSMPC_CREATE_ADJOINT_RECORD"):
            r.backward(lb, sb, params=True, traj=True)
    finally:
        r.close()
