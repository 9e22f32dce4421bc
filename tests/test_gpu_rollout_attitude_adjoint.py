"""The attitude-track gradients of the rollout adjoint on the device (vsmpc_rollout_set_attitude_tracks_ex with
VSMPC_ATTITUDE_ADJOINT, vsmpc_rollout_backward_attitude[_device], the ATT instantiations of the advance adjoint kernel,
autograd.rollout(att=...)) on the loops of tests/rollout_attitude_adjoint_cases.py, 9 taped ticks at ratio 4, on runtime handles
at (6, 2, 3) and -- `base` -- on the tuned handle at (17, 7, 12):

  the forward loop: taped against untaped on a flagged rollout, and against an unflagged rollout under the same tracks, bit for
      bit;
  against tests/rollout_attitude_adjoint_model.py (itself checked against central differences in
      test_rollout_attitude_adjoint_model.py): every case, grad_state0, grad_gains, grad_params, grad_traj and grad_att, under
      test_gpu_rollout_param_adjoint.py's rule and bar (rollout_param_adjoint_cases.FD_BAR, FLOOR_RATIO);
  against central differences of the device's OWN forward run on the tilted loop, along one direction of the RPY track and one
      of the RPYDot track, judged as test_central_differences_of_the_device_rollout judges them: max(10 e_cpu, bar);
  the flag with both tracks NULL against a rollout without the flag (another instantiation: at the bar), grad_att against the
      model and not zero in the RPYDot block;
  bitwise: backward / backward_full / backward_attitude on what they share; the host and `_device` entries; two sweeps of one
      tape; a permuted batch; batches of 1 and 257 against the case's own rows;
  the tree plant under both flags; the loop that is never Solved; the refusals that stay and the new one; autograd.

Measured on an MI355X, in units of the bar: every output of every loop at most 2.7e-8 at (6, 2, 3) (gains, the clamped loop;
grad_att at most 9.4e-10) and 3.1e-9 at (17, 7, 12); the device's quotients 5.3e-11 (RPY) and 1.1e-11 (RPYDot) of the directional
derivative off its adjoint, the CPU model's 1.4e-10 and 1.1e-11; with both tracks NULL the shared outputs came out equal to the
unflagged sweep's in every bit.
"""
import importlib
import os

import numpy as np
import pytest

import adjoint_model as am
import rollout_adjoint_model as ram
import rollout_attitude_adjoint_cases as ac
import rollout_param_adjoint_cases as pc
import rollout_param_adjoint_model as rpm
import rollout_tree_adjoint_cases as tc
from conftest import PKG, ROOT

pytestmark = pytest.mark.gpu

L = ac.L
T = ac.TICKS
HANDLES = {(6, 2, 3): "always", (17, 7, 12): "never"}      # the runtime-sized kernel | the tuned instantiation
CASES = ac.PARAMETRIC + ("tree",)
KEYS = ("grad_state0", "grad_gains", "flags")
FULL_KEYS = ("grad_params", "grad_traj_pos", "grad_traj_vel", "grad_traj_alpha")
ATT_KEYS = ("grad_traj_rpy", "grad_traj_rpy_dot")
BAR, FLOOR = ac.FD_BAR, ac.FD_FLOOR


@pytest.fixture(scope="module")
def ro(solver_mod):
    return importlib.import_module(PKG + ".rollout")


@pytest.fixture(scope="module")
def ag(solver_mod):
    return importlib.import_module(PKG + ".autograd")


def _inputs(case, horizon=ac.HORIZON, idx=None):
    st, pa = ac.plants(case)
    lb, sb = ac.loss_weights(case)
    g = ac.gains(L.MPCConfig, case, horizon)
    if idx is not None:
        st, pa, g, lb, sb = st[idx], pa[idx], g[idx], lb[:, idx], sb[idx]
    return st, pa, g, lb, sb


def _rollout(ro, ag, case, st, pa, gains, horizon=ac.HORIZON, att="case", flag=True, traj=None, adjoint=True):
    """a rollout of len(st) loops of `case` under their own rows of gains and the case's attitude tracks (att: others; None:
    set_attitude_tracks is not called), reset, and flown through the ticks in front of the taped run"""
    cfg = ac.config(L.MPCConfig, horizon)
    pos, vel, alpha, adt = ac.trajectory(case) if traj is None else traj
    r = ro.ClosedLoopRollout(cfg, len(st), pos, vel, alpha, adt, device=0, runtime=HANDLES[tuple(horizon)], adjoint=adjoint)
    try:
        if case == "tree":
            r.set_tree(tc.tree(), adjoint=True)
        if att is not None:
            r.set_attitude_tracks(*(ac.attitude_tracks(case) if isinstance(att, str) else att), adjoint=flag)
        r.set_tunables(configs=ag.configs_of(cfg, gains))
        r.reset(st, pa)
        if ac.ticks_before(case):
            r.run(ac.ticks_before(case), log=False)
    except Exception:
        r.close()
        raise
    return r


def _sweep(ro, ag, case, horizon=ac.HORIZON, idx=None):
    """(log, final state, backward_attitude, backward_full, backward) of the case's loops (or loops idx)"""
    st, pa, g, lb, sb = _inputs(case, horizon, idx)
    r = _rollout(ro, ag, case, st, pa, g, horizon)
    try:
        log = r.run(T, tape=True)
        final = r.state()
        return log, final, r.backward(lb, sb, params=True, traj=True, att=True), r.backward(lb, sb, params=True, traj=True), r.backward(lb, sb)
    finally:
        r.close()


@pytest.fixture(scope="module")
def sweeps(ro, ag):
    out = {(case, ac.HORIZON): _sweep(ro, ag, case) for case in CASES}
    out[("base", ac.HORIZONS[1])] = _sweep(ro, ag, "base", ac.HORIZONS[1])
    return out


def _against_model(out, i, m):
    """loop row i of the device against the model m: the worst error of each group of outputs in units of the bar"""
    n_traj, n_alpha = out["grad_traj_pos"].shape[1], out["grad_traj_alpha"].shape[1]
    row = np.concatenate([out[k][i].reshape(-1) for k in FULL_KEYS[1:]])
    arow = np.concatenate([out[k][i].reshape(-1) for k in ATT_KEYS])
    return {"state0": ram.field_errors(out["grad_state0"][i, :ram.NS], m["grad_state0"], ram.STATE_FIELDS, BAR, FLOOR),
            "gains": ram.field_errors(out["grad_gains"][i], m["grad_cfg"], am.GRAD_FIELDS, BAR, FLOOR),
            "params": ram.field_errors(out["grad_params"][i], m["grad_params"], rpm.PARAM_FIELDS, BAR, FLOOR),
            "tracks": ram.field_errors(row, pc.traj_row(m), pc.traj_fields(n_traj, n_alpha), BAR, FLOOR),
            "att": ram.field_errors(arow, ac.att_row(m), ac.att_fields(n_traj), BAR, FLOOR)}


def _check_case(sweeps, case, horizon):
    log, final, att, full, plain = sweeps[(case, horizon)]
    for b in range(log.shape[1]):
        m = ac.model((case, b), horizon)
        assert np.array_equal(log[:, b, 14], m["log"][:, 14]) and (log[:, b, 14] == L.STATUS_SOLVED).all(), (case, b)
        assert np.abs(log[:, b, :14] - m["log"][:, :14]).max() <= 1e-8 * np.abs(m["log"][:, :14]).max(), (case, b)
        errs = _against_model(att, b, m)
        print(f"{case} {horizon} loop {b}: " + ", ".join(f"{k} {e:.2e} of the bar ({f})" for k, (e, f) in errs.items()))
        assert all(e <= 1.0 for e, _ in errs.values()), (case, b, errs)
        assert att["flags"][b] == m["flags"] == 0
        for k in ATT_KEYS:           # a sample that no window column of the run holds: +0.0
            zero = m[k] == 0.0
            assert (att[k][b][zero] == 0.0).all() and not np.signbit(att[k][b][zero]).any(), (case, b, k)
    # what the three entries share, bit for bit
    for k in KEYS:
        assert np.array_equal(att[k], plain[k]) and np.array_equal(full[k], plain[k]), (case, k)
    for k in FULL_KEYS:
        assert np.array_equal(att[k], full[k]), (case, k)


@pytest.mark.parametrize("case", CASES)
def test_sweep_matches_model(sweeps, case):
    _check_case(sweeps, case, ac.HORIZON)


def test_tuned_handle(sweeps):
    _check_case(sweeps, "base", ac.HORIZONS[1])


def test_taped_untaped_and_unflagged_runs_are_bit_identical(ro, ag, sweeps):
    st, pa, g, lb, sb = _inputs("base")
    log, final = sweeps[("base", ac.HORIZON)][:2]
    for flag in (True, False):
        r = _rollout(ro, ag, "base", st, pa, g, flag=flag)
        try:
            assert np.array_equal(r.run(T), log) and np.array_equal(r.state(), final), flag
        finally:
            r.close()
    none = _rollout(ro, ag, "base", st, pa, g, att=None)       # and the tracks do move the loop
    try:
        assert not np.array_equal(none.run(T), log)
    finally:
        none.close()


def test_central_differences_of_the_device_rollout(ro, ag, sweeps, ref):
    """the tilted loop, +-h along one random direction of the RPY track and one of the RPYDot track, on the device's own forward
    run; the same quotient of the CPU model shows the step's error: the bar is 10 times its error"""
    rng = np.random.default_rng(ac.rc.SEED + 61)
    case, b = "base", ac.TILTED
    st, pa, g, lb, sb = _inputs(case)
    rpy, rpyd = ac.attitude_tracks(case)
    out = sweeps[(case, ac.HORIZON)][2]
    m = ac.model((case, b))
    h = 1e-3

    def loss_of(att):
        r = _rollout(ro, ag, case, st[b:b + 1], pa[b:b + 1], g[b:b + 1], att=att, flag=False, adjoint=False)
        try:
            log = r.run(T)
            return ram.loss(log[:, 0], r.state()[0], lb[:, b], sb[b])
        finally:
            r.close()
    for name, k in (("rpy", ATT_KEYS[0]), ("rpy_dot", ATT_KEYS[1])):
        d = rng.normal(size=rpy.shape)
        tr = lambda s: (rpy + s * h * d, rpyd) if name == "rpy" else (rpy, rpyd + s * h * d)
        fd = (loss_of(tr(1.0)) - loss_of(tr(-1.0))) / (2 * h)
        dev, mod = (out[k][b] * d).sum(), (m[k] * d).sum()
        cpu = ac.central(ref, (case, b), **{"d_" + name: d}, step=h, richardson=False)
        e_dev, e_cpu = abs(fd - dev) / abs(mod), abs(cpu - mod) / abs(mod)
        print(f"{case} loop {b}, {name}: quotient against adjoint: device {e_dev:.2e}, CPU model {e_cpu:.2e}")
        assert e_dev <= max(10.0 * e_cpu, BAR), (name, e_dev, e_cpu)


def test_flag_with_both_tracks_null(ro, ag, sweeps):
    """the ATT kernels on the loops a rollout without the flag flies too: the outputs they share agree at the bar (another
    instantiation, so not bit for bit), and grad_att is the gradient at the zero tracks"""
    log, final, att, full, plain = sweeps[("null_both", ac.HORIZON)]
    st, pa, g, lb, sb = _inputs("null_both")
    r = _rollout(ro, ag, "null_both", st, pa, g, att=None)
    try:
        assert np.array_equal(r.run(T, tape=True), log) and np.array_equal(r.state(), final)
        want = r.backward(lb, sb, params=True, traj=True)
    finally:
        r.close()
    n_traj, n_alpha = want["grad_traj_pos"].shape[1], want["grad_traj_alpha"].shape[1]
    for b in range(ac.B):
        row = lambda o: np.concatenate([o[k][b].reshape(-1) for k in FULL_KEYS[1:]])
        errs = (ram.field_errors(att["grad_state0"][b, :ram.NS], want["grad_state0"][b, :ram.NS], ram.STATE_FIELDS, BAR, FLOOR),
                ram.field_errors(att["grad_gains"][b], want["grad_gains"][b], am.GRAD_FIELDS, BAR, FLOOR),
                ram.field_errors(att["grad_params"][b], want["grad_params"][b], rpm.PARAM_FIELDS, BAR, FLOOR),
                ram.field_errors(row(att), row(want), pc.traj_fields(n_traj, n_alpha), BAR, FLOOR))
        print(f"both NULL, loop {b}: " + ", ".join(f"{e:.2e} ({f})" for e, f in errs))
        assert all(e <= 1.0 for e, _ in errs), (b, errs)
        assert np.array_equal(att["flags"], want["flags"])
        assert np.abs(att["grad_traj_rpy_dot"][b]).max() > 0.0 and np.abs(att["grad_traj_rpy"][b]).max() > 0.0


def test_batches_permutations_and_repeated_sweeps_are_bit_identical(ro, ag, sweeps):
    base = sweeps[("base", ac.HORIZON)][2]
    for idx in (np.array([3]), np.arange(257) % ac.B, np.array([2, 0, 3, 1, 1, 3, 0, 2])):     # 1 | more loops than CUs | permuted
        _, _, att, full, plain = _sweep(ro, ag, "base", idx=idx)
        for k in KEYS + FULL_KEYS + ATT_KEYS:
            assert np.array_equal(att[k], base[k][idx]), (len(idx), k)
        for k in KEYS:
            assert np.array_equal(full[k], plain[k]) and np.array_equal(att[k], plain[k]), (len(idx), k)


def test_host_and_device_entries_and_two_sweeps_agree(ro, ag, sweeps):
    import torch
    st, pa, g, lb, sb = _inputs("base")
    base = sweeps[("base", ac.HORIZON)][2]
    r = _rollout(ro, ag, "base", st, pa, g)
    try:
        r.run(T, tape=True)
        one, two = r.backward(lb, sb, params=True, traj=True, att=True), r.backward(lb, sb, att=True)
        for k in KEYS + FULL_KEYS + ATT_KEYS:
            assert np.array_equal(one[k], base[k]), k
        for k in KEYS + ATT_KEYS:                               # grad_att alone: the same sweep
            assert np.array_equal(two[k], base[k]), k
        assert "grad_params" not in two
        dev = "cuda"
        t = lambda a: torch.tensor(a, dtype=torch.float64, device=dev).contiguous()
        e = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
        g0, gg, gp, gt, ga = e(ac.B, L.PLANT_STATE), e(ac.B, L.GRAD_SIZE), e(ac.B, L.PLANT_PARAMS), e(ac.B, r.traj_grad_size), e(ac.B, r.att_grad_size)
        fl = torch.empty(ac.B, dtype=torch.int32, device=dev)
        r.backward_device(t(lb), t(sb), g0, gg, fl, d_grad_params=gp, d_grad_traj=gt, d_grad_att=ga)
        torch.cuda.synchronize()
        assert np.array_equal(g0.cpu().numpy(), base["grad_state0"]) and np.array_equal(gg.cpu().numpy(), base["grad_gains"])
        assert np.array_equal(gp.cpu().numpy(), base["grad_params"]) and np.array_equal(fl.cpu().numpy(), base["flags"])
        assert np.array_equal(gt.cpu().numpy(), np.concatenate([base[k].reshape(ac.B, -1) for k in FULL_KEYS[1:]], axis=1))
        arow = np.concatenate([base[k].reshape(ac.B, -1) for k in ATT_KEYS], axis=1)
        assert r.att_grad_size == arow.shape[1] == 6 * r.n_traj
        assert np.array_equal(ga.cpu().numpy(), arow)
        with pytest.raises(ValueError, match="d_grad_att"):
            r.backward_device(t(lb), t(sb), g0, gg, fl, d_grad_att=ga[:, :-1].contiguous())
    finally:
        r.close()


def test_a_loop_that_is_never_solved(ro, ag, ref):
    st, pa, g, lb, sb = _inputs("unsolved")
    r = _rollout(ro, ag, "unsolved", st, pa, g)
    try:
        log = r.run(T, tape=True)
        out = r.backward(lb, sb, params=True, traj=True, att=True)
    finally:
        r.close()
    u = ac.UNSOLVED_LOOP
    others = [b for b in range(ac.B) if b != u]
    assert (log[:, u, 14] != L.STATUS_SOLVED).all() and (log[:, others, 14] == L.STATUS_SOLVED).all()
    assert out["flags"][u] & L.ADJ_UNSOLVED and not (out["flags"][others] & L.ADJ_UNSOLVED).any()
    for k in ATT_KEYS:
        assert (out[k][u] == 0.0).all() and not np.signbit(out[k][u]).any(), k
    for b in others:                                            # the loops beside it are what they are without it
        errs = _against_model(out, b, ac.model(("unsolved", b)))
        assert all(e <= 1.0 for e, _ in errs.values()), (b, errs)


def test_refusals(ro, ag):
    st, pa, g, lb, sb = _inputs("base")
    rpy, rpyd = ac.attitude_tracks("base")
    jp = importlib.import_module(PKG + ".jet_plant")
    gold = np.load(os.path.join(ROOT, "tests", "golden", "jet_lstm.npz"))
    jm = jp.JetModelTotal(gold["w_ih"], gold["w_hh"], gold["b_ih"], gold["b_hh"], gold["fc_w"], gold["fc_b"], gold["norm"],
                          device=0, max_series=64)
    r = _rollout(ro, ag, "base", st, pa, g, flag=False)
    try:
        # without the flag an RPYDot track is refused by name, by the taped run and by all three sweeps
        with pytest.raises(Exception, match="run_taped.*RPYDot"):
            r.run(T, tape=True)
        r._taped = T
        with pytest.raises(Exception, match="backward_full.*RPYDot"):
            r.backward(lb, sb, params=True, traj=True)
        with pytest.raises(Exception, match="VSMPC_ATTITUDE_ADJOINT"):
            r.backward(lb, sb, att=True)
        with pytest.raises(Exception, match="invalid argument"):    # (no tape: the plain sweep has nothing to refuse by name)
            r.backward(lb, sb)
        # without an RPYDot track and without the flag: taped and swept as before, `_attitude` names the flag
        r.set_attitude_tracks(rpy, None)
        r.reset(st, pa)
        r.run(T, tape=True)
        assert np.isfinite(r.backward(lb, sb, params=True, traj=True)["grad_params"]).all()
        with pytest.raises(Exception, match="VSMPC_ATTITUDE_ADJOINT"):
            r.backward(lb, sb, att=True)
        # unknown bits: refused, and the rollout (its tape too) is as it was
        assert r.lib.vsmpc_rollout_set_attitude_tracks_ex(r._r, None, None, 2) != 0
        assert np.isfinite(r.backward(lb, sb)["grad_state0"]).all()
        # the jet plant under the flag is still refused
        r.set_attitude_tracks(rpy, rpyd, adjoint=True)
        r.set_jet_plant(jm)
        r.reset(st, pa)
        with pytest.raises(Exception, match="run_taped.*jet plant"):
            r.run(T, tape=True)
        r._taped = T
        with pytest.raises(Exception, match="backward_full.*jet plant"):
            r.backward(lb, sb, att=True)
        r.set_jet_plant(None)
        # and so is a tree set without VSMPC_TREE_ADJOINT
        r.set_tree(tc.tree())
        r.reset(st, pa)
        with pytest.raises(Exception, match="run_taped.*tree"):
            r.run(T, tape=True)
    finally:
        r.close()


def test_autograd_rollout(ro, ag, sweeps):
    import torch
    st, pa, g, lb, sb = _inputs("base")
    log, _, base, _, _ = sweeps[("base", ac.HORIZON)]
    pos, vel, alpha, adt = ac.trajectory("base")
    rpy, rpyd = ac.attitude_tracks("base")
    r = ro.ClosedLoopRollout(ac.config(L.MPCConfig), ac.B, pos, vel, alpha, adt, device=0, runtime="always", adjoint=True)
    try:
        t = lambda a, grad=True, dev="cuda": torch.tensor(a, dtype=torch.float64, device=dev, requires_grad=grad)
        weights = (t(lb[:, :, :14], False), t(sb[:, :ram.NS], False))
        state0, gains = t(st[:, :ram.NS]), t(g)
        tracks = (t(rpy), t(rpyd, dev="cpu"))                    # one on the device, one on the host: each gets its gradient there
        tlog, tfinal = ag.rollout(r, state0, gains, pa, T, None, att=tracks)
        assert np.array_equal(tlog.detach().cpu().numpy(), log[:, :, :14])
        ((tlog * weights[0]).sum() + (tfinal * weights[1]).sum()).backward()
        assert np.array_equal(state0.grad.cpu().numpy(), base["grad_state0"][:, :ram.NS])
        assert np.array_equal(gains.grad.cpu().numpy(), base["grad_gains"])
        assert tracks[0].grad.is_cuda and not tracks[1].grad.is_cuda
        for tr, k in zip(tracks, ATT_KEYS):                      # summed over the loops
            assert np.abs(tr.grad.cpu().numpy() - base[k].sum(axis=0)).max() <= 1e-12 * np.abs(base[k]).sum(axis=0).max(), k
        # one of the two None: all zero, and no gradient asked for
        s2 = t(st[:, :ram.NS])
        only = t(rpyd)
        tlog2, tfinal2 = ag.rollout(r, s2, t(g), pa, T, None, att=(None, only))
        ((tlog2 * weights[0]).sum() + (tfinal2 * weights[1]).sum()).backward()
        assert only.grad is not None and np.isfinite(only.grad.cpu().numpy()).all()
    finally:
        r.close()
