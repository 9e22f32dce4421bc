"""Noise in the closed loop on the device (vsmpc_rollout_set_noise, vsmpc_rollout_noise_draws; the NOISE instantiations of
record_kernel and advance_kernel) against tests/rollout_noise_model.py:

  draws    the generator's words bit for bit, the normals to 1e-13 max(1, |z|) (sqrt is correctly rounded, log and sincos are a
           few ulp: about 1e-15 is expected), with loop indices that cross the 32-bit word of the counter;
  parity   every tick's record against build_record on measured_state of the device's own previous state (1e-13) and the state
           behind the tick against advance_with_gust (1e-12), the bars of test_gpu_rollout.py, on the parametric and the tree plant;
  bitwise  same seed, split runs, graph replay, a slice of a sharded batch, batches of 1 and 257;
  off      sigmas of zero and set_noise(None) against a rollout that never heard of noise, and what each sigma alone moves;
  refusals run before reset, the taped run and the sweep.
The configuration is (6, 2, 3) on the runtime-sized kernel unless a test says otherwise."""
import importlib

import numpy as np
import pytest

import rollout_model as rm
import rollout_noise_model as nm
from conftest import PKG, relerr

pytestmark = pytest.mark.gpu

SEED = 2025
SIGMAS = dict(pos=0.01, lin_vel=0.015, rpy=0.02, ang_vel=0.015, force=20.0, torque=5.0)   # m, m/s, rad, rad/s, N, Nm
SIG = tuple(SIGMAS[k] for k in nm.SIGMA_NAMES)
OFF = dict.fromkeys(nm.SIGMA_NAMES, 0.0)


@pytest.fixture(scope="module")
def ro(solver_mod):
    return importlib.import_module(PKG + ".rollout")


@pytest.fixture(scope="module")
def small(ro, layout):
    """(cfg, trajectory, state, params) of 257 montecarlo loops at (6, 2, 3), made once; the tests take slices"""
    cfg = layout.MPCConfig(n_iter=6, n_iter_small=2, control_horizon=3)
    st, pa = ro.make_plant(cfg, 257, workload="montecarlo")
    return cfg, ro.make_trajectory(cfg, "hover", 20.0), st, pa


def _loops(ro, small, lo, hi, adjoint=False):
    cfg, (pos, vel, alpha, adt), st, pa = small
    return ro.ClosedLoopRollout(cfg, hi - lo, pos, vel, alpha, adt, device=0, runtime="always", adjoint=adjoint), st[lo:hi], pa[lo:hi]


def _fly(ro, small, lo, hi, ticks, noise=None, **kw):
    """(logs of the runs in `ticks`, concatenated; final state) of loops lo..hi-1; noise = set_noise's keywords or None"""
    r, st, pa = _loops(ro, small, lo, hi)
    try:
        if noise is not None:
            r.set_noise(**noise)
        r.reset(st, pa)
        logs = [r.run(t) for t in ticks]
        return np.concatenate(logs), r.state()
    finally:
        r.close()


def test_draws_match_model(ro, small):
    first = 2 ** 32 - 2                                        # loops 0..4 cross the word boundary of the counter
    r, st, pa = _loops(ro, small, 0, 5)
    try:
        r.set_noise(SEED, first_index=first)
        worst = 0.0
        for tick0, ticks in ((0, 4), (1000, 2)):
            z, w = r.noise_draws(tick0, ticks, words=True)
            zm, wm = nm.draws(SEED, first, 5, tick0, ticks)
            np.testing.assert_array_equal(w, wm)
            err = float((np.abs(z - zm) / np.maximum(1.0, np.abs(zm))).max())
            worst = max(worst, err)
            np.testing.assert_array_equal(r.noise_draws(tick0, ticks), z)
        print(f"noise draws: worst |z - model| / max(1, |z|) = {worst:.3e}")
        assert worst <= 1e-13
        assert len({tuple(row) for row in w.reshape(-1, 4)}) == w.size // 4       # no block repeats another
    finally:
        r.close()


def _parity(ro, cfg, st, pa, traj, ticks, rec_bar, state_bar, tree=None):
    """the shape of test_gpu_rollout.py::test_record_and_advance_kernels_match_model, with all six sigmas"""
    pos, vel, alpha, adt = traj
    B = len(st)
    r = ro.ClosedLoopRollout(cfg, B, pos, vel, alpha, adt, device=0)
    worst_rec = worst_state = 0.0
    try:
        if tree is not None:
            r.set_tree(tree)
            rm.set_tree(tree)
        r.set_noise(SEED, **SIGMAS)
        with pytest.raises(Exception):
            r.run(1)                                           # the records hold the other measurement: reset() first
        r.reset(st, pa)
        s_host = st.copy()
        z = nm.draws(SEED, 0, B, 0, ticks + 1)[0]
        meas = lambda b, k: nm.measured_state(s_host[b], pa[b], rm.inertia_body(s_host[b], pa[b]), z[k, b], SIG)
        models = [rm.make_tick_model(cfg, meas(b, 0), pa[b], pos, vel, alpha) for b in range(B)]
        recs = r.next_records()
        for tick in range(ticks):
            log = r.run(1)
            x, fm, status, iters = r.mpc.solve(recs)          # same kernel, same records -> the first move the loop used
            after = r.state()
            for b in range(B):
                e = relerr(recs[b], rm.build_record(cfg, models[b], meas(b, tick), pa[b]))
                worst_rec = max(worst_rec, e)
                print(f"tick {tick} loop {b}: record {e:.2e}", end="")
                assert e < rec_bar, (tick, b)
                models[b].consume(fm[b], status[b])
                s_m = nm.advance_with_gust(cfg, s_host[b], pa[b], tick, fm[b], status[b], alpha, adt, z[tick, b], SIG)
                e = relerr(after[b], s_m)
                worst_state = max(worst_state, e)
                print(f" state {e:.2e}")
                assert e < state_bar, (tick, b)
                assert log[0, b, 14] == status[b] and log[0, b, 15] == iters[b]
                # the log row is the TRUE state: neither the measured one nor the one without the gust
                np.testing.assert_array_equal(log[0, b, 0:3], after[b, 0:3])
                np.testing.assert_array_equal(log[0, b, 3:6], after[b, 6:9])
                np.testing.assert_array_equal(log[0, b, 6:10], after[b, 12:16])
            # and the noise is in both: the record is off the true state, the state off the plant without the gust
            assert np.abs(recs[:, rm.L.IN_X0:rm.L.IN_X0 + 3] - s_host[:, 0:3]).max(axis=1).min() > 1e-6
            plain = rm.advance(cfg, s_host[0], pa[0], tick, fm[0], status[0], alpha, adt)
            assert np.abs(after[0, 3:6] - plain[3:6]).max() > 1e-3
            recs = r.next_records()
            s_host = after
        print(f"worst record {worst_rec:.3e} (bar {rec_bar:g}), worst state {worst_state:.3e} (bar {state_bar:g})")
    finally:
        rm.set_tree(None)
        r.close()


def test_record_and_advance_match_model_with_noise(ro, layout):
    cfg = layout.paper_config()
    st, pa = ro.make_plant(cfg, 12, workload="montecarlo")
    _parity(ro, cfg, st, pa, ro.make_trajectory(cfg, "hover", 60.0), 3, 1e-13, 1e-12)


def test_tree_plant_with_noise_matches_model(ro, layout):
    """I_B of the measured angular momentum is the tree's I_B(q).  The same bars as on the parametric plant (measured on an
    MI355X: worst record 1.7e-16, worst state 9.3e-18; the parametric plant's 1.0e-17 and 8.8e-18)."""
    RT = importlib.import_module(PKG + ".robot_tree")
    tree = RT.default_tree()
    cfg = layout.paper_config()
    st, pa = ro.make_plant_tree(cfg, 2, tree, workload="montecarlo")
    _parity(ro, cfg, st, pa, ro.make_trajectory(cfg, "hover", 20.0), 2, 1e-13, 1e-12, tree=tree)


def test_same_seed_is_bitwise_reproducible_and_another_seed_is_not(ro, small):
    noise = dict(seed=SEED, **SIGMAS)
    log_a, fin_a = _fly(ro, small, 0, 8, [6], noise)
    log_b, fin_b = _fly(ro, small, 0, 8, [6], noise)
    np.testing.assert_array_equal(log_a, log_b)
    np.testing.assert_array_equal(fin_a, fin_b)
    log_c, fin_c = _fly(ro, small, 0, 8, [6], dict(noise, seed=SEED + 1))
    assert (np.abs(fin_c[:, 0:12] - fin_a[:, 0:12]).max(axis=1) > 0).all()     # in every loop
    assert (np.abs(log_c - log_a).max(axis=(0, 2)) > 0).all()


def test_graph_replay_split_runs_and_single_ticks_agree(ro, small):
    noise = dict(seed=SEED, **SIGMAS)
    log, fin = _fly(ro, small, 0, 8, [30], noise)              # one graph replay of 25 ticks + 5 direct ticks
    log1, fin1 = _fly(ro, small, 0, 8, [1] * 30, noise)
    np.testing.assert_array_equal(log, log1)
    np.testing.assert_array_equal(fin, fin1)
    log2, fin2 = _fly(ro, small, 0, 8, [10, 20], noise)
    np.testing.assert_array_equal(log, log2)
    np.testing.assert_array_equal(fin, fin2)
    assert np.isfinite(log).all() and (log[:, :, 14] == 1).all()


def test_a_slice_draws_what_the_whole_batch_draws(ro, small):
    noise = dict(seed=SEED, **SIGMAS)
    log, fin = _fly(ro, small, 0, 8, [5], noise)
    log_s, fin_s = _fly(ro, small, 4, 8, [5], dict(noise, first_index=4))
    np.testing.assert_array_equal(log[:, 4:8], log_s)
    np.testing.assert_array_equal(fin[4:8], fin_s)
    log_w, _ = _fly(ro, small, 4, 8, [5], noise)               # (and without first_index it does not)
    assert (np.abs(log_w - log_s).max(axis=(0, 2)) > 0).all()


def test_batches_of_1_and_257(ro, small):
    noise = dict(seed=SEED, **SIGMAS)
    log, fin = _fly(ro, small, 0, 257, [3], noise)
    assert np.isfinite(log).all() and np.isfinite(fin).all()
    for b in (0, 256):
        log_1, fin_1 = _fly(ro, small, b, b + 1, [3], dict(noise, first_index=b))
        np.testing.assert_array_equal(log[:, b:b + 1], log_1)
        np.testing.assert_array_equal(fin[b:b + 1], fin_1)
    r, st, pa = _loops(ro, small, 0, 257)
    try:
        r.set_noise(SEED)
        z, w = r.noise_draws(2, 1, words=True)
        np.testing.assert_array_equal(w, nm.draws(SEED, 0, 257, 2, 1)[1])
    finally:
        r.close()


def test_noise_off_is_the_rollout_without_noise(ro, small):
    log, fin = _fly(ro, small, 0, 8, [30])
    log0, fin0 = _fly(ro, small, 0, 8, [30], dict(seed=SEED, **OFF))
    np.testing.assert_array_equal(log0, log)
    np.testing.assert_array_equal(fin0, fin)
    r, st, pa = _loops(ro, small, 0, 8)
    try:
        r.set_noise(SEED, **SIGMAS)
        r.reset(st, pa)
        noisy = r.run(30)
        assert np.abs(noisy - log).max() > 1e-6
        r.set_noise(None)
        with pytest.raises(Exception):
            r.run(1)
        r.reset(st, pa)
        np.testing.assert_array_equal(r.run(30), log)
        np.testing.assert_array_equal(r.state(), fin)
    finally:
        r.close()


def _one_tick(ro, small, noise):
    """(record of tick 0, first move and status of its solve, state behind tick 0) of loops 0..3"""
    r, st, pa = _loops(ro, small, 0, 4)
    try:
        if noise is not None:
            r.set_noise(**noise)
        r.reset(st, pa)
        recs = r.next_records()
        _, fm, status, _ = r.mpc.solve(recs)
        r.run(1, log=False)
        return recs, fm, status, r.state()
    finally:
        r.close()


def test_each_sigma_moves_only_what_it_should(ro, small, layout):
    cfg, (pos, vel, alpha, adt), st, pa = small
    L = layout
    recs0, fm0, status0, after0 = _one_tick(ro, small, None)
    assert (status0 == L.STATUS_SOLVED).all()
    span = lambda off, n: set(range(off, off + n))
    x0 = lambda a, b: span(L.IN_X0 + a, b - a)
    window_hlin = {L.IN_XREF + 12 * j + i for j in range(cfg.n_ref_cols) for i in (3, 4, 5, 9, 10, 11)}   # columns hold R^T m v, I W rpy'
    may_move = {
        "pos": x0(0, 3) | x0(20, 23),
        "lin_vel": x0(3, 6),
        "rpy": x0(6, 9) | x0(23, 26) | span(L.IN_RPY, 3) | span(L.IN_WRB, 9) | span(L.IN_INERTIA, 9) | window_hlin,
        "ang_vel": x0(9, 12) | span(L.IN_OMEGA, 3),
    }
    must_move = {"pos": x0(0, 3), "lin_vel": x0(3, 6), "rpy": x0(6, 9) | span(L.IN_WRB, 9), "ang_vel": x0(9, 12) | span(L.IN_OMEGA, 3)}
    for name in ("pos", "lin_vel", "rpy", "ang_vel"):
        recs, fm, status, after = _one_tick(ro, small, dict(seed=SEED, **dict(OFF, **{name: SIGMAS[name]})))
        for b in range(4):
            moved = set(np.nonzero(recs[b] != recs0[b])[0].tolist())
            assert moved <= may_move[name], (name, b, sorted(moved - may_move[name]))
            assert must_move[name] <= moved, (name, b, sorted(must_move[name] - moved))
            # the plant saw the noise through the first move alone: the tick-0 record rebuilt without it is the plain one, and
            # the state behind tick 0 is the plain plant's under the noisy record's move
            s_m = rm.advance(cfg, st[b], pa[b], 0, fm[b], status[b], alpha, adt)
            assert relerr(after[b], s_m) < 1e-12, (name, b)
        assert np.abs(fm - fm0).max() > 0
    # the force reaches h_lin and through it p; the torque reaches h_ang, then the attitude, then through R the rest of 0..11
    for name, moves, must in (("force", span(0, 6), span(3, 3)), ("torque", span(0, 12), span(6, 6))):
        recs, fm, status, after = _one_tick(ro, small, dict(seed=SEED, **dict(OFF, **{name: SIGMAS[name]})))
        np.testing.assert_array_equal(recs, recs0)             # the gust of tick 0 is not in the record of tick 0
        np.testing.assert_array_equal(fm, fm0)
        for b in range(4):
            moved = set(np.nonzero(after[b] != after0[b])[0].tolist())
            assert moved <= moves and must <= moved and moved & span(0, 3), (name, b, sorted(moved))


def test_refusals(ro, small):
    r, st, pa = _loops(ro, small, 0, 4, adjoint=True)
    try:
        r.reset(st, pa)
        r.set_noise(SEED)
        with pytest.raises(Exception):
            r.run(1)                                           # reset() first
        r.reset(st, pa)
        r.run(2)
        with pytest.raises(Exception, match="noise"):
            r.run(2, tape=True)
        with pytest.raises(Exception, match="noise"):
            r.backward(state_bar=np.ones((4, rm.L.PLANT_STATE)))
        with pytest.raises(Exception, match="sigma_rpy"):
            r.set_noise(SEED, rpy=-1.0)
        r.run(1)                                               # a refused set_noise leaves the rollout as it was
        r.set_noise(None)
        r.reset(st, pa)
        r.run(2, tape=True)
        out = r.backward(state_bar=np.ones((4, rm.L.PLANT_STATE)))
        assert np.isfinite(out["grad_state0"]).all() and np.abs(out["grad_state0"]).max() > 0
    finally:
        r.close()
