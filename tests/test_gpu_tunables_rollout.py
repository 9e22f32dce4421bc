"""Closed loops that each carry their own weights and throttle box (vsmpc_rollout_set_tunables): 8 hover loops with
distinct tunables over 50 ticks (two releases of the 20-tick hold, across the 25-tick chunk of the captured graph), tick
by tick against tests/rollout_model.py driven by the oracle with every loop's own configuration, against one
single-configuration rollout per loop, graph replay against direct launches, and NULL restoring the shared configuration."""
import dataclasses
import importlib

import numpy as np
import pytest

import rollout_model as rm
from conftest import PKG, relerr

pytestmark = pytest.mark.gpu

B, TICKS = 8, 50


@pytest.fixture(scope="module")
def ro(solver_mod):
    return importlib.import_module(PKG + ".rollout")


def loop_configs(layout, ref):
    """8 loops: distinct (w_throttle, w_initial_throttle), joint weights, state weights and throttle boxes"""
    out = []
    for b in range(B):
        kw = dict(w_throttle=40000.0 + 15000.0 * b, w_initial_throttle=120000.0 - 9000.0 * b,
                  w_delta_joint=tuple(65000.0 / (1.0 + 0.5 * ((b + j) % 5)) for j in range(8)),
                  w_com_pos=(500.0 + 40.0 * b, 500.0 + 25.0 * b, 5000.0 - 300.0 * b), w_reg_joint_pos=5.0 * b,
                  throttle_min=2.0 * b, throttle_max=100.0 - 3.0 * b)
        out.append((layout.MPCConfig(**kw), ref.Config(**kw)))
    return out


def run_loops(ro, cfg, st, pa, traj, configs=None, chunks=(TICKS,)):
    pos, vel, alpha, adt = traj
    r = ro.ClosedLoopRollout(cfg, len(st), pos, vel, alpha, adt, device=0)
    try:
        if configs is not None:
            r.set_tunables(configs=configs)
        r.reset(st, pa)
        logs = [r.run(n) for n in chunks]
        return np.concatenate(logs), r.state()
    finally:
        r.close()


def test_distinct_tunables_per_loop(ro, layout, ref):
    cfg = layout.paper_config()
    st, pa = ro.make_plant(cfg, B, workload="hover")
    traj = ro.make_trajectory(cfg, "hover", 60.0)
    pos, vel, alpha, adt = traj
    cfgs = loop_configs(layout, ref)
    log, state = run_loops(ro, cfg, st, pa, traj, configs=[c for c, _ in cfgs])           # 2 graph replays of 25 ticks
    assert (log[:, :, 14] == layout.STATUS_SOLVED).all()
    # the loops do differ from one another and from the shared configuration
    shared_log, _ = run_loops(ro, cfg, st, pa, traj)
    assert (np.abs(log[-1, :, 10:14] - shared_log[-1, :, 10:14]).max(axis=1) > 1e-6).all()
    # tick by tick against the model, the oracle solving every loop's QP under that loop's configuration
    for b in range(B):
        s = st[b].copy()
        model = rm.make_tick_model(cfg, s, pa[b], pos, vel, alpha)
        for tick in range(TICKS):
            rec = rm.build_record(cfg, model, s, pa[b])
            x, _, _, _ = ref.solve_instance(cfgs[b][1], rec)  # (the oracle ends on the exact optimum: Solved)
            fm = ref.first_move_vector(cfgs[b][1], x)
            model.consume(fm, 1)
            s = rm.advance(cfg, s, pa[b], tick, fm, 1, alpha, adt)
            row = log[tick, b]
            assert relerr(row[0:3], s[layout.PS_P:layout.PS_P + 3]) < 1e-8, (b, tick)
            assert relerr(row[3:6], s[layout.PS_RPY:layout.PS_RPY + 3]) < 1e-8, (b, tick)
            assert relerr(row[6:10], s[layout.PS_T:layout.PS_T + 4]) < 1e-8, (b, tick)
            assert relerr(row[10:14], s[layout.PS_U:layout.PS_U + 4]) < 1e-8, (b, tick)
        assert relerr(state[b], s) < 1e-8, b
    # one single-configuration rollout per loop: the same kernels' shared kind, bit for bit
    for b in range(B):
        own = dataclasses.replace(cfgs[b][0])
        one_log, one_state = run_loops(ro, own, st[b:b + 1], pa[b:b + 1], traj)
        assert np.array_equal(one_log[:, 0], log[:, b]), (b, relerr(one_log[:, 0], log[:, b]))
        assert np.array_equal(one_state[0], state[b]), b
    # direct launches (runs shorter than the captured chunk) agree with the graph replay
    direct_log, direct_state = run_loops(ro, cfg, st, pa, traj, configs=[c for c, _ in cfgs], chunks=(20, 20, 10))
    assert np.array_equal(direct_log, log) and np.array_equal(direct_state, state)
    # 30 ticks in one run: 25 replayed, 5 launched directly
    mixed_log, _ = run_loops(ro, cfg, st, pa, traj, configs=[c for c, _ in cfgs], chunks=(30,))
    assert np.array_equal(mixed_log, log[:30])


def test_null_restores_the_shared_configuration(ro, layout, ref):
    cfg = layout.paper_config()
    st, pa = ro.make_plant(cfg, B, workload="hover")
    traj = ro.make_trajectory(cfg, "hover", 60.0)
    pos, vel, alpha, adt = traj
    plain_log, plain_state = run_loops(ro, cfg, st, pa, traj, chunks=(30,))
    r = ro.ClosedLoopRollout(cfg, B, pos, vel, alpha, adt, device=0)
    try:
        r.set_tunables(configs=[c for c, _ in loop_configs(layout, ref)])
        r.reset(st, pa)
        tuned_log = r.run(30)
        assert not np.array_equal(tuned_log, plain_log)
        with pytest.raises(Exception):
            r.set_tunables(None), r.run(1)                     # a change of tunables asks for a reset
        r.set_tunables(None)
        r.reset(st, pa)
        back_log = r.run(30)
        assert np.array_equal(back_log, plain_log) and np.array_equal(r.state(), plain_state)
        # rows of the shared configuration: the tuned kind computes what the shared kind computes
        r.set_tunables(configs=[cfg] * B)
        r.reset(st, pa)
        assert np.array_equal(r.run(30), plain_log)
    finally:
        r.close()
