#!/usr/bin/env python3
"""Closed-loop rollout throughput: `batch` resident loops advanced `ticks` MPC periods (3 kernels per tick).
Usage: python tools/rollout_bench.py [batch] [ticks] [workload] [jetnn|tree] [--noise]
`jetnn` selects the jet plant option (LSTM thrust dynamics + EKF, weights of tests/golden/jet_lstm.npz), `tree` the
kinematic-tree plant (provider + kinematics kernels on the plant's joints every tick: six launches per tick).
`--noise`: the cost of set_noise (all six sigmas on) -- windows of `ticks` ticks, alternately without and with noise, five of
each on one rollout, every window from a reset and without a log (give enough ticks for a window of a few tenths of a
second); prints every window and the ratio of the medians."""
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "paper_gorbani_2025_humanoids_multi-rate-mpc-ironcub_amd"


NOISE = dict(seed=2025, pos=0.01, lin_vel=0.015, rpy=0.02, ang_vel=0.015, force=20.0, torque=5.0)


def noise_windows(r, st, pa, batch, ticks, pairs=5):
    """alternating windows on one rollout: us per tick without / with noise, and the ratio of the medians"""
    import statistics
    us = {False: [], True: []}
    for on in (False, True):                      # both captured graphs and both kernel pairs warm
        r.set_noise(**NOISE) if on else r.set_noise(None)
        r.reset(st, pa)
        r.run(50, log=False)
    for w in range(2 * pairs):
        on = w % 2 == 1
        r.set_noise(**NOISE) if on else r.set_noise(None)
        r.reset(st, pa)
        log = r.run(25, log=True)                 # (set_noise dropped the captured ticks: capture outside the window)
        t0 = time.perf_counter()
        r.run(ticks, log=False)                   # returns after the last tick has completed
        us[on].append(1e6 * (time.perf_counter() - t0) / ticks)
        print(json.dumps({"window": w, "noise": on, "batch": batch, "ticks": ticks, "us_per_tick": us[on][-1],
                          "solved_fraction_first_25": float((log[:, :, 14] == 1).mean()),
                          "final_state_finite": bool(__import__("numpy").isfinite(r.state()).all())}))
    plain, noisy = statistics.median(us[False]), statistics.median(us[True])
    print(json.dumps({"what": "closed-loop rollout, noise against none", "batch": batch, "ticks": ticks,
                      "us_per_tick_plain_median": plain, "us_per_tick_noise_median": noisy, "ratio": noisy / plain,
                      "plain_spread": max(us[False]) / min(us[False]) - 1.0, "noise_spread": max(us[True]) / min(us[True]) - 1.0}))


def main():
    noise = "--noise" in sys.argv
    sys.argv = [a for a in sys.argv if a != "--noise"]
    batch = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    ticks = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
    workload = sys.argv[3] if len(sys.argv) > 3 else "hover"
    jetnn = len(sys.argv) > 4 and sys.argv[4] == "jetnn"
    tree = len(sys.argv) > 4 and sys.argv[4] == "tree"
    import torch  # noqa: F401  (HIP runtime first)
    import __graft_entry__ as ge
    ge.build()
    pkg = importlib.import_module(PKG)
    ro = importlib.import_module(PKG + ".rollout")
    cfg = pkg.paper_config()
    st, pa = ro.make_plant(cfg, batch, workload=workload)
    tr = None
    if tree:
        tr = importlib.import_module(PKG + ".robot_tree").default_tree()
        st, pa = ro.make_plant_tree(cfg, batch, tr, workload=workload)
    pos, vel, alpha, adt = ro.make_trajectory(cfg, "takeoff" if workload == "takeoff" else "hover", 60.0)
    r = ro.ClosedLoopRollout(cfg, batch, pos, vel, alpha, adt)
    if tree:
        r.set_tree(tr)
    jm = None
    if jetnn:
        import numpy as np
        g = np.load(os.path.join(ROOT, "tests", "golden", "jet_lstm.npz"))
        jm = importlib.import_module(PKG + ".jet_plant").JetModelTotal(g["w_ih"], g["w_hh"], g["b_ih"], g["b_hh"], g["fc_w"],
                                                                       g["fc_b"], g["norm"], device=0, max_series=64)
        r.set_jet_plant(jm)
    if noise:
        noise_windows(r, st, pa, batch, ticks)
        r.close()
        return
    r.reset(st, pa)
    r.run(50, log=False)
    r.reset(st, pa)
    t0 = time.perf_counter()
    log = r.run(ticks, log=True)
    dt = time.perf_counter() - t0
    solved = float((log[:, :, 14] == 1).mean())
    print(json.dumps({"what": "closed-loop rollout", "batch": batch, "ticks": ticks, "workload": workload,
                      "us_per_tick": 1e6 * dt / ticks, "instance_ticks_per_s": batch * ticks / dt,
                      "realtime_factor": batch * ticks * cfg.period_mpc / dt, "solved_fraction": solved,
                      "mean_active_set_iters": float(log[:, :, 15].mean()), "jet_plant": "lstm+ekf" if jetnn else "polynomial", "plant": "kinematic tree" if tree else "parametric",
                      "final_altitude_error_mean_m": float(abs(log[-1, :, 2] - pa[:, 236] - (pos[min(len(pos) - 1, 0), 2])).mean())
                      if workload != "takeoff" else None,
                      "final_thrust_mean_N": float(log[-1, :, 6:10].mean())}))
    r.close()


if __name__ == "__main__":
    main()
