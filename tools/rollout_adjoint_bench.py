"""Time per tick of the rollout's backward sweep (vsmpc_rollout_backward_device) against the forward tick (vsmpc_rollout_run,
graph replay), the taped forward tick (vsmpc_rollout_run_taped, direct launches and the tape's copies) and the record-adjoint
launch alone (vsmpc_adjoint_record_batch_device on the records of one tick, the launch every tick of the sweep contains), and
of the sweep that also returns the parameter and track gradients (vsmpc_rollout_backward_full_device: the same launches, the
second instantiation of advance_adjoint_kernel).

    python tools/rollout_adjoint_bench.py [--out profiles/rollout_adjoint_bench.txt] [--rounds 7] [--tree | --attitude]

--tree: instead, a backward tick on the kinematic-tree plant (set_tree(tree, adjoint=True)) against a backward tick on the
parametric plant of the same build -- two rollouts of the same workloads in one process, their sweeps alternating -- with
the Jacobian launch every launch of the tree sweep contains (vsmpc_tree_jacobian_batch_device on a row of plant states) alone
beside them.

--attitude: instead, a backward tick of a rollout whose attitude tracks were set with VSMPC_ATTITUDE_ADJOINT (an RPY and an
RPYDot track; the ATT instantiations of the advance adjoint kernel) against a backward tick of a rollout without the flag (the
same RPY track, no RPYDot track: that one it would refuse) -- on the parametric and on the tree plant, two rollouts of the same
workloads in one process, their sweeps alternating; the flagged one also with grad_att asked for.

Workloads: batch 256 hover and batch 4096 take-off at the paper horizon (17, 7, 12), tuned handle.  Host clock around calls
that end in a synchronise; the five kinds ALTERNATE, `rounds` windows each after a warm-up window of all, and the report is
the median and the min..max spread of each and the ratios of the medians -- all in one process, one box.  A record, not a
gate."""
from __future__ import annotations

import argparse
import importlib
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "paper_gorbani_2025_humanoids_multi-rate-mpc-ironcub_amd"
CASES = [("hover", 256, 50), ("takeoff", 4096, 25)]            # workload, batch, ticks per window (>= the graph's 25)


def run_case(workload, batch, ticks, rounds):
    import torch
    layout = importlib.import_module(PKG + ".layout")
    ro = importlib.import_module(PKG + ".rollout")
    cfg = layout.paper_config()
    st, pa = ro.make_plant(cfg, batch, workload=workload)
    pos, vel, alpha, adt = ro.make_trajectory(cfg, workload, 60.0)
    r = ro.ClosedLoopRollout(cfg, batch, pos, vel, alpha, adt, device=0, adjoint=True)
    m = r.mpc
    dev = torch.device("cuda:0")
    f64, i32 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.int32, device=dev)
    rng = np.random.default_rng(0)
    d_lb = torch.from_numpy(rng.standard_normal((ticks, batch, layout.ROLLOUT_LOG))).to(dev)
    d_sb = torch.from_numpy(rng.standard_normal((batch, layout.PLANT_STATE))).to(dev)
    d_g0, d_gg, d_fl = torch.empty((batch, layout.PLANT_STATE), **f64), torch.empty((batch, layout.GRAD_SIZE), **f64), torch.empty(batch, **i32)
    d_xbar, d_fmbar = torch.zeros((batch, m.n_var), **f64), torch.from_numpy(rng.standard_normal((batch, 24))).to(dev)
    d_st, d_gc, d_gin = torch.empty(batch, **i32), torch.empty((batch, layout.GRAD_SIZE), **f64), torch.empty((batch, m.n_in), **f64)
    d_afl = torch.empty(batch, **i32)
    d_gp, d_gt = torch.empty((batch, layout.PLANT_PARAMS), **f64), torch.empty((batch, 6 * len(pos) + len(alpha)), **f64)
    r.reset(st, pa)
    d_rec = torch.from_numpy(r.next_records()).to(dev)
    s = torch.cuda.current_stream(dev)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / ticks         # us per tick

    def record_alone():
        for _ in range(ticks):
            m.solve_adjoint_record_device(d_rec, None, d_xbar, d_fmbar, None, None, d_st, None, None, d_gc, None, d_afl, d_gin,
                                          None, stream=s)

    kinds = {
        "forward": lambda: r.run(ticks, log=False),
        "forward_taped": lambda: r.run(ticks, log=False, tape=True),
        "backward": lambda: r.backward_device(d_lb, d_sb, d_g0, d_gg, d_fl, stream=s),      # (sweeps the tape in front of it)
        "record_alone": record_alone,
        "backward_full": lambda: r.backward_device(d_lb, d_sb, d_g0, d_gg, d_fl, stream=s, d_grad_params=d_gp, d_grad_traj=d_gt),
    }
    for fn in kinds.values():                                    # warm-up window of all (builds the graph, grows the tape)
        timed(fn)
    r.reset(st, pa)
    t = {k: [] for k in kinds}
    for _ in range(rounds):
        for k, fn in kinds.items():
            t[k].append(timed(fn))
    flags = d_fl.cpu().numpy()
    med = {k: statistics.median(v) for k, v in t.items()}
    lines = [f"paper {workload} batch {batch} ({m.kernel_name}), {rounds} alternating windows of {ticks} ticks; last sweep: "
             f"{int((flags & layout.ADJ_UNSOLVED != 0).sum())} loops with an unsolved tick, "
             f"{int((flags & layout.ADJ_DEGENERATE != 0).sum())} with a degenerate one, "
             f"gradients finite: {bool(torch.isfinite(d_g0).all()) and bool(torch.isfinite(d_gg).all())}"]
    for k in kinds:
        lines.append(f"  {k:14s}  median {med[k]:10.2f} us/tick  ({med[k] / batch:.4f} us per loop and tick)  min {min(t[k]):10.2f}  "
                     f"max {max(t[k]):10.2f}  spread {100.0 * (max(t[k]) - min(t[k])) / med[k]:.2f} %")
    for k, base in (("forward_taped", "forward"), ("backward", "forward"), ("backward", "record_alone"),
                    ("backward_full", "backward"), ("backward_full", "record_alone")):
        ratios = [a / b for a, b in zip(t[k], t[base])]
        lines.append(f"  {k} / {base} (medians) {med[k] / med[base]:.4f}   per round min {min(ratios):.4f} max {max(ratios):.4f}")
    lines.append(f"  backward_full - backward (medians) {med['backward_full'] - med['backward']:.2f} us/tick: the parameter and track shares "
                 f"(one dependent load, {8 * (layout.PLANT_PARAMS)} B row read and written per instance and launch); gradients finite: "
                 f"{bool(torch.isfinite(d_gp).all()) and bool(torch.isfinite(d_gt).all())}")
    lines.append(f"  backward - record_alone (medians) {med['backward'] - med['record_alone']:.2f} us/tick: advance_adjoint_kernel and "
                 f"the gaps between the two launches of a tick")
    r.close()
    return lines


def run_tree_case(workload, batch, ticks, rounds):
    """a backward tick on the tree plant against one on the parametric plant, and the Jacobian launch alone"""
    import torch
    layout = importlib.import_module(PKG + ".layout")
    ro = importlib.import_module(PKG + ".rollout")
    tree = importlib.import_module(PKG + ".robot_tree").default_tree()
    cfg = layout.paper_config()
    pos, vel, alpha, adt = ro.make_trajectory(cfg, workload, 60.0)
    dev = torch.device("cuda:0")
    f64, i32 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.int32, device=dev)
    rng = np.random.default_rng(0)
    d_lb = torch.from_numpy(rng.standard_normal((ticks, batch, layout.ROLLOUT_LOG))).to(dev)
    d_sb = torch.from_numpy(rng.standard_normal((batch, layout.PLANT_STATE))).to(dev)
    d_g0, d_gg, d_fl = torch.empty((batch, layout.PLANT_STATE), **f64), torch.empty((batch, layout.GRAD_SIZE), **f64), torch.empty(batch, **i32)
    d_gp, d_gt = torch.empty((batch, layout.PLANT_PARAMS), **f64), torch.empty((batch, 6 * len(pos) + len(alpha)), **f64)
    s = torch.cuda.current_stream(dev)
    rolls = {}
    for plant in ("parametric", "tree"):
        r = ro.ClosedLoopRollout(cfg, batch, pos, vel, alpha, adt, device=0, adjoint=True)
        if plant == "tree":
            r.set_tree(tree, adjoint=True)
            st, pa = ro.make_plant_tree(cfg, batch, tree, workload=workload)
        else:
            st, pa = ro.make_plant(cfg, batch, workload=workload)
        r.reset(st, pa)
        r.run(ticks, log=False, tape=True)
        rolls[plant] = r
    d_q = torch.from_numpy(rolls["tree"].state()[:, layout.PS_Q:layout.PS_Q + 8].copy()).to(dev)
    d_T = torch.from_numpy(rolls["tree"].state()[:, layout.PS_T:layout.PS_T + 4].copy()).to(dev)
    d_tt, d_tj = torch.empty((batch, layout.TT_SIZE), **f64), torch.empty((batch, layout.TT_SIZE, layout.TT_NDIR), **f64)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / ticks         # us per tick

    def jacobian_alone():
        for _ in range(ticks):
            rolls["tree"].mpc.tree_jacobian_device(tree, d_q, d_T, d_tt, d_tj, stream=s)

    kinds = {}
    for plant, r in rolls.items():
        kinds["backward_" + plant] = lambda r=r: r.backward_device(d_lb, d_sb, d_g0, d_gg, d_fl, stream=s)
        kinds["backward_full_" + plant] = lambda r=r: r.backward_device(d_lb, d_sb, d_g0, d_gg, d_fl, stream=s, d_grad_params=d_gp,
                                                                          d_grad_traj=d_gt)
    kinds["jacobian_alone"] = jacobian_alone
    for fn in kinds.values():
        timed(fn)
    t = {k: [] for k in kinds}
    flags = {}
    for _ in range(rounds):
        for k, fn in kinds.items():
            t[k].append(timed(fn))
            if k.startswith("backward_full_"):
                flags[k[len("backward_full_"):]] = (d_fl.cpu().numpy(), bool(torch.isfinite(d_g0).all()) and bool(torch.isfinite(d_gp).all()))
    med = {k: statistics.median(v) for k, v in t.items()}
    lines = [f"paper {workload} batch {batch} ({rolls['tree'].mpc.kernel_name}), {rounds} alternating windows of {ticks} ticks; last sweeps: "
             + "; ".join(f"{plant}: {int((fl & layout.ADJ_UNSOLVED != 0).sum())} loops with an unsolved tick, "
                         f"{int((fl & layout.ADJ_DEGENERATE != 0).sum())} with a degenerate one, gradients finite: {fin}"
                         for plant, (fl, fin) in flags.items())]
    for k in kinds:
        unit = "us/launch" if k == "jacobian_alone" else "us/tick"
        lines.append(f"  {k:24s}  median {med[k]:10.2f} {unit}  min {min(t[k]):10.2f}  max {max(t[k]):10.2f}  "
                     f"spread {100.0 * (max(t[k]) - min(t[k])) / med[k]:.2f} %")
    for k in ("backward", "backward_full"):
        a, b = k + "_tree", k + "_parametric"
        ratios = [x / y for x, y in zip(t[a], t[b])]
        lines.append(f"  {a} / {b} (medians) {med[a] / med[b]:.4f}   per round min {min(ratios):.4f} max {max(ratios):.4f};   "
                     f"difference {med[a] - med[b]:.2f} us/tick, of which the Jacobian launch alone is {med['jacobian_alone']:.2f}")
    for r in rolls.values():
        r.close()
    return lines


def run_attitude_case(workload, batch, ticks, rounds, plant):
    """a backward tick with VSMPC_ATTITUDE_ADJOINT against one without, on one plant"""
    import torch
    layout = importlib.import_module(PKG + ".layout")
    ro = importlib.import_module(PKG + ".rollout")
    tree = importlib.import_module(PKG + ".robot_tree").default_tree()
    cfg = layout.paper_config()
    pos, vel, alpha, adt = ro.make_trajectory(cfg, workload, 60.0)
    tt = np.arange(len(pos)) * cfg.period_large
    rpy = 0.05 * np.sin(3.0 * tt)[:, None] * np.array([1.0, -0.6, 0.4])
    rpyd = 0.15 * np.cos(3.0 * tt)[:, None] * np.array([1.0, -0.5, 0.2]) + 0.02
    dev = torch.device("cuda:0")
    f64, i32 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.int32, device=dev)
    rng = np.random.default_rng(0)
    d_lb = torch.from_numpy(rng.standard_normal((ticks, batch, layout.ROLLOUT_LOG))).to(dev)
    d_sb = torch.from_numpy(rng.standard_normal((batch, layout.PLANT_STATE))).to(dev)
    d_g0, d_gg, d_fl = torch.empty((batch, layout.PLANT_STATE), **f64), torch.empty((batch, layout.GRAD_SIZE), **f64), torch.empty(batch, **i32)
    d_gp, d_gt = torch.empty((batch, layout.PLANT_PARAMS), **f64), torch.empty((batch, 6 * len(pos) + len(alpha)), **f64)
    d_ga = torch.empty((batch, 6 * len(pos)), **f64)
    s = torch.cuda.current_stream(dev)
    rolls = {}
    for kind in ("unflagged", "flagged"):
        r = ro.ClosedLoopRollout(cfg, batch, pos, vel, alpha, adt, device=0, adjoint=True)
        if plant == "tree":
            r.set_tree(tree, adjoint=True)
            st, pa = ro.make_plant_tree(cfg, batch, tree, workload=workload)
        else:
            st, pa = ro.make_plant(cfg, batch, workload=workload)
        r.set_attitude_tracks(rpy, rpyd if kind == "flagged" else None, adjoint=kind == "flagged")
        r.reset(st, pa)
        r.run(ticks, log=False, tape=True)
        rolls[kind] = r

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / ticks         # us per tick

    kinds = {}
    for kind, r in rolls.items():
        kinds["backward_" + kind] = lambda r=r: r.backward_device(d_lb, d_sb, d_g0, d_gg, d_fl, stream=s)
        kinds["backward_full_" + kind] = lambda r=r: r.backward_device(d_lb, d_sb, d_g0, d_gg, d_fl, stream=s, d_grad_params=d_gp,
                                                                        d_grad_traj=d_gt)
    kinds["backward_attitude_flagged"] = lambda: rolls["flagged"].backward_device(d_lb, d_sb, d_g0, d_gg, d_fl, stream=s, d_grad_params=d_gp,
                                                                                   d_grad_traj=d_gt, d_grad_att=d_ga)
    for fn in kinds.values():
        timed(fn)
    t = {k: [] for k in kinds}
    for _ in range(rounds):
        for k, fn in kinds.items():
            t[k].append(timed(fn))
    fl = d_fl.cpu().numpy()
    med = {k: statistics.median(v) for k, v in t.items()}
    lines = [f"paper {workload} batch {batch}, {plant} plant ({rolls['flagged'].mpc.kernel_name}), {rounds} alternating windows of {ticks} "
             f"ticks; last sweep: {int((fl & layout.ADJ_UNSOLVED != 0).sum())} loops with an unsolved tick, "
             f"{int((fl & layout.ADJ_DEGENERATE != 0).sum())} with a degenerate one, gradients finite: "
             f"{bool(torch.isfinite(d_g0).all()) and bool(torch.isfinite(d_gp).all()) and bool(torch.isfinite(d_ga).all())}"]
    for k in kinds:
        lines.append(f"  {k:28s}  median {med[k]:10.2f} us/tick  min {min(t[k]):10.2f}  max {max(t[k]):10.2f}  "
                     f"spread {100.0 * (max(t[k]) - min(t[k])) / med[k]:.2f} %")
    for a, b in (("backward_flagged", "backward_unflagged"), ("backward_full_flagged", "backward_full_unflagged"),
                 ("backward_attitude_flagged", "backward_full_unflagged"), ("backward_attitude_flagged", "backward_full_flagged")):
        ratios = [x / y for x, y in zip(t[a], t[b])]
        lines.append(f"  {a} / {b} (medians) {med[a] / med[b]:.4f}   per round min {min(ratios):.4f} max {max(ratios):.4f};   "
                     f"difference {med[a] - med[b]:.2f} us/tick")
    for r in rolls.values():
        r.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--tree", action="store_true", help="the tree plant's backward tick against the parametric plant's")
    ap.add_argument("--attitude", action="store_true", help="a backward tick with VSMPC_ATTITUDE_ADJOINT against one without")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    mode = " --tree" if a.tree else " --attitude" if a.attitude else ""
    lines = [f"python tools/rollout_adjoint_bench.py --rounds {a.rounds}{mode} on {torch.cuda.get_device_name(0)}"]
    for workload, batch, ticks in CASES:
        if a.attitude:
            for plant in ("parametric", "tree"):
                lines += run_attitude_case(workload, batch, ticks, a.rounds, plant)
        else:
            lines += (run_tree_case if a.tree else run_case)(workload, batch, ticks, a.rounds)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
