"""Bit identity of the closed-loop rollout and its adjoint between two builds: dump the outputs from each build, then compare.

    python tools/rollout_identity.py dump OUT.npz [--tree DIR]   # on a GPU; DIR: the tree whose package and library run
    python tools/rollout_identity.py compare A.npz B.npz         # anywhere: tools/runtime_identity.py's compare

dump runs, on the library of `--tree` (default: the tree this file lies in) and on the inputs of THIS tree's tests/:
  the ten cases of tests/rollout_adjoint_edge_cases.py and the four loops of tests/rollout_adjoint_cases.py at both of its
      horizons, each run plain (log, final state, next records), taped (the same) and swept backward twice: plain
      (backward/: grad_state0, grad_gains, flags) and with the parameter and track gradients (backward_full/: those and
      grad_params, grad_traj_pos, grad_traj_vel, grad_traj_alpha) -- the two instantiations of advance_adjoint_kernel;
  the kinematic-tree plant with set_tree(tree, adjoint=True), as tests/test_gpu_rollout_tree_adjoint.py builds its rollouts:
      the five loops of tests/rollout_tree_adjoint_cases.py at HORIZONS[0], SELECTED under its joint selector, and
      TUNED_LOOPS at HORIZONS[1], each run plain, taped and swept plain and full -- the two instantiations of
      advance_tree_adjoint_kernel behind tree_jacobian_kernel;
  hover, take-off and Monte-Carlo at batch 6 for 30 ticks at the paper horizon: one replay of the captured 25 ticks and five
      direct ticks;
  one kinematic-tree loop and one jet-plant loop as tests/test_gpu_rollout.py builds them, 6 ticks each.
Every array is compared with np.array_equal, NaN patterns included.  The tool runs on the inputs and with the cases of the
tree it lies in whatever `--tree` names, so a dump of an earlier commit comes from this file with `--tree` on a checkout of
that commit that has been built."""
from __future__ import annotations

import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "paper_gorbani_2025_humanoids_multi-rate-mpc-ironcub_amd"


def _mod(name):
    return importlib.import_module(f"{PKG}.{name}")


def _swept(make, ticks, lb, sb):
    """plain run, then taped run and the two sweeps of its tape, each run on a rollout of its own from make()"""
    out = {}
    r = make()
    try:
        out["plain/log"], out["plain/state"], out["plain/next_records"] = r.run(ticks), r.state(), r.next_records()
    finally:
        r.close()
    r = make()
    try:
        out["taped/log"], out["taped/state"], out["taped/next_records"] = r.run(ticks, tape=True), r.state(), r.next_records()
        for k, v in r.backward(lb, sb).items():
            out[f"backward/{k}"] = np.asarray(v)
        for k, v in r.backward(lb, sb, params=True, traj=True).items():
            out[f"backward_full/{k}"] = np.asarray(v)
    finally:
        r.close()
    return out


def dump(path):
    import rollout_adjoint_cases as rc
    import rollout_adjoint_edge_cases as ec
    import rollout_tree_adjoint_cases as tc
    L, ro, ag = _mod("layout"), _mod("rollout"), _mod("autograd")
    out = {}

    def rollout(cfg, rows, st, pa, traj, runtime):
        pos, vel, alpha, adt = traj
        r = ro.ClosedLoopRollout(cfg, len(st), pos, vel, alpha, adt, device=0, runtime=runtime, adjoint=True)
        r.set_tunables(configs=rows)
        r.reset(st, pa)
        return r

    for case, c in ec.CASES.items():
        cfg, (st, pa) = ec.config(L.MPCConfig, case), ec.plants(case)
        rows = ag.configs_of(cfg, ec.gains(L.MPCConfig, case))
        lb, sb = ec.case_loss_weights(case)
        for k, v in _swept(lambda: rollout(cfg, rows, st, pa, ec.trajectory(case), c.runtime), c.ticks, lb, sb).items():
            out[f"edge_{case}/{k}"] = v
        print(f"edge case {case}: {len(st)} loops, {c.ticks} ticks", flush=True)
    for hz in rc.HORIZONS:
        cfg, (st, pa) = rc.config(L.MPCConfig, hz), rc.plants()
        rows = ag.configs_of(cfg, rc.gains(L.MPCConfig, hz))
        lb, sb = rc.loss_weights()
        runtime = "always" if hz == rc.HORIZONS[0] else "never"
        for k, v in _swept(lambda: rollout(cfg, rows, st, pa, rc.trajectory(), runtime), rc.TICKS, lb, sb).items():
            out[f"four_loops_{'_'.join(map(str, hz))}/{k}"] = v
        print(f"four loops at {hz}: {rc.TICKS} ticks", flush=True)

    def tree_rollout(hz, idx, selector):
        cfg, (st, pa) = tc.config(L.MPCConfig, hz), tc.plants()
        pos, vel, alpha, adt = tc.trajectory()
        r = ro.ClosedLoopRollout(cfg, len(idx), pos, vel, alpha, adt, device=0, runtime="always" if hz == tc.HORIZONS[0] else "never",
                                 adjoint=True)
        try:
            if selector is not None:
                r.mpc.set_kinematics_options(selector)
            r.set_tree(tc.tree(), adjoint=True)
            r.set_tunables(configs=ag.configs_of(cfg, tc.gains(L.MPCConfig, hz)[idx]))
            r.reset(st[idx], pa[idx])
        except Exception:
            r.close()
            raise
        return r

    for name, hz, idx, selector in (("tree_loops", tc.HORIZONS[0], list(range(tc.B)), None),
                                    ("tree_selected", tc.HORIZONS[0], [tc.SELECTED[0]], tc.SELECTED[1]),
                                    ("tree_tuned", tc.HORIZONS[1], list(tc.TUNED_LOOPS), None)):
        lb, sb = tc.loss_weights()
        for k, v in _swept(lambda: tree_rollout(hz, idx, selector), tc.TICKS, lb[:, idx], sb[idx]).items():
            out[f"{name}_{'_'.join(map(str, hz))}/{k}"] = v
        print(f"tree plant, loops {idx} at {hz}{'' if selector is None else ' under ' + str(selector)}: {tc.TICKS} ticks", flush=True)

    cfg = L.paper_config()
    for workload in ("hover", "takeoff", "montecarlo"):
        st, pa = ro.make_plant(cfg, 6, workload=workload)
        pos, vel, alpha, adt = ro.make_trajectory(cfg, "takeoff" if workload == "takeoff" else "hover", 60.0)
        r = ro.ClosedLoopRollout(cfg, 6, pos, vel, alpha, adt, device=0)
        try:
            r.reset(st, pa)
            out[f"{workload}_30/run/log"], out[f"{workload}_30/run/state"] = r.run(30), r.state()
            out[f"{workload}_30/run/next_records"] = r.next_records()
        finally:
            r.close()
        print(f"{workload}: batch 6, 30 ticks", flush=True)

    tree = _mod("robot_tree").default_tree()
    st, pa = ro.make_plant_tree(cfg, 6, tree, workload="montecarlo")
    pos, vel, alpha, adt = ro.make_trajectory(cfg, "hover", 20.0)
    r = ro.ClosedLoopRollout(cfg, 6, pos, vel, alpha, adt, device=0)
    try:
        r.set_tree(tree)
        r.reset(st, pa)
        out["tree_6/run/log"], out["tree_6/run/state"], out["tree_6/run/next_records"] = r.run(6), r.state(), r.next_records()
    finally:
        r.close()
    gold = np.load(os.path.join(ROOT, "tests", "golden", "jet_lstm.npz"))
    jm = _mod("jet_plant").JetModelTotal(gold["w_ih"], gold["w_hh"], gold["b_ih"], gold["b_hh"], gold["fc_w"], gold["fc_b"],
                                         gold["norm"], device=0, max_series=64)
    st, pa = ro.make_plant(cfg, 8, workload="montecarlo")
    pos, vel, alpha, adt = ro.make_trajectory(cfg, "hover", 60.0)
    r = ro.ClosedLoopRollout(cfg, 8, pos, vel, alpha, adt, device=0)
    try:
        r.set_jet_plant(jm)
        r.reset(st, pa)
        out["jet_6/run/log"], out["jet_6/run/state"], out["jet_6/run/next_records"] = r.run(6), r.state(), r.next_records()
    finally:
        r.close()
    print("tree plant and jet plant: 6 ticks each", flush=True)
    np.savez_compressed(path, **out)
    solved = sum(int((v[:, :, 14] == L.STATUS_SOLVED).sum()) for k, v in out.items() if k.endswith("/log"))
    # (the tree plant's loop that is never Solved carries NaN thrust references: NaN where the final state's cotangent meets them)
    grads = {k: np.delete(v, tc.UNSOLVED, axis=0) if k.startswith("tree_loops_") else v
             for k, v in out.items() if "/backward/grad" in k or "/backward_full/grad" in k}
    print(f"{len(out)} arrays; {solved} solved ticks in the logs; {len(grads)} gradient arrays, finite: "
          f"{all(np.isfinite(v).all() for v in grads.values())}")
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    d = sub.add_parser("dump")
    d.add_argument("out")
    d.add_argument("--tree", default=ROOT)
    c = sub.add_parser("compare")
    c.add_argument("a")
    c.add_argument("b")
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    if args.cmd == "compare":
        from runtime_identity import compare
        return compare(args.a, args.b)
    for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), os.path.abspath(args.tree)):
        sys.path.insert(0, p)
    return dump(args.out)


if __name__ == "__main__":
    sys.exit(main())
