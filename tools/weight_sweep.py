"""A gain study on the batch axis: ONE closed-loop rollout of 256 hover loops, each with its own
(w_throttle, w_initial_throttle) pair (ClosedLoopRollout.set_tunables), every other setting the paper's.

    python tools/weight_sweep.py [--ticks 4000] [--segments 8] [--out profiles/weight_sweep.txt]

All loops start from the same plant state (make_plant's first hover instance), so the weights are the only difference
between them.  Prints, per loop: the two weights, the altitude error at the end, and the amplitude of the lateral
momentum h_lin,y and of the differential thrusts T0 - T1 and T2 - T3 (DESIGN.md section 6 finds the hover loop's slowest
mode in lateral momentum against the arm jets' differential thrust rate) over the first and the last segment of the run,
with their ratio as the drift.  It is a tool, not a test: it claims nothing about the spectral radius of the loop beyond
the figures it prints."""
from __future__ import annotations

import argparse
import dataclasses
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "paper_gorbani_2025_humanoids_multi-rate-mpc-ironcub_amd"
GRID = 16                                                            # 16 x 16 pairs
W_THROTTLE = np.geomspace(5e3, 1.28e6, GRID)                         # paper: 8e4
W_INITIAL = np.geomspace(5e3, 1.28e6, GRID)                          # paper: 8e4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=4000)               # 20 s of flight at 200 Hz
    ap.add_argument("--segments", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    L = importlib.import_module(PKG + ".layout")
    ro = importlib.import_module(PKG + ".rollout")
    cfg = L.paper_config()
    B = GRID * GRID
    pairs = [(wt, wi) for wt in W_THROTTLE for wi in W_INITIAL]
    cfgs = [dataclasses.replace(cfg, w_throttle=float(wt), w_initial_throttle=float(wi)) for wt, wi in pairs]
    st1, pa1 = ro.make_plant(cfg, 1, workload="hover")
    st, pa = np.repeat(st1, B, axis=0), np.repeat(pa1, B, axis=0)
    pos, vel, alpha, adt = ro.make_trajectory(cfg, "hover", 60.0)
    r = ro.ClosedLoopRollout(cfg, B, pos, vel, alpha, adt, device=0)
    r.set_tunables(configs=cfgs)
    r.reset(st, pa)
    per = a.ticks // a.segments
    hy, d01, d23, solved = [], [], [], np.ones(B, dtype=bool)
    for _ in range(a.segments):
        log = r.run(per)
        solved &= (log[:, :, 14] == L.STATUS_SOLVED).all(axis=0)
        T = log[:, :, 6:10]
        d01.append(np.ptp(T[:, :, 0] - T[:, :, 1], axis=0))
        d23.append(np.ptp(T[:, :, 2] - T[:, :, 3], axis=0))
        hy.append(np.abs(r.state()[:, L.PS_HLIN + 1]))
    z_ref = pa[:, L.PP_PINIT + 2] + pos[min(a.ticks // max(1, cfg.ratio), len(pos) - 1), 2]
    z_err = log[-1, :, 2] - z_ref
    r.close()
    lines = [f"tools/weight_sweep.py: {B} hover loops in one rollout, {a.ticks} ticks in {a.segments} segments of {per}; "
             f"first / last = first and last segment",
             "w_throttle w_initial_throttle | all_solved | z_err[m] | |h_lin,y| first last ratio | ptp(T0-T1) first last ratio | "
             "ptp(T2-T3) first last ratio"]

    def trio(v, b):
        first, last = float(v[0][b]), float(v[-1][b])
        return f"{first:10.3e} {last:10.3e} {last / first if first > 0 else float('nan'):8.3f}"
    for b, (wt, wi) in enumerate(pairs):
        lines.append(f"{wt:10.4g} {wi:10.4g} | {int(solved[b])} | {z_err[b]:+.3e} | {trio(hy, b)} | {trio(d01, b)} | {trio(d23, b)}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
