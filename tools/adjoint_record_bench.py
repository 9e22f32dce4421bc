"""Device time per launch of the record-adjoint entry (vsmpc_adjoint_record_batch_device) against the adjoint entry
(vsmpc_adjoint_batch_device) and the runtime-sized solve (vsmpc_solve_batch_device on a runtime handle of the same build), on
the same device-resident records.

    python tools/adjoint_record_bench.py [--out profiles/adjoint_record_bench.txt] [--rounds 9] [--launches N]

Workloads: batch 256 hover and batch 4096 take-off at the paper horizon (17, 7, 12).  HIP events (vsmpc_timing_begin /
vsmpc_timing_end) around `launches` back-to-back launches on one stream; the entries ALTERNATE, `rounds` windows each after
warm-up windows of all, and the report is the median and the min..max spread of each entry and the ratios of the medians --
all in one process, one box.  solve_kernel_rt and adjoint_kernel_rt[_tuned] of this build are instruction for instruction
the parent's (profiles/adjoint_record_isa_identity.txt), so their windows are the parent's figures.  The record entry is
timed with both outputs (grad_in and grad_model), with grad_in alone, and with per-instance rows
(adjoint_record_kernel_rt_tuned)."""
from __future__ import annotations

import argparse
import importlib
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "paper_gorbani_2025_humanoids_multi-rate-mpc-ironcub_amd"
CASES = [("hover", 256, 400), ("takeoff", 4096, 40)]           # workload, batch, launches per window


def run_case(workload, batch, launches, rounds):
    import torch
    layout = importlib.import_module(PKG + ".layout")
    synth = importlib.import_module(PKG + ".synth")
    solver = importlib.import_module(PKG + ".solver")
    cfg = layout.paper_config()
    recs = synth.make_batch(cfg, batch, workload=workload)
    m = solver.BatchedVSMPC(cfg, device=0, max_batch=batch, runtime="always", adjoint_record=True)
    dev = torch.device("cuda:0")
    f64, i32 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.int32, device=dev)
    rng = np.random.default_rng(0)
    d_in = torch.from_numpy(recs).to(dev)
    d_xbar = torch.from_numpy(rng.standard_normal((batch, m.n_var))).to(dev)
    d_fmbar = torch.from_numpy(rng.standard_normal((batch, 24))).to(dev)
    d_tun = torch.from_numpy(solver.pack_tunables(m, [cfg] * batch)).to(dev)
    d_x, d_fm = torch.empty((batch, m.n_var), **f64), torch.empty((batch, 24), **f64)
    d_st, d_it = torch.empty(batch, **i32), torch.empty(batch, **i32)
    d_g0, d_gc = torch.empty((batch, 26), **f64), torch.empty((batch, layout.GRAD_SIZE), **f64)
    d_gin, d_gm = torch.empty((batch, m.n_in), **f64), torch.empty((batch, layout.GRAD_MODEL_SIZE), **f64)
    d_act, d_fl = torch.empty((batch, m.n_v), **i32), torch.empty(batch, **i32)
    s = torch.cuda.current_stream(dev)
    head = (d_xbar, d_fmbar, d_x, d_fm, d_st, d_it, d_g0, d_gc, d_act, d_fl)
    fns = {
        "solve": lambda: m.solve_device(d_in, d_x, d_fm, d_st, d_it, stream=s),
        "adjoint": lambda: m.solve_adjoint_device(d_in, None, *head, stream=s),
        "record": lambda: m.solve_adjoint_record_device(d_in, None, *head, d_gin, d_gm, stream=s),
        "record_in": lambda: m.solve_adjoint_record_device(d_in, None, *head, d_gin, None, stream=s),
        "record_rows": lambda: m.solve_adjoint_record_device(d_in, d_tun, *head, d_gin, d_gm, stream=s),
    }

    def window(fn):
        m.timing_begin(s)
        for _ in range(launches):
            fn()
        return m.timing_end(s, launches) * 1e3                   # us per launch

    for _ in range(2):                                           # warm-up windows of all
        for fn in fns.values():
            window(fn)
    torch.cuda.synchronize()
    solved = int((d_st.cpu().numpy() == layout.STATUS_SOLVED).sum())
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            t[k].append(window(fn))
    med = {k: statistics.median(v) for k, v in t.items()}
    lines = [f"paper {workload} batch {batch}, runtime handle ({m.kernel_name}), {rounds} alternating windows of {launches} "
             f"launches; {solved} of {batch} Solved"]
    for k in fns:
        lines.append(f"  {k:12s}  median {med[k]:10.3f} us/launch  ({med[k] / batch:.4f} us/instance)  min {min(t[k]):10.3f}  "
                     f"max {max(t[k]):10.3f}  spread {100.0 * (max(t[k]) - min(t[k])) / med[k]:.2f} %")
    for k, base in (("adjoint", "solve"), ("record", "solve"), ("record", "adjoint"), ("record_in", "adjoint"),
                    ("record_rows", "adjoint")):
        ratios = [a / b for a, b in zip(t[k], t[base])]
        lines.append(f"  {k} / {base} (medians) {med[k] / med[base]:.4f}   per round min {min(ratios):.4f} max {max(ratios):.4f}")
    m.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--launches", type=int, default=0, help="launches per window of every entry (default: per case)")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    lines = [f"python tools/adjoint_record_bench.py --rounds {a.rounds}" + (f" --launches {a.launches}" if a.launches else "")
             + f" on {torch.cuda.get_device_name(0)}"]
    for workload, batch, n in CASES:
        lines += run_case(workload, batch, a.launches or n, a.rounds)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
