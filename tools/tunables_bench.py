"""Device time per launch of the per-instance-tunables entry (vsmpc_solve_batch_tuned_device) against the plain entry
(vsmpc_solve_batch_device) on the same handle and the same device-resident records.

    python tools/tunables_bench.py [--out profiles/tunables_bench.txt] [--rounds 9] [--launches N]

Workloads: batch 256 hover and batch 4096 take-off at the paper horizon (tuned handle, default condensing form).  Every
instance of the tuned entry carries the handle's own configuration, so both entries solve the same problems.  HIP events
(vsmpc_timing_begin / vsmpc_timing_end) around `launches` back-to-back launches on one stream, long enough for a window of
a tenth of a second or more; the two entries ALTERNATE, `rounds` windows each after warm-up windows of both, and the
report is the median, the min..max spread of each entry and the ratio of the medians -- all in one process, one box."""
from __future__ import annotations

import argparse
import importlib
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "paper_gorbani_2025_humanoids_multi-rate-mpc-ironcub_amd"
CASES = [("hover", 256, 4000), ("takeoff", 4096, 400)]           # workload, batch, launches per window


def run_case(workload, batch, launches, rounds):
    import torch
    layout = importlib.import_module(PKG + ".layout")
    synth = importlib.import_module(PKG + ".synth")
    solver = importlib.import_module(PKG + ".solver")
    cfg = layout.paper_config()
    recs = synth.make_batch(cfg, batch, workload=workload)
    m = solver.BatchedVSMPC(cfg, device=0, max_batch=batch)
    dev = torch.device("cuda:0")
    f64, i32 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.int32, device=dev)
    d_in = torch.from_numpy(recs).to(dev)
    d_tun = torch.from_numpy(solver.pack_tunables(m, [cfg] * batch)).to(dev)
    d_x, d_fm = torch.empty((batch, m.n_var), **f64), torch.empty((batch, 24), **f64)
    d_st, d_it = torch.empty(batch, **i32), torch.empty(batch, **i32)
    s = torch.cuda.current_stream(dev)

    def plain():
        m.solve_device(d_in, d_x, d_fm, d_st, d_it, stream=s)

    def tuned():
        m.solve_device_tuned(d_in, d_tun, d_x, d_fm, d_st, d_it, stream=s)

    def window(fn):
        m.timing_begin(s)
        for _ in range(launches):
            fn()
        return m.timing_end(s, launches) * 1e3                   # us per launch

    outs = {}
    for name, fn in (("plain", plain), ("tuned", tuned)):        # the two entries compute the same thing
        fn()
        torch.cuda.synchronize()
        outs[name] = (d_x.cpu().numpy().copy(), d_st.cpu().numpy().copy())
    same = bool((outs["plain"][0] == outs["tuned"][0]).all() and (outs["plain"][1] == outs["tuned"][1]).all())
    for _ in range(2):                                           # warm-up windows of both
        window(plain), window(tuned)
    t = {"plain": [], "tuned": []}
    for _ in range(rounds):
        t["plain"].append(window(plain))
        t["tuned"].append(window(tuned))
    med = {k: statistics.median(v) for k, v in t.items()}
    lines = [f"{workload} batch {batch}, {m.kernel_name}, {rounds} alternating windows of {launches} launches; outputs equal: {same}"]
    for k in ("plain", "tuned"):
        lines.append(f"  {k:5s}  median {med[k]:9.3f} us/launch  ({med[k] / batch:.4f} us/solve)  min {min(t[k]):9.3f}  max {max(t[k]):9.3f}  "
                     f"spread {100.0 * (max(t[k]) - min(t[k])) / med[k]:.2f} %")
    lines.append(f"  tuned / plain (medians) {med['tuned'] / med['plain']:.4f}")
    m.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--launches", type=int, default=0, help="launches per window (default: per case)")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    lines = [f"tools/tunables_bench.py on {torch.cuda.get_device_name(0)}"]
    for workload, batch, launches in CASES:
        lines += run_case(workload, batch, a.launches or launches, a.rounds)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
