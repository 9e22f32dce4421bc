"""Device time per launch of the duals / certificate entry (vsmpc_certify_batch_device) against the solve entry
(vsmpc_solve_batch_device) on the same handle and the same device-resident records; the certificate is taken of the
solve's own x.

    python tools/certify_bench.py [--out profiles/certify_bench.txt] [--rounds 9] [--launches N]

Workloads: batch 256 hover and batch 4096 take-off at the paper horizon, batch 4096 take-off at the 2x horizon (tuned
handles, default condensing form).  HIP events (vsmpc_timing_begin / vsmpc_timing_end) around `launches` back-to-back
launches on one stream; the two entries ALTERNATE, `rounds` windows each after warm-up windows of both, and the report is
the median, the min..max spread of each entry and the ratio of the medians -- all in one process, one box."""
from __future__ import annotations

import argparse
import importlib
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "paper_gorbani_2025_humanoids_multi-rate-mpc-ironcub_amd"
# configuration, workload, batch, launches per window (solve, certify)
CASES = [("paper", "hover", 256, 3000, 20000), ("paper", "takeoff", 4096, 300, 3000), ("horizon2x", "takeoff", 4096, 60, 1500)]


def run_case(config, workload, batch, launches, rounds):
    import torch
    layout = importlib.import_module(PKG + ".layout")
    synth = importlib.import_module(PKG + ".synth")
    solver = importlib.import_module(PKG + ".solver")
    cfg = layout.paper_config() if config == "paper" else layout.horizon2x_config()
    recs = synth.make_batch(cfg, batch, workload=workload)       # distinct records, as tools/tunables_bench.py uses
    m = solver.BatchedVSMPC(cfg, device=0, max_batch=batch)
    dev = torch.device("cuda:0")
    f64, i32 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.int32, device=dev)
    d_in = torch.from_numpy(recs).to(dev)
    d_x, d_fm = torch.empty((batch, m.n_var), **f64), torch.empty((batch, 24), **f64)
    d_st, d_it = torch.empty(batch, **i32), torch.empty(batch, **i32)
    d_y, d_c = torch.empty((batch, m.n_con), **f64), torch.empty((batch, layout.CERT_SIZE), **f64)
    s = torch.cuda.current_stream(dev)

    def solve():
        m.solve_device(d_in, d_x, d_fm, d_st, d_it, stream=s)

    def certify():
        m.certify_device(d_in, d_x, None, d_y, d_c, stream=s)

    def window(fn, n):
        m.timing_begin(s)
        for _ in range(n):
            fn()
        return m.timing_end(s, n) * 1e3                          # us per launch

    solve()
    certify()
    torch.cuda.synchronize()
    cert = d_c.cpu().numpy()
    ok = bool(solver.certified(cert, d_x.cpu().numpy()).all())
    fns = {"solve": (solve, launches[0]), "certify": (certify, launches[1])}
    for _ in range(2):                                           # warm-up windows of both
        for fn, n in fns.values():
            window(fn, n)
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, (fn, n) in fns.items():
            t[k].append(window(fn, n))
    med = {k: statistics.median(v) for k, v in t.items()}
    lines = [f"{config} {workload} batch {batch}, {m.kernel_name} / certify_kernel, {rounds} alternating windows of "
             f"{launches[0]} / {launches[1]} launches; every instance certified at 1e-9: {ok}"]
    for k in fns:
        lines.append(f"  {k:7s}  median {med[k]:9.3f} us/launch  ({med[k] / batch:.4f} us/instance)  min {min(t[k]):9.3f}  "
                     f"max {max(t[k]):9.3f}  spread {100.0 * (max(t[k]) - min(t[k])) / med[k]:.2f} %")
    lines.append(f"  certify / solve (medians) {med['certify'] / med['solve']:.4f}")
    m.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--launches", type=int, default=0, help="launches per window of either entry (default: per case)")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    lines = [f"python tools/certify_bench.py --rounds {a.rounds}" + (f" --launches {a.launches}" if a.launches else "")
             + f" on {torch.cuda.get_device_name(0)}"]
    for config, workload, batch, n_solve, n_cert in CASES:
        lines += run_case(config, workload, batch, (a.launches or n_solve, a.launches or n_cert), a.rounds)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
