"""Solves/s and microseconds per launch of the runtime-sized solve kernel (vsmpc_create_ex), against the tuned kernel
where the horizon has one.

    python tools/runtime_horizon_bench.py [--out profiles/runtime_horizon_bench.json] [--step-timeout 240]

Every case runs in a child process of its own under a time limit (--step-timeout seconds); a case that fails or runs
over ends the sweep there.  Records: hover and take-off instances alternating (synth.make_batch), device-resident,
vsmpc_solve_batch_device on one stream, device time from the handle's HIP events (vsmpc_timing_*).
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "paper_gorbani_2025_humanoids_multi-rate-mpc-ironcub_amd"

# (horizon, runtime mode, batch)
CASES = [
    ((17, 7, 12), "never", 256), ((17, 7, 12), "always", 256),
    ((17, 7, 12), "never", 4096), ((17, 7, 12), "always", 4096),
    ((20, 5, 9), "fallback", 256), ((34, 14, 24), "always", 256), ((40, 2, 40), "fallback", 256),
]


def run_case(horizon, mode, batch, launches, warmup):
    sys.path.insert(0, ROOT)
    import importlib

    import numpy as np
    import torch
    layout = importlib.import_module(PKG + ".layout")
    synth = importlib.import_module(PKG + ".synth")
    solver = importlib.import_module(PKG + ".solver")
    cfg = layout.MPCConfig(n_iter=horizon[0], n_iter_small=horizon[1], control_horizon=horizon[2])
    half = batch // 2
    recs = np.concatenate([synth.make_batch(cfg, half, workload="hover"),
                           synth.make_batch(cfg, batch - half, workload="takeoff")])
    m = solver.BatchedVSMPC(cfg, device=0, max_batch=batch, runtime=mode)
    dev = torch.device("cuda:0")
    d_in = torch.from_numpy(recs).to(dev)
    d_x = torch.empty((batch, m.n_var), dtype=torch.float64, device=dev)
    d_fm = torch.empty((batch, 24), dtype=torch.float64, device=dev)
    d_st = torch.empty(batch, dtype=torch.int32, device=dev)
    d_it = torch.empty(batch, dtype=torch.int32, device=dev)
    s = torch.cuda.current_stream(dev)
    for _ in range(warmup):
        m.solve_device(d_in, d_x, d_fm, d_st, d_it, stream=s)
    torch.cuda.synchronize()
    m.timing_begin(s)
    for _ in range(launches):
        m.solve_device(d_in, d_x, d_fm, d_st, d_it, stream=s)
    ms = m.timing_end(s, launches)
    st = d_st.cpu().numpy()
    it = d_it.cpu().numpy()
    out = {"horizon": list(horizon), "mode": mode, "kernel": m.kernel_name, "batch": batch, "launches": launches,
           "us_per_launch": ms * 1e3, "solves_per_s": batch / (ms * 1e-3), "solved": int((st == 1).sum()),
           "max_iters": int(it.max()), "workspace_bytes_per_instance": (m.n_p * (m.n_p + 1) // 2) * 8
           if m.uses_runtime_kernel else 0}
    m.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--step-timeout", type=float, default=240.0)
    ap.add_argument("--case", default=None, help=argparse.SUPPRESS)   # child process: "n,ns,hc:mode:batch"
    args = ap.parse_args()
    if args.case:
        h, mode, batch = args.case.split(":")
        horizon = tuple(int(v) for v in h.split(","))
        batch = int(batch)
        launches = 20 if horizon[2] >= 30 else 50
        print(json.dumps(run_case(horizon, mode, batch, launches, warmup=3)))
        return 0
    results = []
    for horizon, mode, batch in CASES:
        case = f"{','.join(map(str, horizon))}:{mode}:{batch}"
        try:
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", case], capture_output=True,
                                 text=True, timeout=args.step_timeout)
        except subprocess.TimeoutExpired:
            print(f"{case}: over the {args.step_timeout:.0f} s limit; sweep ends here", flush=True)
            break
        if res.returncode != 0:
            print(f"{case}: exit {res.returncode}; sweep ends here\n{res.stderr[-2000:]}", flush=True)
            break
        r = json.loads(res.stdout.strip().splitlines()[-1])
        results.append(r)
        print(f"{case:>22}  {r['kernel'][:34]:34}  {r['us_per_launch']:10.1f} us/launch  {r['solves_per_s']:12.0f} solves/s"
              f"  solved {r['solved']}/{r['batch']}  max iters {r['max_iters']}", flush=True)
    ratios = {}
    for b in (256, 4096):
        t = [r for r in results if r["horizon"] == [17, 7, 12] and r["batch"] == b]
        tuned = [r for r in t if r["mode"] == "never"]
        rt = [r for r in t if r["mode"] == "always"]
        if tuned and rt:
            ratios[f"17,7,12 batch {b}: runtime / tuned time"] = rt[0]["us_per_launch"] / tuned[0]["us_per_launch"]
    for k, v in ratios.items():
        print(f"{k}: {v:.1f}x")
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"results": results, "ratios": ratios}, f, indent=1)
    return 0 if len(results) == len(CASES) else 1


if __name__ == "__main__":
    sys.exit(main())
