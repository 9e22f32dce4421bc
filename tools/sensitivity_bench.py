"""Device time per launch of the sensitivity entry (vsmpc_sensitivity_batch_device, sens_kernel_rt) against the solve of
the same handle (vsmpc_solve_batch_device: the tuned kernel on a tuned handle, solve_kernel_rt on a runtime-only one).

    python tools/sensitivity_bench.py [--out profiles/sensitivity_bench.json] [--step-timeout 300]

Every case runs in a child process of its own under a time limit; a case that fails or runs over ends the sweep there.
Records: hover and take-off instances alternating (synth.make_batch), device-resident, one stream; HIP events around
`launches` back-to-back launches of each entry, after warm-up launches of both.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "paper_gorbani_2025_humanoids_multi-rate-mpc-ironcub_amd"

# (horizon, runtime mode of the handle, batch): the paper horizon at 256 and 4096 and the 2x horizon at 4096 on tuned
# handles, the paper horizon on a runtime-only handle (sens_kernel_rt against solve_kernel_rt, the same body)
CASES = [((17, 7, 12), "never", 256), ((17, 7, 12), "never", 4096), ((34, 14, 24), "never", 4096),
         ((17, 7, 12), "always", 256), ((17, 7, 12), "always", 4096)]


def run_case(horizon, mode, batch, launches, warmup):
    sys.path.insert(0, ROOT)
    import importlib

    import numpy as np
    import torch
    layout = importlib.import_module(PKG + ".layout")
    synth = importlib.import_module(PKG + ".synth")
    solver = importlib.import_module(PKG + ".solver")
    cfg = layout.MPCConfig(n_iter=horizon[0], n_iter_small=horizon[1], control_horizon=horizon[2])
    if horizon == (34, 14, 24):
        cfg = layout.horizon2x_config()
    half = batch // 2
    recs = np.concatenate([synth.make_batch(cfg, half, workload="hover"),
                           synth.make_batch(cfg, batch - half, workload="takeoff")])
    m = solver.BatchedVSMPC(cfg, device=0, max_batch=batch, runtime=mode, sensitivity=True)
    dev = torch.device("cuda:0")
    f64 = dict(dtype=torch.float64, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    d_in = torch.from_numpy(recs).to(dev)
    d_x, d_fm = torch.empty((batch, m.n_var), **f64), torch.empty((batch, 24), **f64)
    d_st, d_it = torch.empty(batch, **i32), torch.empty(batch, **i32)
    d_dx, d_dfm = torch.empty((batch, m.n_var, 26), **f64), torch.empty((batch, 24, 26), **f64)
    d_act, d_fl = torch.empty((batch, m.n_v), **i32), torch.empty(batch, **i32)
    s = torch.cuda.current_stream(dev)

    def solve():
        m.solve_device(d_in, d_x, d_fm, d_st, d_it, stream=s)

    def sens():
        m.solve_sensitivity_device(d_in, d_x, d_fm, d_st, d_it, d_dx, d_dfm, d_act, d_fl, stream=s)

    def timed(fn):
        for _ in range(warmup):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        for _ in range(launches):
            fn()
        e1.record(s)
        e1.synchronize()
        return e0.elapsed_time(e1) / launches * 1e3     # us per launch

    us_solve = timed(solve)
    us_sens = timed(sens)
    st, fl = d_st.cpu().numpy(), d_fl.cpu().numpy()
    out = {"horizon": list(horizon), "mode": mode, "solve_kernel": m.kernel_name, "batch": batch, "launches": launches,
           "us_solve": us_solve, "us_sensitivity": us_sens, "ratio": us_sens / us_solve,
           "solved": int((st == 1).sum()), "degenerate": int(((fl & layout.SENS_DEGENERATE) != 0).sum()),
           "workspace_bytes_per_instance": (m.n_p + 26) * (m.n_p + 27) // 2 * 8}
    m.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--step-timeout", type=float, default=300.0)
    ap.add_argument("--case", default=None, help=argparse.SUPPRESS)   # child process: "n,ns,hc:mode:batch"
    args = ap.parse_args()
    if args.case:
        h, mode, batch = args.case.split(":")
        horizon = tuple(int(v) for v in h.split(","))
        batch = int(batch)
        launches = 5 if (batch >= 4096 and (mode != "never" or horizon[2] >= 24)) else 20
        print(json.dumps(run_case(horizon, mode, batch, launches, warmup=2)))
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
        print(f"{case:>20}  solve {r['solve_kernel'][:30]:30} {r['us_solve']:11.1f} us  sens_kernel_rt {r['us_sensitivity']:11.1f} us"
              f"  x{r['ratio']:5.2f}  solved {r['solved']}/{r['batch']}  degenerate {r['degenerate']}", flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"results": results}, f, indent=1)
    return 0 if len(results) == len(CASES) else 1


if __name__ == "__main__":
    sys.exit(main())
