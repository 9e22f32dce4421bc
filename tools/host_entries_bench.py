"""Wall time per call of the host-pointer entries, host code included: vsmpc_solve_batch on a tuned and on a runtime handle
(batch 1 and 8: the zero-copy path, microseconds of host code around one launch; batch 256: the pipelined path) and the three
chunked entries vsmpc_sensitivity_batch, vsmpc_adjoint_batch and vsmpc_adjoint_record_batch (batch 64: one chunk; 300: two).

    python tools/host_entries_bench.py [--rounds 7]

Paper horizon, hover records, pageable numpy buffers whose pointers are taken once, every output wanted.  Each case is timed
over `rounds` windows of back-to-back calls after a warm-up window; the line is the median window and the min..max spread, in
microseconds per call.  To compare two builds run it from each tree, alternating, in one session."""
from __future__ import annotations

import argparse
import ctypes
import importlib
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "paper_gorbani_2025_humanoids_multi-rate-mpc-ironcub_amd"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=7)
    rounds = ap.parse_args().rounds
    sys.path.insert(0, ROOT)
    import torch  # noqa: F401  (first: the library binds to the HIP runtime torch brings along)
    L, synth, solver = (importlib.import_module(f"{PKG}.{m}") for m in ("layout", "synth", "solver"))
    lib = importlib.import_module(f"{PKG}._lib").load()
    cfg = L.paper_config()
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)                     # noqa: E731
    f64, i32 = (lambda *s: np.empty(s)), (lambda *s: np.empty(s, dtype=np.int32))  # noqa: E731

    def timed(name, B, calls, call, status):
        for _ in range(calls):
            assert call() == 0, name
        assert (status == L.STATUS_SOLVED).all(), name
        us = []
        for _ in range(rounds):
            t = time.perf_counter()
            for _ in range(calls):
                call()
            us.append((time.perf_counter() - t) / calls * 1e6)
        print(f"{name:28s} batch {B:4d}  {statistics.median(us):10.2f} us/call  ({min(us):.2f} .. {max(us):.2f}, "
              f"{calls} calls x {rounds})", flush=True)

    for runtime in ("never", "always"):
        m = solver.BatchedVSMPC(cfg, device=0, max_batch=256, runtime=runtime)
        for B, calls in ((1, 2000), (8, 2000), (256, 50)) if runtime == "never" else ((1, 500), (8, 500), (256, 20)):
            rec, x, fm, st, it = synth.make_batch(cfg, B, workload="hover"), f64(B, m.n_var), f64(B, 24), i32(B), i32(B)
            a = (m._h, P(rec), B, P(x), P(fm), P(st), P(it), None)
            timed(f"solve_batch ({m.kernel_name})", B, calls, lambda: lib.vsmpc_solve_batch(*a), st)
        m.close()
    m = solver.BatchedVSMPC(cfg, device=0, max_batch=300, sensitivity=True, adjoint_record=True)
    for B in (64, 300):
        rec, x, fm, st, it = synth.make_batch(cfg, B, workload="hover"), f64(B, m.n_var), f64(B, 24), i32(B), i32(B)
        act, fl = i32(B, m.n_v), i32(B)
        dx, dfm = f64(B, m.n_var, 26), f64(B, 24, 26)
        s = (m._h, P(rec), B, P(x), P(fm), P(st), P(it), P(dx), P(dfm), P(act), P(fl), None)
        timed("sensitivity_batch", B, 10, lambda: lib.vsmpc_sensitivity_batch(*s), st)
        xbar, fmbar = np.ones((B, m.n_var)), np.ones((B, 24))
        gx0, gcfg, gin, gmodel = f64(B, 26), f64(B, L.GRAD_SIZE), f64(B, m.n_in), f64(B, L.GRAD_MODEL_SIZE)
        a = (m._h, P(rec), None, P(xbar), P(fmbar), B, P(x), P(fm), P(st), P(it), P(gx0), P(gcfg), P(act), P(fl))
        timed("adjoint_batch", B, 10, lambda: lib.vsmpc_adjoint_batch(*a, None), st)
        timed("adjoint_record_batch", B, 10, lambda: lib.vsmpc_adjoint_record_batch(*a, P(gin), P(gmodel), None), st)
    m.close()


if __name__ == "__main__":
    main()
