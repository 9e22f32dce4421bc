"""The box QP (P4b) of a paper-horizon launch in four parts, from a measurement build of the diagnostic kernel:

    VSMPC_HIPCC_FLAGS=-DVS_DIAG_QP python -c "import __graft_entry__ as g; g.build()"
    python tools/qp_tail.py [workload [batch]]          (default: hover 256, the headline launch)

Wavefront 0's cycles inside box_qp, dual form: set-up up to the second barrier (what is left of it in box_qp), columns of
P (up front and on demand), the K x K system solves, and the updates with their checks; per active-set iteration count,
next to the stamped P4b and P4a of the same instances and the launch's P4b maximum."""
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.getcwd())
PKG = "paper_gorbani_2025_humanoids_multi-rate-mpc-ironcub_amd"
pkg = importlib.import_module(PKG)
synth = importlib.import_module(PKG + ".synth")
solver = importlib.import_module(PKG + ".solver")
workload = sys.argv[1] if len(sys.argv) > 1 else "hover"
batch = int(sys.argv[2]) if len(sys.argv) > 2 else 256
cfg = pkg.paper_config()
X = synth.make_batch(cfg, batch, workload=workload, first_index=0)
m = solver.BatchedVSMPC(cfg, device=0, max_batch=batch)
m.phase_cycles(X)                                   # first launch: code object load
st = m.phase_cycles(X).astype(np.int64)
x, fm, status, iters = m.solve(X)
d = np.diff(st[:, :10], axis=1)
p4a, p4b, tot = d[:, 4], d[:, 5], st[:, 9] - st[:, 0]
parts = st[:, 10:14]
print(f"== {workload} batch {batch}, kernel {m.kernel_name}: total median {int(np.median(tot))} max {tot.max()} cycles; "
      f"P4a median {int(np.median(p4a))}; P4b median {int(np.median(p4b))} max {p4b.max()} (instance {int(p4b.argmax())}, "
      f"{iters[p4b.argmax()]} iterations)")
print("   iters count |  P4b med   max |  set-up  columns   solves  update+check (medians) | of the slowest instance")
for it in sorted(set(iters)):
    sel = np.flatnonzero(iters == it)
    w = sel[p4b[sel].argmax()]
    med = [int(np.median(parts[sel, i])) for i in range(4)]
    print(f"   {it:5d} {len(sel):5d} | {int(np.median(p4b[sel])):8d} {p4b[sel].max():5d} | {med[0]:7d} {med[1]:8d} {med[2]:8d} {med[3]:8d}"
          f"                  | {parts[w].tolist()} of {p4b[w]}")
qp = iters > 1
if qp.any():
    per_it = parts[qp, 1:].sum(axis=1) / (iters[qp] - 1)
    print(f"   per iteration behind the first (columns + solve + update, {int(qp.sum())} instances): median {int(np.median(per_it))} cycles")
m.close()
