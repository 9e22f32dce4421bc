"""Bit identity of the runtime-sized entries between two builds: dump every entry's outputs from each build, then compare.

    python tools/runtime_identity.py dump OUT.npz         # on a GPU, with the build under test
    python tools/runtime_identity.py compare A.npz B.npz  # anywhere; exit status 1 unless everything is equal

dump runs, per shape, on the library of the tree it is started from: solve on a runtime="always" handle, solve(configs=...)
with rows that differ per instance, solve_sensitivity(jacobian=True), solve_adjoint and solve_adjoint_record without and with
the rows, certify of the solve's primals, and linearize.  The records and the configuration rows are stored beside the
outputs, so that compare can tell that both dumps answered the same questions.

Shapes (nIter, nIterSmall, controlHorizon), the smallest that reach every loop bound: (2,2,2) one throttle block, so that a
held tick has an empty free set and every substitution runs with n = 0; (6,2,3); (12,12,12); (20,5,9); the paper's (17,7,12),
which also gets records of tests/boxqp_cases.py; (40,2,40), the largest, solved one instance per launch.
Records: hover and take-off of synth.make_batch, the saturated free-tick records of tests/config_cases.py (both
directions), held ticks, a NaN in X0, an infinite inertia entry and a NaN mass (Numerical), and a free-tick hover record whose row
of the `configs` batch puts throttleMax on its largest free throttle (tests/test_gpu_sensitivity.py's construction of a
degenerate instance).  dump counts the classes a comparison has to contain and fails if one is empty.

compare prints one line per shape and entry: np.array_equal (NaN == NaN) over every array.  One exception: an instance
whose status is Numerical in both dumps has no defined states -- nothing wrote z, the states of x and first_move are
formed from what LDS held -- so those two arrays may differ there, and only there; its status, iterations, the z part of
x and every other array must still be equal."""
from __future__ import annotations

import argparse
import dataclasses
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "paper_gorbani_2025_humanoids_multi-rate-mpc-ironcub_amd"
SHAPES = [(2, 2, 2), (6, 2, 3), (12, 12, 12), (20, 5, 9), (17, 7, 12), (40, 2, 40)]
ONE_PER_LAUNCH = {(40, 2, 40)}
BOXQP = [("one", 0), ("two", 0), ("two", 3), ("three_four", 0), ("three_four", 3), ("five_sixteen", 0), ("five_sixteen", 6),
         ("above_sixteen", 0), ("above_sixteen", 3)]                    # (class, row) of boxqp_cases.DEFAULT
CLASSES = ("Solved in 1 iteration", "Solved in 3 or more iterations", "held tick with an empty free set at (2,2,2)",
           "non-finite record ending Numerical", "instance carrying the degenerate flag",
           "batch with per-instance configs that differ")
PROBE = 0                                                               # the record that is made degenerate: first of the batch


def _mod(name):
    return importlib.import_module(f"{PKG}.{name}")


def records(shape):
    """(MPCConfig, records) of a shape; record PROBE is a free-tick hover record"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import boxqp_cases
    import config_cases as cc
    L, synth = _mod("layout"), _mod("synth")
    cfg = L.MPCConfig(n_iter=shape[0], n_iter_small=shape[1], control_horizon=shape[2])
    probe = synth.make_batch(cfg, 1, workload="hover", first_index=5)
    probe[:, L.IN_HOLD] = 0.0
    hover = synth.make_batch(cfg, 2, workload="hover", first_index=6)
    takeoff = synth.make_batch(cfg, 2, workload="takeoff", first_index=5)
    held = np.concatenate([hover[:1], takeoff[:1]])
    held[:, L.IN_HOLD] = 1.0
    nan_x0, inf_inertia, nan_mass = hover[:1].copy(), takeoff[:1].copy(), hover[1:2].copy()
    nan_x0[0, L.IN_X0 + 4] = np.nan
    inf_inertia[0, L.IN_INERTIA] = np.inf
    nan_mass[0, L.IN_MASS] = np.nan
    recs = [probe, hover, takeoff, cc.saturated(cfg), held, nan_x0, inf_inertia, nan_mass]
    if shape == cc.PAPER:
        for name, row in BOXQP:
            workload, index, hold, _ = boxqp_cases.DEFAULT[name][row]
            rec = synth.make_batch(cfg, 1, workload=workload, first_index=index)
            rec[:, L.IN_HOLD] = float(hold)
            recs.append(rec)
    return cfg, np.ascontiguousarray(np.concatenate(recs))


def instance_configs(cfg, B, probe_v):
    """one MPCConfig per instance: weights and throttle box varied by instance; the probe's throttleMax on its largest
    free throttle `probe_v` (warped; None: the probe was not solved), so that the box changes nothing there and the
    instance is degenerate"""
    JetModel = _mod("jet_model").JetModel
    out = []
    for b in range(B):
        out.append(dataclasses.replace(cfg, w_throttle=cfg.w_throttle * (1.0 + 0.25 * (b % 3)),
                                       w_reg_joint_pos=cfg.w_reg_joint_pos + 0.5 * (b % 2),
                                       throttle_min=cfg.throttle_min + 2.0 * (b % 4), throttle_max=cfg.throttle_max - 1.5 * (b % 5)))
    cap = float(JetModel().destandardizeThrottle_u2T(probe_v)) if probe_v is not None else cfg.throttle_max
    if cfg.throttle_min < cap < cfg.throttle_max:
        out[PROBE] = dataclasses.replace(cfg, throttle_max=cap)
    return out


def _per_launch(fn, B, one):
    """fn(slice) over the whole batch, or one instance per launch; dicts / tuples of arrays are concatenated"""
    if not one:
        return fn(slice(0, B))
    parts = [fn(slice(b, b + 1)) for b in range(B)]
    if isinstance(parts[0], dict):
        return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(len(parts[0])))


def dump(path):
    L, solver = _mod("layout"), _mod("solver")
    out, count = {}, dict.fromkeys(CLASSES, 0)
    for shape in SHAPES:
        tag = "_".join(str(v) for v in shape)
        cfg, recs = records(shape)
        B, one = len(recs), shape in ONE_PER_LAUNCH
        rng = np.random.default_rng(17)
        xbar, fmbar = rng.standard_normal((B, cfg.n_var)), rng.standard_normal((B, L.FM_SIZE))
        m = solver.BatchedVSMPC(cfg, device=0, max_batch=1 if one else B, runtime="always", sensitivity=True, tunables=True,
                                certify=True, adjoint_record=True)
        try:
            assert m.uses_runtime_kernel
            x, fm, st, it = _per_launch(lambda s: m.solve(recs[s]), B, one)
            v = x[PROBE, cfg.off_throttle:cfg.off_throttle + m.n_v]
            rows = solver.pack_tunables(m, instance_configs(cfg, B, float(v.max()) if st[PROBE] == L.STATUS_SOLVED else None))
            ent = {"solve": dict(x=x, first_move=fm, status=st, iters=it)}
            ent["solve_configs"] = dict(zip(("x", "first_move", "status", "iters"),
                                            _per_launch(lambda s: m.solve(recs[s], tunables=rows[s]), B, one)))
            ent["solve_sensitivity"] = _per_launch(lambda s: m.solve_sensitivity(recs[s], jacobian=True), B, one)
            ent["solve_adjoint"] = _per_launch(lambda s: m.solve_adjoint(recs[s], xbar[s], fmbar[s]), B, one)
            ent["solve_adjoint_configs"] = _per_launch(lambda s: m.solve_adjoint(recs[s], xbar[s], fmbar[s], tunables=rows[s]),
                                                       B, one)
            ent["solve_adjoint_record"] = _per_launch(lambda s: m.solve_adjoint_record(recs[s], xbar[s], fmbar[s]), B, one)
            ent["solve_adjoint_record_configs"] = _per_launch(
                lambda s: m.solve_adjoint_record(recs[s], xbar[s], fmbar[s], tunables=rows[s]), B, one)
            xc = np.where((st == L.STATUS_NUMERICAL)[:, None], 0.0, x)  # (certify judges any x: no LDS residue in its input)
            ent["certify"] = dict(zip(("y", "cert"), _per_launch(lambda s: m.certify(recs[s], xc[s]), B, one)))
            ent["linearize"] = dict(zip(("A", "Bj", "Bt", "c"), _per_launch(lambda s: m.linearize(recs[s])[:4], B, one)),
                                    dt=m.linearize(recs[:1])[4])
        finally:
            m.close()
        out[f"{tag}/records"], out[f"{tag}/tunables"] = recs, rows
        for e, arrays in ent.items():
            for k, a in arrays.items():
                out[f"{tag}/{e}/{k}"] = a
        solved = st == L.STATUS_SOLVED
        count[CLASSES[0]] += int((solved & (it == 1)).sum())
        count[CLASSES[1]] += int((solved & (it >= 3)).sum())
        if shape == (2, 2, 2):
            count[CLASSES[2]] += int((solved & (recs[:, L.IN_HOLD] != 0.0)).sum())
        count[CLASSES[3]] += int((~np.isfinite(recs).all(axis=1) & (st == L.STATUS_NUMERICAL)).sum())
        count[CLASSES[4]] += sum(int((ent[e]["flags"] & L.SENS_DEGENERATE != 0).sum())
                                 for e in ("solve_sensitivity", "solve_adjoint", "solve_adjoint_configs", "solve_adjoint_record",
                                           "solve_adjoint_record_configs"))
        count[CLASSES[5]] += int(len(np.unique(rows, axis=0)) > 1)
        print(f"{tag}: {B} instances, status {np.bincount(st, minlength=4)[1:]}, iterations up to {it.max()}", flush=True)
    np.savez_compressed(path, **out)
    print("dump contains: " + "; ".join(f"{k}: {n}" for k, n in count.items()))
    empty = [k for k, n in count.items() if n == 0]
    print("rich enough: " + ("yes" if not empty else "NO, empty: " + ", ".join(empty)))
    return 1 if empty else 0


def compare(pa, pb):
    NUMERICAL = 3                                                       # VSMPC_STATUS_NUMERICAL
    a, b = np.load(pa), np.load(pb)
    if sorted(a.files) != sorted(b.files):
        print("the dumps hold different arrays: " + " ".join(sorted(set(a.files) ^ set(b.files))))
        return 1
    bad = 0
    groups = {}
    for key in a.files:
        tag, _, rest = key.partition("/")
        entry, _, name = rest.rpartition("/")
        groups.setdefault((tag, entry), []).append(name)
    for (tag, entry), names in sorted(groups.items()):
        if not entry:                                                   # the inputs
            same = all(np.array_equal(a[f"{tag}/{n}"], b[f"{tag}/{n}"], equal_nan=True) for n in names)
            print(f"{tag:>10s} {'inputs':28s} {' '.join(sorted(names))}: {'equal' if same else 'DIFFERENT'}")
            bad += not same
            continue
        get = lambda d, n: d[f"{tag}/{entry}/{n}"]                      # noqa: E731
        excepted, wrong = set(), []
        for n in sorted(names):
            u, w = get(a, n), get(b, n)
            if u.shape != w.shape:
                wrong.append(n)
                continue
            if np.array_equal(u, w, equal_nan=True):
                continue
            diff = [i for i in range(len(u)) if not np.array_equal(u[i], w[i], equal_nan=True)] if u.ndim and n != "dt" else [-1]
            for i in diff:
                residue = (n in ("x", "first_move") and "status" in names and i >= 0
                           and get(a, "status")[i] == NUMERICAL and get(b, "status")[i] == NUMERICAL)
                if residue and n == "x":                                # the z part (behind the states) must still be equal
                    nz = u.shape[1] - 26 * (int(tag.split("_")[0]) + 1)
                    residue = np.array_equal(u[i, -nz:], w[i, -nz:], equal_nan=True)
                if residue:
                    excepted.add(i)
                elif n not in wrong:
                    wrong.append(n)
        count = len(get(a, sorted(names)[0])) if entry != "linearize" else len(get(a, "A"))
        text = f"{tag:>10s} {entry:28s} {count:2d} instances  {' '.join(sorted(names))}: "
        if wrong:
            text += "DIFFERENT in " + " ".join(wrong)
        else:
            text += "array_equal"
            if excepted:
                text += (f", but for the states of x and first_move of instance {sorted(excepted)} (Numerical in both: formed "
                         "from z, which no phase has written)")
        print(text)
        bad += bool(wrong)
    print("ALL EQUAL WHERE DEFINED" if not bad else f"{bad} entries DIFFER")
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    sub.add_parser("dump").add_argument("out")
    c = sub.add_parser("compare")
    c.add_argument("a")
    c.add_argument("b")
    args = ap.parse_args()
    if args.cmd == "compare":
        return compare(args.a, args.b)
    sys.path.insert(0, ROOT)
    return dump(args.out)


if __name__ == "__main__":
    sys.exit(main())
