"""Records chosen by what the LATER passes of the throttle box QP's active-set loop do (plain helper module, imported by
tests).

tests/boxqp_cases.py picks records by the size of the FIRST violated set, which is what box_qp (csrc/vsmpc_p4.hpp) picks
its entry path by.  Behind the entry, every pass of dual_active_set solves one active set; at two throttle tile rows sets
of up to SMALL_PASS_MAX bounds take the straight-line pass small_set_pass<K>, larger ones the register solvers and the
update loop.  In the
synthetic workloads at the default configuration the later sets are subsets of the first (the rule releases the earliest
block of one jet per pass), so no column of P is formed behind the first pass and no free throttle meets a bound there.
The tables below list, per record, the whole sequence of active sets (throttle indices, the empty first solve left
out), picked on the CPU with the oracle's pivoting rule (test_boxqp_pass_cases.py keeps them honest):

  shrinking   default configuration: every size from 1 to 6 solved in a pass behind the second
  growing     the box 30..85 with the CoM height reference shifted by dz: a later pass ADDS a bound (a column of P on
              demand inside the loop, a free-to-bound flip inside the small-set pass); lower and upper bounds
  H21, H21_box, H34   records chosen the same way at the horizons (21, 9, 15) (two throttle tile rows, 28 throttles) and
              (34, 14, 24) (three tile rows, dense X with all of P up front: that accessor keeps the loop without the
              straight-line pass -- XDense::KPASS = 0 -- so sets of up to 10 take small_spd_solve<K> and the update loop,
              larger ones the row-per-lane solver; Monte-Carlo 39 grows from 3 to 5 bounds there)

An entry is (workload, index, dz, sequence): record `index` of synth.make_batch(cfg, ., workload), hold forced to 0, the
CoM height reference shifted by dz (as config_cases.saturated does)."""
import importlib

import numpy as np

import config_cases as cc

SMALL_PASS_MAX = 6          # csrc/vsmpc_p4.hpp (test_boxqp_pass_cases.py checks the copy against the source text)
BOX_30_85 = dict(throttle_min=30.0, throttle_max=85.0)

TABLES = {}                 # name -> (horizon, settings, entries)
TABLES["shrinking"] = ((17, 7, 12), {}, [
    ("hover", 4, 0.0, [(12, 16, 20), (16, 20), (20,)]),
    ("hover", 60, 0.0, [(9, 13, 17, 21), (13, 17, 21), (17, 21)]),
    ("hover", 222, 0.0, [(4, 8, 12, 16, 20), (8, 12, 16, 20), (12, 16, 20)]),
    ("montecarlo", 66, 0.0, [(5, 9, 13, 17, 21), (9, 13, 17, 21), (13, 17, 21), (17, 21)]),
    ("montecarlo", 4, 0.0, [(0, 4, 8, 12, 16, 20), (4, 8, 12, 16, 20), (8, 12, 16, 20)]),
])
TABLES["growing"] = ((17, 7, 12), BOX_30_85, [
    ("montecarlo", 16, 0.5, [(3,), (3, 21)]),
    ("montecarlo", 10, 1.5, [(1, 5, 9), (1,), (1, 3)]),
    ("takeoff", 23, 1.5, [(15, 19, 23), (19, 22, 23), (22, 23)]),
    ("hover", 14, 1.0, [(4, 8, 12, 16, 20), (8, 12, 16, 20), (12, 16, 20, 23)]),
])
TABLES["H21"] = ((21, 9, 15), {}, [
    ("hover", 5, 0.0, [(13, 17, 21, 25), (17, 21, 25), (21, 25)]),
    ("hover", 35, 0.0, [(13, 17, 21, 25), (17, 21, 25), (21, 25), (25,)]),
    ("hover", 4, 0.0, [(4, 8, 12, 16, 20, 24), (8, 12, 16, 20, 24), (12, 16, 20, 24)]),
    ("hover", 14, 0.0, [(8, 12, 16, 20, 24, 27), (12, 16, 20, 24, 27), (16, 20, 24, 27)]),
    ("montecarlo", 14, 0.0, [(8, 12, 16, 19, 20, 23, 24, 27), (12, 16, 20, 23, 24, 27), (16, 20, 24, 27)]),
    ("montecarlo", 17, 0.0, [(8, 12, 13, 16, 17, 20, 21, 23, 24, 25, 27), (12, 16, 17, 20, 21, 24, 25, 27), (16, 20,
        21, 24, 25, 27), (16, 20, 24, 25, 27)]),
])
TABLES["H21_box"] = ((21, 9, 15), BOX_30_85, [
    ("montecarlo", 4, -1.5, [(0, 4, 8, 12, 14, 16, 18, 20, 22, 24, 26), (0, 4, 8, 12, 16, 18, 20, 22, 24, 25, 26), (0,
        4, 8, 12, 16, 20, 22, 24, 25, 26)]),
    ("hover", 2, -0.5, [(17, 21, 25), (21, 25), (25,)]),
    ("hover", 4, -0.5, [(0, 4, 8, 12, 16, 20, 22, 24, 26), (4, 8, 12, 16, 20, 24, 26), (4, 8, 12, 16, 20, 24)]),
])
TABLES["H34"] = ((34, 14, 24), {}, [
    ("hover", 0, 0.0, [(29, 33, 37, 41), (33, 37, 41), (37, 41), (41,)]),
    ("hover", 2, 0.0, [(29, 33, 37, 41), (33, 37), (33,)]),
    ("hover", 22, 0.0, [(24, 28, 32, 36, 40), (28, 32, 36, 40), (32, 36, 40)]),
    ("hover", 11, 0.0, [(12, 16, 20, 24, 28, 32, 36, 40), (16, 20, 24, 28, 32, 36), (20, 24, 28, 32)]),
    ("hover", 8, 0.0, [(8, 12, 16, 20, 24, 28, 32, 36, 40), (12, 16, 20, 24, 28, 32, 36, 40), (16, 20, 24, 28, 32, 36,
        40)]),
    ("montecarlo", 7, 0.0, [(11, 15, 19, 23, 27, 28, 31, 32, 33, 35, 36, 37, 39, 40, 41), (15, 19, 23, 27, 31, 32, 35,
        36, 37, 40, 41), (15, 19, 23, 27, 31, 36, 40, 41), (19, 23, 27, 40, 41), (15, 19, 23, 40), (19, 23, 40)]),
    ("montecarlo", 39, 0.0, [(15, 19, 21, 22, 23, 25, 26, 27, 29, 30, 31, 33, 34, 35, 37, 38, 39, 41, 42, 43), (19,
        23, 25, 26, 27, 29, 30, 31, 33, 34, 37, 38, 41), (23, 27, 29, 30, 33, 34, 37, 41), (23, 30, 33, 37, 41), (33,
        37, 41), (30, 33, 34, 37, 41), (30, 33, 37, 41)]),
    ("takeoff", 4, 0.0, [(8, 12, 16, 20, 24, 28, 32, 36, 40), (12, 16, 20, 24, 27, 28, 32, 36, 40)]),
])


def _mod(name):
    return importlib.import_module(f"{cc.PKG}.{name}")


def record(cfg, workload, index, dz):
    L = _mod("layout")
    rec = _mod("synth").make_batch(cfg, 1, workload=workload, first_index=index)[0]
    rec[L.IN_HOLD] = 0.0
    if dz != 0.0:
        rec[L.IN_XREF + 2::12] += dz
        rec[22] = rec[2] - rec[L.IN_XREF + 2]                 # keep X0's position error consistent
    return rec


def batch(ref, table):
    """(MPCConfig, oracle Config, records) of a table, one record per entry, in order"""
    horizon, settings, rows = TABLES[table]
    cfg, rcfg = cc.configs(ref, horizon, settings)
    recs = [record(cfg, w, i, dz) for w, i, dz, _ in rows]
    return cfg, rcfg, np.ascontiguousarray(np.array(recs))


def sequence(ref, rcfg, rec):
    """The active sets of the oracle's pivoting rule (vsmpc_ref._box_qp_active_set: block principal pivoting, patience
    10, least-index fallback) on the reduced problem of vsmpc_ref.solve_exact, one tuple of (throttle index, side) per
    solve behind the first (whose set is empty): side -1 at the lower bound, +1 at the upper.  Pinned throttles are left
    out, as in the kernel's masks.  Returns (sets, final state of the throttles)."""
    H, g, Ac, lo, hi = ref.assemble_dense(rcfg, rec)
    nxs = 26 * (rcfg.n_iter + 1)
    nz = rcfg.n_var - nxs
    sol = np.linalg.solve(Ac[:nxs, :nxs], np.column_stack([lo[:nxs], Ac[:nxs, nxs:]]))
    Z = np.vstack([-sol[:, 1:], np.eye(nz)])
    xp = np.concatenate([sol[:, 0], np.zeros(nz)])
    Hr = Z.T @ H @ Z
    Hr = 0.5 * (Hr + Hr.T)
    gr = Z.T @ (H @ xp + g)
    o, nthr = 8 * rcfg.control_horizon, 4 * rcfg.n_vblocks
    zlo, zhi = np.full(nz, -np.inf), np.full(nz, np.inf)
    zlo[o:o + nthr], zhi[o:o + nthr] = lo[nxs:nxs + nthr], hi[nxs:nxs + nthr]
    fixed = zlo == zhi
    state = np.zeros(nz, dtype=int)
    state[fixed] = -1
    z = np.zeros(nz)
    best, patience, sets = nz + 1, 10, []
    for it in range(500):
        F = state == 0
        if it > 0:
            sets.append(tuple((int(i) - o, int(state[i])) for i in np.flatnonzero(~F & ~fixed)))
        z[state == -1], z[state == 1] = zlo[state == -1], zhi[state == 1]
        z[F] = np.linalg.solve(Hr[np.ix_(F, F)], -(gr[F] + Hr[np.ix_(F, ~F)] @ z[~F]))
        grad = Hr @ z + gr
        tol = 1e-12 * (1.0 + np.abs(z))
        gtol = 1e-10 * (1.0 + np.abs(gr).max())
        vlo, vhi = F & (z < zlo - tol), F & (z > zhi + tol)
        rel = (state != 0) & ~fixed & np.where(state == -1, grad < -gtol, grad > gtol)
        inf = vlo | vhi | rel
        ninf = int(inf.sum())
        if ninf == 0:
            return sets, state[o:o + nthr].copy()
        pick = inf
        if ninf < best:
            best, patience = ninf, 10
        elif patience > 0:
            patience -= 1
        else:
            pick = np.zeros(nz, dtype=bool)
            pick[np.flatnonzero(inf).max()] = True
        state[pick & vlo], state[pick & vhi], state[pick & rel] = -1, 1, 0
    raise RuntimeError("no termination")


def indices(sets):
    """the sets as tuples of throttle indices"""
    return [tuple(i for i, _ in s) for s in sets]
