"""The small-batch kind of the paper-horizon solve kernel (solve_kernel_small, vsmpc_set_small_batch_kernel) against the
shipped kernel, bit for bit.

The kind forms most Hessian tiles beside the first two panel streams of P3 instead of in front of them, from LDS arrays its
carve-up keeps apart from the ring; per tile the operations and their order are the shipped kernel's, so every output must
be array_equal.  Each comparison runs on ONE handle, solved once with the override at "never" and once at "always".  The
kernel is per instance, so the batches are tiny; what they cover is every path through P3..P6 behind the moved work:

  * a batch of one on its own;
  * fourteen records at the default configuration (tests/boxqp_cases.py, tests/boxqp_pass_cases.py "shrinking"): no box QP
    and 2, 3, 4 and 5 active-set iterations, first active sets of 1, 2, 3, 4, 5, 12, 16 and 17 bounds (dual form one column,
    columns per wavefront, all columns, register solvers, primal form), held ticks among them;
  * growing active sets (boxqp_pass_cases "growing", box 30..85: a handle of its own);
  * one all-distinct record (tests/record_cases.py) under config_cases.ALL_DISTINCT;
  * a non-finite record beside a valid one: status Numerical from both kernels (the only output defined there), the
    neighbour bit for bit;
  * the fourteen against the oracle at the project's 1e-8 bar with equal iteration counts, so that the comparison above is not
    one of two equally wrong kernels;
  * the selection rule at "auto": the small-batch kind at batch = CU count, the shipped kernel at CU count + 1, and a solve of
    CU count + 1 copies of a record gives the rows of a solve of that record alone;
  * vsmpc_debug_phase_cycles on the kind: finite, increasing stamps.

The per-instance-tunables entries keep the shipped kernel (include/vsmpc.h), so there is no tuned case here."""
import numpy as np
import pytest

import boxqp_cases as bq
import boxqp_pass_cases as bp
import config_cases as cc
import record_cases as rc
from test_gpu_config_parity import _check_solution

pytestmark = pytest.mark.gpu

# (class in boxqp_cases.DEFAULT, workload, index, hold)
PICKS = [("never", "hover", 0, 0), ("never", "takeoff", 2, 1), ("one", "hover", 29, 0), ("one", "hover", 170, 1),
         ("two", "hover", 17, 0), ("two", "takeoff", 19, 1), ("three_four", "hover", 4, 0), ("three_four", "hover", 19, 0),
         ("five_sixteen", "hover", 222, 0), ("five_sixteen", "takeoff", 0, 0), ("five_sixteen", "takeoff", 92, 0),
         ("above_sixteen", "takeoff", 1, 0)]
SHRINKING = [("hover", 60), ("montecarlo", 66)]      # boxqp_pass_cases "shrinking": 4 and 5 active-set iterations
_cache = {}


def _dozen(ref):
    """(cfg, rcfg, records): PICKS out of boxqp_cases' default table + SHRINKING out of boxqp_pass_cases', built once"""
    if "dozen" not in _cache:
        cfg, rcfg, recs = bq.batch(ref, "default")
        rows = {(n, w, i, h): k for k, (n, w, i, h, _) in enumerate(bq.entries("default"))}
        picked = [recs[rows[p]] for p in PICKS]
        table = {(w, i): k for k, (w, i, _, _) in enumerate(bp.TABLES["shrinking"][2])}
        _, _, srecs = bp.batch(ref, "shrinking")
        picked += [srecs[table[s]] for s in SHRINKING]
        _cache["dozen"] = (cfg, rcfg, np.ascontiguousarray(np.array(picked)))
    return _cache["dozen"]


def _both(m, recs):
    """the records on the shipped kernel and on the small-batch kind, one handle"""
    recs = np.ascontiguousarray(recs)
    m.set_small_batch_kernel("never")
    assert not m.uses_small_batch_kernel(len(recs))
    shipped = m.solve(recs)
    m.set_small_batch_kernel("always")
    assert m.uses_small_batch_kernel(len(recs))
    small = m.solve(recs)
    return shipped, small


def _assert_equal(shipped, small, what=""):
    for name, a, b in zip(("x", "first_move", "status", "iters"), shipped, small):
        np.testing.assert_array_equal(b, a, err_msg=f"{what} {name}")


def _solved_dozen(solver_mod, ref):
    if "solved" not in _cache:
        cfg, _, recs = _dozen(ref)
        m = solver_mod.BatchedVSMPC(cfg, device=0, max_batch=len(recs))
        try:
            _cache["solved"] = _both(m, recs)
        finally:
            m.close()
    return _cache["solved"]


def test_batch_of_one(solver_mod, ref, layout):
    cfg, _, recs = _dozen(ref)
    m = solver_mod.BatchedVSMPC(cfg, device=0, max_batch=1)
    try:
        assert m.set_small_batch_kernel("auto") == 0          # what a new handle starts with, returned as the previous setting
        shipped, small = _both(m, recs[6:7])                  # a record that enters the box QP
    finally:
        m.close()
    assert shipped[2][0] == layout.STATUS_SOLVED and shipped[3][0] > 1
    _assert_equal(shipped, small, "batch of one")


def test_every_path_behind_the_moved_work_is_bit_identical(solver_mod, ref, layout):
    shipped, small = _solved_dozen(solver_mod, ref)
    assert (shipped[2] == layout.STATUS_SOLVED).all(), shipped[2]
    assert {1, 2, 3, 4, 5} <= set(int(i) for i in shipped[3]), shipped[3]     # no QP, and 2..5 active-set iterations
    _assert_equal(shipped, small, "default configuration")


def test_growing_active_sets(solver_mod, ref, layout):
    cfg, _, recs = bp.batch(ref, "growing")
    m = solver_mod.BatchedVSMPC(cfg, device=0, max_batch=len(recs))
    try:
        shipped, small = _both(m, recs)
    finally:
        m.close()
    assert (shipped[2] == layout.STATUS_SOLVED).all() and (shipped[3] >= 3).all(), (shipped[2], shipped[3])
    _assert_equal(shipped, small, "growing sets")


def test_all_distinct_record_and_configuration(solver_mod, ref, layout):
    cfg, _ = cc.configs(ref, cc.PAPER, cc.all_distinct(cc.PAPER))
    recs = rc.distinct_records(cfg)[2:4]                      # a take-off record with the hold released, one HELD
    m = solver_mod.BatchedVSMPC(cfg, device=0, max_batch=len(recs))
    try:
        shipped, small = _both(m, recs)
    finally:
        m.close()
    assert (shipped[2] == layout.STATUS_SOLVED).all(), shipped[2]
    _assert_equal(shipped, small, "all distinct")


def test_non_finite_record(solver_mod, ref, layout):
    cfg, _, recs = _dozen(ref)
    pair = recs[[6, 0]].copy()
    pair[0, layout.IN_INERTIA] = np.nan
    m = solver_mod.BatchedVSMPC(cfg, device=0, max_batch=2)
    try:
        shipped, small = _both(m, pair)
    finally:
        m.close()
    assert shipped[2][0] == layout.STATUS_NUMERICAL and small[2][0] == layout.STATUS_NUMERICAL, (shipped[2], small[2])
    assert shipped[2][1] == layout.STATUS_SOLVED
    for a, b in zip(shipped, small):                          # the valid neighbour: every output
        np.testing.assert_array_equal(b[1], a[1])


def test_small_kind_matches_the_oracle(solver_mod, ref, layout):
    cfg, rcfg, recs = _dozen(ref)
    _, small = _solved_dozen(solver_mod, ref)
    _check_solution(ref, rcfg, layout, recs, *small)


def test_selection_rule(solver_mod, ref, layout):
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    cfg, _, recs = _dozen(ref)
    one = recs[7:8]                                           # enters the box QP (first active set of four)
    m = solver_mod.BatchedVSMPC(cfg, device=0, max_batch=cus + 1)
    try:
        assert m.set_small_batch_kernel("auto") == 0
        assert m.uses_small_batch_kernel(1) and m.uses_small_batch_kernel(cus)
        assert not m.uses_small_batch_kernel(cus + 1)
        alone = m.solve(one)                                  # the small-batch kind
        many = m.solve(np.repeat(one, cus + 1, axis=0))       # the shipped kernel
        assert m.set_kernel_form(solver_mod.KERNEL_FORM_SYRK) == 0
        assert not m.uses_small_batch_kernel(1)               # the kind is the structured form only
        m.set_kernel_form(0)
        assert m.set_small_batch_kernel("never") == 0 and not m.uses_small_batch_kernel(1)
        assert m.set_small_batch_kernel("always") == 1 and m.uses_small_batch_kernel(cus + 1)
    finally:
        m.close()
    assert alone[2][0] == layout.STATUS_SOLVED and alone[3][0] > 1
    for name, a, b in zip(("x", "first_move", "status", "iters"), alone, many):
        np.testing.assert_array_equal(b, np.repeat(a, cus + 1, axis=0), err_msg=name)
    # a horizon without the kind refuses "always" and answers the query with the shipped kernel
    m2 = solver_mod.BatchedVSMPC(layout.horizon2x_config(), device=0, max_batch=2)
    try:
        assert not m2.uses_small_batch_kernel(1)
        with pytest.raises(ValueError, match="unsupported|small-batch"):
            m2.set_small_batch_kernel("always")
        assert m2.set_small_batch_kernel("never") == 0
    finally:
        m2.close()


def test_phase_stamps_of_the_small_kind(solver_mod, ref):
    cfg, _, recs = _dozen(ref)
    m = solver_mod.BatchedVSMPC(cfg, device=0, max_batch=len(recs))
    try:
        m.set_small_batch_kernel("always")
        st = m.phase_cycles(recs).astype(np.int64)
    finally:
        m.close()
    stamps = st[:, :10]                                       # VS_STAMP(0) .. VS_STAMP(9)
    assert (stamps > 0).all(), stamps
    d = np.diff(stamps, axis=1)
    assert (d >= 0).all() and (d[:, [0, 1, 3, 4, 6, 7]] > 0).all(), d      # (stamps 2 and 3, and 5 and 6 without a box QP, may coincide)
    total = stamps[:, 9] - stamps[:, 0]
    assert (total > 20_000).all() and (total < 2_000_000).all(), total   # a solve is tens of thousands of cycles
