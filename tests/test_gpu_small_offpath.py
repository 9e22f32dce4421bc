"""The work the small-batch kind of the paper-horizon solve kernel (solve_kernel_small) does off its critical path.

The kind forms the contraction sAc = A_mom^T W beside panel stream 0, in wavefronts 1..3 at the head of their second
instalment of tiles, instead of on all threads behind a barrier of its own in front of the column-0 tiles; only the throttle x
throttle tiles (5,5), (6,5), (6,6) read it, and they are formed one stream later.  It also meets one barrier less in front of
stream 0.  No arithmetic operation and no order of operations changes, so:

  * the kind against the shipped kernel, one handle, override "never" / "always", every output array_equal -- on the
    selection of tests/boxqp_cases.py (default classes) and tests/boxqp_pass_cases.py ("shrinking": 4 and 5 active-set
    iterations), and on the "growing" table on a handle of its own (box 30..85).  Every record's Hessian has the three
    throttle x throttle tiles the moved contraction feeds;
  * BOTH kernels against the oracle on the same records at the project's 1e-8 bar with equal iteration counts, no record
    skipped: first active sets of 1, 2..4 and more than 4 bounds, with and without the hold;
  * a batch of one that enters the box QP, and a non-finite record beside a valid one (status Numerical; the neighbour bit
    for bit);
  * vsmpc_debug_phase_cycles on the kind: finite, increasing stamps.

The kernel is per instance, so the batches are one to fourteen records."""
import numpy as np
import pytest

from conftest import relerr
import boxqp_cases as bq
import boxqp_pass_cases as bp

pytestmark = pytest.mark.gpu
TOL = 1e-8

# (class in boxqp_cases.DEFAULT, workload, index, hold): no box QP, first active sets of 1, 2, 3..4, 5..16 and 17 bounds
PICKS = [("never", "hover", 0, 0), ("never", "takeoff", 2, 1), ("one", "hover", 29, 0), ("one", "hover", 170, 1),
         ("two", "hover", 17, 0), ("two", "takeoff", 19, 1), ("three_four", "hover", 4, 0), ("three_four", "hover", 19, 0),
         ("five_sixteen", "hover", 222, 0), ("five_sixteen", "takeoff", 0, 0), ("five_sixteen", "takeoff", 92, 0),
         ("above_sixteen", "takeoff", 1, 0)]
SHRINKING = [("hover", 60), ("montecarlo", 66)]      # 4 and 5 active-set iterations (hover 60 sets the batch-256 launch time)
ENTERS_QP = 6                                         # position in PICKS of a record that enters the box QP
_cache = {}


def _records(ref):
    """(cfg, rcfg, the fourteen records), built once"""
    if "records" not in _cache:
        cfg, rcfg, recs = bq.batch(ref, "default")
        rows = {(n, w, i, h): k for k, (n, w, i, h, _) in enumerate(bq.entries("default"))}
        picked = [recs[rows[p]] for p in PICKS]
        table = {(w, i): k for k, (w, i, _, _) in enumerate(bp.TABLES["shrinking"][2])}
        _, _, srecs = bp.batch(ref, "shrinking")
        picked += [srecs[table[s]] for s in SHRINKING]
        _cache["records"] = (cfg, rcfg, np.ascontiguousarray(np.array(picked)))
    return _cache["records"]


def _growing(ref):
    if "growing" not in _cache:
        cfg, rcfg, recs = bp.batch(ref, "growing")
        _cache["growing"] = (cfg, rcfg, np.ascontiguousarray(recs))
    return _cache["growing"]


def _both(solver_mod, cfg, recs):
    """(shipped, small): the records on the shipped kernel and on the small-batch kind, one handle"""
    recs = np.ascontiguousarray(recs)
    m = solver_mod.BatchedVSMPC(cfg, device=0, max_batch=len(recs))
    try:
        m.set_small_batch_kernel("never")
        assert not m.uses_small_batch_kernel(len(recs))
        shipped = m.solve(recs)
        m.set_small_batch_kernel("always")
        assert m.uses_small_batch_kernel(len(recs))
        small = m.solve(recs)
    finally:
        m.close()
    return shipped, small


def _solved(solver_mod, ref, which):
    """both kernels' outputs on the fourteen (`records`) or on the growing table (`growing`), solved once and shared"""
    key = "solved_" + which
    if key not in _cache:
        cfg, _, recs = _records(ref) if which == "records" else _growing(ref)
        _cache[key] = _both(solver_mod, cfg, recs)
    return _cache[key]


def _oracle(ref, which):
    """the oracle's (solution, iteration count, first move) per record, computed once and shared"""
    key = "oracle_" + which
    if key not in _cache:
        _, rcfg, recs = _records(ref) if which == "records" else _growing(ref)
        out = []
        for rec in recs:
            xr, _, itr, _ = ref.solve_instance(rcfg, rec)
            out.append((xr, itr, ref.first_move_vector(rcfg, xr)))
        _cache[key] = out
    return _cache[key]


def _assert_equal(shipped, small, what):
    for name, a, b in zip(("x", "first_move", "status", "iters"), shipped, small):
        np.testing.assert_array_equal(b, a, err_msg=f"{what}: {name}")


def _assert_oracle(layout, rcfg, oracle, outputs, what):
    x, fm, st, it = outputs
    assert (st == layout.STATUS_SOLVED).all(), (what, st)
    oj, ov = rcfg.off_joints, rcfg.off_throttle
    worst = {"x": 0.0, "traj": 0.0, "dq": 0.0, "v": 0.0, "fm": 0.0}
    for b, (xr, itr, fmr) in enumerate(oracle):
        assert it[b] == itr, (what, b, it[b], itr)          # the active-set path of the oracle's pivoting rule
        worst["x"] = max(worst["x"], relerr(x[b], xr))
        worst["traj"] = max(worst["traj"], relerr(x[b, :oj], xr[:oj]))
        worst["dq"] = max(worst["dq"], relerr(x[b, oj:ov], xr[oj:ov]))
        worst["v"] = max(worst["v"], relerr(x[b, ov:], xr[ov:]))
        worst["fm"] = max(worst["fm"], relerr(fm[b], fmr))
    print(f"{what}, worst against the oracle:", {k: f"{v:.2e}" for k, v in worst.items()})
    for k, v in worst.items():
        assert v < TOL, (what, k, v)


@pytest.mark.parametrize("which", ["records", "growing"])
def test_small_kind_equals_the_shipped_kernel(solver_mod, ref, layout, which):
    shipped, small = _solved(solver_mod, ref, which)
    assert (shipped[2] == layout.STATUS_SOLVED).all(), shipped[2]
    if which == "records":
        assert {1, 2, 3, 4, 5} <= set(int(i) for i in shipped[3]), shipped[3]   # no QP, and 2..5 active-set iterations
    else:
        assert (shipped[3] >= 3).all(), shipped[3]
    _assert_equal(shipped, small, which)


@pytest.mark.parametrize("kernel", ["shipped", "small"])
@pytest.mark.parametrize("which", ["records", "growing"])
def test_both_kernels_match_the_oracle(solver_mod, ref, layout, which, kernel):
    _, rcfg, recs = _records(ref) if which == "records" else _growing(ref)
    shipped, small = _solved(solver_mod, ref, which)
    oracle = _oracle(ref, which)
    assert len(oracle) == len(recs)                           # no record skipped
    _assert_oracle(layout, rcfg, oracle, shipped if kernel == "shipped" else small, f"{kernel} kernel, {which}")


def test_batch_of_one_that_enters_the_box_qp(solver_mod, ref, layout):
    cfg, _, recs = _records(ref)
    shipped, small = _both(solver_mod, cfg, recs[ENTERS_QP:ENTERS_QP + 1])
    assert shipped[2][0] == layout.STATUS_SOLVED and shipped[3][0] > 1
    _assert_equal(shipped, small, "batch of one")
    full, _ = _solved(solver_mod, ref, "records")             # ... and it is the row of the batch of fourteen
    for a, b in zip(shipped, full):
        np.testing.assert_array_equal(a[0], b[ENTERS_QP])


def test_non_finite_record_beside_a_valid_one(solver_mod, ref, layout):
    cfg, _, recs = _records(ref)
    pair = recs[[ENTERS_QP, 0]].copy()
    pair[0, layout.IN_INERTIA] = np.nan
    shipped, small = _both(solver_mod, cfg, pair)
    assert shipped[2][0] == layout.STATUS_NUMERICAL and small[2][0] == layout.STATUS_NUMERICAL, (shipped[2], small[2])
    assert shipped[2][1] == layout.STATUS_SOLVED and small[2][1] == layout.STATUS_SOLVED
    full, _ = _solved(solver_mod, ref, "records")
    for a, b, c in zip(shipped, small, full):                 # the valid neighbour: every output, and as solved without the NaN
        np.testing.assert_array_equal(b[1], a[1])
        np.testing.assert_array_equal(b[1], c[0])


def test_phase_stamps_of_the_small_kind(solver_mod, ref):
    cfg, _, recs = _records(ref)
    m = solver_mod.BatchedVSMPC(cfg, device=0, max_batch=len(recs))
    try:
        m.set_small_batch_kernel("always")
        st = m.phase_cycles(recs).astype(np.int64)
    finally:
        m.close()
    stamps = st[:, :10]                                       # VS_STAMP(0) .. VS_STAMP(9)
    assert np.isfinite(stamps.astype(np.float64)).all() and (stamps > 0).all(), stamps
    d = np.diff(stamps, axis=1)
    # stamps 2 and 3 both mark "column 0 is in the ring", and 5 and 6 coincide without a box QP; every other phase takes time
    assert (d >= 0).all() and (d[:, [0, 1, 3, 4, 6, 7]] > 0).all(), d
    total = stamps[:, 9] - stamps[:, 0]
    assert (total > 20_000).all() and (total < 2_000_000).all(), total   # a solve is tens of thousands of cycles
