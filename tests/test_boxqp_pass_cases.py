"""tests/boxqp_pass_cases.py: the oracle's pivoting rule takes every committed record through the sequence of active sets
its entry names, and the tables cover what test_gpu_boxqp_passes.py is there for -- a condition on that test's inputs,
not on the kernel."""
import os
import re

import numpy as np
import pytest

import boxqp_pass_cases as bp
import config_cases as cc

P4 = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), cc.PKG, "csrc", "vsmpc_p4.hpp")


@pytest.mark.parametrize("table", list(bp.TABLES))
def test_every_record_takes_its_sequence(ref, table):
    _, rcfg, recs = bp.batch(ref, table)
    ov, nthr = rcfg.off_throttle, 4 * rcfg.n_vblocks
    for (workload, index, dz, tabled), rec in zip(bp.TABLES[table][2], recs):
        sets, state = bp.sequence(ref, rcfg, rec)
        assert bp.indices(sets) == tabled, (table, workload, index, dz)
        # the tracer against the oracle's own loop: as many solves, and the last set is what the solution has on a bound
        x, _, iters, (_, _, _, lo, hi) = ref.solve_instance(rcfg, rec)
        assert iters == len(tabled) + 1, (table, workload, index, dz)
        nxs = 26 * (rcfg.n_iter + 1)
        v, vlo, vhi = x[ov:ov + nthr], lo[nxs:nxs + nthr], hi[nxs:nxs + nthr]
        assert tuple(np.flatnonzero((v == vlo) | (v == vhi))) == tabled[-1], (table, workload, index, dz)
        assert (np.flatnonzero(state) == np.array(tabled[-1])).all()


def _later(table):
    """the sets solved behind the first pass, with the set in front of each"""
    return [(a, b) for *_, seq in bp.TABLES[table][2] for a, b in zip(seq, seq[1:])]


def test_tables_cover_the_later_passes(ref):
    src = open(P4).read()
    assert re.search(r"SMALL_SOLVE_MAX = (\d+);", src).group(1) == str(bp.SMALL_PASS_MAX)
    assert "SMALL_PASS_MAX = SMALL_SOLVE_MAX;" in src
    ks = bp.SMALL_PASS_MAX
    # paper horizon: every size the straight-line pass has, solved behind the first pass
    assert {len(b) for _, b in _later("shrinking")} >= set(range(1, ks + 1)) - {ks} and \
        any(len(seq[0]) == ks for *_, seq in bp.TABLES["shrinking"][2])
    assert {len(seq[k]) for *_, seq in bp.TABLES["shrinking"][2] for k in range(2, len(seq))} >= {1, 2, 3, 4}
    # a bound ADDED behind the first pass: with a first set of at most four the column of P is formed on demand inside the
    # loop (box_qp forms all columns up front for more), with more the flip alone; both inside the small-set pass
    grown = [(seq[0], a, b) for *_, seq in bp.TABLES["growing"][2] for a, b in zip(seq, seq[1:]) if not set(b) <= set(a)]
    assert any(len(first) <= 4 and len(b) <= ks for first, _, b in grown)
    assert any(len(first) > 4 and len(b) <= ks for first, _, b in grown)
    # lower and upper bounds
    _, rcfg, recs = bp.batch(ref, "growing")
    assert {s for rec in recs[-2:] for st in bp.sequence(ref, rcfg, rec)[0] for _, s in st} == {-1, 1}
    assert re.search(r"struct XDense \{.*?KPASS = 0;", src, re.S) and re.search(r"struct XTiles \{.*?KPASS = SMALL_PASS_MAX;", src, re.S)
    # the other horizons: small sets (the straight-line pass at two tile rows, small_spd_solve<K> and the update loop at
    # three), and the solvers for larger sets behind the first pass as well
    for table, big in (("H21", range(ks + 1, 17)), ("H34", range(ks + 1, 11))):
        sizes = {len(b) for _, b in _later(table)}
        assert sizes & set(range(1, ks + 1)) and sizes & set(big), (table, sizes)
    assert any(len(b) > 10 for _, b in _later("H34"))                      # and the row-per-lane solver there
    assert any(len(b) <= ks and not set(b) <= set(a) for a, b in _later("H34"))
    for table, (horizon, _, rows) in bp.TABLES.items():
        assert max(len(seq[0]) for *_, seq in rows) <= cc.DUAL_FORM_MAX.get(horizon, 16), table   # dual form throughout
