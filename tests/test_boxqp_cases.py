"""tests/boxqp_cases.py: the oracle puts every committed record into the class its entry names, and every class has at
least two records -- a condition on the inputs of test_gpu_boxqp_entry_paths.py, not on the kernel."""
import pytest

import boxqp_cases as bq
import config_cases as cc


@pytest.mark.parametrize("table", list(bq.TABLES))
def test_every_record_is_in_its_class(ref, table):
    _, rcfg, recs = bq.batch(ref, table)
    assert len(recs) <= 64
    for (name, workload, index, hold, size), rec in zip(bq.entries(table), recs):
        lo, hi = bq.CLASSES[name]
        assert lo <= size <= hi, (name, size)
        assert cc.first_violated(ref, rcfg, rec) == size, (table, name, workload, index, hold)


def test_every_class_has_two_records_and_both_hold_flags():
    for name in bq.CLASSES:
        rows = bq.DEFAULT[name]
        assert len(rows) >= 2, name
        assert {e[2] for e in rows} == {0, 1}, name
    sizes = {e[3] for e in bq.DEFAULT["five_sixteen"]}
    # both register solvers (up to 6, 7..16 active bounds) and both sides of the dual / primal threshold
    assert min(sizes) <= 6 and any(7 <= s < 16 for s in sizes) and cc.DUAL_FORM_MAX[cc.PAPER] in sizes
    assert cc.DUAL_FORM_MAX[cc.PAPER] + 1 in {e[3] for e in bq.DEFAULT["above_sixteen"]}
    assert {e[3] for e in bq.DEFAULT["three_four"]} == {3, 4}
    for name in bq.NARROW:
        assert len(bq.NARROW[name]) >= 2 and {e[2] for e in bq.NARROW[name]} == {0, 1}
