"""The passes of the throttle box QP's active-set loop behind the first one (tests/boxqp_pass_cases.py).

tests/test_gpu_boxqp_entry_paths.py covers every way INTO the box QP; the records here are chosen by what the later
passes do: active sets of every size the straight-line pass small_set_pass<K> of csrc/vsmpc_p4.hpp has (1..6), solved
behind the first pass; a bound added in a later pass, with its column of P formed on demand inside the loop and with all
columns there from the start; lower and upper bounds; and, at the horizons (21, 9, 15) and (34, 14, 24), sequences that
pass through the register solvers for larger sets on their way down to the small ones: the accessor for two throttle tile
rows runs the straight-line pass at another throttle count, the one for three (XDense, KPASS = 0) the loop without it.  Each table is solved as one small batch, by the production kind
in both condensing forms and by the per-instance-tunables kind, and checked
  * against the oracle at the project's bar (test_gpu_config_parity._check_solution: x and first move 1e-8 relative per
    output group, statuses and iteration counts equal);
  * for the sequence: every record takes exactly as many passes as its tabled sequence has sets, plus the first solve."""
import numpy as np
import pytest

import boxqp_pass_cases as bp
from test_gpu_boxqp_entry_paths import IDS, KINDS, _Handle
from test_gpu_config_parity import _check_solution

pytestmark = pytest.mark.gpu

_batches = {}


def _batch(ref, table):
    if table not in _batches:
        _batches[table] = bp.batch(ref, table)
    return _batches[table]


@pytest.mark.parametrize("kind, form", KINDS, ids=IDS)
@pytest.mark.parametrize("table", list(bp.TABLES))
def test_later_passes_match_oracle(solver_mod, ref, layout, table, kind, form):
    cfg, rcfg, recs = _batch(ref, table)
    assert len(recs) <= 64
    h = _Handle(solver_mod, cfg, len(recs), kind, form)
    try:
        x, fm, st, it = h.solve(recs)
    finally:
        h.close()
    print("passes:", it.tolist())
    _check_solution(ref, rcfg, layout, recs, x, fm, st, it)
    want = np.array([len(seq) + 1 for *_, seq in bp.TABLES[table][2]])
    np.testing.assert_array_equal(it, want)
