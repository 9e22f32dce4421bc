"""Every way into the throttle box QP of the tuned solve kernels, paper horizon (tests/boxqp_cases.py).

The dual form's set-up (rows 16.. of X = L22^-1, s and max |s|) runs beside the throttle sweep for EVERY instance, and
the columns of P for a first active set of two to four throttles are formed one per wavefront; the paths for one, for
five to sixteen and for more than sixteen violated bounds branch off behind them.  Checked here, for the production
kind in both condensing forms and for the per-instance-tunables kind (rows packed from the handle's configuration), with
the hold set and released:
  * every class against the oracle at the project's bar (test_gpu_config_parity._check_solution: x and first move 1e-8
    relative per output group, iteration counts and statuses equal);
  * a batch that mixes instances that enter the box QP with instances that do not, bit for bit against every instance
    solved in a batch of one -- set-up that leaked into an instance that never uses it would show here;
  * a non-finite record next to a valid one: Numerical for the first, the neighbour unchanged."""
import numpy as np
import pytest

import boxqp_cases as bq
from test_gpu_config_parity import _check_solution

pytestmark = pytest.mark.gpu

KINDS = [("plain", "auto"), ("plain", "syrk"), ("tuned", "auto")]
IDS = [f"{k}-{f}" for k, f in KINDS]
_batches = {}


def _batch(ref, table):
    if table not in _batches:
        _batches[table] = bq.batch(ref, table)
    return _batches[table]


class _Handle:
    def __init__(self, solver_mod, cfg, n, kind, form):
        self.m = solver_mod.BatchedVSMPC(cfg, device=0, max_batch=n, runtime="never", tunables=(kind == "tuned"))
        assert not self.m.uses_runtime_kernel
        if form == "syrk":
            self.m.set_kernel_form(solver_mod.KERNEL_FORM_SYRK)
        self.pack = (lambda b: solver_mod.pack_tunables(self.m, [self.m.cfg] * b)) if kind == "tuned" else None

    def solve(self, recs):
        recs = np.ascontiguousarray(recs)
        if self.pack is None:
            return self.m.solve(recs)
        return self.m.solve(recs, tunables=self.pack(len(recs)))

    def close(self):
        self.m.close()


@pytest.mark.parametrize("kind, form", KINDS, ids=IDS)
@pytest.mark.parametrize("table", list(bq.TABLES))
def test_every_class_matches_oracle(solver_mod, ref, layout, table, kind, form):
    cfg, rcfg, recs = _batch(ref, table)
    h = _Handle(solver_mod, cfg, len(recs), kind, form)
    try:
        x, fm, st, it = h.solve(recs)
    finally:
        h.close()
    _check_solution(ref, rcfg, layout, recs, x, fm, st, it)
    for (name, *_), n in zip(bq.entries(table), it):
        assert (n == 1) == (name == "never"), (name, n)        # exactly the "never" class skips the box QP


@pytest.mark.parametrize("kind, form", KINDS, ids=IDS)
def test_mixed_batch_is_bit_identical_to_batches_of_one(solver_mod, ref, layout, kind, form):
    cfg, _, recs = _batch(ref, "default")
    names = [e[0] for e in bq.entries("default")]
    order = np.argsort([i % 6 for i in range(len(recs))], kind="stable")     # classes interleaved, not class by class
    recs = recs[order]
    assert "never" in names and len(set(names)) == len(bq.CLASSES)
    h = _Handle(solver_mod, cfg, len(recs), kind, form)
    try:
        together = h.solve(recs)
        for b in range(len(recs)):
            alone = h.solve(recs[b:b + 1])
            for a, t in zip(alone, together):
                np.testing.assert_array_equal(a[0], t[b], err_msg=f"{names[order[b]]} record {b}")
    finally:
        h.close()
    assert (together[2] == layout.STATUS_SOLVED).all()


@pytest.mark.parametrize("kind, form", KINDS, ids=IDS)
def test_non_finite_record_beside_valid_ones(solver_mod, ref, layout, kind, form):
    cfg, _, recs = _batch(ref, "default")
    names = [e[0] for e in bq.entries("default")]
    pick = [names.index("two"), names.index("never"), names.index("three_four"), names.index("five_sixteen")]
    good = recs[pick]
    bad = good.copy()
    bad[0::2, layout.IN_INERTIA] = np.nan          # records 0 and 2 non-finite, 1 (no box QP) and 3 (box QP) valid
    h = _Handle(solver_mod, cfg, len(good), kind, form)
    try:
        ref_out = h.solve(good)
        out = h.solve(bad)
    finally:
        h.close()
    assert (ref_out[2] == layout.STATUS_SOLVED).all()
    assert out[2][0] == layout.STATUS_NUMERICAL and out[2][2] == layout.STATUS_NUMERICAL, out[2]
    for b in (1, 3):                                # the valid neighbours: every output bit for bit what it was
        for a, r in zip(out, ref_out):
            np.testing.assert_array_equal(a[b], r[b])
