"""The adjoint kernels (adjoint_kernel_rt, adjoint_kernel_rt_tuned) on records away from the synthetic workloads and on the
active sets the box-QP tests were built around (tests/derivative_cases.py; tests/test_derivative_cases.py keeps the
families and their references honest on the CPU).

test_gpu_adjoint.py draws every input from synth.make_batch, on which a reference window read one column late or a hold
read as == 1.0 changes no gradient.  Here every instance of every family is compared with both routes of
tests/adjoint_model.py -- none is skipped: the references raise no flag and agree on every active set -- the per-instance
kernel is compared with the dense route under each instance's own configuration, grad_x0 with the sensitivity entry, and
the hold is read as != 0."""
import numpy as np
import pytest

from conftest import relerr
import derivative_cases as dc
from test_gpu_adjoint import MIRROR_BAR, _field_errors

pytestmark = pytest.mark.gpu

_outputs = {}


def _solve_family(solver_mod, ref, name):
    """one launch per family; the outputs are shared and read-only"""
    if name not in _outputs:
        _, cfg, rcfg, recs, _ = dc.family(ref, name)
        assert len(recs) <= 20
        xbar, fmbar = dc.cotangents(len(recs), cfg.n_var)
        runtime = dc.runtime_of(cfg)
        m = solver_mod.BatchedVSMPC(cfg, device=0, max_batch=len(recs), runtime=runtime, adjoint=True)
        try:
            assert m.uses_runtime_kernel == (runtime != "never")
            out = m.solve_adjoint(recs, xbar, fmbar)
        finally:
            m.close()
        for v in out.values():
            v.setflags(write=False)
        _outputs[name] = out
    return _outputs[name]


def _check(layout, out, b, k, c, label):
    """instance b of `out` against the dense route k and the mirror c; returns the two errors in units of the bar"""
    got = {"grad_x0": out["grad_x0"][b], "grad_cfg": out["grad_cfg"][b]}
    assert out["status"][b] == layout.STATUS_SOLVED, (label, out["status"][b])
    assert out["grad_cfg"][b, 31] == 0.0, label
    assert c["flags"] == 0 and out["flags"][b] == c["flags"], (label, out["flags"][b])
    np.testing.assert_array_equal(out["active"][b], c["active"], err_msg=label)
    np.testing.assert_array_equal(out["active"][b], k["active"], err_msg=label)
    em = _field_errors(got, c["grad_x0"], c["grad_cfg"])
    ek = _field_errors(got, k["grad_x0"], k["grad_cfg"])
    print(f"{label}: {em:.2e} of the bar against the mirror, {ek:.2e} against the dense route")
    return em, ek


@pytest.mark.parametrize("name", dc.FAMILIES)
def test_gradients_match_models_on_every_record(solver_mod, ref, layout, name):
    _, cfg, rcfg, recs, names = dc.family(ref, name)
    out = _solve_family(solver_mod, ref, name)
    assert (out["status"] == layout.STATUS_SOLVED).all(), out["status"]
    assert (out["grad_cfg"][:, 31] == 0.0).all()
    worst_m = worst_k = (0.0, None)
    checked = 0
    for b in range(len(recs)):
        k, c = dc.adjoint_refs(ref, name, b)
        em, ek = _check(layout, out, b, k, c, names[b])
        worst_m, worst_k = max(worst_m, (em, names[b])), max(worst_k, (ek, names[b]))
        assert ek <= 1.0, (names[b], ek)
        assert em <= MIRROR_BAR, (names[b], em)
        checked += 1
    print(f"{name}: worst {worst_m[0]:.2e} of the bar against the mirror ({worst_m[1]}), "
          f"{worst_k[0]:.2e} against the dense route ({worst_k[1]})")
    assert checked == len(recs) == dc.SIZES[name]


def test_tuned_rows_match_the_dense_route(solver_mod, ref, layout):
    """adjoint_kernel_rt_tuned against a model: every instance under its own weights and throttle box.  The box gradients
    of the third group (30..85) are in percent of that group's limits -- the factor sqrt(1 + 4 c12 v) / sigma_u is taken at
    the instance's warped limits, not at the handle's (0..100), which would miss the bar by more than three orders of
    magnitude (test_derivative_cases.test_tuned_groups_are_flag_free)."""
    cfg, recs, names, cfgs, rcfgs = dc.tuned_cases(ref)
    B = len(recs)
    xbar, fmbar = dc.cotangents(B, cfg.n_var)
    m = solver_mod.BatchedVSMPC(cfg, device=0, max_batch=B, runtime="fallback", adjoint=True)
    try:
        assert m.uses_runtime_kernel
        out = m.solve_adjoint(recs, xbar, fmbar, configs=cfgs)
    finally:
        m.close()
    worst_m = worst_k = (0.0, None)
    box = np.zeros(2, dtype=bool)
    for b in range(B):
        k, c = dc.tuned_refs(ref, b)
        em, ek = _check(layout, out, b, k, c, f"{names[b]} (configuration {b % 3})")
        worst_m, worst_k = max(worst_m, (em, names[b])), max(worst_k, (ek, names[b]))
        assert ek <= 1.0, (names[b], ek)
        if b % 3 == 2:
            box |= out["grad_cfg"][b, layout.GRAD_THROTTLE_MIN:layout.GRAD_THROTTLE_MAX + 1] != 0.0
    print(f"tuned rows: worst {worst_m[0]:.2e} of the bar against the mirror ({worst_m[1]}), "
          f"{worst_k[0]:.2e} against the dense route ({worst_k[1]})")
    assert box.all(), box


def test_grad_x0_matches_the_sensitivity_entry_on_distinct_records(solver_mod, ref, layout):
    """dL/dX0 = dx_dx0^T xbar + dfm_dx0^T fmbar with the Jacobians the same handle ships: needs no oracle"""
    _, cfg, _, recs, names = dc.family(ref, "records_17_7_12")
    assert cfg == layout.paper_config()
    xbar, fmbar = dc.cotangents(len(recs), cfg.n_var, seed=6)
    m = solver_mod.BatchedVSMPC(cfg, device=0, max_batch=len(recs), sensitivity=True, adjoint=True)
    try:
        sens = m.solve_sensitivity(recs)
        out = m.solve_adjoint(recs, xbar, fmbar)
    finally:
        m.close()
    assert (out["status"] == layout.STATUS_SOLVED).all(), out["status"]
    np.testing.assert_array_equal(out["active"], sens["active"])
    np.testing.assert_array_equal(out["flags"], sens["flags"])
    for b in range(len(recs)):
        want = sens["dx_dx0"][b].T @ xbar[b] + sens["dfm_dx0"][b].T @ fmbar[b]
        assert relerr(out["grad_x0"][b], want) < 1e-8, (names[b], relerr(out["grad_x0"][b], want))


@pytest.mark.parametrize("name", ["records_17_7_12", "records_20_5_9"])
def test_hold_values(solver_mod, ref, layout, name):
    """"held" is IN_HOLD != 0, whatever the value; a pinned first block is on neither limit of the box, even where its
    value equals one (uprev_at_the_ends_held pins 0 and 100 % under the default limits 0..100)"""
    _, cfg, rcfg, recs, names = dc.family(ref, name)
    out = _solve_family(solver_mod, ref, name)
    lo, hi = layout.GRAD_THROTTLE_MIN, layout.GRAD_THROTTLE_MAX
    for held in ("all_distinct_1", "hold_-1", "hold_1e-300", "uprev_at_the_ends_held"):
        b = names.index(held)
        assert recs[b, layout.IN_HOLD] not in (0.0, 1.0)
        assert (out["active"][b, :4] == layout.ACTIVE_PINNED).all(), (held, out["active"][b])
        assert not (out["active"][b, 4:] == layout.ACTIVE_PINNED).any(), held
        k, _ = dc.adjoint_refs(ref, name, b)
        gall = np.abs(np.concatenate([k["grad_x0"], k["grad_cfg"]])).max()
        for g in (lo, hi):
            want = k["grad_cfg"][g]
            assert abs(out["grad_cfg"][b, g] - want) <= 1e-6 * abs(want) + 1e-12 * gall, (held, g, out["grad_cfg"][b, g], want)
            if not (k["active"] == (layout.ACTIVE_LOWER if g == lo else layout.ACTIVE_UPPER)).any():
                assert out["grad_cfg"][b, g] == 0.0, (held, g)      # no non-pinned throttle on that limit: an empty sum
    b = names.index("hold_-0.0")
    assert not (out["active"][b] == layout.ACTIVE_PINNED).any(), out["active"][b]
    if name == "records_17_7_12":
        b = names.index("uprev_at_the_ends_held")                   # pinned at the upper limit's value, none bound there
        vmin, vmax = ref.throttle_bounds(rcfg)
        np.testing.assert_allclose(out["x"][b, rcfg.off_throttle:rcfg.off_throttle + 4], [vmin, vmax, vmin, vmax], rtol=0,
                                   atol=1e-12)
        assert out["grad_cfg"][b, hi] == 0.0 and out["grad_cfg"][b, lo] != 0.0
