"""The debug dumps of the solve kernel (condensed Hessian before P3, factor after it; vsmpc_debug_condensed) at every
horizon and condensing form that has a copy of the dump code: the SYRK form's run-time loop over kTileTab and the
structured form's unrolled copy inside the fused tail, at (17,7,12), (21,9,15) -- SYRK form only, joint rows share a tile
row with throttle rows, three corner tile rows -- and (34,14,24).  (The structured form of the paper horizon against the
model is test_gpu_parity.py::test_condensed_hessian_and_factor.)

One record per case (the second take-off record), one launch of one instance per dump; the dumps and the model's
matrices are formed once per horizon and shared.  Compared: the four quantities of test_condensed_hessian_and_factor --
M, the gradient row g, L and L^-1 g -- against tests/algo_model.py: reduced_condensed, and between the two forms.

Bars (profiles/solve_body_dumps.txt holds the measurement): ten times the worst relative error measured on the commit before
the dump helpers existed, never below the paper horizon's 1e-12 (M, g) / 1e-11 (L, L^-1 g)."""
import numpy as np
import pytest

from conftest import relerr

pytestmark = pytest.mark.gpu

PAPER, ODD, LONG = (17, 7, 12), (21, 9, 15), (34, 14, 24)
STRUCT, SYRK = "structured", "syrk"
FLOOR = (1e-12, 1e-12, 1e-11, 1e-11)   # M, g, L, L^-1 g at the paper horizon (test_condensed_hessian_and_factor)
# (horizon, what) -> bars for (M, g, L, L^-1 g).  Beside each: the relative errors measured before the helpers existed; ten
# times the worst of them (2.2e-12, L^-1 g at the 2x horizon) lies under the floor, so every bar is the floor
BARS = {
    (PAPER, SYRK): FLOOR,       # 1.80e-16 1.11e-16 1.31e-15 1.20e-13
    (PAPER, "forms"): FLOOR,    # 1.80e-16 1.11e-16 1.42e-16 2.42e-16
    (ODD, SYRK): FLOOR,         # 1.80e-16 2.10e-16 1.84e-15 1.76e-13
    (LONG, STRUCT): FLOOR,      # 1.74e-16 1.36e-15 4.63e-15 2.15e-13
    (LONG, SYRK): FLOOR,        # 1.74e-16 1.36e-15 5.67e-15 2.15e-13
    (LONG, "forms"): FLOOR,     # 1.74e-16 2.47e-16 1.20e-15 2.52e-15
}


class _Horizon:
    """handle, record, the model's (M, g, L) and the dumps taken so far of one horizon"""

    def __init__(self, solver_mod, ref, synth, layout, horizon):
        n, ns, hc = horizon
        self.solver_mod = solver_mod
        more = dict(period_small=0.0025) if horizon == LONG else {}   # BASELINE.json's 2x configuration (horizon2x_config)
        cfg = layout.MPCConfig(n_iter=n, n_iter_small=ns, control_horizon=hc, **more)
        self.rcfg = ref.Config(n_iter=n, n_iter_small=ns, control_horizon=hc, **more)
        self.ref = ref
        self.rec = synth.make_batch(cfg, 2, workload="takeoff")[1]
        self.mpc = solver_mod.BatchedVSMPC(cfg, device=0, max_batch=1)
        self.model = None
        self.dumps = {}

    def expected(self):
        if self.model is None:
            import algo_model
            self.model = algo_model.reduced_condensed(self.rcfg, self.ref, self.rec)
        return self.model

    def dump(self, form):
        if form not in self.dumps:
            code = self.solver_mod.KERNEL_FORM_STRUCTURED if form == STRUCT else self.solver_mod.KERNEL_FORM_SYRK
            prev = self.mpc.set_kernel_form(code)
            try:
                self.dumps[form] = self.mpc.debug_condensed(self.rec)
            finally:
                self.mpc.set_kernel_form(prev)
        return self.dumps[form]


@pytest.fixture(scope="module")
def horizons(solver_mod, ref, synth, layout):
    made = {}

    def get(horizon):
        if horizon not in made:
            made[horizon] = _Horizon(solver_mod, ref, synth, layout, horizon)
        return made[horizon]
    yield get
    for h in made.values():
        h.mpc.close()


def _check(what, errs, bars):
    print(f"{what}: M {errs[0]:.2e} g {errs[1]:.2e} L {errs[2]:.2e} L^-1 g {errs[3]:.2e}")
    for name, e, bar in zip(("M", "g", "L", "L^-1 g"), errs, bars):
        assert e < bar, (what, name, e, bar)


@pytest.mark.parametrize("horizon,form", [(PAPER, SYRK), (ODD, SYRK), (LONG, STRUCT), (LONG, SYRK)])
def test_dump_matches_model(horizons, horizon, form):
    h = horizons(horizon)
    M, Lf = h.dump(form)
    Me, ge, Le = h.expected()
    nz = Me.shape[0]
    assert M.shape[0] == ((nz + 1 + 15) // 16) * 16
    Mh = np.tril(M[:nz, :nz])
    Mh = Mh + np.tril(Mh, -1).T
    errs = (relerr(Mh, Me), relerr(M[nz, :nz], ge), relerr(np.tril(Lf[:nz, :nz]), Le),
            relerr(Lf[nz, :nz], np.linalg.solve(Le, ge)))
    _check(f"{horizon} {form} against the model", errs, BARS[horizon, form])


@pytest.mark.parametrize("horizon", [PAPER, LONG])
def test_structured_dump_matches_syrk_dump(horizons, horizon):
    h = horizons(horizon)
    (Ma, La), (Mb, Lb) = h.dump(STRUCT), h.dump(SYRK)
    nz = h.expected()[0].shape[0]
    # (entry [NZ, NZ], the constant term of the cost, is not formed by the structured form: nothing reads it)
    errs = (relerr(np.tril(Ma[:nz, :nz]), np.tril(Mb[:nz, :nz])), relerr(Ma[nz, :nz], Mb[nz, :nz]),
            relerr(np.tril(La[:nz, :nz]), np.tril(Lb[:nz, :nz])), relerr(La[nz, :nz], Lb[nz, :nz]))
    _check(f"{horizon} structured against SYRK", errs, BARS[horizon, "forms"])
