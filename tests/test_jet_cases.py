"""CPU checks of the inputs of tests/test_gpu_jet_shapes.py (tests/jet_cases.py): the float32 oracle the kernels are
compared with sits well inside the bars, every mistake the GPU tests are aimed at moves the oracle by at least ten times
the bar it is judged with, and the EKF reference stays finite on the non-symmetric covariances."""
import json
import os

import numpy as np
import pytest

import jet_cases as jc
import jet_ref
from conftest import ROOT


@pytest.fixture(scope="module")
def dt():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "reference_constants.json")))["jet"]["ekf"]["timestep"]


@pytest.mark.parametrize("H", jc.HIDDEN)
def test_oracle_is_inside_the_bars(H):
    """jet_ref.JetLSTM (float32 numpy) against lstm_f64 on N(0, 1.5) inputs, n = 257, L = 1, 2, 12: at most one fifth of
    the sequence bars (h 5e-6, c 1e-5, T_dot_norm 1e-5), which leaves four fifths to the kernel.  One step (L = 1) is also
    held to one fifth of the one-step bar of 2e-6 on h and c.  Measured: h <= 2.7e-7, c <= 7.0e-7, out <= 8.1e-7 (at H = 1,
    where |out| reaches 4) over all cases; h, c <= 1.6e-7 at L = 1."""
    w = jc.weights(H)
    lstm = jet_ref.JetLSTM(**w)
    for L in (1, 2, 12):
        x = jc.sequences(257, L)
        _, out32, h32, c32, _ = lstm.get_state_sequence(x, 0.001)
        h, c, out = jc.lstm_f64(w, x)
        eh, ec, eo = np.abs(h32 - h).max(), np.abs(c32 - c).max(), np.abs(out32 - out).max()
        print(f"H {H} L {L}: float32 oracle against float64: h {eh:.2e} c {ec:.2e} out {eo:.2e}; |out| max {np.abs(out).max():.2f}")
        assert eh <= jc.BAR_SEQ_H / 5 and ec <= jc.BAR_SEQ_C / 5 and eo <= jc.BAR_TDOT_NORM / 5
        if L == 1:
            assert eh <= jc.BAR_STEP_HC / 5 and ec <= jc.BAR_STEP_HC / 5
        assert np.abs(out).max() > 0.3                       # O(1) outputs: an absolute bar means something


def test_transposed_covariances_are_visible(dt):
    """one EKF update with P0, Q or R read transposed: state and P move by more than 10x their bars for EVERY series"""
    n = 64
    Q, R, P0 = jc.full_ekf_matrices(0, n)
    assert Q[0, 1] != Q[1, 0] and R[0, 1] != R[1, 0] and (P0[:, 0, 1] != P0[:, 1, 0]).all()
    for M in (Q, R, *P0):
        assert np.linalg.eigvalsh(0.5 * (M + M.T)).min() > 0
    assert len({tuple(p.reshape(-1)) for p in P0}) == n
    x, u, z = jc.ekf_inputs(n, 1)
    for name, variant in (("P0", lambda i: (P0[i].T, Q, R)), ("Q", lambda i: (P0[i], Q.T, R)), ("R", lambda i: (P0[i], Q, R.T))):
        dx, dP = [], []
        for i in range(n):
            xr, Pr = jet_ref.ekf_update(x[i], P0[i], u[i], z[0, i], dt, Q, R)
            Pw, Qw, Rw = variant(i)
            xv, Pv = jet_ref.ekf_update(x[i], Pw, u[i], z[0, i], dt, Qw, Rw)
            dx.append(np.abs((xv - xr) / np.maximum(1.0, np.abs(xr))).max())
            dP.append(np.abs(Pv - Pr).max())
        print(f"{name} transposed: state moves by {min(dx):.1e}..{max(dx):.1e} relative, P by {min(dP):.1e}..{max(dP):.1e}")
        assert min(dx) >= 10 * jc.BAR_EKF_X_REL and min(dP) >= 10 * jc.BAR_EKF_P


def test_schedule_mistakes_are_visible(dt):
    """the fused plant with the schedule read one step late, and with its first row held for every step: thrust, estimate
    and log each move by more than 10x their bars"""
    n, steps = 16, 7
    w = jc.weights(37)
    lstm = jet_ref.JetLSTM(**w)
    Q, R, _ = jc.full_ekf_matrices(0)
    T0, x0, P0 = jc.plant_inputs(n)
    thr = jc.schedule(steps + 1, n)
    right = jet_ref.plant_run(lstm, T0, x0, P0, thr[:steps], steps, dt, Q, R)
    for name, wrong_thr in (("shifted", thr[1:steps + 1]), ("first row held", thr[0])):
        wrong = jet_ref.plant_run(lstm, T0, x0, P0, wrong_thr, steps, dt, Q, R)
        dT, dx, dl = (float(np.abs(a - b).max()) for a, b in zip((right[0], right[1], right[3]), (wrong[0], wrong[1], wrong[3])))
        print(f"schedule {name}: T_nn {dT:.2e} N, estimate {dx:.2e}, log {dl:.2e}")
        assert dT >= 10 * jc.BAR_PLANT_T and dx >= 10 * jc.BAR_PLANT_X and dl >= 10 * jc.BAR_PLANT_X


@pytest.mark.parametrize("H", (65, 128))
def test_a_single_pass_over_the_hidden_units_is_visible(H):
    """hidden units 64 and above left out of the fc sum (one pass of a 64-lane wavefront instead of two)"""
    w = jc.weights(H)
    x = jc.sequences(257, 1)
    h, _, out = jc.lstm_f64(w, x)
    short = h[:, :64] @ np.asarray(w["fc_w"], np.float64)[:64] + float(w["fc_b"][0])
    d = np.abs(short - out)
    print(f"H {H}: units >= 64 dropped: output moves by {d.max():.2e} (median {np.median(d):.2e})")
    assert d.max() >= 10 * jc.BAR_TDOT_NORM and np.median(d) >= 10 * jc.BAR_TDOT_NORM


def test_ekf_reference_stays_finite(dt):
    """50 repeated updates from full_ekf_matrices: the non-symmetric covariances do not blow the filter up"""
    n = 64
    Q, R, P0 = jc.full_ekf_matrices(0, n)
    x0, u, z = jc.ekf_inputs(n, 50)
    worst_x, worst_P = 0.0, 0.0
    for i in range(n):
        x, P = x0[i], P0[i]
        for k in range(50):
            x, P = jet_ref.ekf_update(x, P, u[i], z[k, i], dt, Q, R)
            assert np.isfinite(x).all() and np.isfinite(P).all()
            worst_x, worst_P = max(worst_x, np.abs(x).max()), max(worst_P, np.abs(P).max())
    print(f"50 updates: |x| <= {worst_x:.1f}, |P| <= {worst_P:.3f}")
    assert worst_x < 1e3 and worst_P < 10.0
