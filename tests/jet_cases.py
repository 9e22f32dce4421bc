"""Inputs of the jet-side shape tests (tests/test_gpu_jet_shapes.py) and a float64 evaluator of the network.  Helper, no
tests; tests/test_jet_cases.py checks on the CPU that these inputs can tell a right kernel from a wrong one.

The reference's checkpoint is one network (H = 80) with one estimator setting (Q, R, P0 multiples of the identity), so it
cannot see a kernel that is only right at H = 80, or one that reads a 2x2 matrix transposed.  Here: random networks of
every hidden size at which the kernels take another path, covariances that are NOT symmetric (so row-major against
column-major is a different number, not the same one), and a throttle schedule that differs at every step."""
from __future__ import annotations

import os

import numpy as np

from conftest import ROOT

# 1: a single unit; 37: one partial pass over a wavefront; 64 / 65: exactly one pass / one unit into the second;
# 128: JET_HMAX, two full passes and the largest weight block in LDS
HIDDEN = (1, 37, 64, 65, 128)
# around the 64-lane wavefront and the 256-thread block: one live thread, a partial wavefront, one short of a block, a
# full block, a second block with one live thread, a third with one
SERIES = (1, 63, 255, 256, 257, 513)

# The project's bars (tests/test_gpu_jet.py, tests/test_gpu_rollout.py); nothing here is new.
BAR_STEP_HC = 2e-6          # h, c after one step, absolute
BAR_SEQ_H, BAR_SEQ_C = 5e-6, 1e-5
BAR_TDOT_NORM, BAR_TNEXT_NORM = 1e-5, 1e-6
BAR_TDOT_REL, BAR_TNEXT = 1e-5, 1e-4
BAR_EKF_X_REL, BAR_EKF_P = 1e-11, 1e-13
BAR_PLANT_T, BAR_PLANT_X, BAR_PLANT_P = 2e-3, 5e-3, 1e-7
BAR_ROLLOUT = 2e-6


def golden_norm():
    """thrust_mean, thrust_std, throttle_mean, throttle_std of the reference's checkpoint"""
    return np.load(os.path.join(ROOT, "tests", "golden", "jet_lstm.npz"))["norm"].astype(np.float64)


def weights(H, seed=0):
    """float32 weights with the shapes torch gives LSTM(2, H) + Linear(H, 1), uniform in +-4/sqrt(H): four times torch's
    default init scale, so that the gates leave the linear part of the sigmoids and the outputs are O(1).  The keys are
    the argument names of jet_ref.JetLSTM and jet_plant.JetModelTotal."""
    rng = np.random.default_rng([int(H), int(seed), 7])
    k = 4.0 / np.sqrt(H)
    u = lambda *shape: rng.uniform(-k, k, size=shape).astype(np.float32)
    return dict(w_ih=u(4 * H, 2), w_hh=u(4 * H, H), b_ih=u(4 * H), b_hh=u(4 * H), fc_w=u(H), fc_b=u(1), norm=golden_norm())


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def lstm_f64(w, x):
    """The network of `w` in float64: x [n, L, 2] (normalised inputs), gate order i, f, g, o, zero initial state, state
    carried along L.  Returns h [n, H], c [n, H] after the last sample and out [n] = fc(h) (the normalised thrust rate)."""
    w_ih, w_hh = np.asarray(w["w_ih"], np.float64), np.asarray(w["w_hh"], np.float64)
    b = np.asarray(w["b_ih"], np.float64) + np.asarray(w["b_hh"], np.float64)
    fc_w, fc_b = np.asarray(w["fc_w"], np.float64).reshape(-1), float(np.asarray(w["fc_b"]).reshape(-1)[0])
    x = np.asarray(x, np.float64)
    n, L, _ = x.shape
    H = w_hh.shape[1]
    h, c = np.zeros((n, H)), np.zeros((n, H))
    for t in range(L):
        g = x[:, t, :] @ w_ih.T + h @ w_hh.T + b
        i, f, gg, o = _sigmoid(g[:, 0:H]), _sigmoid(g[:, H:2 * H]), np.tanh(g[:, 2 * H:3 * H]), _sigmoid(g[:, 3 * H:4 * H])
        c = f * c + i * gg
        h = o * np.tanh(c)
    return h, c, h @ fc_w + fc_b


def sequences(n, L, seed=0):
    """normalised inputs x [n, L, 2], N(0, 1.5): past the +-1 sigma of the training data on both channels"""
    return np.random.default_rng([n, L, int(seed), 11]).normal(0.0, 1.5, size=(n, L, 2)).astype(np.float32)


def step_inputs(n, seed=0):
    """thrust [n] (N) and throttle [n] (percent), float32, over the range the jets work in"""
    rng = np.random.default_rng([n, int(seed), 13])
    return rng.uniform(5.0, 240.0, n).astype(np.float32), rng.uniform(0.0, 100.0, n).astype(np.float32)


def _spd_plus_antisymmetric(rng, scale, n=None):
    """[[a, b + e], [b - e, d]] with a, d > 0, b^2 < a d / 4 and |e| between 5 and 15 % of scale: the symmetric part is
    positive definite, and the matrix differs from its transpose by 2 |e|."""
    shape = () if n is None else (n,)
    a, d = rng.uniform(0.5, 1.5, shape) * scale, rng.uniform(0.5, 1.5, shape) * scale
    b = rng.uniform(-0.5, 0.5, shape) * np.sqrt(a * d)
    e = rng.uniform(0.05, 0.15, shape) * scale * rng.choice([-1.0, 1.0], shape)
    return np.stack([np.stack([a, b + e], axis=-1), np.stack([b - e, d], axis=-1)], axis=-2)


def full_ekf_matrices(seed=0, n=1):
    """Q, R [2, 2] and P0 [n, 2, 2] (another one for every series), at the magnitudes of the reference's constants
    (Q = P0 = 0.1 I, R = 0.5 I): symmetric positive definite plus an antisymmetric part, so Q[0, 1] != Q[1, 0] and a
    transposed read changes the result."""
    rng = np.random.default_rng([int(seed), 17])
    Q = _spd_plus_antisymmetric(rng, 0.1)
    R = _spd_plus_antisymmetric(rng, 0.5)
    P0 = _spd_plus_antisymmetric(np.random.default_rng([int(seed), 19]), 0.1, n)
    return Q, R, P0


def ekf_inputs(n, updates, seed=0):
    """x0 [n, 2], u [n], z [updates, n, 2]: states over the jets' range, one measurement per update around x0"""
    rng = np.random.default_rng([int(seed), 23])
    x = np.stack([rng.uniform(5, 240, n), rng.uniform(-100, 100, n)], axis=1)
    u = rng.uniform(0, 100, n)
    z = x[None] + rng.normal(0, 2.0, (updates, n, 2))
    return x, u, z


def schedule(steps, n, seed=0):
    """throttle [steps, n] float32, uniform in 10 to 95 percent, drawn independently per step and per series"""
    return np.random.default_rng([steps, n, int(seed), 29]).uniform(10.0, 95.0, size=(steps, n)).astype(np.float32)


def plant_inputs(n, seed=0):
    """T_nn [n] float32, x_est [n, 2] (the estimate starts beside the plant thrust, with a rate), P0 [n, 2, 2]"""
    rng = np.random.default_rng([n, int(seed), 31])
    T0 = rng.uniform(20.0, 220.0, n).astype(np.float32)
    x0 = np.stack([T0.astype(np.float64) + rng.normal(0, 2.0, n), rng.normal(0, 20.0, n)], axis=1)
    return T0, x0, full_ekf_matrices(seed, n)[2]
