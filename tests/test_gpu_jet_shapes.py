"""GPU tests of the jet plant / estimator kernels away from the reference's checkpoint (include/vsmpc_jet.h, and the jet
plant option of the rollout): every hidden size at which a kernel takes another path, series counts around the wavefront
and the block, covariances that are not symmetric, a throttle schedule that differs at every step, the device entry, the
staging that grows, the optional outputs, the argument contracts.  Inputs: tests/jet_cases.py, whose CPU checks
(tests/test_jet_cases.py) show that the float32 oracle uses at most a fifth of each bar and that every mistake aimed at
here moves the oracle by ten bars or more.  References: oracle/jet_ref.py (float32 network, float64 EKF) and
jet_cases.lstm_f64 (the network in float64).  The bars are the ones of tests/test_gpu_jet.py and
tests/test_gpu_rollout.py.  Every test prints its worst figure."""
import ctypes
import importlib
import json
import os

import numpy as np
import pytest

import jet_cases as jc
import jet_ref
import rollout_model as rm
from conftest import PKG, ROOT, relerr

pytestmark = pytest.mark.gpu

MAXN = 513
DTF = 0.001                      # the plant step of the golden vectors
OK, ERR_INVALID_ARG, ERR_BATCH_TOO_LARGE = 0, -1, -3


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope="module")
def jp(solver_mod):
    return importlib.import_module(PKG + ".jet_plant")


@pytest.fixture(scope="module")
def dt():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "reference_constants.json")))["jet"]["ekf"]["timestep"]


@pytest.fixture(scope="module")
def nets(jp):
    """(handle, weights, float32 oracle) per hidden size: one handle per H, max_series = 513, shared by the tests"""
    made = {}

    def get(H):
        if H not in made:
            w = jc.weights(H)
            made[H] = (jp.JetModelTotal(**w, device=0, max_series=MAXN), w, jet_ref.JetLSTM(**w))
        return made[H]

    yield get
    for m, _, _ in made.values():
        m.close()


def _fresh(jp, H):
    return jp.JetModelTotal(**jc.weights(H), device=0, max_series=MAXN)


def _dev(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


def _raw_step(m, thrust, throttle, want_h, want_c):
    n, H = thrust.size, m.hidden
    Tn, Td = np.empty(n, np.float32), np.empty(n, np.float32)
    h = np.empty((n, H), np.float32) if want_h else None
    c = np.empty((n, H), np.float32) if want_c else None
    assert m.lib.vsmpc_jet_nn_step(m._h, _p(thrust), _p(throttle), n, DTF, _p(Tn), _p(Td), _p(h), _p(c)) == OK
    return Tn, Td, h, c


@pytest.mark.parametrize("H", jc.HIDDEN)
def test_step_every_hidden_size_and_series_count(nets, H):
    """jet_nn_step_kernel at every (H, n): thrusts and states against the float32 oracle, h, c and the normalised output
    against float64; h_out alone and c_out alone (lstm_step_from_zero<true> with one null pointer) give the bits of the
    call that asks for both.  The references are computed once for 513 series; n series are the first n of them."""
    m, w, lstm = nets(H)
    thrust, throttle = jc.step_inputs(MAXN)
    Tn_r, Td_r, h_r, c_r = lstm.get_state(thrust, throttle, DTF)
    h64, c64, out64 = jc.lstm_f64(w, lstm.normalize(thrust, throttle)[:, None, :])
    std32 = float(np.float32(lstm.thrust_std))
    worst = dict.fromkeys(("T_next", "T_dot_rel", "h", "c", "h64", "c64", "out64"), 0.0)
    for n in jc.SERIES:
        Tn, Td, h, c = m.get_state(thrust[:n], throttle[:n], DTF, with_state=True)
        fig = {"T_next": _dev(Tn, Tn_r[:n]), "T_dot_rel": _dev(Td, Td_r[:n]) / float(np.abs(Td_r[:n]).max()),
               "h": _dev(h, h_r[:n]), "c": _dev(c, c_r[:n]), "h64": _dev(h, h64[:n]), "c64": _dev(c, c64[:n]),
               "out64": _dev(Td.astype(np.float64) / std32, out64[:n])}
        print(f"H {H} n {n}: " + " ".join(f"{k} {v:.2e}" for k, v in fig.items()))
        assert fig["T_next"] < jc.BAR_TNEXT and fig["T_dot_rel"] < jc.BAR_TDOT_REL, (H, n)
        assert max(fig["h"], fig["c"], fig["h64"], fig["c64"]) < jc.BAR_STEP_HC, (H, n)
        assert fig["out64"] < jc.BAR_TDOT_NORM, (H, n)
        worst = {k: max(worst[k], fig[k]) for k in worst}
        Tn_h, Td_h, h_only, none_c = _raw_step(m, thrust[:n], throttle[:n], True, False)
        Tn_c, Td_c, none_h, c_only = _raw_step(m, thrust[:n], throttle[:n], False, True)
        Tn_0, Td_0, _, _ = _raw_step(m, thrust[:n], throttle[:n], False, False)
        assert none_c is None and none_h is None
        assert np.array_equal(h_only, h) and np.array_equal(c_only, c), (H, n)
        for a, b in ((Tn_h, Td_h), (Tn_c, Td_c), (Tn_0, Td_0)):
            assert np.array_equal(a, Tn) and np.array_equal(b, Td), (H, n)
    print(f"H {H} worst over n: " + " ".join(f"{k} {v:.2e}" for k, v in worst.items()))


@pytest.mark.parametrize("H", jc.HIDDEN)
def test_sequence_every_hidden_size(nets, H):
    """jet_nn_sequence_kernel (a workgroup of H threads rounded up to a wavefront, W_hh in play) at L = 1, 2, 12 and
    n = 1, 65: against the float32 oracle and against float64"""
    m, w, lstm = nets(H)
    worst = dict.fromkeys(("h", "c", "T_dot_norm", "T_next_norm", "h64", "c64", "out64"), 0.0)
    for L in (1, 2, 12):
        x = jc.sequences(65, L)
        tn_r, td_r, h_r, c_r, _ = lstm.get_state_sequence(x, DTF)
        h64, c64, out64 = jc.lstm_f64(w, x)
        tn64 = x[:, -1, 0].astype(np.float64) + out64 * DTF
        for n in (1, 65):
            tn, td, h, c = m.get_state_sequence(x[:n], DTF)
            fig = {"h": _dev(h, h_r[:n]), "c": _dev(c, c_r[:n]), "T_dot_norm": _dev(td, td_r[:n]),
                   "T_next_norm": _dev(tn, tn_r[:n]), "h64": _dev(h, h64[:n]), "c64": _dev(c, c64[:n]),
                   "out64": _dev(td, out64[:n])}
            print(f"H {H} L {L} n {n}: " + " ".join(f"{k} {v:.2e}" for k, v in fig.items()))
            assert max(fig["h"], fig["h64"]) < jc.BAR_SEQ_H and max(fig["c"], fig["c64"]) < jc.BAR_SEQ_C, (H, L, n)
            assert max(fig["T_dot_norm"], fig["out64"]) < jc.BAR_TDOT_NORM, (H, L, n)
            assert fig["T_next_norm"] < jc.BAR_TNEXT_NORM and _dev(tn, tn64[:n]) < jc.BAR_TNEXT_NORM, (H, L, n)
            worst = {k: max(worst[k], fig[k]) for k in worst}
    print(f"H {H} worst over L, n: " + " ".join(f"{k} {v:.2e}" for k, v in worst.items()))


def _all_calls(jp, m, n, seed, dt):
    """one call of every host entry on `n` series with inputs of their own; the results as a flat list of arrays"""
    thrust, throttle = jc.step_inputs(n, seed)
    out = list(m.get_state(thrust, throttle, DTF, with_state=True))
    out += list(m.get_state_sequence(jc.sequences(n, 3, seed), DTF))
    Q, R, P0 = jc.full_ekf_matrices(seed, n)
    x, u, z = jc.ekf_inputs(n, 1, seed)
    ekf = jp.EKFJetsTotal(m, R, Q, P0[0], dt, n)
    ekf.P = P0.reshape(n, 4).copy()
    out += list(ekf.update(x[:, 0], x[:, 1], u, z[0, :, 0], z[0, :, 1])) + [ekf.P]
    T0, x0, Pp = jc.plant_inputs(n, seed)
    out += list(jp.JetPlant(m, R, Q, dt).run(T0, x0, Pp, jc.schedule(4, n, seed), 4, log=True))
    return out


def test_handle_reuse_leaves_nothing_behind(jp, dt):
    """n = 513, then 1, then 257 on one handle, other inputs each time: the staging buffers still hold the larger call's
    data beyond n, and no result may depend on it -- each call gives the bits of the same call on a fresh handle"""
    H = 65
    used = _fresh(jp, H)
    try:
        for seed, n in enumerate((513, 1, 257)):
            got = _all_calls(jp, used, n, seed, dt)
            fresh = _fresh(jp, H)
            try:
                want = _all_calls(jp, fresh, n, seed, dt)
            finally:
                fresh.close()
            assert len(got) == len(want) == 15
            for k, (a, b) in enumerate(zip(got, want)):
                assert a.shape == b.shape and np.isfinite(a).all() and np.array_equal(a, b), (n, k)
        print("513 -> 1 -> 257 on one handle: 15 result arrays per call bit-equal to a fresh handle's")
    finally:
        used.close()


def _ekf_reference(x0, P0, u, z, dt, Q, R):
    """x [updates, n, 2], P [updates, n, 2, 2] of repeated jet_ref.ekf_update, every series on its own"""
    K, n = z.shape[0], x0.shape[0]
    xs, Ps = np.empty((K, n, 2)), np.empty((K, n, 2, 2))
    for i in range(n):
        x, P = x0[i], P0[i]
        for k in range(K):
            x, P = jet_ref.ekf_update(x, P, u[i], z[k, i], dt, Q, R)
            xs[k, i], Ps[k, i] = x, P
    return xs, Ps


def test_ekf_full_matrices(jp, nets, dt):
    """jet_ekf_kernel with Q, R and a per-series P0 that are not symmetric (row-major as the header says: a transposed
    read moves the state by 1e-5 and more, tests/test_jet_cases.py), every n of SERIES, 21 updates in a row with the
    device's own state and P fed back: state to 1e-11 relative and P to 1e-13 after every update.  The reference is
    computed once for 513 series.  And P, Q, R symmetric in gives P symmetric out, after every one of 21 updates."""
    m = nets(1)[0]
    K = 21
    Q, R, P0 = jc.full_ekf_matrices(0, MAXN)
    x0, u, z = jc.ekf_inputs(MAXN, K)
    xs, Ps = _ekf_reference(x0, P0, u, z, dt, Q, R)
    worst_x, worst_P, first_x, first_P = 0.0, 0.0, 0.0, 0.0
    for n in jc.SERIES:
        ekf = jp.EKFJetsTotal(m, R, Q, P0[0], dt, n)
        ekf.P = P0[:n].reshape(n, 4).copy()             # (update() works in place)
        T, Td = x0[:n, 0], x0[:n, 1]
        for k in range(K):
            T, Td = ekf.update(T, Td, u[:n], z[k, :n, 0], z[k, :n, 1])
            ex = float((np.abs(np.stack([T, Td], axis=1) - xs[k, :n]) / np.maximum(1.0, np.abs(xs[k, :n]))).max())
            eP = _dev(ekf.P.reshape(n, 2, 2), Ps[k, :n])
            assert ex < jc.BAR_EKF_X_REL and eP < jc.BAR_EKF_P, (n, k, ex, eP)
            worst_x, worst_P = max(worst_x, ex), max(worst_P, eP)
            if k == 0:
                first_x, first_P = max(first_x, ex), max(first_P, eP)
    print(f"EKF, full matrices: one update state {first_x:.2e} rel, P {first_P:.2e}; over {K} updates state {worst_x:.2e} rel, "
          f"P {worst_P:.2e}")
    n = 257
    sym = lambda M: 0.5 * (M + np.swapaxes(M, -1, -2))
    Qs, Rs, Psym = sym(Q), sym(R), sym(P0[:n])
    ekf = jp.EKFJetsTotal(m, Rs, Qs, Psym[0], dt, n)
    ekf.P = Psym.reshape(n, 4).copy()
    xr, Pr = _ekf_reference(x0[:n], Psym, u[:n], z[:, :n], dt, Qs, Rs)
    T, Td = x0[:n, 0], x0[:n, 1]
    asym, eP, ex = 0.0, 0.0, 0.0
    for k in range(K):                                       # symmetric after every one of the 21 updates, not only the first
        T, Td = ekf.update(T, Td, u[:n], z[k, :n, 0], z[k, :n, 1])
        Pd = ekf.P.reshape(n, 2, 2)
        asym = max(asym, float(np.abs(Pd[:, 0, 1] - Pd[:, 1, 0]).max()))
        eP = max(eP, _dev(Pd, Pr[k]))
        ex = max(ex, float((np.abs(np.stack([T, Td], axis=1) - xr[k]) / np.maximum(1.0, np.abs(xr[k]))).max()))
    print(f"symmetric P, Q, R in, {K} updates: |P01 - P10| out {asym:.2e}, P against the oracle {eP:.2e}, state {ex:.2e} rel")
    assert asym <= 1e-13 and eP < jc.BAR_EKF_P and ex < jc.BAR_EKF_X_REL


def _check_plant(got, want, tag):
    Tn, xe, Pe, log = got
    Tn_r, xe_r, Pe_r, log_r = want
    fig = (_dev(Tn, Tn_r), _dev(xe, xe_r), _dev(log, log_r), _dev(Pe, Pe_r))
    print(f"{tag}: T_nn {fig[0]:.2e} N, estimate {fig[1]:.2e}, log {fig[2]:.2e}, P {fig[3]:.2e}")
    assert np.isfinite(xe).all() and np.isfinite(Pe).all() and np.isfinite(log).all(), tag
    assert fig[0] < jc.BAR_PLANT_T and fig[1] < jc.BAR_PLANT_X and fig[2] < jc.BAR_PLANT_X and fig[3] < jc.BAR_PLANT_P, tag
    return fig


@pytest.mark.parametrize("steps", (1, 7))
@pytest.mark.parametrize("n", (1, 257))
@pytest.mark.parametrize("H", (37, 128))
def test_plant_schedule_and_held(jp, nets, dt, H, n, steps):
    """jet_plant_kernel with throttle[steps][n] (another value at every step and series) and with a held throttle[n],
    full Q, R and a per-series non-symmetric P0: final thrust, estimate, P and the whole log against the oracle; the two
    runs differ by more than the bars, so the comparison tells them apart."""
    m, w, lstm = nets(H)
    Q, R, _ = jc.full_ekf_matrices(0)
    T0, x0, P0 = jc.plant_inputs(n)
    thr = jc.schedule(steps, n)
    held = jc.schedule(1, n, seed=1)[0]
    plant = jp.JetPlant(m, R, Q, dt)
    got_s = plant.run(T0, x0, P0, thr, steps, log=True)
    got_h = plant.run(T0, x0, P0, held, steps, log=True)
    _check_plant(got_s, jet_ref.plant_run(lstm, T0, x0, P0, thr, steps, dt, Q, R), f"H {H} n {n} steps {steps} schedule")
    _check_plant(got_h, jet_ref.plant_run(lstm, T0, x0, P0, held, steps, dt, Q, R), f"H {H} n {n} steps {steps} held")
    apart = _dev(got_s[3], got_h[3])
    print(f"schedule against held: the logs are {apart:.2e} apart")
    assert apart > jc.BAR_PLANT_X and not np.array_equal(got_s[0], got_h[0])


def test_plant_staging_grows_and_shrinks(jp, dt):
    """d_thr_steps and d_log of one handle through (steps, n) = (3, 257), (7, 257), (2, 63), (7, 513): first use, growth
    at the same n, a smaller call inside the larger buffers, growth again -- every call against the oracle"""
    H = 37
    m, lstm = _fresh(jp, H), jet_ref.JetLSTM(**jc.weights(H))
    Q, R, _ = jc.full_ekf_matrices(0)
    plant = jp.JetPlant(m, R, Q, dt)
    try:
        for seed, (steps, n) in enumerate(((3, 257), (7, 257), (2, 63), (7, 513))):
            T0, x0, P0 = jc.plant_inputs(n, seed)
            thr = jc.schedule(steps, n, seed)
            _check_plant(plant.run(T0, x0, P0, thr, steps, log=True), jet_ref.plant_run(lstm, T0, x0, P0, thr, steps, dt, Q, R),
                         f"steps {steps} n {n}")
    finally:
        m.close()


@pytest.mark.parametrize("n", (257, 1))
def test_plant_device_entry_and_guards(jp, nets, dt, n):
    """vsmpc_jet_plant_run_device on torch tensors, 5 steps with a schedule.  T_nn, x_est, P and the log carry 256 more
    series than are live, filled with a sentinel (the schedule, which is only read, carries 256 valid values more): what
    a thread past n would write lands in memory the test owns and is seen.  The live part has the bits of the host
    entry's result, no sentinel has moved, and log = NULL gives the same state."""
    import torch
    m = nets(65)[0]
    steps, PAD, SENT = 5, 256, -777.25
    Q, R, _ = jc.full_ekf_matrices(0)
    Qc, Rc = np.ascontiguousarray(Q).reshape(4), np.ascontiguousarray(R).reshape(4)
    T0, x0, P0 = jc.plant_inputs(n)
    thr = jc.schedule(steps, n)
    Tn_h, xe_h, Pe_h, log_h = jp.JetPlant(m, R, Q, dt).run(T0, x0, P0, thr, steps, log=True)
    dev = torch.device("cuda:0")

    def padded(live, per_series, dtype, fill=SENT):
        t = torch.full((live.size + PAD * per_series,), fill, dtype=dtype, device=dev)
        t[:live.size] = torch.from_numpy(np.ascontiguousarray(live).reshape(-1)).to(dev)
        return t

    d_thr = padded(thr, 1, torch.float32, fill=50.0)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for with_log in (True, False):
        d_T, d_x, d_P = padded(T0, 1, torch.float32), padded(x0, 2, torch.float64), padded(P0, 4, torch.float64)
        d_log = torch.full((steps * n * 2 + PAD * 2,), SENT, dtype=torch.float64, device=dev)
        assert d_T.numel() == n + PAD and d_x.numel() == 2 * (n + PAD) and d_P.numel() == 4 * (n + PAD)
        rc = m.lib.vsmpc_jet_plant_run_device(m._h, d_T.data_ptr(), d_x.data_ptr(), d_P.data_ptr(), d_thr.data_ptr(), steps, n,
                                              steps, dt, _p(Qc), _p(Rc), d_log.data_ptr() if with_log else None, stream)
        assert rc == OK
        torch.cuda.synchronize()
        T, x, P, log = d_T.cpu().numpy(), d_x.cpu().numpy(), d_P.cpu().numpy(), d_log.cpu().numpy()
        assert np.array_equal(T[:n], Tn_h) and np.array_equal(x[:2 * n], xe_h.reshape(-1))
        assert np.array_equal(P[:4 * n], Pe_h.reshape(-1))
        assert (T[n:] == SENT).all() and (x[2 * n:] == SENT).all() and (P[4 * n:] == SENT).all()
        if with_log:
            assert np.array_equal(log[:steps * n * 2], log_h.reshape(-1)) and (log[steps * n * 2:] == SENT).all()
        else:
            assert (log == SENT).all()
    print(f"device entry, n {n}: state, P and log bit-equal to the host entry's, {PAD} sentinel series behind each untouched")


def test_contracts(jp, dt):
    """What include/vsmpc_jet.h says about n = 0, steps = 0 and refused arguments, and that a refusal leaves the handle
    in working order."""
    H, n = 37, 5
    w = jc.weights(H)
    m, lstm = jp.JetModelTotal(**w, device=0, max_series=8), jet_ref.JetLSTM(**w)
    lib = m.lib
    Q, R, _ = jc.full_ekf_matrices(0)
    Qc, Rc = np.ascontiguousarray(Q).reshape(4), np.ascontiguousarray(R).reshape(4)
    thrust, throttle = jc.step_inputs(n)
    T0, x0, P0 = jc.plant_inputs(n)
    thr = jc.schedule(3, n)
    plant = jp.JetPlant(m, R, Q, dt)
    first = list(m.get_state(thrust, throttle, DTF)) + list(plant.run(T0, x0, P0, thr, 3, log=True))
    Tn_r, Td_r, _, _ = lstm.get_state(thrust, throttle, DTF)
    assert _dev(first[0], Tn_r) < jc.BAR_TNEXT and _dev(first[1], Td_r) / np.abs(Td_r).max() < jc.BAR_TDOT_REL
    _check_plant(first[2:], jet_ref.plant_run(lstm, T0, x0, P0, thr, 3, dt, Q, R), "before any refusal")
    checks = [0]

    def still_right():
        again = list(m.get_state(thrust, throttle, DTF)) + list(plant.run(T0, x0, P0, thr, 3, log=True))
        assert all(np.array_equal(a, b) for a, b in zip(again, first))
        checks[0] += 1

    SENT = -777.25
    f32 = lambda k: np.full(k, SENT, np.float32)
    f64 = lambda k: np.full(k, SENT, np.float64)
    untouched = lambda *arrays: all((a == SENT).all() for a in arrays)
    big = 9                                                     # max_series + 1
    try:
        # n = 0 and steps = 0: OK, nothing written
        a, b, c, d = f32(8), f32(8), f32(8 * H), f32(8 * H)
        assert lib.vsmpc_jet_nn_step(m._h, _p(thrust), _p(throttle), 0, DTF, _p(a), _p(b), _p(c), _p(d)) == OK and untouched(a, b, c, d)
        xs = jc.sequences(big, 2)
        assert lib.vsmpc_jet_nn_sequence(m._h, _p(xs), 0, 2, DTF, _p(a), _p(b), _p(c), _p(d)) == OK and untouched(a, b, c, d)
        ex, eP, eu, ez = f64(16), f64(32), f64(8), f64(16)
        assert lib.vsmpc_jet_ekf_update(m._h, _p(ex), _p(eP), _p(eu), _p(ez), 0, dt, _p(Qc), _p(Rc)) == OK and untouched(ex, eP)
        pT, plog = f32(8), f64(3 * 8 * 2)
        for nn, steps in ((0, 3), (n, 0), (0, 0)):
            assert lib.vsmpc_jet_plant_run(m._h, _p(pT), _p(ex), _p(eP), _p(thr), steps or 1, nn, steps, dt,
                                           _p(Qc), _p(Rc), _p(plog)) == OK
            assert untouched(pT, ex, eP, plog), (nn, steps)
        still_right()
        # more series than the handle was created for
        tb, ub = np.full(big, 100.0, np.float32), np.full(big, 50.0, np.float32)
        ob, oc = f32(big), f32(big)
        assert lib.vsmpc_jet_nn_step(m._h, _p(tb), _p(ub), big, DTF, _p(ob), _p(oc), None, None) == ERR_BATCH_TOO_LARGE
        still_right()
        assert lib.vsmpc_jet_nn_sequence(m._h, _p(xs), big, 2, DTF, _p(ob), _p(oc), None, None) == ERR_BATCH_TOO_LARGE
        still_right()
        bx, bP, bu, bz = f64(2 * big), f64(4 * big), f64(big), f64(2 * big)
        assert lib.vsmpc_jet_ekf_update(m._h, _p(bx), _p(bP), _p(bu), _p(bz), big, dt, _p(Qc), _p(Rc)) == ERR_BATCH_TOO_LARGE
        still_right()
        assert lib.vsmpc_jet_plant_run(m._h, _p(ob), _p(bx), _p(bP), _p(ub), 1, big, 3, dt, _p(Qc), _p(Rc), None) == ERR_BATCH_TOO_LARGE
        assert untouched(ob, oc, bx, bP)
        still_right()
        # a schedule that is neither held nor one row per step, on both entries (refused before any pointer is used)
        import torch
        dev = torch.device("cuda:0")
        thr4 = jc.schedule(4, n)
        T1, x1, P1 = T0.copy(), x0.copy(), P0.reshape(n, 4).copy()
        d_T, d_x, d_P, d_thr = (torch.from_numpy(v).to(dev) for v in (T1, x1, P1, thr4))    # the device entry gets device memory
        dptr = (d_T.data_ptr(), d_x.data_ptr(), d_P.data_ptr(), d_thr.data_ptr())
        for tsteps in (2, 4, 0, -1):
            assert lib.vsmpc_jet_plant_run(m._h, _p(T1), _p(x1), _p(P1), _p(thr4), tsteps, n, 3, dt, _p(Qc), _p(Rc), None) == ERR_INVALID_ARG
            assert lib.vsmpc_jet_plant_run_device(m._h, *dptr, tsteps, n, 3, dt, _p(Qc), _p(Rc), None, None) == ERR_INVALID_ARG
            still_right()
        # n = 0 and steps = 0 on the device entry: OK, nothing enqueued that writes
        for nn, steps in ((0, 3), (n, 0), (0, 0)):
            assert lib.vsmpc_jet_plant_run_device(m._h, *dptr, steps or 1, nn, steps, dt, _p(Qc), _p(Rc), None, None) == OK
        still_right()
        # dt <= 0 (and not a number)
        for bad in (0.0, -dt, float("nan")):
            assert lib.vsmpc_jet_plant_run(m._h, _p(T1), _p(x1), _p(P1), _p(thr), 3, n, 3, bad, _p(Qc), _p(Rc), None) == ERR_INVALID_ARG
            assert lib.vsmpc_jet_plant_run_device(m._h, *dptr, 3, n, 3, bad, _p(Qc), _p(Rc), None, None) == ERR_INVALID_ARG
            xe, ze = x0.copy(), x0.copy()
            assert lib.vsmpc_jet_ekf_update(m._h, _p(xe), _p(P1), _p(bu), _p(ze), n, bad, _p(Qc), _p(Rc)) == ERR_INVALID_ARG
            assert np.array_equal(xe, x0)
            still_right()
        torch.cuda.synchronize()
        assert np.array_equal(d_T.cpu().numpy(), T0) and np.array_equal(d_x.cpu().numpy(), x0)
        assert np.array_equal(T1, T0) and np.array_equal(x1, x0) and np.array_equal(P1, P0.reshape(n, 4))
        # L <= 0
        for L in (0, -1):
            assert lib.vsmpc_jet_nn_sequence(m._h, _p(xs), n, L, DTF, _p(a), _p(b), None, None) == ERR_INVALID_ARG
            still_right()
        assert untouched(a, b)
        # a NULL pointer that is not optional, a negative count
        assert lib.vsmpc_jet_nn_step(m._h, None, _p(throttle), n, DTF, _p(a), _p(b), None, None) == ERR_INVALID_ARG
        assert lib.vsmpc_jet_nn_step(m._h, _p(thrust), _p(throttle), -1, DTF, _p(a), _p(b), None, None) == ERR_INVALID_ARG
        assert lib.vsmpc_jet_ekf_update(m._h, _p(xe), _p(P1), _p(bu), _p(ze), n, dt, None, _p(Rc)) == ERR_INVALID_ARG
        assert lib.vsmpc_jet_plant_run(m._h, _p(T1), _p(x1), _p(P1), _p(thr), 3, n, 3, dt, _p(Qc), None, None) == ERR_INVALID_ARG
        assert lib.vsmpc_jet_plant_run(m._h, _p(T1), _p(x1), _p(P1), _p(thr), 3, n, -3, dt, _p(Qc), _p(Rc), None) == ERR_INVALID_ARG
        assert untouched(a, b) and np.array_equal(T1, T0) and np.array_equal(xe, x0)
        still_right()
        # create: hidden outside 1..128, a standard deviation that is not positive
        f = lambda k: np.ascontiguousarray(w[k], dtype=np.float32)
        args = [_p(f(k)) for k in ("w_ih", "w_hh", "b_ih", "b_hh", "fc_w", "fc_b")]
        norm = np.ascontiguousarray(w["norm"], dtype=np.float64)
        for hidden in (0, 129, -1):
            h = ctypes.c_void_p(1)
            assert lib.vsmpc_jet_create(*args, _p(norm), hidden, 0, 8, ctypes.byref(h)) == ERR_INVALID_ARG and not h
            still_right()
        for k, v in ((1, 0.0), (1, -1.0), (3, 0.0), (3, -2.5), (1, float("nan"))):
            bad_norm = norm.copy()
            bad_norm[k] = v
            h = ctypes.c_void_p(1)
            assert lib.vsmpc_jet_create(*args, _p(bad_norm), H, 0, 8, ctypes.byref(h)) == ERR_INVALID_ARG and not h
            still_right()
        print(f"contracts: the handle gave the bits of its first answer after each of {checks[0]} groups of refused / empty calls")
    finally:
        m.close()


@pytest.mark.parametrize("H", (37, 64, 65, 128))
def test_rollout_jet_plant_other_networks(solver_mod, layout, H):
    """vsmpc_rollout_set_jet_plant (lstm_step_from_zero_wave: hidden units strided over a wavefront, one partial pass, one
    exact pass, one unit into the second pass, two passes; the issue lists 37, 64, 128, 65 is added) with full Q, R and a non-symmetric covariance per jet in the start state: records and plant
    states of 4 Monte-Carlo loops over 3 ticks against tests/rollout_model.py, at the 2e-6 of
    test_gpu_rollout.test_jet_plant_option_matches_model.  Whatever status the solves return: the model applies the
    device's first move under the device's status, and a random network is not a jet."""
    ro = importlib.import_module(PKG + ".rollout")
    jpm = importlib.import_module(PKG + ".jet_plant")
    w = jc.weights(H)
    jm = jpm.JetModelTotal(**w, device=0, max_series=64)
    lstm = jet_ref.JetLSTM(**w)
    B = 4
    Q, Rm, P0 = jc.full_ekf_matrices(H, 4 * B)
    cfg = layout.paper_config()
    st, pa = ro.make_plant(cfg, B, workload="montecarlo")
    st[:, layout.PS_EKFP:layout.PS_EKFP + 16] = P0.reshape(B, 16)
    pos, vel, alpha, adt = ro.make_trajectory(cfg, "hover", 60.0)
    r = ro.ClosedLoopRollout(cfg, B, pos, vel, alpha, adt, device=0)
    worst_rec, worst_state = 0.0, 0.0
    try:
        r.set_jet_plant(jm, Q, Rm)
        r.reset(st, pa)
        jet = (lstm, Q, Rm)
        s_host = st.copy()
        models = [rm.make_tick_model(cfg, rm.measured(st[b], jet), pa[b], pos, vel, alpha) for b in range(B)]
        recs = r.next_records()
        for tick in range(3):
            r.run(1, log=False)
            x, fm, status, iters = r.mpc.solve(recs)
            after = r.state()
            for b in range(B):
                rec_m = rm.build_record(cfg, models[b], rm.measured(s_host[b], jet), pa[b])
                models[b].consume(fm[b], status[b])
                s_m = rm.advance(cfg, s_host[b], pa[b], tick, fm[b], status[b], alpha, adt, jet=jet)
                worst_rec, worst_state = max(worst_rec, relerr(recs[b], rec_m)), max(worst_state, relerr(after[b], s_m))
                assert relerr(recs[b], rec_m) < jc.BAR_ROLLOUT, (tick, b)
                assert relerr(after[b], s_m) < jc.BAR_ROLLOUT, (tick, b)
            moved = np.abs(after[:, layout.PS_TNN:layout.PS_TNN + 4] - s_host[:, layout.PS_TNN:layout.PS_TNN + 4]).max()
            assert moved > 0.0                                 # the network really drives the thrust
            recs = r.next_records()
            s_host = after
        print(f"rollout, H {H}: records {worst_rec:.2e}, plant state {worst_state:.2e} relative; status {status.tolist()}")
    finally:
        r.close()
        jm.close()
