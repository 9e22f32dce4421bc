"""The executable model of the rollout adjoint's attitude-track gradients (tests/rollout_attitude_adjoint_model.py) on the CPU:
the numpy sweep against central differences of the forward loop model on the loops of
tests/rollout_attitude_adjoint_cases.py, and planted defects.

Conditions of the cases, asserted first: every tick of every loop but the never-Solved one is Solved and not degenerate, at
(6, 2, 3) and, `base`, at (17, 7, 12); the h_ang reference reaches 1.4; a run of 9 ticks reaches samples 0 .. 3 (the fill holds
samples 0 and 1, the two pushes bring 2 and 3) and a run of 21 ticks 0 .. 6; loop 0 fills from shifted samples; the 3-sample track
puts several slots on one sample; step-halving quotients along random directions of both tracks agree to 1e-7 of the
direction's own scale sum_i |g_i d_i|.

Against central differences, Richardson extrapolated (step STEP times rollout_attitude_adjoint_model.ATT_SCALE): every entry of
both tracks that the run reaches, on every loop of CPU_LOOPS -- for the run that does not begin at a reset with the window of
the earlier ticks held fixed -- and, beside them, the old outputs where the attitude rows reach them: grad_state0 along the
three attitude entries, a random direction in the joints and one in the whole state, grad_params on the nine entries of
INERTIA_B.

Bar.  rollout_param_adjoint_cases.py's rule and constants: |err| <= FD_BAR (|field|_inf + FLOOR_RATIO max |gradient|), FD_BAR
= 9.2e-7.  Measured here on the two new fields, worst of all loops: 3.1e-8 of that scale (loop 0 of `late`, rpy, whose
gradients are the smallest; the other loops lie between 5e-10 and 4.4e-9), the quotients' own step-halving error being 4e-10
and less.  That is within a tenth of FD_BAR, so the bar stays; the test asserts it.  The planted defects miss the bar by the
factors of profiles/rollout_attitude_adjoint_mutations.txt, from 1e4 upwards (the tree's: see there)."""
import numpy as np
import pytest

import rollout_adjoint_model as ram
import rollout_attitude_adjoint_cases as ac
import rollout_attitude_adjoint_model as atm

L = ac.L
STEP = 1e-2
FLOOR_RATIO, FD_BAR, FD_FLOOR = ac.FLOOR_RATIO, ac.FD_BAR, ac.FD_FLOOR
MUTATION_MISS = 10.0                   # a planted defect misses the bar by at least this factor on some loop
HALVING = 1e-7
STATE_FIELDS = (("state directions", 0, 5),)
IB_FIELDS = (("INERTIA_B", 0, 9),)
ids = lambda k: f"{k[0]}-{k[1]}"


def all_keys():
    keys = [(c, b) for c in ac.PARAMETRIC for b in range(ac.B)] + [("tree", 0)]
    return keys + [("unsolved", b) for b in range(ac.B) if b != ac.UNSOLVED_LOOP]


def state_directions():
    rng = np.random.default_rng(ac.rc.SEED + 53)
    d = np.zeros((5, ram.NS))
    d[0, 6], d[1, 7], d[2, 8] = 1e-2, 1e-2, 1e-2
    d[3, L.PS_Q:L.PS_Q + 8] = rng.normal(size=8) * 1e-2            # the joints alone: where the tree's I_B share arrives
    d[4] = rng.normal(size=ram.NS) * ram.state_scale() * 1e-2
    return d


def central_gradients(ref, key):
    """(grad_att row with the reached samples filled, the 5 state directions, the 9 entries of INERTIA_B or None) of one loop
    by Richardson-extrapolated central differences"""
    n = ac.n_traj_of(key[0])
    rs = ac.reached(ref, key)
    g = {"rpy": np.zeros((n, 3)), "rpy_dot": np.zeros((n, 3))}
    for name in g:
        for k in np.nonzero(rs)[0]:
            for c in range(3):
                d = np.zeros((n, 3))
                d[k, c] = 1.0
                g[name][k, c] = ac.central(ref, key, **{"d_" + name: d}, step=STEP * atm.ATT_SCALE[name])
    gs = gib = None
    if ac.ticks_before(key[0]) == 0:
        gs = np.array([ac.central(ref, key, d_state=d, step=STEP) for d in state_directions()])
        if key[0] != "tree":
            gib = np.zeros(9)
            for i in range(9):
                d = np.zeros(atm.NP)
                d[L.PP_INERTIA_B + i] = 1.0
                gib[i] = ac.central(ref, key, d_params=d, step=STEP * 1e-1)
    return np.concatenate([g["rpy"].reshape(-1), g["rpy_dot"].reshape(-1)]), gs, gib


@pytest.fixture(scope="module")
def central(ref):
    return {key: central_gradients(ref, key) for key in ac.CPU_LOOPS}


def errors(out, fd, n_traj):
    """(the worst error of the two new track fields, of the old outputs) of a sweep in units of the bar, and where"""
    row, gs, gib = fd
    new = ram.field_errors(ac.att_row(out), row, ac.att_fields(n_traj), FD_BAR, FD_FLOOR)
    old = [(0.0, None)]
    if gs is not None:
        old.append(ram.field_errors(state_directions() @ out["grad_state0"], gs, STATE_FIELDS, FD_BAR, FD_FLOOR))
    if gib is not None:
        old.append(ram.field_errors(out["grad_params"][L.PP_INERTIA_B:L.PP_INERTIA_B + 9], gib, IB_FIELDS, FD_BAR, FD_FLOOR))
    return new, max(old, key=lambda ef: ef[0])


def test_every_tick_is_solved_and_not_degenerate():
    for key in all_keys():
        m = ac.model(key)
        assert (m["log"][:, 14] == L.STATUS_SOLVED).all(), key
        assert m["flags"] == 0 and all(f == 0 for f in m["tick_flags"]), key
    for b in range(ac.B):
        m = ac.model(("base", b), ac.HORIZONS[1])
        assert (m["log"][:, 14] == L.STATUS_SOLVED).all() and m["flags"] == 0, b
    m = ac.model(("unsolved", ac.UNSOLVED_LOOP))
    assert (m["log"][:, 14] != L.STATUS_SOLVED).all()
    for k in ("grad_traj_rpy", "grad_traj_rpy_dot"):
        assert (m[k] == 0.0).all() and not np.signbit(m[k]).any(), k


def test_cases_cross_what_they_are_meant_to(ref):
    cfg, _, p, traj, att, _, _ = ac.loop_inputs(ref, ("base", 3))
    nref = cfg.n_ref_cols
    hang = max(np.linalg.norm(rec[ref.IN_XREF:ref.IN_XREF + 12 * nref].reshape(nref, 12)[:, 9:12], axis=1).max()
               for key in (("base", b) for b in range(ac.B)) for _, rec, _, _ in ac.model(key)["tape"])
    print(f"largest |h_ang reference| of a window column (Euclidean): {hang:.3f}")
    assert hang >= 1.4
    assert np.array_equal(np.nonzero(ac.reached(ref, ("base", 3)))[0], np.arange(4))
    assert np.array_equal(np.nonzero(atm.reached(cfg, p, len(traj[0]), 21))[0], np.arange(7))
    assert ac.loop_inputs(ref, ("base", 0))[2][L.PP_TICK0] == 2.0
    assert tuple(ac.loop_inputs(ref, ("base", ac.TILTED))[1][L.PS_RPY:L.PS_RPY + 3]) == ac.TILT
    # the 3-sample track: the fill and the second push both sit on samples other slots hold too
    assert len(ac.trajectory("short3")[0]) == 3 and ac.reached(ref, ("short3", 0)).all()
    # no fill in a run that does not begin at a reset: the pushes of ticks 3, 7, 11 alone
    assert np.array_equal(np.nonzero(ac.reached(ref, ("late", ac.TILTED)))[0], [2, 3, 4])
    assert ac.attitude_tracks("null_rpyd")[1] is None
    ib = ac.plants("offdiag")[1][ac.TILTED, L.PP_INERTIA_B:L.PP_INERTIA_B + 9]
    assert len(set(ib)) == 9 and not np.allclose(ib.reshape(3, 3), ib.reshape(3, 3).T)


def test_step_halving_quotients_agree(ref):
    rng = np.random.default_rng(ac.rc.SEED + 59)
    for key in (("base", 0), ("base", 3)):
        m = ac.model(key)
        rs = ac.reached(ref, key)
        for name in ("rpy", "rpy_dot"):
            d = np.zeros((ac.n_traj_of(key[0]), 3))
            d[rs] = rng.normal(size=(rs.sum(), 3))
            _, q1, q2 = ac.central(ref, key, **{"d_" + name: d}, step=STEP * atm.ATT_SCALE[name], both_steps=True)
            scale = np.abs(m["grad_traj_" + name] * d).sum()
            print(f"{key} {name}: step-halving {abs(q1 - q2) / scale:.2e} of sum |g d|")
            assert abs(q1 - q2) <= HALVING * scale, (key, name)


@pytest.mark.parametrize("key", ac.CPU_LOOPS, ids=ids)
def test_sweep_matches_central_differences(central, key):
    (e, f), (eo, fo) = errors(ac.model(key), central[key], ac.n_traj_of(key[0]))
    print(f"loop {key}: tracks {e:.2e} of the bar ({f}) = {e * FD_BAR:.2e} of |field|_inf + {FLOOR_RATIO} max |gradient|; "
          f"old outputs {eo:.2e} of the bar ({fo})")
    assert e <= 1.0 and eo <= 1.0, (key, e, f, eo, fo)
    assert e * FD_BAR <= 0.1 * FD_BAR                               # the model's own error leaves the bar where it was


def test_every_field_is_above_the_floor_and_zero_where_unreached(ref):
    for key in ac.CPU_LOOPS:
        m = ac.model(key)
        row = ac.att_row(m)
        for name, off, n in ac.att_fields(ac.n_traj_of(key[0])):
            assert np.abs(row[off:off + n]).max() > FLOOR_RATIO * np.abs(row).max(), (key, name)
        rs = ac.reached(ref, key)
        for g in (m["grad_traj_rpy"][~rs], m["grad_traj_rpy_dot"][~rs]):
            assert (g == 0.0).all() and not np.signbit(g).any(), key
    z = ac.model(("null_rpyd", ac.TILTED))["grad_traj_rpy_dot"]
    assert np.abs(z).max() > 1.0                                      # W^T R I_B^T R^T w at the zero track is not zero


@pytest.mark.parametrize("mutation", atm.MUTATIONS)
def test_planted_defects_miss_the_bar(ref, central, mutation):
    worst, where = 0.0, None
    for key in ac.CPU_LOOPS:
        if (mutation in atm.TREE_MUTATIONS) != (key[0] == "tree"):
            continue
        (e, f), (eo, fo) = errors(ac.sweep(ref, key, mutation=mutation, tape=ac.model(key)["tape"]), central[key], ac.n_traj_of(key[0]))
        if max(e, eo) > worst:
            worst, where = max(e, eo), (key, f if e >= eo else fo)
    print(f"{mutation}: misses the bar by {worst:.3g} ({where})")
    assert worst >= MUTATION_MISS, (mutation, worst, where)
