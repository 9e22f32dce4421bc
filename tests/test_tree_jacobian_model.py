"""The numpy Jacobian of the kinematic-tree plant's terms (tests/tree_jacobian_model.py) against Richardson-extrapolated
central differences of rollout_model.tree_terms itself -- the oracle's route, robot_tree_ref.forward ->
vsmpc_ref.kinematics_terms -- entry by entry, on the default tree at q = 0 and at joints drawn up to +-1.2 rad, on a chain of
eight with jets on three different bodies, and under a joint selector that is not the default.

Bar.  The reference is the central difference with steps h and h / 2 extrapolated to O(h^4); its own error is measured as the
difference between that and the same with h / 2 and h / 4.  A block of the Jacobian -- A_mom, Lambda, I_B, whose entries
differ by three decades (|dA/dq| ~ 0.9, |dLambda/dq| ~ 1e2, |dI_B/dq| ~ 0.25), so each is judged against its own largest
entry -- may differ from the reference by ten times that.  Measured over the cases below: the reference's own error is
2.1e-13 .. 2.4e-12 of the block's largest entry for A_mom and Lambda and 4.7e-12 .. 2.3e-11 for I_B, the model's distance from
it 1.8e-13 .. 1.7e-11 (I_B, default tree at q = 0); the bars are therefore 2.1e-12 .. 2.3e-10 of the block's largest entry, case
by case (the test prints all three figures for every case and block)."""
import importlib

import numpy as np
import pytest

import rollout_model as pm
import tree_jacobian_model as tj

RT = importlib.import_module(tj.PKG + ".robot_tree")
H = 1e-3
SELECTOR = (10, 3, 5, 4, 9, 8, 7, 6)
CASES = {
    "default_q0": ("default", "zero", None),
    "default_posed": ("default", "drawn", None),
    "chain_posed": ("chain", "drawn", None),
    "default_selector": ("default", "drawn", SELECTOR),
    "chain_selector": ("chain", "drawn", SELECTOR),
}


def _case(name):
    which, pose, sel = CASES[name]
    tree = RT.default_tree() if which == "default" else tj.chain_tree()
    rng = np.random.default_rng(sorted(CASES).index(name) + 11)
    q = np.zeros(8) if pose == "zero" else rng.uniform(-1.2, 1.2, 8)
    T = rng.uniform(90.0, 160.0, 4)
    return tree, q, T, sel


def _oracle(tree, sel):
    """x [12] -> terms [81] by the forward model's own function where it can serve (the default selector)"""
    if sel is not None:
        return lambda x: tj.oracle_terms(tree, x[:8], x[8:], sel)

    def f(x):
        pm.set_tree(tree)
        try:
            a, lam, ib = pm.tree_terms(x[:8], x[8:])
        finally:
            pm.set_tree(None)
        return np.concatenate([a.reshape(-1), lam.reshape(-1), ib.reshape(-1)])
    return f


def _richardson(f, x, h):
    def cd(step):
        return np.stack([(f(x + step * e) - f(x - step * e)) / (2.0 * step) for e in np.eye(tj.TT_NDIR)], axis=1)
    return (4.0 * cd(0.5 * h) - cd(h)) / 3.0


def test_the_chain_is_another_valid_tree():
    t, d = tj.chain_tree(), RT.default_tree()
    assert t["parent"] != d["parent"] and all(0 <= t["parent"][b] < b for b in range(1, 9))
    assert len(set(t["jet_body"])) >= 3 and sorted(t["robot_joint"]) == list(range(3, 11))


@pytest.mark.parametrize("name", sorted(CASES))
def test_terms_are_the_oracles(name):
    tree, q, T, sel = _case(name)
    want = _oracle(tree, sel)(np.concatenate([q, T]))
    got = tj.terms(tree, q, T, sel)
    for block, lo, hi in tj.BLOCKS:
        assert np.abs(got[lo:hi] - want[lo:hi]).max() <= 1e-13 * np.abs(want[lo:hi]).max(), (name, block)


@pytest.mark.parametrize("name", sorted(CASES))
def test_jacobian_matches_central_differences(name):
    tree, q, T, sel = _case(name)
    f, x = _oracle(tree, sel), np.concatenate([q, T])
    ref1, ref2 = _richardson(f, x, H), _richardson(f, x, 0.5 * H)
    _, J = tj.jacobian(tree, q, T, sel)
    for block, lo, hi in tj.BLOCKS:
        scale = np.abs(J[lo:hi]).max()
        own = np.abs(ref1[lo:hi] - ref2[lo:hi]).max() / scale
        err = np.abs(J[lo:hi] - ref2[lo:hi]).max() / scale
        print(f"{name} {block}: largest entry {scale:.3g}, reference's own error {own:.2e}, model against it {err:.2e}, "
              f"bar {10.0 * own:.2e}")
        assert err <= 10.0 * own, (name, block, err, own)
    # Lambda is linear in T, nothing else reads it
    assert (J[tj.TT_AMOM:tj.TT_LLIN, 8:] == 0.0).all() and (J[tj.TT_IB:, 8:] == 0.0).all()
    assert np.abs(J[tj.TT_LLIN:tj.TT_IB, 8:] @ T - tj.terms(tree, q, T, sel)[tj.TT_LLIN:tj.TT_IB]).max() <= 1e-12 * np.abs(J).max()


def test_every_joint_is_seen():
    """all eight joint columns are there and independent: the Jacobian to the joints has rank 8"""
    tree, q, T, _ = _case("default_posed")
    _, J = tj.jacobian(tree, 0.4 * np.sign(q), T)
    assert (np.abs(J[:, :8]).max(axis=0) > 0.1).all() and np.linalg.matrix_rank(J[:, :8]) == 8
    for block, lo, hi in tj.BLOCKS:
        assert np.abs(J[lo:hi, :8]).max() > 0.1, block
