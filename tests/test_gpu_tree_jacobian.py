"""vsmpc_tree_jacobian_batch[_device] on the device (tree_jacobian_kernel): the terms the kinematic-tree plant hands a tick
and their Jacobian to (q | T).

  terms   against the existing route on the device (provider_batch at the body-frame pose -> kinematics_batch) and against the
          oracle (robot_tree_ref.forward -> vsmpc_ref.kinematics_terms), under test_provider_matches_oracle's bar: relerr
          (conftest) below 1e-14 for A_mom,body and 1e-13 for the record-derived blocks.  Measured on an MI355X: 8.6e-16 against the route, 5.5e-16 against the oracle.
  jac     against tests/tree_jacobian_model.py (itself held to central differences in test_tree_jacobian_model.py), under the
          project's parity bar of 1e-8 of each block's largest entry.  Measured worst on an MI355X: 7.0e-16.
  Batches of 1, 5 and 257 (more workgroups than one, a last workgroup that is not full), every row bit-identical to the same
  instance in a batch of 4; the `_device` entry between sentinel rows; terms only and jac only; the default tree and a chain
  of eight; a joint selector that is not the default; the refusal under jointsLambdaOption "constant"; NULL tree, q or thrust,
  a batch <= 0 and invalid trees with a live handle."""
import importlib

import numpy as np
import pytest

import robot_tree_ref as rt
import tree_jacobian_model as tj
from conftest import PKG, relerr

pytestmark = pytest.mark.gpu

SELECTOR = (10, 3, 5, 4, 9, 8, 7, 6)
PARITY = 1e-8
N = 257


@pytest.fixture(scope="module")
def RT(solver_mod):
    return importlib.import_module(PKG + ".robot_tree")


@pytest.fixture(scope="module")
def mpc(solver_mod, layout):
    m = solver_mod.BatchedVSMPC(layout.paper_config(), device=0, max_batch=N)
    yield m
    m.close()


def _inputs(n=N, seed=5):
    rng = np.random.default_rng(seed)
    q = rng.uniform(-1.2, 1.2, (n, 8))
    q[0] = 0.0
    return q, rng.uniform(90.0, 160.0, (n, 4))


@pytest.fixture(scope="module")
def reference(RT):
    """the model's (terms, jac) of the first 12 instances, per tree and selector: computed once"""
    q, T = _inputs()
    out = {}
    for name, tree in (("default", RT.default_tree()), ("chain", tj.chain_tree())):
        for sel in (None, SELECTOR):
            out[name, sel] = [tj.jacobian(tree, q[b], T[b], sel) for b in range(12)]
    return out


@pytest.mark.parametrize("name", ["default", "chain"])
def test_terms_and_jacobian(mpc, RT, layout, ref, reference, name):
    tree = RT.default_tree() if name == "default" else tj.chain_tree()
    q, T = _inputs()
    terms, jac = mpc.tree_jacobian(tree, q, T)
    assert terms.shape == (N, layout.TT_SIZE) and jac.shape == (N, layout.TT_SIZE, layout.TT_NDIR)
    # the existing route on the device, at the pose the rollout evaluates it at
    states = np.stack([RT.pack_state(np.zeros(3), np.eye(3), np.zeros(3), np.zeros(3), q[b], np.zeros(8), T[b]) for b in range(N)])
    kin, robot = mpc.provider(tree, states)
    llin, lang, ib = mpc.kinematics(kin)
    route = np.concatenate([robot[:, RT.RO_AMOMB:RT.RO_AMOMB + 24], llin.reshape(N, -1), lang.reshape(N, -1), ib.reshape(N, -1)], axis=1)
    worst = {}
    for block, lo, hi in tj.BLOCKS:
        bar = 1e-14 if block == "A_mom" else 1e-13
        e_route = max(relerr(terms[b, lo:hi], route[b, lo:hi]) for b in range(N))
        e_oracle = max(relerr(terms[b, lo:hi], tj.oracle_terms(tree, q[b], T[b])[lo:hi]) for b in range(12))
        worst[block] = (e_route, e_oracle)
        assert e_route < bar and e_oracle < bar, (name, block, e_route, e_oracle)
    print(f"{name}: terms against the device route / the oracle (relerr): {worst}")
    errs = {}
    for block, lo, hi in tj.BLOCKS:
        errs[block] = max(np.abs(jac[b, lo:hi] - J[lo:hi]).max() / np.abs(J[lo:hi]).max() for b, (_, J) in enumerate(reference[name, None]))
        assert errs[block] <= PARITY, (name, block, errs[block])
    print(f"{name}: Jacobian against the model, of each block's largest entry: {errs}")
    assert (jac[:, :24, 8:] == 0.0).all() and (jac[:, 72:, 8:] == 0.0).all() and not np.signbit(jac[:, :24, 8:]).any()
    assert np.linalg.matrix_rank(jac[3, :, :8]) == 8


def test_batches_are_bit_identical(mpc, RT):
    tree = RT.default_tree()
    q, T = _inputs()
    terms, jac = mpc.tree_jacobian(tree, q, T)
    for n in (1, 4, 5):
        for first in (0, 7):
            t, j = mpc.tree_jacobian(tree, q[first:first + n], T[first:first + n])
            assert np.array_equal(t, terms[first:first + n]) and np.array_equal(j, jac[first:first + n]), (n, first)
    t, j = mpc.tree_jacobian(tree, q[::-1], T[::-1])                   # every instance in another lane group and workgroup
    assert np.array_equal(t[::-1], terms) and np.array_equal(j[::-1], jac)


def test_null_outputs_and_the_device_entry(mpc, RT, layout):
    import torch
    tree = RT.default_tree()
    q, T = _inputs(9)
    terms, jac = mpc.tree_jacobian(tree, q, T)
    t_only, none = mpc.tree_jacobian(tree, q, T, jac=False)
    none2, j_only = mpc.tree_jacobian(tree, q, T, terms=False)
    assert none is None and none2 is None and np.array_equal(t_only, terms) and np.array_equal(j_only, jac)
    dev = "cuda"
    dq, dT = torch.tensor(q, device=dev), torch.tensor(T, device=dev)
    SENT = -777.0
    dt = torch.full((9 + 2, layout.TT_SIZE), SENT, dtype=torch.float64, device=dev)
    dj = torch.full((9 + 2, layout.TT_SIZE, layout.TT_NDIR), SENT, dtype=torch.float64, device=dev)
    mpc.tree_jacobian_device(tree, dq, dT, dt[1:10], dj[1:10])
    torch.cuda.synchronize()
    assert np.array_equal(dt[1:10].cpu().numpy(), terms) and np.array_equal(dj[1:10].cpu().numpy(), jac)
    for buf in (dt, dj):
        assert (buf[0] == SENT).all() and (buf[10] == SENT).all()
    dj.fill_(SENT)
    mpc.tree_jacobian_device(tree, dq, dT, None, dj[1:10])
    torch.cuda.synchronize()
    assert np.array_equal(dj[1:10].cpu().numpy(), jac) and (dj[0] == SENT).all() and (dj[10] == SENT).all()


def test_selector_and_constant_lambda(mpc, RT, reference):
    tree = tj.chain_tree()
    q, T = _inputs()
    base_terms, _ = mpc.tree_jacobian(tree, q[:12], T[:12])
    try:
        mpc.set_kinematics_options(SELECTOR)
        terms, jac = mpc.tree_jacobian(tree, q[:12], T[:12])
        for b, (t, J) in enumerate(reference["chain", SELECTOR]):
            for block, lo, hi in tj.BLOCKS:
                assert relerr(terms[b, lo:hi], t[lo:hi]) < 1e-13, (b, block)
                assert np.abs(jac[b, lo:hi] - J[lo:hi]).max() <= PARITY * np.abs(J[lo:hi]).max(), (b, block)
        assert np.array_equal(terms[:, :48], base_terms[:, :48]) and np.array_equal(terms[:, 72:], base_terms[:, 72:])
        assert not np.array_equal(terms[:, 48:72], base_terms[:, 48:72])          # Lambda_ang alone reads the selector
        mpc.set_kinematics_options(None, constant_lambda=True)
        with pytest.raises(Exception, match="(?i)unsupported|not supported"):
            mpc.tree_jacobian(tree, q[:2], T[:2])
    finally:
        mpc.set_kinematics_options(range(3, 11), constant_lambda=False)
    again, _ = mpc.tree_jacobian(tree, q[:12], T[:12])
    assert np.array_equal(again, base_terms)


def test_refusals_with_a_live_handle(mpc, RT):
    """NULL tree, q or thrust, a batch <= 0 and an invalid tree: VSMPC_ERR_INVALID_ARG from both entries, outputs untouched"""
    import ctypes
    q, T = _inputs(2)
    terms, jac = np.full((2, 81), -7.0), np.full((2, 81, 12), -7.0)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    good = RT.to_c(RT.default_tree())
    bad_parent, bad_jet, bad_joint = RT.default_tree(), RT.default_tree(), RT.default_tree()
    bad_parent["parent"] = [-1, 0, 3, 2, 3, 0, 5, 6, 7]          # a parent behind its child
    bad_jet["jet_body"] = [4, 9, 0, 0]
    bad_joint["robot_joint"] = [3, 4, 5, 6, 7, 8, 9, 23]
    for fn, tail in ((mpc.lib.vsmpc_tree_jacobian_batch, ()), (mpc.lib.vsmpc_tree_jacobian_batch_device, (None,))):
        h, t = mpc._h, ctypes.byref(good)
        assert fn(h, None, p(q), p(T), 2, p(terms), p(jac), *tail) == -1
        assert fn(h, t, None, p(T), 2, p(terms), p(jac), *tail) == -1
        assert fn(h, t, p(q), None, 2, p(terms), p(jac), *tail) == -1
        assert fn(h, t, p(q), p(T), 0, p(terms), p(jac), *tail) == -1
        assert fn(h, t, p(q), p(T), -2, p(terms), p(jac), *tail) == -1
        for bad in (bad_parent, bad_jet, bad_joint):
            assert fn(h, ctypes.byref(RT.to_c(bad)), p(q), p(T), 2, p(terms), p(jac), *tail) == -1
    assert (terms == -7.0).all() and (jac == -7.0).all()
    assert mpc.lib.vsmpc_strerror(-1) == b"invalid argument"
