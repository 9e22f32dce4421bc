"""Staging of the host-pointer entries across chunk boundaries: vsmpc_solve_batch and vsmpc_solve_batch_tuned over three
pipelined chunks with a ragged tail (pageable and pinned caller buffers), vsmpc_sensitivity_batch over two chunks.

Each case is compared with the device entry on the same records, on a handle whose max_batch is the batch.  The kernels
are deterministic and independent of the batch position (test_gpu_parity.py:
test_solves_are_deterministic_and_independent_of_batch_position), so the comparison is bit for bit: a wrong row offset
of a chunk's upload, launch or download shows as a different result.  Paper horizon (17, 7, 12), distinct take-off records.
"""
import ctypes

import numpy as np
import pytest

import config_cases as cc

pytestmark = pytest.mark.gpu

PIPE_BATCH = 2 * 1024 + 5      # VS_PIPE_CHUNK = 1024 (csrc): chunks 0 and 2 share a stream, the last one has 5 instances
SENS_BATCH = 256 + 3           # SENS_CHUNK = 256 (csrc): the second chunk reuses the chunk-local staging at offset 0
_cache = {}


def records(synth, layout, n):
    if n not in _cache:
        recs = synth.make_batch(layout.paper_config(), n, workload="takeoff")
        assert len(np.unique(recs, axis=0)) == n
        recs.setflags(write=False)
        _cache[n] = recs
    return _cache[n]


def device_solve(mpc, recs, rows=None):
    import torch
    dev = torch.device("cuda:0")
    B = len(recs)
    d_in = torch.from_numpy(np.array(recs)).to(dev)
    d_x = torch.zeros((B, mpc.n_var), dtype=torch.float64, device=dev)
    d_fm = torch.zeros((B, 24), dtype=torch.float64, device=dev)
    d_st = torch.zeros(B, dtype=torch.int32, device=dev)
    d_it = torch.zeros(B, dtype=torch.int32, device=dev)
    if rows is None:
        mpc.solve_device(d_in, d_x, d_fm, d_st, d_it)
    else:
        mpc.solve_device_tuned(d_in, torch.from_numpy(rows).to(dev), d_x, d_fm, d_st, d_it)
    torch.cuda.synchronize()
    return d_x.cpu().numpy(), d_fm.cpu().numpy(), d_st.cpu().numpy(), d_it.cpu().numpy()


class Buffers:
    """in | tunables | x | first_move | status | iters of one host call, pageable (numpy) or from vsmpc_alloc_host"""

    def __init__(self, mpc, recs, rows, pinned):
        B = len(recs)
        self.lib, self.ptrs = mpc.lib, []
        shapes = [((B, mpc.n_in), np.float64), ((B, 1 if rows is None else rows.shape[1]), np.float64), ((B, mpc.n_var), np.float64),
                  ((B, 24), np.float64), ((B,), np.int32), ((B,), np.int32)]
        arrays = [self.alloc(s, d) if pinned else np.empty(s, dtype=d) for s, d in shapes]
        self.inp, self.tun, self.x, self.fm, self.st, self.it = arrays
        self.inp[:] = recs
        if rows is not None:
            self.tun[:] = rows
        self.tuned = rows is not None

    def alloc(self, shape, dtype):
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        ptr = self.lib.vsmpc_alloc_host(n)
        assert ptr
        self.ptrs.append(ptr)
        return np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(ctypes.c_uint8)), (n,)).view(dtype).reshape(shape)

    def poison(self):
        self.x[:] = np.nan; self.fm[:] = np.nan; self.st[:] = -7; self.it[:] = -7

    def call(self, mpc, want_x_iters=True):
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        x, it = (vp(self.x), vp(self.it)) if want_x_iters else (None, None)
        if self.tuned:
            return self.lib.vsmpc_solve_batch_tuned(mpc._h, vp(self.inp), vp(self.tun), len(self.inp), x, vp(self.fm),
                                                    vp(self.st), it, None)
        return self.lib.vsmpc_solve_batch(mpc._h, vp(self.inp), len(self.inp), x, vp(self.fm), vp(self.st), it, None)

    def free(self):
        for ptr in self.ptrs:
            self.lib.vsmpc_free_host(ptr)


def check_pipelined(mpc, recs, rows):
    want = device_solve(mpc, recs, rows)
    assert (want[2] == 1).any() and not np.array_equal(want[0][0], want[0][1024])     # (1: Solved)
    for pinned in (False, True):
        b = Buffers(mpc, recs, rows, pinned)
        try:
            for _ in range(2):
                b.poison()
                assert b.call(mpc) == 0
                for got, exp, name in zip((b.x, b.fm, b.st, b.it), want, ("x", "first_move", "status", "iters")):
                    np.testing.assert_array_equal(got, exp, err_msg=f"{name}, pinned={pinned}")
            b.poison()
            assert b.call(mpc, want_x_iters=False) == 0          # x and iters null
            np.testing.assert_array_equal(b.fm, want[1], err_msg=f"first_move without x, pinned={pinned}")
            np.testing.assert_array_equal(b.st, want[2], err_msg=f"status without x, pinned={pinned}")
            assert np.isnan(b.x).all() and (b.it == -7).all()
        finally:
            b.free()


def test_pipelined_host_solve_three_chunks_ragged_tail(solver_mod, synth, layout):
    recs = records(synth, layout, PIPE_BATCH)
    mpc = solver_mod.BatchedVSMPC(layout.paper_config(), device=0, max_batch=PIPE_BATCH)
    try:
        check_pipelined(mpc, recs, None)
    finally:
        mpc.close()


def test_pipelined_tuned_host_solve_heterogeneous_rows(solver_mod, ref, synth, layout):
    """The rows alternate between two configurations with period 3 (other, base, base): 1024 % 3 = 1 and 2048 % 3 = 2, so
    a chunk that reads the staged rows of another chunk, or its own from row 0, meets the wrong configuration."""
    recs = records(synth, layout, PIPE_BATCH)
    base, _ = cc.configs(ref, cc.PAPER, {})
    other, _ = cc.configs(ref, cc.PAPER, {k: v for k, v in cc.all_distinct(cc.PAPER).items() if not k.startswith("period_")})
    mpc = solver_mod.BatchedVSMPC(base, device=0, max_batch=PIPE_BATCH, tunables=True)
    try:
        rows = solver_mod.pack_tunables(mpc, [other if i % 3 == 0 else base for i in range(PIPE_BATCH)])
        plain = device_solve(mpc, recs)
        tuned = device_solve(mpc, recs, rows)
        assert (tuned[0][0::3] != plain[0][0::3]).any(axis=1).all()          # the other configuration really acts
        check_pipelined(mpc, recs, rows)
    finally:
        mpc.close()


@pytest.mark.parametrize("jacobian", [True, False])
def test_sensitivity_host_entry_two_chunks(solver_mod, synth, layout, jacobian):
    import torch
    recs = records(synth, layout, SENS_BATCH)
    B = SENS_BATCH
    m = solver_mod.BatchedVSMPC(layout.paper_config(), device=0, max_batch=B, sensitivity=True)
    try:
        if "sens" not in _cache:                          # the device entry, once for both cases
            dev = torch.device("cuda:0")
            t = {"x": torch.empty((B, m.n_var), dtype=torch.float64, device=dev),
                 "first_move": torch.empty((B, 24), dtype=torch.float64, device=dev),
                 "status": torch.empty(B, dtype=torch.int32, device=dev), "iters": torch.empty(B, dtype=torch.int32, device=dev),
                 "dx_dx0": torch.empty((B, m.n_var, 26), dtype=torch.float64, device=dev),
                 "dfm_dx0": torch.empty((B, 24, 26), dtype=torch.float64, device=dev),
                 "active": torch.empty((B, m.n_v), dtype=torch.int32, device=dev),
                 "flags": torch.empty(B, dtype=torch.int32, device=dev)}
            m.solve_sensitivity_device(torch.from_numpy(np.array(recs)).to(dev), t["x"], t["first_move"], t["status"],
                                       t["iters"], t["dx_dx0"], t["dfm_dx0"], t["active"], t["flags"])
            torch.cuda.synchronize()
            _cache["sens"] = {k: v.cpu().numpy() for k, v in t.items()}
        want = _cache["sens"]
        assert (want["status"] == layout.STATUS_SOLVED).any()
        out = m.solve_sensitivity(recs, jacobian=jacobian)
        assert ("dx_dx0" in out) == jacobian
        for name, got in out.items():
            np.testing.assert_array_equal(got, want[name], err_msg=name)
    finally:
        m.close()
