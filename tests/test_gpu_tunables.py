"""Per-instance tunables on the device (vsmpc_solve_batch_tuned, vsmpc_solve_batch_tuned_device): every instance of a
launch solves under its own weights and throttle box.  Run at the three tabled horizons, for both condensing forms where
the horizon has both, and on a runtime handle (solve_kernel_rt_tuned).

The handle's structure is the default one of the horizon (paper periods); configuration i = that structure + the tunables of
  ALL_DISTINCT                 (its three periods are structural: they stay the handle's)
  every one-field case of config_cases.one_at_a_time() whose structural fields equal the handle's (period_small and
                               period_large are left out by construction)
  every edge configuration test_gpu_config_parity.py compares at the parity bar, except `periods_0047_093` (structural)
No configuration has w_throttle < 10 (config_cases.W_THROTTLE_PARITY_MIN): the edge case sits at 10."""
import numpy as np
import pytest

import config_cases as cc

pytestmark = pytest.mark.gpu

TOL = 1e-8                      # the project's parity bar
FORMS = {(17, 7, 12): (1, 2), (21, 9, 15): (2,), (34, 14, 24): (1, 2)}       # 1 structured, 2 SYRK (vsmpc_set_kernel_form)
VARIANTS = [(h, "never", f) for h in cc.HORIZONS for f in FORMS[h]] + [(h, "always", 0) for h in cc.HORIZONS]
IDS = [f"{h[0]}_{h[1]}_{h[2]}-{'rt' if r == 'always' else ('struct' if f == 1 else 'syrk')}" for h, r, f in VARIANTS]
STRUCTURAL = ("period_mpc", "period_small", "period_large")
_cache = {}


def tunables_only(settings):
    return {k: v for k, v in settings.items() if k not in STRUCTURAL}


def heterogeneous(ref, layout, horizon):
    """[(name, MPCConfig, oracle Config, record)]: the batch of the module docstring, with records on which the fields act"""
    key = ("het", horizon)
    if key in _cache:
        return _cache[key]
    base, _ = cc.configs(ref, horizon, {})
    generic = cc.records(base)
    out = []
    cfg, rcfg = cc.configs(ref, horizon, tunables_only(cc.all_distinct(horizon)))
    for i in (0, 4, 9, 12):
        out.append(("ALL_DISTINCT", cfg, rcfg, generic[i]))
    k = 0
    for name, settings, recs in cc.one_at_a_time():
        if any(f in settings for f in STRUCTURAL):
            continue
        assert settings.get("w_throttle", 1e9) >= cc.W_THROTTLE_PARITY_MIN
        cfg, rcfg = cc.configs(ref, horizon, settings)
        if horizon == cc.PAPER:
            rec = recs[k % len(recs)]                    # the case's own records (built for the paper horizon)
        else:                                            # the same kinds of record at this horizon
            L = layout
            pool = cc.saturated(base, n=6)[3:] if name == "throttle_min" else (
                cc.saturated(base, n=6)[:3] if name == "throttle_max" else generic[:9].copy())
            if name == "w_initial_throttle":
                pool[:, L.IN_HOLD] = 0.0
                pool[:, L.IN_UPREV:L.IN_UPREV + 4] = np.clip(pool[:, L.IN_UPREV:L.IN_UPREV + 4] + 25.0, 0.0, 100.0)
            if name == "w_reg_joint_pos":
                pool[:, L.IN_QERR:L.IN_QERR + 8] *= 10.0
            rec = pool[k % len(pool)]
        out.append((name, cfg, rcfg, rec))
        k += 1
    for name, settings in cc.EDGE.items():
        if any(f in settings for f in STRUCTURAL):
            continue
        assert settings.get("w_throttle", 1e9) >= cc.W_THROTTLE_PARITY_MIN
        cfg, rcfg = cc.configs(ref, horizon, settings)
        recs = cc.edge_records(name, base)
        for i in (0, 5, len(recs) - 1):
            out.append((name, cfg, rcfg, recs[i]))
    _cache[key] = out
    return out


def oracle(ref, horizon, batch):
    key = ("oracle", horizon)
    if key not in _cache:
        res = []
        for _, _, rcfg, rec in batch:
            xr, _, it, _ = ref.solve_instance(rcfg, rec)          # (the oracle ends on the exact optimum: Solved)
            res.append((xr, it))
        _cache[key] = res
    return _cache[key]


def make(solver_mod, ref, horizon, runtime, form, max_batch, settings=None, tunables=True):
    cfg, _ = cc.configs(ref, horizon, settings or {})
    mpc = solver_mod.BatchedVSMPC(cfg, device=0, max_batch=max_batch, runtime=runtime, tunables=tunables)
    if form:
        mpc.set_kernel_form(form)
    return mpc


def solve_tuned_device(mpc, recs, rows):
    import torch
    dev = torch.device("cuda:0")
    B = recs.shape[0]
    d_in, d_tun = torch.from_numpy(recs).to(dev), torch.from_numpy(rows).to(dev)
    d_x = torch.zeros((B, mpc.n_var), dtype=torch.float64, device=dev)
    d_fm = torch.zeros((B, 24), dtype=torch.float64, device=dev)
    d_st = torch.zeros(B, dtype=torch.int32, device=dev)
    d_it = torch.zeros(B, dtype=torch.int32, device=dev)
    mpc.solve_device_tuned(d_in, d_tun, d_x, d_fm, d_st, d_it)
    torch.cuda.synchronize()
    return d_x.cpu().numpy(), d_fm.cpu().numpy(), d_st.cpu().numpy(), d_it.cpu().numpy()


def relerr_rows(x, xr):
    return np.abs(x - xr).max(axis=1) / np.maximum(1.0, np.abs(xr).max(axis=1))


def test_form_table_is_complete(solver_mod, ref):
    for h in cc.HORIZONS:
        mpc = make(solver_mod, ref, h, "never", 0, 2)
        for f in (1, 2):
            if f in FORMS[h]:
                mpc.set_kernel_form(f)
            else:
                with pytest.raises(ValueError):
                    mpc.set_kernel_form(f)
        mpc.close()


@pytest.mark.parametrize("horizon, runtime, form", VARIANTS, ids=IDS)
def test_same_configuration_everywhere(solver_mod, ref, layout, horizon, runtime, form):
    """1: rows packed from the handle's configuration -- host and device tuned entries identical, and identical to
    vsmpc_solve_batch (the instruction stream after P0 is the same source)"""
    mpc = make(solver_mod, ref, horizon, runtime, form, 64, settings=tunables_only(cc.all_distinct(horizon)))
    recs = np.ascontiguousarray(cc.records(mpc.cfg))
    B = len(recs)
    rows = solver_mod.pack_tunables(mpc, [mpc.cfg] * B)
    host = mpc.solve(recs, tunables=rows)
    dev = solve_tuned_device(mpc, recs, rows)
    for a, b in zip(host, dev):
        assert np.array_equal(a, b)
    plain = mpc.solve(recs)
    assert np.array_equal(host[2], plain[2]) and np.array_equal(host[3], plain[3])
    assert (plain[2] == layout.STATUS_SOLVED).all()
    err = relerr_rows(host[0], plain[0])
    print(f"tuned kind against vsmpc_solve_batch: max rel {err.max():.3e}, bit-equal x {np.array_equal(host[0], plain[0])}, "
          f"fm {np.array_equal(host[1], plain[1])}")
    assert err.max() <= TOL
    assert np.array_equal(host[0], plain[0]) and np.array_equal(host[1], plain[1])
    # a small batch goes through the mapped staging buffer, a configs= call through the packer
    small = mpc.solve(recs[:3], configs=[mpc.cfg] * 3)
    for a, b in zip(small, host):
        assert np.array_equal(a, b[:3])
    mpc.close()


@pytest.mark.parametrize("horizon, runtime, form", VARIANTS, ids=IDS)
def test_heterogeneous_batch(solver_mod, ref, layout, horizon, runtime, form):
    """2, 3, 4: one batch, instance i under configuration i -- against the oracle with that configuration (no instance
    excluded), against one handle per configuration, and with the batch permuted and embedded in a larger one"""
    batch = heterogeneous(ref, layout, horizon)
    B = len(batch)
    recs = np.ascontiguousarray(np.stack([b[3] for b in batch]))
    cfgs = [b[1] for b in batch]
    mpc = make(solver_mod, ref, horizon, runtime, form, 2 * B + 8)
    rows = solver_mod.pack_tunables(mpc, cfgs)
    x, fm, st, it = mpc.solve(recs, tunables=rows)
    dev = solve_tuned_device(mpc, recs, rows)
    for a, b in zip((x, fm, st, it), dev):
        assert np.array_equal(a, b)
    # 2: the oracle
    orc = oracle(ref, horizon, batch)
    xr = np.stack([o[0] for o in orc])
    err = relerr_rows(x, xr)
    worst = int(err.argmax())
    print(f"{B} instances, {len(set(b[0] for b in batch))} configurations: max rel err {err.max():.3e} ({batch[worst][0]})")
    assert (st == layout.STATUS_SOLVED).all(), [(batch[i][0], st[i]) for i in range(B) if st[i] != layout.STATUS_SOLVED]
    assert np.array_equal(it, np.array([o[1] for o in orc])), [(batch[i][0], it[i], orc[i][1]) for i in range(B) if it[i] != orc[i][1]]
    assert (err <= TOL).all(), [(batch[i][0], err[i]) for i in range(B) if err[i] > TOL]
    # 3: one handle per configuration
    own = {}
    for i, (name, cfg, _, rec) in enumerate(batch):
        key = repr(cfg)
        if key not in own:
            h = solver_mod.BatchedVSMPC(cfg, device=0, max_batch=1, runtime=runtime)
            if form:
                h.set_kernel_form(form)
            own[key] = h
        xs, fms, sts, its = own[key].solve(rec[None, :])
        assert sts[0] == st[i] and its[0] == it[i], (name, sts[0], st[i], its[0], it[i])
        assert np.array_equal(xs[0], x[i]) and np.array_equal(fms[0], fm[i]), (name, relerr_rows(xs, x[i:i + 1]))
    for h in own.values():
        h.close()
    # 4: neighbours do not matter -- permuted, and embedded in a larger batch of other configurations
    rng = np.random.default_rng(11)
    perm = rng.permutation(B)
    filler = rng.integers(0, B, size=B + 8)
    order = np.concatenate([filler[:5], perm, filler[5:]])
    big = mpc.solve(np.ascontiguousarray(recs[order]), tunables=np.ascontiguousarray(rows[order]))
    for k, i in enumerate(perm):
        for a, b in zip(big, (x, fm, st, it)):
            assert np.array_equal(a[5 + k], b[i]), (batch[i][0], k)
    mpc.close()


@pytest.mark.parametrize("horizon, runtime, form", VARIANTS, ids=IDS)
def test_saturating_boxes_side_by_side(solver_mod, ref, layout, horizon, runtime, form):
    """5: a 45/55 box beside a 0/100 box on the same records -- feasibility against each instance's own box, different
    iteration counts: the box is read per instance in P4"""
    base, rbase = cc.configs(ref, horizon, {})
    narrow, rnarrow = cc.configs(ref, horizon, cc.EDGE["throttle_box_45_55"])
    r = cc.edge_records("throttle_box_45_55", base)[:-1]           # free ticks, previous throttle inside both boxes
    n = len(r)
    recs = np.ascontiguousarray(np.repeat(r, 2, axis=0))           # records 2k, 2k + 1 equal; narrow box on the odd ones
    cfgs = [base, narrow] * n
    mpc = make(solver_mod, ref, horizon, runtime, form, 2 * n)
    x, fm, st, it = mpc.solve(recs, configs=cfgs)
    assert (st == layout.STATUS_SOLVED).all()
    rows = solver_mod.pack_tunables(mpc, cfgs)
    ov = base.off_throttle
    for b in range(2 * n):
        v = x[b, ov:]
        lo, hi = rows[b, 29], rows[b, 30]
        assert (v >= lo - 1e-12).all() and (v <= hi + 1e-12).all(), (b, v.min(), lo, v.max(), hi)
        assert (fm[b, 12:16] >= cfgs[b].throttle_min - 1e-9).all() and (fm[b, 12:16] <= cfgs[b].throttle_max + 1e-9).all()
    assert (it[1::2] != it[0::2]).any(), (it[0::2], it[1::2])
    assert (np.abs(x[1::2, ov:] - x[0::2, ov:]).max(axis=1) > 1e-3).all()    # the narrow box binds on every record
    for b in (1, 2 * n - 1):
        xr, _, ir, _ = ref.solve_instance(rnarrow, recs[b])
        assert ir == it[b] and relerr_rows(x[b:b + 1], xr[None, :])[0] <= TOL
    mpc.close()


@pytest.mark.parametrize("horizon, runtime, form", VARIANTS, ids=IDS)
def test_edge_batches_and_non_finite_tunables(solver_mod, ref, layout, horizon, runtime, form):
    """6: batch 0, batch 1, batch > handle; a non-finite tunable ends like a non-finite record (status Numerical) and
    leaves its neighbours alone"""
    mpc = make(solver_mod, ref, horizon, runtime, form, 8)
    recs = np.ascontiguousarray(cc.records(mpc.cfg)[:8])
    rows = solver_mod.pack_tunables(mpc, [mpc.cfg] * 8)
    lib, p = mpc.lib, solver_mod._ptr
    st = np.full(16, -7, dtype=np.int32)
    assert lib.vsmpc_solve_batch_tuned(mpc._h, p(recs), p(rows), 0, None, None, p(st), None, None) == 0
    assert (st == -7).all()
    big_r, big_t = np.tile(recs, (2, 1))[:9], np.tile(rows, (2, 1))[:9]
    assert lib.vsmpc_solve_batch_tuned(mpc._h, p(big_r), p(big_t), 9, None, None, p(st), None, None) == -3
    one = mpc.solve(recs[:1], tunables=rows[:1])
    ref8 = mpc.solve(recs, tunables=rows)
    for a, b in zip(one, ref8):
        assert np.array_equal(a[0], b[0])
    assert (ref8[2] == layout.STATUS_SOLVED).all()
    for col, val in ((0, np.nan), (20, np.inf), (27, np.nan), (29, np.nan), (30, -np.inf)):
        bad = rows.copy()
        bad[3, col] = val
        x, fm, st8, it = mpc.solve(recs, tunables=bad)
        assert st8[3] == layout.STATUS_NUMERICAL, (col, val, st8)
        keep = [b for b in range(8) if b != 3]
        assert np.array_equal(st8[keep], ref8[2][keep]) and np.array_equal(x[keep], ref8[0][keep])
    nanrec = recs.copy()
    nanrec[3, layout.IN_INERTIA] = np.nan                      # (as tests/test_gpu_parity.py does it)
    assert mpc.solve(nanrec, tunables=rows)[2][3] == layout.STATUS_NUMERICAL      # what a non-finite record does
    mpc.close()
