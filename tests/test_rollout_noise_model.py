"""CPU side of the noise of the closed-loop rollout (vsmpc_rollout_set_noise): the model's generator (tests/rollout_noise_model.py)
against Random123's known answers, against a second restatement in plain integers and against the moments a standard normal
sample has; the struct against the header; the entries' refusals that need no device.  The draws are a fixed function of the
seed, so the statistical bounds are conditions on fixed numbers, not tests that can flake; every bound is a number of standard
errors of the statistic under the hypothesis (or a tabulated point), none is read off the sample.  Each planted defect of the
generator has to break at least one of these checks."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import rollout_noise_model as nm
from conftest import ROOT

LOOPS, TICKS = 256, 40
N = LOOPS * TICKS * nm.DRAWS          # 184,320
BIG = 2 ** 32 - 2                     # first_index at which loops 0..4 cross the word boundary of the counter


def known_answers_hold(gen):
    return all(tuple(int(v) for v in gen.block(np.array(c), np.array(k))) == out for c, k, out in nm.KNOWN_ANSWERS)


def restatements_agree(gen):
    """the vectorised draws against scalar_draws at the word boundary of the loop index and at two distant ticks"""
    for first, loops, tick0, ticks in ((BIG, 5, 0, 2), (BIG, 5, 1000, 1), (0, 3, 7, 1)):
        z, _ = gen.draws(2025, first, loops, tick0, ticks)
        for t in range(ticks):
            for b in range(loops):
                zs = nm.scalar_draws(2025, first + b, tick0 + t)
                if not (np.abs(z[t, b] - zs) <= 1e-14 * np.maximum(1.0, np.abs(zs))).all():   # (log, sin, cos: a few ulp)
                    return False
    return True


def _corr(a, b):
    a, b = a.ravel() - a.mean(), b.ravel() - b.mean()
    return float((a * b).sum() / math.sqrt((a * a).sum() * (b * b).sum()))


def statistics(z):
    """name -> (value in units of its bound): |value| <= 1 passes.  z [TICKS, LOOPS, 18]"""
    x = z.ravel()
    n = x.size
    out = {}
    m, v = x.mean(), x.var()
    out["mean"] = m / (4.0 / math.sqrt(n))
    out["variance"] = (v - 1.0) / (4.0 * math.sqrt(2.0 / n))
    out["excess kurtosis"] = (((x - m) ** 4).mean() / v ** 2 - 3.0) / (4.0 * math.sqrt(24.0 / n))
    for name, a, b in (("next loop", z[:, :-1], z[:, 1:]), ("next tick", z[:-1], z[1:]), ("next channel", z[..., :-1], z[..., 1:])):
        out["lag-1 correlation, " + name] = _corr(a, b) / (4.0 / math.sqrt(a.size))
    per = z.reshape(-1, nm.DRAWS)
    nc = per.shape[0]
    out["channel means"] = np.abs(per.mean(axis=0)).max() / (5.0 / math.sqrt(nc))
    out["channel variances"] = np.abs(per.var(axis=0) - 1.0).max() / (5.0 * math.sqrt(2.0 / nc))
    # measurement against gust channels of the same tick, and every other pair: 153 correlations of nc samples each
    c = np.corrcoef(per.T) - np.eye(nm.DRAWS)
    out["channel cross-correlations"] = np.abs(c).max() / (5.0 / math.sqrt(nc))
    xs = np.sort(x)
    cdf = 0.5 * (1.0 + np.vectorize(math.erf)(xs / math.sqrt(2.0)))
    i = np.arange(1, n + 1)
    ks = max(float((i / n - cdf).max()), float((cdf - (i - 1) / n).max()))
    out["Kolmogorov-Smirnov"] = ks * math.sqrt(n) / 1.63                    # the 1 % point of the limiting distribution
    big = float(np.abs(x).max())                                            # P(max < 4) = 8e-6, P(max > 6) = 4e-4 at this n
    out["max |z|"] = 1.0 if 4.0 <= big <= 6.0 else 2.0
    return out


def failed_checks(gen, verbose=False):
    bad = []
    if not known_answers_hold(gen):
        bad.append("known answers")
    if not restatements_agree(gen):
        bad.append("second restatement")
    for seed in (2025, 0):
        z, _ = gen.draws(seed, 0, LOOPS, 0, TICKS)
        assert z.size == N
        for name, val in statistics(z).items():
            if verbose:
                print(f"seed {seed}: {name}: {val:+.3f} of its bound")
            if not abs(val) <= 1.0:
                bad.append(f"seed {seed}: {name}")
    return bad


def test_known_answers():
    assert known_answers_hold(nm.Generator())
    c, k, out = nm.KNOWN_ANSWERS[2]
    w = nm.Generator().block(np.array([c, c]), np.array([k, k]))           # and over an array
    assert w.shape == (2, 4) and [int(v) for v in w[1]] == list(out)


def test_generator_passes_every_check():
    assert failed_checks(nm.Generator(), verbose=True) == []


DEFECTS = {
    "9 rounds instead of 10": dict(rounds=9),
    "swapped multipliers": dict(swap_multipliers=True),
    "key not bumped": dict(bump_key=False),
    "tick and loop swapped in the counter": dict(swap_tick_loop=True),
    "32-bit first_index + b": dict(loop_bits=32),
    "w1 >> 11 dropped": dict(low_word=False),
    "gust drawn from blocks 0..2": dict(gust_block0=0),
}


@pytest.mark.parametrize("defect", list(DEFECTS))
def test_planted_defect_breaks_a_check(defect):
    bad = failed_checks(nm.Generator(**DEFECTS[defect]))
    print(defect, "->", bad)
    assert bad, defect


def test_gust_from_the_measurement_blocks_shows_in_the_statistics():
    """that defect needs no second restatement to be seen: the gust channels then repeat measurement channels"""
    z, _ = nm.Generator(gust_block0=0).draws(2025, 0, LOOPS, 0, TICKS)
    assert statistics(z)["channel cross-correlations"] > 1.0


def test_struct_matches_header(layout):
    text = open(os.path.join(ROOT, "include", "vsmpc.h")).read()
    body = re.search(r"typedef struct vsmpc_noise \{(.*?)\} vsmpc_noise;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(unsigned long long|long long|double)\s+(.*)", decl)
        ctype, names = m.group(1), [n.strip() for n in m.group(2).split(",")]
        fields += [(n, ctype) for n in names]
    want = {"unsigned long long": ctypes.c_ulonglong, "long long": ctypes.c_longlong, "double": ctypes.c_double}
    assert [(n, want[t]) for n, t in fields] == list(layout.CNoise._fields_)
    assert [n for n, _ in fields] == ["seed", "first_index", "sigma_pos", "sigma_lin_vel", "sigma_rpy", "sigma_ang_vel",
                                      "sigma_force", "sigma_torque"]
    assert ctypes.sizeof(layout.CNoise) == 64
    assert layout.NOISE_DRAWS == nm.DRAWS == 2 * layout.NOISE_BLOCKS


def test_entries_refuse_null_and_bad_fields_without_a_device(solver_mod, pkg, layout):
    import importlib
    _lib = importlib.import_module(pkg.__name__ + "._lib")
    lib = _lib.load()
    good = dict(seed=1, first_index=0, sigma_pos=0.0, sigma_lin_vel=0.015, sigma_rpy=0.0, sigma_ang_vel=0.015, sigma_force=0.0,
                sigma_torque=0.0)
    assert lib.vsmpc_rollout_set_noise(None, None) == -1
    assert lib.vsmpc_rollout_set_noise(None, ctypes.byref(layout.CNoise(**good))) == -1
    assert lib.vsmpc_strerror(-1) == b"invalid argument"
    for field, _ in layout.CNoise._fields_[1:]:
        for bad in ((-1,) if field == "first_index" else (-1e-300, math.inf, math.nan)):
            n = layout.CNoise(**dict(good, **{field: bad}))
            assert lib.vsmpc_rollout_set_noise(None, ctypes.byref(n)) == -1, (field, bad)
            text = lib.vsmpc_strerror(-1).decode()
            assert field in text and "vsmpc_rollout_set_noise" in text, (field, bad, text)
    z = np.zeros(18)
    assert lib.vsmpc_rollout_noise_draws(None, 0, 1, z.ctypes.data_as(ctypes.c_void_p), None) == -1
    assert lib.vsmpc_strerror(-1) == b"invalid argument"                    # (the text of the last refusal, not of an earlier one)


def test_sharding_hands_a_rank_its_first_index(pkg):
    import importlib
    sh = importlib.import_module(pkg.__name__ + ".sharding")
    firsts = [sh.rank_first_index(10, r, 4) for r in range(4)]
    assert firsts == [sh.shard_range(10, r, 4)[0] for r in range(4)] == [0, 3, 6, 8]
    z, _ = nm.draws(5, 0, 10, 0, 2)
    for r in range(4):
        first, count = sh.shard_range(10, r, 4)
        np.testing.assert_array_equal(nm.draws(5, firsts[r], count, 0, 2)[0], z[:, first:first + count])
