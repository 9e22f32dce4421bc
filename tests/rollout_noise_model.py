"""numpy model of the noise of the closed-loop rollout (vsmpc_rollout_set_noise, csrc/vsmpc_noise_device.hpp): Philox4x32-10 on
uint64 arrays, the draws z(seed, loop, tick), the measured state the record is built from and the tick with the gust.  Beside
the vectorised generator stands a second restatement in plain Python integers (scalar_draws), written from the formulas of
include/vsmpc.h alone: the two are held against each other, and the device against the first.
Test infrastructure: nothing here is read by the product path."""
from __future__ import annotations

import math

import numpy as np

import rollout_model as rm

L = rm.L

M0, M1 = 0xD2511F53, 0xCD9E8D57          # multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85          # Weyl constants of the key schedule
MASK = np.uint64(0xFFFFFFFF)
BLOCKS, DRAWS = 9, 18                    # per loop and tick; blocks 0..5 = z[0:12] measurement, 6..8 = z[12:18] gust
S32 = np.uint64(32)

# Random123's known answers of philox4x32-10: (counter, key, output)
KNOWN_ANSWERS = (
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)


class Generator:
    """The generator as specified (no arguments), or with one planted defect (tests/test_rollout_noise_model.py)."""

    def __init__(self, rounds=10, swap_multipliers=False, bump_key=True, swap_tick_loop=False, loop_bits=64, low_word=True,
                 gust_block0=6):
        self.rounds, self.bump_key, self.swap_tick_loop = rounds, bump_key, swap_tick_loop
        self.m0, self.m1 = (M1, M0) if swap_multipliers else (M0, M1)
        self.loop_bits, self.low_word, self.gust_block0 = loop_bits, low_word, gust_block0

    def block(self, ctr, key):
        """ctr [..., 4], key [..., 2]: arrays of 32-bit values -> the block function's output [..., 4] (uint64 holding 32 bit)"""
        ctr, key = np.asarray(ctr, dtype=np.uint64), np.asarray(key, dtype=np.uint64)
        c0, c1, c2, c3 = (ctr[..., i] for i in range(4))
        k0, k1 = key[..., 0], key[..., 1]
        m0, m1 = np.uint64(self.m0), np.uint64(self.m1)
        for _ in range(self.rounds):
            p0, p1 = m0 * c0, m1 * c2                     # 32 x 32 -> 64 bit: exact in uint64
            c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ k0, p1 & MASK, (p0 >> S32) ^ c3 ^ k1, p0 & MASK
            if self.bump_key:
                k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
        return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1)

    def words(self, seed, first_index, loops, tick0, ticks):
        """[ticks, loops, 9, 4]: block j of loop first_index + b at tick tick0 + t"""
        loop = np.uint64(first_index) + np.arange(loops, dtype=np.uint64)
        if self.loop_bits == 32:
            loop = loop & MASK
        k = (tick0 + np.arange(ticks)).astype(np.uint64)
        j = np.concatenate([np.arange(6), self.gust_block0 + np.arange(3)]).astype(np.uint64)
        shape = (ticks, loops, BLOCKS)
        J = np.broadcast_to(j[None, None, :], shape)
        K = np.broadcast_to(k[:, None, None], shape)
        LO = np.broadcast_to((loop & MASK)[None, :, None], shape)
        HI = np.broadcast_to((loop >> S32)[None, :, None], shape)
        ctr = np.stack([J, LO, K, HI] if self.swap_tick_loop else [J, K, LO, HI], axis=-1)
        key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint64)
        return self.block(ctr, np.broadcast_to(key, shape + (2,)))

    def uniform(self, hi, lo):
        n = (hi << np.uint64(21)) | ((lo >> np.uint64(11)) if self.low_word else np.uint64(0))
        return (n.astype(np.float64) + 0.5) * 2.0 ** -53

    def draws(self, seed, first_index, loops, tick0, ticks):
        """(z [ticks, loops, 18], words [ticks, loops, 9, 4] uint32)"""
        w = self.words(seed, first_index, loops, tick0, ticks)
        u1, u2 = self.uniform(w[..., 0], w[..., 1]), self.uniform(w[..., 2], w[..., 3])
        rad, ang = np.sqrt(-2.0 * np.log(u1)), 2.0 * math.pi * u2
        z = np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=-1).reshape(ticks, loops, DRAWS)
        return z, w.astype(np.uint32)


def draws(seed, first_index, loops, tick0, ticks):
    return Generator().draws(seed, first_index, loops, tick0, ticks)


def scalar_draws(seed, loop, tick):
    """The 18 normals of one loop (global index) and tick in plain Python integers and math: the second restatement"""
    z = []
    for j in range(BLOCKS):
        c = [j, tick, loop & 0xFFFFFFFF, loop >> 32]
        k = [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF]
        for r in range(10):
            if r > 0:
                k = [(k[0] + W0) & 0xFFFFFFFF, (k[1] + W1) & 0xFFFFFFFF]
            p0, p1 = M0 * c[0], M1 * c[2]
            c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
        u1 = (float((c[0] << 21) | (c[1] >> 11)) + 0.5) * 2.0 ** -53
        u2 = (float((c[2] << 21) | (c[3] >> 11)) + 0.5) * 2.0 ** -53
        rad = math.sqrt(-2.0 * math.log(u1))
        z += [rad * math.cos(2.0 * math.pi * u2), rad * math.sin(2.0 * math.pi * u2)]
    return np.array(z)


SIGMA_NAMES = ("pos", "lin_vel", "rpy", "ang_vel", "force", "torque")


def measured_state(s, p, IB, z, sigmas):
    """The state the record is assembled from: the plant state s with its first twelve entries measured under z[0:12];
    sigmas = (pos, lin_vel, rpy, ang_vel, ...), IB the plant's body inertia, R of the TRUE attitude."""
    m = s.copy()
    R = rm.rot(s[L.PS_RPY:L.PS_RPY + 3])
    m[L.PS_P:L.PS_P + 3] += sigmas[0] * z[0:3]
    m[L.PS_HLIN:L.PS_HLIN + 3] += p[L.PP_MASS] * (R.T @ (sigmas[1] * z[3:6]))
    m[L.PS_RPY:L.PS_RPY + 3] += sigmas[2] * z[6:9]
    m[L.PS_HANG:L.PS_HANG + 3] += IB @ (R.T @ (sigmas[3] * z[9:12]))
    return m


def advance_with_gust(cfg, s, p, tick, fm, status, traj_alpha, alpha_dt, z, sigmas, substeps=5):
    """rollout_model.advance of the polynomial jet plant with the gust sigma_force z[12:15] (world force) and sigma_torque
    z[15:18] (body torque) held over the tick: every sub-step is rollout_model.substep on a parameter row whose push fields hold
    push + gust and whose window is open.  `tick` counts from the reset, like the draws."""
    s = s.copy()
    if status == 1:
        s[L.PS_Q:L.PS_Q + 8] += fm[L.FM_DQ:L.FM_DQ + 8]
        s[L.PS_U:L.PS_U + 4] = fm[L.FM_THROTTLE:L.FM_THROTTLE + 4]
        s[L.PS_TDES:L.PS_TDES + 4] = fm[L.FM_THRUST:L.FM_THRUST + 4]
        s[L.PS_TDDES:L.PS_TDDES + 4] = fm[L.FM_THRUSTDOT:L.FM_THRUSTDOT + 4]
    tk = tick + int(p[L.PP_TICK0])
    IB = rm.inertia_body(s, p)
    A, _ = rm.amom_of_q(s, p)
    vthr = np.array([rm._JET.compute_v(rm._JET.standardizeThrottle_u2T(u)) for u in s[L.PS_U:L.PS_U + 4]])
    x = s[0:20].copy()
    for ss in range(substeps):
        t = (tk + ss / substeps) * cfg.period_mpc
        push = p[L.PP_DIST_T0] <= t < p[L.PP_DIST_T1]
        q = p.copy()
        q[L.PP_DIST_F:L.PP_DIST_F + 3] = (p[L.PP_DIST_F:L.PP_DIST_F + 3] if push else 0.0) + sigmas[4] * z[12:15]
        q[L.PP_DIST_TAU:L.PP_DIST_TAU + 3] = (p[L.PP_DIST_TAU:L.PP_DIST_TAU + 3] if push else 0.0) + sigmas[5] * z[15:18]
        q[L.PP_DIST_T0], q[L.PP_DIST_T1] = -math.inf, math.inf
        x = rm.substep(cfg, x, q, tk, ss, substeps, A, IB, vthr, traj_alpha, alpha_dt)
    s[0:20] = x
    return s
