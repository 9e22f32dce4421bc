// Random draws of the closed-loop rollout (vsmpc_rollout_set_noise): a counter-based generator, so that a draw is a function
// of (seed, loop, tick, block) and of nothing stored anywhere -- graph replay, split runs and sharded batches reproduce each
// other bit for bit.  Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11) in plain integer
// arithmetic; executable restatement: tests/rollout_noise_model.py.
//
//   counter = (block j, tick k, loop_lo, loop_hi)      key = (seed_lo, seed_hi)
//   loop = first_index + b, 64 bit: the loop's global index; k = ticks since the reset (PP_TICK0 is not added)
//
// One block (w0, w1, w2, w3) gives two standard normals by Box-Muller on 53-bit uniforms in (0, 1]:
//   u1 = (((uint64)w0 << 21 | w1 >> 11) + 0.5) 2^-53,  u2 likewise from (w2, w3)
//   z[2j] = sqrt(-2 ln u1) cos(2 pi u2),  z[2j+1] = sqrt(-2 ln u1) sin(2 pi u2)      (evaluated as sincospi(2 u2))
// A tick has nine blocks: z[0:12] (blocks 0..5) are the measurement of tick k, z[12:18] (blocks 6..8) the gust held over it.
#pragma once
#include "vsmpc_device.hpp"
#include "vsmpc_launch.hpp"
#include "vsmpc_rollout_device.hpp"

namespace vsmpc {

constexpr int NOISE_BLOCKS = 9;                 // per loop and tick
constexpr int NOISE_DRAWS = 2 * NOISE_BLOCKS;
constexpr int NOISE_MEAS_BLOCKS = 6;            // blocks 0..5: z[0:12]
constexpr int NOISE_LDS = NOISE_DRAWS + 6;      // doubles of LDS: the draws of a tick, and sin | cos of the true roll, pitch, yaw

VS_HD void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned* w) {
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
        const unsigned n0 = unsigned(p1 >> 32) ^ c1 ^ k0, n2 = unsigned(p0 >> 32) ^ c3 ^ k1;
        c1 = unsigned(p1);
        c3 = unsigned(p0);
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;   // (the bump behind the last round is dead)
        k1 += 0xBB67AE85u;
    }
    w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}

VS_HD double uniform53(unsigned hi, unsigned lo) {   // in (0, 1]: the logarithm below is finite
    return (double((static_cast<unsigned long long>(hi) << 21) | (lo >> 11)) + 0.5) * 0x1p-53;
}

// block j of loop first_index + b at tick k: its words, and the two normals z[2j], z[2j+1]
VS_DEV void noise_block(const RolloutNoise& nz, int b, int k, int j, unsigned* w, double& za, double& zb) {
    const unsigned long long loop = nz.first_index + static_cast<unsigned long long>(b);
    philox4x32_10(unsigned(j), unsigned(k), unsigned(loop), unsigned(loop >> 32), unsigned(nz.seed), unsigned(nz.seed >> 32), w);
    const double rad = sqrt(-2.0 * log(uniform53(w[0], w[1])));
    double sn, cs;
    sincospi(2.0 * uniform53(w[2], w[3]), &sn, &cs);   // the angle 2 pi u2 without its rounding, and without a range reduction
    za = rad * cs;
    zb = rad * sn;
}

// z[0:12] of tick k into zn (LDS), a block per lane 0..5.  The caller's barrier follows.
VS_DEV void draw_measurement(const RolloutNoise& nz, int b, int k, double* zn, int lane) {
    if (lane < NOISE_MEAS_BLOCKS) {
        unsigned w[4];
        noise_block(nz, b, k, lane, w, zn[2 * lane], zn[2 * lane + 1]);
    }
}
// what the NOISE instantiation of advance_kernel draws, a block per lane 0..8: the measurement of tick k + 1 (the record it leaves) and the gust
// of tick k (the one it flies)
VS_DEV void draw_tick(const RolloutNoise& nz, int b, int k, double* zn, int lane) {
    if (lane < NOISE_BLOCKS) {
        unsigned w[4];
        noise_block(nz, b, lane < NOISE_MEAS_BLOCKS ? k + 1 : k, lane, w, zn[2 * lane], zn[2 * lane + 1]);
    }
}

// The measured state in place of the plant state s (LDS; its copy in HBM and the log row are written before this):
//   p += sigma_pos z[0:3]            h_lin += m   R^T (sigma_lin_vel z[3:6])     (a world-frame velocity error, as the reference's
//   rpy += sigma_rpy z[6:9]          h_ang += I_B R^T (sigma_ang_vel z[9:12])     simulate_noise adds it)
// with R = R(rpy) of the TRUE attitude and I_B the plant's.  zn: the draws, with six doubles of scratch behind them.  The
// three sincos run side by side in lanes 0..2, as in substep_preamble (a wavefront per instance: what one lane does alone,
// the others wait for); every lane then forms R in registers.  Ends with a barrier.
VS_DEV void measure_state(const RolloutNoise& nz, double* zn, double m, const double* IB, double* s, int lane) {
    double* sc = zn + NOISE_DRAWS;
    if (lane < 3) {
        double sn, cs;
        sincos(s[VSMPC_PS_RPY + lane], &sn, &cs);
        sc[2 * lane] = sn;
        sc[2 * lane + 1] = cs;
    }
    __syncthreads();
    double R[9];
    rot_from_sincos(sincos_of(sc), R);
    if (lane < 3) {
        s[VSMPC_PS_P + lane] += nz.sigma_pos * zn[lane];
    } else if (lane < 6) {
        const int c = lane - 3;
        const double v0 = nz.sigma_lin_vel * zn[3], v1 = nz.sigma_lin_vel * zn[4], v2 = nz.sigma_lin_vel * zn[5];
        s[VSMPC_PS_HLIN + c] += m * (R[c] * v0 + R[3 + c] * v1 + R[6 + c] * v2);
    } else if (lane < 9) {
        s[VSMPC_PS_RPY + lane - 6] += nz.sigma_rpy * zn[lane];
    } else if (lane < 12) {
        const int r = lane - 9;
        const double v0 = nz.sigma_ang_vel * zn[9], v1 = nz.sigma_ang_vel * zn[10], v2 = nz.sigma_ang_vel * zn[11];
        double acc = 0.0;
        for (int c = 0; c < 3; ++c) acc += IB[3 * r + c] * (R[c] * v0 + R[3 + c] * v1 + R[6 + c] * v2);
        s[VSMPC_PS_HANG + r] += acc;
    }
    __syncthreads();
}

// The gust's share of the momentum rates, beside substep_rate's push: R^T (sigma_force z[12:15]) on lanes 3..5, the body
// torque sigma_torque z[15:18] on lanes 9..11
VS_DEV double gust_rate(const RolloutNoise& nz, const double* zn, const double* R, int lane) {
    if (lane >= 3 && lane < 6) {
        const int r = lane - 3;
        return R[r] * (nz.sigma_force * zn[12]) + R[3 + r] * (nz.sigma_force * zn[13]) + R[6 + r] * (nz.sigma_force * zn[14]);
    }
    if (lane >= 9 && lane < 12) return nz.sigma_torque * zn[15 + lane - 9];
    return 0.0;
}

}  // namespace vsmpc
