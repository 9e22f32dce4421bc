// P5 of the tuned solve kernels: back-substitution from the register-resident factor, and what wavefront 0 of the
// pipelined schedule does beside it.
#pragma once
#include "vsmpc_p3.hpp"

namespace vsmpc {

// ------------------------------------------------------------------------------------------------
// Sum of a per-lane value over the four 16-lane rows of a wavefront (lanes l, l^16, l^32, l^48), result in every lane.
// gfx950's v_permlane16_swap / v_permlane32_swap exchange rows / halves between two registers at VALU latency
// (a ds_bpermute-based __shfl_xor costs an LDS round trip per step).
// ------------------------------------------------------------------------------------------------
VS_DEV double row_sum4(double x) {
    unsigned lo = __double2loint(x), hi = __double2hiint(x);
    auto l2 = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
    auto h2 = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
    const double s = __hiloint2double(h2[0], l2[0]) + __hiloint2double(h2[1], l2[1]);
    lo = __double2loint(s);
    hi = __double2hiint(s);
    auto l3 = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
    auto h3 = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
    return __hiloint2double(h3[0], l3[0]) + __hiloint2double(h3[1], l3[1]);
}

// ------------------------------------------------------------------------------------------------
// P5 for wavefront W: back-substitution L^T z = w from the REGISTER-resident factor, tile row by tile row from
// the bottom.  z_r is known (throttle rows: sZ) or formed by every wavefront redundantly and bit-identically on the
// matrix core: z_r = X_r^T d, d = w_r - sum of the wavefronts' published partial sums, as D = A B with A = X_r^T and
// every column of B = d -- the result arrives in the accumulator layout, i.e. lane (g, j) holds z[g + 4 i], exactly
// the operand layout of the owned tiles (lane (g, j) holds L[g + 4 i][j]).  Every owned tile (r, q) then adds
// L_rq^T z_r to this wavefront's partial sum u_q, kept in registers; the partial sums of column r - 1 are published
// before the barrier that ends step r (fixed summation order -> deterministic).  One workgroup barrier per tile row.
// ------------------------------------------------------------------------------------------------
template <class D, int TPW, int W, bool PIPE = false>
VS_DEV void backsub_wave(const d4 (&acc)[TPW], const double* __restrict__ sW, double* __restrict__ sZ,
                         const double* __restrict__ sXinv, double* __restrict__ sU, int lane) {
    constexpr WaveLists<D, TPW, W, PIPE> wl{};
    constexpr TileTab<D, PIPE> tab{};
    constexpr int PVT = D::PVT;
    double* myU = sU + W * D::NP;
    const int j = lane & 15, g4 = lane >> 4;
    double up[PVT];
#pragma unroll
    for (int q = 0; q < PVT; ++q) up[q] = 0.0;
    double xop[4];  // A operand of the next joint tile row: X_r[g4 + 4 ks][j], requested one step ahead
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) xop[ks] = sXinv[(PVT - 1) * D::TS + (g4 + 4 * ks) * 17 + j];
#pragma unroll
    for (int r = D::NT - 1; r >= 0; --r) {
        double zz[4];
        if (r < PVT) {
            double dop[4];
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const int row = 16 * r + g4 + 4 * ks;
                double usum = sU[row];
#pragma unroll
                for (int w = 1; w < D::NWAVES; ++w) usum += sU[w * D::NP + row];
                dop[ks] = sW[row] - usum;
            }
            // two accumulators, summed: two dependent pairs instead of a chain of four (~95 cycles per dependent step)
            d4 zt = d4{0.0, 0.0, 0.0, 0.0}, zu = d4{0.0, 0.0, 0.0, 0.0};
            zt = __builtin_amdgcn_mfma_f64_16x16x4f64(xop[0], dop[0], zt, 0, 0, 0);
            zu = __builtin_amdgcn_mfma_f64_16x16x4f64(xop[1], dop[1], zu, 0, 0, 0);
            zt = __builtin_amdgcn_mfma_f64_16x16x4f64(xop[2], dop[2], zt, 0, 0, 0);
            zu = __builtin_amdgcn_mfma_f64_16x16x4f64(xop[3], dop[3], zu, 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 4; ++i) zt[i] += zu[i];
            if (r > 0) {
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) xop[ks] = sXinv[(r - 1) * D::TS + (g4 + 4 * ks) * 17 + j];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) zz[i] = zt[i];
            if (W == (PIPE ? 1 : 0) && j == 0) {   // (PIPE: wavefront 0 is not here, see p5_wave0_jets)
#pragma unroll
                for (int i = 0; i < 4; ++i) sZ[16 * r + g4 + 4 * i] = zz[i];
            }
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) zz[i] = sZ[16 * r + g4 + 4 * i];
        }
        if (r > 0) {
#pragma unroll
            for (int a = 0; a < TPW; ++a) {
                if (a < wl.nrow[r]) {
                    const int q = wl.row[r][a];
                    const int t = q * D::NWAVES + W;
                    double part = acc[q][0] * zz[0];
#pragma unroll
                    for (int i = 1; i < 4; ++i) part = fma(acc[q][i], zz[i], part);
                    up[tab.tj[t]] += part;   // per 16-lane row; the four rows are summed once, when the column is published
                }
            }
            if (r - 1 < PVT) {
                const double usum = row_sum4(up[r - 1]);
                if (lane < 16) myU[16 * (r - 1) + j] = usum;
                __syncthreads();   // (a step that publishes nothing -- the corner tile rows above the first joint row -- needs none:
                                   // PVT barriers in all, which p5_wave0_jets matches)
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// P5, wavefront 0 of the pipelined schedule (kernel v29).  It holds no tile, so the back-substitution has nothing for it to do
// but meet its barriers -- and the first link of P6's cascade, the jets, depends on the throttles only, which are final
// since P4: their input terms and their whole two-state recursion (systemDynamicsVSMPC.cpp:384-429) run here, beside P5,
// CHJ stages per barrier interval.  P6 then starts at the momenta with every T_k in sX: its input-term pass forms the whole
// forcing A_mom T_k + f_k, and the momenta and CoM / RPY links run as one stream with no barrier inside.  (Wavefront 0's slot
// of the partial sums is zeroed once; wavefront 1 stores z.)
// ------------------------------------------------------------------------------------------------
template <class D>
VS_DEV void p5_wave0_jets(double* __restrict__ smem, int lane) {
    using S = Smem<D>;
    // Stages per barrier interval.  P5 has one barrier per joint tile row (PVT of them; the corner tile rows in front publish
    // nothing and have none): a chunk behind every barrier but the last, beside the other wavefronts' joint-row steps (~0.9 k
    // cycles each).  Measured (when the corner rows still had barriers): 3 stages in every interval P5 6.1 k cycles, 6 in the
    // first three 6.8 k, 9 in the first two 7.2 k (5.5 k without the jets); chunks beside the short corner-row steps delay them.
    constexpr int BI0 = 0;                                 // first interval that gets a chunk
    constexpr int NIV = D::PVT - 1;                        // intervals with a chunk
    constexpr int CHJ = (D::N + NIV - 1) / NIV, NCJ = (D::N + CHJ - 1) / CHJ;
    static_assert(NIV >= 1 && NCJ <= NIV, "the jets fit the barrier intervals of P5");
    const double* sIn = smem + S::oIn;
    const double* sA = smem + S::oA;
    const double* sBt = smem + S::oBt;
    const double* sC = smem + S::oC;
    const double* sZ = smem + S::oZ;
    const double* sDt = smem + S::oDt;
    double* sU = smem + S::oU;
    double* sX = smem + S::oX;
    for (int i = lane; i < D::NP; i += 64) sU[i] = 0.0;
    const int jl = lane < NTH ? lane : 0;     // (lanes >= NTH shadow jet 0 and store nothing)
    const double jon = sA[(12 + jl) * NX + 16 + jl], ja = sA[(16 + jl) * NX + 12 + jl], jb = sA[(16 + jl) * NX + 16 + jl];
    const double c12 = sC[12 + jl], c16 = sC[16 + jl];
    double bt12[NTH], bt16[NTH];
#pragma unroll
    for (int c = 0; c < NTH; ++c) { bt12[c] = sBt[(12 + jl) * NTH + c]; bt16[c] = sBt[(16 + jl) * NTH + c]; }
    double jT = sIn[VSMPC_IN_X0 + 12 + jl], jTd = sIn[VSMPC_IN_X0 + 16 + jl];
    double fa = 0.0, fb = 0.0;   // input terms of the current throttle block
    if (lane < NTH) {
        sX[12 + lane] = jT;
        sX[16 + lane] = jTd;
    }
    static_for<0, D::PVT>([&](auto bcst) __attribute__((always_inline)) {
        constexpr int bi = decltype(bcst)::value;
        __syncthreads();
        if constexpr (bi >= BI0 && bi - BI0 < NCJ) {
            // input terms of the jet rows in place: f = Bt v_{tb(k)} + c (the joints do not reach these rows); v: uniform
            // addresses (LDS broadcasts), shared by the stages of a throttle block
            static_for<0, CHJ>([&](auto ucst) __attribute__((always_inline)) {
                constexpr int k = (bi - BI0) * CHJ + decltype(ucst)::value;
                if constexpr (k < D::N) {
                    constexpr int tb = throttle_block_of_stage<D>(k);
                    constexpr int tb_prev = k == 0 ? -1 : throttle_block_of_stage<D>(k == 0 ? 0 : k - 1);
                    if constexpr (tb != tb_prev) {   // the input term changes with the throttle block only
                        constexpr int vq = tb == 0 ? D::NV - 4 : 4 * (tb - 1);   // internal offset of reference block tb
                        fa = c12;
                        fb = c16;
#pragma unroll
                        for (int c = 0; c < NTH; ++c) {
                            const double vc = sZ[D::NU + vq + c];
                            fa = fma(bt12[c], vc, fa);
                            fb = fma(bt16[c], vc, fb);
                        }
                    }
                    const double dt = sDt[k];
                    const double dT = fma(jon, jTd, fa);
                    const double dTd = fma(ja, jT, fma(jb, jTd, fb));
                    jT = fma(dt, dT, jT);
                    jTd = fma(dt, dTd, jTd);
                    if (lane < NTH) {
                        sX[NX * (k + 1) + 12 + lane] = jT;
                        sX[NX * (k + 1) + 16 + lane] = jTd;
                    }
                }
            });
        }
    });
}

}  // namespace vsmpc
