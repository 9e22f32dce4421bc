// P0 of the solve kernels (linearisation into LDS) and the FP64 helpers it uses; shared by the tuned per-horizon kernels
// (vsmpc_kernels.hip) and the runtime-sized kernel (vsmpc_runtime.hip) so that both linearise with the same formulas.
#pragma once
#include "vsmpc_device.hpp"

namespace vsmpc {

VS_DEV double readlane_f64(double x, int lane) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(x), lane);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(x), lane);
    return __hiloint2double(hi, lo);
}

// 1/sqrt(d) and 1/d: hardware seed + refinement (full double precision to ~2 ulp)
// The v_rsq_f64 / v_rcp_f64 seeds are good to 5e-8 (profiles/r01_microbench_rsq_accuracy.txt).  One cubically
// convergent (Halley) step y (1 + e/2 + 3 e^2/8), e = 1 - d y^2, reaches full precision in 5 instructions; two Newton
// steps need 7.  (With the pivots' reciprocal square roots on the critical path the Halley form measured slower; since
// the panel code overlaps them with the previous pivot's update, the instruction count is what matters.)
VS_DEV double fast_rsqrt(double d) {
    const double y = __builtin_amdgcn_rsq(d);
    const double e = fma(-d * y, y, 1.0);
    return fma(y * e, fma(0.375, e, 0.5), y);
}
VS_DEV double fast_rcp(double d) {
    double y = __builtin_amdgcn_rcp(d);
    y = y * fma(-d, y, 2.0);
    y = y * fma(-d, y, 2.0);
    return y;
}

// ------------------------------------------------------------------------------------------------
// P0: linearisation into LDS (dense, row-major) — also the body of the linearise-only kernel
// ------------------------------------------------------------------------------------------------
// LAMBDA_BJ = false (the solve kernel): Bj is not filled with Lambda here -- p0_joint_reduction writes the reduced input
// matrix R^T into it instead.
template <bool ZERO = true, bool SYNC = true, bool LAMBDA_BJ = true>
VS_DEV void p0_linearize(int use_jet, const double* __restrict__ sIn, double* __restrict__ sA,
                         double* __restrict__ sBj, double* __restrict__ sBt, double* __restrict__ sC,
                         double* __restrict__ sVprev, int tid, int nthreads) {
    if constexpr (ZERO) {
        for (int i = tid; i < NX * NX + NX * NJ + NX * NTH + 28; i += nthreads) sA[i] = 0.0;  // A,Bj,Bt,c contiguous
        __syncthreads();
    }
    // The independent pieces run in different wavefronts (0: attitude kinematics, 1: jets, 2: CoM / gravity, 2-3: copies)
    // so that their divergent paths overlap instead of serialising inside one wavefront; needs >= 256 threads.
    if (tid < 64) {
        // A[rpy, angMom] = W(rpy)^-1 * I_G^-1                       (systemDynamicsVSMPC.cpp:86-87,140-147)
        // One wavefront: even lanes take sin / cos of the roll, odd lanes of the pitch (ONE sincos instead of two in a row:
        // it is the longest dependent chain of P0), lanes 0..8 then form one entry (i, j) each.
        const double* I = sIn + VSMPC_IN_INERTIA;
        const double a = I[0], b = I[1], c = I[2], d = I[3], e = I[4], f = I[5], g = I[6], h = I[7], k = I[8];
        double sn, cs;
        sincos(sIn[VSMPC_IN_RPY + (tid & 1)], &sn, &cs);
        const double A00 = e * k - f * h, A01 = c * h - b * k, A02 = b * f - c * e;
        const double A10 = f * g - d * k, A11 = a * k - c * g, A12 = c * d - a * f;
        const double A20 = d * h - e * g, A21 = b * g - a * h, A22 = a * e - b * d;
        const double idet = fast_rcp(a * A00 + b * A10 + c * A20);
        const double sr = readlane_f64(sn, 0), cr = readlane_f64(cs, 0), sp = readlane_f64(sn, 1), cp = readlane_f64(cs, 1);
        const double icp = fast_rcp(cp), tp = sp * icp;
        const int i = tid / 3, j = tid - 3 * i;                      // entry (i, j), tid < 9
        // row i of W^-1 = [1, sr tp, cr tp; 0, cr, -sr; 0, sr / cp, cr / cp], column j of I^-1 = adj[:, j] / det
        const double w0 = i == 0 ? 1.0 : 0.0;
        const double w1 = i == 0 ? sr * tp : (i == 1 ? cr : sr * icp);
        const double w2 = i == 0 ? cr * tp : (i == 1 ? -sr : cr * icp);
        const double c0 = j == 0 ? A00 : (j == 1 ? A01 : A02);
        const double c1 = j == 0 ? A10 : (j == 1 ? A11 : A12);
        const double c2 = j == 0 ? A20 : (j == 1 ? A21 : A22);
        if (tid < 9) sA[(6 + i) * NX + 9 + j] = (w0 * c0 + w1 * c1 + w2 * c2) * idet;
    } else if (tid >= 64 && tid < 68) {
        // jets                                                      (systemDynamicsVSMPC.cpp:384-429)
        const int i = tid - 64;
        sVprev[i] = Jet::v_of_throttle_div(sIn[VSMPC_IN_UPREV + i]);
        if (use_jet) {
            const double T0 = sIn[VSMPC_IN_T0 + i], Td0 = sIn[VSMPC_IN_TD0 + i], up = sIn[VSMPC_IN_UPREV + i];
            const double dhT = Jet::dh_dT(T0, Td0, up), dhTd = Jet::dh_dTd(T0, Td0, up);
            sA[(12 + i) * NX + 16 + i] = 1.0;
            sA[(16 + i) * NX + 12 + i] = dhT;
            sA[(16 + i) * NX + 16 + i] = dhTd;
            sBt[(16 + i) * NTH + i] = Jet::G(sIn[VSMPC_IN_TDES + i], sIn[VSMPC_IN_TDDES + i]);
            sC[16 + i] = Jet::F(T0, Td0) - dhT * T0 - dhTd * Td0;
        } else {
            sBt[(12 + i) * NTH + i] = 1.0;
        }
    } else if (tid == 128) {
        // CoM kinematics, -S(omega) blocks, gravity term, integrators  (systemDynamicsVSMPC.cpp:90-91,296-316)
        const double m = sIn[VSMPC_IN_MASS], im = fast_rcp(m);
        const double* R = sIn + VSMPC_IN_WRB;
        const double* w = sIn + VSMPC_IN_OMEGA;
        const double* gr = sIn + VSMPC_IN_GRAV;
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) sA[i * NX + 3 + j] = im * R[3 * i + j];
        const double S[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};  // FlightControlUtils.cpp:77-85
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                sA[(3 + i) * NX + 3 + j] = -S[3 * i + j];
                sA[(9 + i) * NX + 9 + j] = -S[3 * i + j];
            }
        const double am = sIn[VSMPC_IN_ALPHA] * m;
        for (int i = 0; i < 3; ++i) {
            sC[3 + i] = am * (R[0 + i] * gr[0] + R[3 + i] * gr[1] + R[6 + i] * gr[2]);  // alpha*m*R^T g
            sA[(20 + i) * NX + i] = 1.0;
            sA[(23 + i) * NX + 6 + i] = 1.0;
            sC[20 + i] = -sIn[VSMPC_IN_PREF + i];
            sC[23 + i] = -sIn[VSMPC_IN_RPYINIT + i];
        }
    } else if (tid >= 192 && tid < 216) {
        // thrust maps A[linMom|angMom, T] = A_mom,body                (systemDynamicsVSMPC.cpp:92-93,303-304)
        const int e = tid - 192, r = e >> 2, j = e & 3;  // r in 0..5
        const int row = r < 3 ? 3 + r : 6 + r;         // 3..5, 9..11
        sA[row * NX + 12 + j] = sIn[VSMPC_IN_AMOM + e];
    } else if (LAMBDA_BJ && tid >= 216 && tid < 240) {
        const int e = tid - 216, r = e >> 3, j = e & 7;  // Lambda_lin,B -> Bj[3..5]   (:305-306)
        sBj[(3 + r) * NJ + j] = sIn[VSMPC_IN_LLIN + e];
    } else if (LAMBDA_BJ && tid >= 136 && tid < 160) {
        const int e = tid - 136, r = e >> 3, j = e & 7;  // Lambda_ang,B -> Bj[9..11]  (:94-95)
        sBj[(9 + r) * NJ + j] = sIn[VSMPC_IN_LANG + e];
    }
    if constexpr (SYNC) __syncthreads();
}

}  // namespace vsmpc
