// Device helpers the rollout's kernels share (vsmpc_rollout.hip: record_kernel, advance_kernel; vsmpc_rollout_adjoint.hip:
// advance_adjoint_kernel): the rotation of the plant's RPY convention, the 3x3 inverse, clamped linear up-sampling and the
// global -> LDS staging of one instance's rows.  The plant state and parameter layouts are VSMPC_PS_* / VSMPC_PP_* of
// include/vsmpc.h; the per-instance tick state is described beside tick_state_doubles in vsmpc_rollout.hip.
#pragma once
#include "vsmpc_device.hpp"

namespace vsmpc {

VS_DEV void rot_from_rpy(const double* rpy, double* R) {  // Rz(yaw) Ry(pitch) Rx(roll), row-major
    double sr, cr, sp, cp, sy, cy;
    sincos(rpy[0], &sr, &cr); sincos(rpy[1], &sp, &cp); sincos(rpy[2], &sy, &cy);
    R[0] = cy * cp; R[1] = cy * sp * sr - sy * cr; R[2] = cy * sp * cr + sy * sr;
    R[3] = sy * cp; R[4] = sy * sp * sr + cy * cr; R[5] = sy * sp * cr - cy * sr;
    R[6] = -sp;     R[7] = cp * sr;                R[8] = cp * cr;
}

VS_DEV void inv3(const double* I, double* Ii) {
    const double a = I[0], b = I[1], c = I[2], d = I[3], e = I[4], f = I[5], g = I[6], h = I[7], k = I[8];
    const double A00 = e * k - f * h, A01 = c * h - b * k, A02 = b * f - c * e;
    const double A10 = f * g - d * k, A11 = a * k - c * g, A12 = c * d - a * f;
    const double A20 = d * h - e * g, A21 = b * g - a * h, A22 = a * e - b * d;
    const double idet = 1.0 / (a * A00 + b * A10 + c * A20);
    Ii[0] = A00 * idet; Ii[1] = A01 * idet; Ii[2] = A02 * idet; Ii[3] = A10 * idet; Ii[4] = A11 * idet;
    Ii[5] = A12 * idet; Ii[6] = A20 * idet; Ii[7] = A21 * idet; Ii[8] = A22 * idet;
}

VS_DEV double interp_clamped(const double* __restrict__ tr, int n, double pos) {  // linear up-sampling, clamped
    if (pos <= 0.0) return tr[0];
    if (pos >= double(n - 1)) return tr[n - 1];
    const int i = int(pos);
    const double f = pos - double(i);
    return tr[i] + f * (tr[i + 1] - tr[i]);
}

// One wavefront per instance.  The plant state and parameters are staged through LDS with coalesced loads, the record
// is assembled in LDS by all 64 lanes (every field is a short independent expression) and written out coalesced.
constexpr int RO_BLOCK = 64;

// global -> LDS staging with all loads in flight before the first store (a load/store loop pays one HBM round trip
// per iteration)
template <int N>
VS_DEV void stage_in(const double* __restrict__ g, double* __restrict__ l, int lane) {
    constexpr int R = (N + RO_BLOCK - 1) / RO_BLOCK;
    double v[R];
#pragma unroll
    for (int k = 0; k < R; ++k) {
        const int i = lane + k * RO_BLOCK;
        v[k] = i < N ? g[i] : 0.0;
    }
#pragma unroll
    for (int k = 0; k < R; ++k) {
        const int i = lane + k * RO_BLOCK;
        if (i < N) l[i] = v[k];
    }
}

}  // namespace vsmpc
