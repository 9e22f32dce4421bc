// Device code the rollout's kernels share (vsmpc_rollout.hip: record_kernel, advance_kernel; vsmpc_rollout_adjoint.hip:
// advance_adjoint_kernel), one copy of each formula that has to agree between the loop and its transpose: the rotation of the
// plant's RPY convention (SinCos, rot_from_sincos), the consumed move, A_mom(q), the explicit Euler sub-step (its time and
// push window; substep_preamble, substep_rate) and which trajectory sample a window column holds;
// beside them the 3x3 inverse, clamped linear up-sampling, the two samples it and the alpha-gravity cursor read (Lerp, for the
// transposes) and the global -> LDS staging of one instance's rows.  The plant state
// and parameter layouts are VSMPC_PS_* / VSMPC_PP_* of include/vsmpc.h; the per-instance tick state is described beside
// tick_state_doubles in vsmpc_rollout.hip.
#pragma once
#include "vsmpc_device.hpp"
#include "vsmpc_launch.hpp"

namespace vsmpc {

struct SinCos { double sr, cr, sp, cp, sy, cy; };   // of roll, pitch, yaw

VS_DEV SinCos sincos_of(const double* sc) { return {sc[0], sc[1], sc[2], sc[3], sc[4], sc[5]}; }   // as substep_preamble leaves them

VS_DEV void rot_from_sincos(const SinCos& a, double* R) {  // Rz(yaw) Ry(pitch) Rx(roll), row-major
    const double sr = a.sr, cr = a.cr, sp = a.sp, cp = a.cp, cy = a.cy, sy = a.sy;
    R[0] = cy * cp; R[1] = cy * sp * sr - sy * cr; R[2] = cy * sp * cr + sy * sr;
    R[3] = sy * cp; R[4] = sy * sp * sr + cy * cr; R[5] = sy * sp * cr - cy * sr;
    R[6] = -sp;     R[7] = cp * sr;                R[8] = cp * cr;
}

VS_DEV SinCos sincos_of_rpy(const double* rpy) {
    SinCos a;
    sincos(rpy[0], &a.sr, &a.cr); sincos(rpy[1], &a.sp, &a.cp); sincos(rpy[2], &a.sy, &a.cy);
    return a;
}

VS_DEV void rot_from_rpy(const double* rpy, double* R) { rot_from_sincos(sincos_of_rpy(rpy), R); }

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

// Which two samples a linearly up-sampled track value reads, for the transposes: v = tr[i0] + f (tr[i1] - tr[i0]), so a cotangent
// g of v hands (1 - f) g to sample i0 and f g to sample i1 (a clamped end: i0 == i1, f = 0)
struct Lerp { int i0, i1; double f; };
VS_DEV Lerp interp_lerp(int n, double pos) {   // of interp_clamped: keep the two together
    if (pos <= 0.0) return {0, 0, 0.0};
    if (pos >= double(n - 1)) return {n - 1, n - 1, 0.0};
    const int i = int(pos);
    return {i, i + 1, pos - double(i)};
}

// of alpha_of_tick (vsmpc_rollout.hip, where the semantics are described; the forward kernels keep their own copy of the
// index arithmetic so that their code does not move): tick tk reads sample tk + 1 of the track up-sampled by `up`
VS_DEV Lerp alpha_tick_lerp(int n, int up, int tk) {
    const int last = up == 1 ? n - 1 : up * (n - 1) - 1;
    int idx = tk + 1;
    idx = idx < last ? idx : last;
    idx = idx > 0 ? idx : 0;
    const int i = idx / up, j = idx - up * i;
    return {i, i + 1 < n ? i + 1 : n - 1, double(j) / double(up)};
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

// ---- the reference window (costsVSMPC.cpp:103-113,121-165) --------------------------------------------------------------
// the throttle-release tick, on which the window shifts and a new sample enters its last column (m_counter == ratio - 1)
VS_DEV bool release_tick(const RolloutDev& rd, int tk) { return tk % rd.ratio == rd.ratio - 1; }

// Trajectory sample in column j of a window built at tick tk.  Shifts made before update() number tk: the one of configure +
// one per earlier release tick; shift number s pushed trajectory sample min(s, n_traj - 1), the initial fill is sample 0.
VS_DEV int window_fill_sample(const RolloutDev& rd, int tk, int j) {
    const int ns0 = 1 + tk / rd.ratio;
    int idx = ns0 - (rd.n_ref - 1 - j);
    idx = idx > 0 ? idx : 0;
    return idx < rd.n_traj ? idx : rd.n_traj - 1;
}
VS_DEV int window_push_sample(const RolloutDev& rd, int tk) {   // the sample release tick tk pushes
    const int idx = 1 + (tk + 1) / rd.ratio;
    return idx < rd.n_traj ? idx : rd.n_traj - 1;
}

// ---- one tick of the plant, as advance_kernel flies it -------------------------------------------------------------------
// The first move is consumed only if the status is Solved (variableSamplingMPC.cpp:91-108): q += dq in lanes 0..7, the
// throttle latched in lanes 8..11 -- with REFS the thrust references beside it, which no derivative of the plant reads.
template <bool REFS>
VS_DEV void consume_move(double* s, const double* f, int lane) {
    if (lane < 8) s[VSMPC_PS_Q + lane] += f[VSMPC_FM_DQ + lane];
    if (lane >= 8 && lane < 12) {
        const int i = lane - 8;
        s[VSMPC_PS_U + i] = f[VSMPC_FM_THROTTLE + i];
        if (REFS) {
            s[VSMPC_PS_TDES + i] = f[VSMPC_FM_THRUST + i];
            s[VSMPC_PS_TDDES + i] = f[VSMPC_FM_THRUSTDOT + i];
        }
    }
}

// entry l of A_mom(q) = A_mom0 + sum_j DJ[j] (q_j - q_ref0_j), row-major 6 x 4 (systemDynamicsVSMPC.cpp:159-206,304)
VS_DEV double amom_entry(const double* p, const double* q, int l) {
    double acc = p[VSMPC_PP_AMOM0 + l];
    for (int j = 0; j < 8; ++j) acc += p[VSMPC_PP_DJ + 24 * j + l] * (q[j] - p[VSMPC_PP_QREF0 + j]);
    return acc;
}

VS_DEV double substep_time(const RolloutDev& rd, int tk, int ss, int substeps) {
    const double ticks = double(tk) + double(ss) / double(substeps);
    return ticks * rd.period_mpc;
}
VS_DEV bool push_active(const double* p, double t) { return t >= p[VSMPC_PP_DIST_T0] && t < p[VSMPC_PP_DIST_T1]; }

// Explicit Euler sub-step, one component of the 20-vector x = (p, h_lin, rpy, h_ang, T, Tdot) per lane.  Preamble: the three
// sincos run side by side in lanes 0..2 (sc: sin, cos of roll | pitch | yaw), the body rates omega = I_B^-1 h_ang in lanes
// 8..10.  A barrier, R from sincos_of(sc) in one lane, another barrier; then every lane forms the rate of its own component.
VS_DEV void substep_preamble(const double* x, const double* IBi, double* sc, double* omv, int lane) {
    if (lane < 3) {
        double sn, cs;
        sincos(x[6 + lane], &sn, &cs);
        sc[2 * lane] = sn;
        sc[2 * lane + 1] = cs;
    } else if (lane >= 8 && lane < 11) {
        const int i = lane - 8;
        omv[i] = IBi[3 * i] * x[9] + IBi[3 * i + 1] * x[10] + IBi[3 * i + 2] * x[11];
    }
}
// d x[lane] / dt (0 in the lanes behind the 20).  Aq = A_mom(q), vthr = v(u) of the four throttles, p the plant parameters, m the
// mass among them (read once, in front of the sub-steps); with jet_nn the thrusts follow the jet plant option's NN, not an ODE.
VS_DEV double substep_rate(const double* x, const double* R, const double* omv, const SinCos& a, const double* Aq, const double* vthr,
                           const double* p, double m, double alpha, bool dist, bool jet_nn, int lane) {
    double d = 0.0;
    if (lane < 3) {                                   // p' = R h_lin / m
        d = (R[3 * lane] * x[3] + R[3 * lane + 1] * x[4] + R[3 * lane + 2] * x[5]) / m;
    } else if (lane < 6 || (lane >= 9 && lane < 12)) { // momentum rates: -omega x h + A_mom(q) T (+ gravity, push)
        const bool lin = lane < 6;
        const int r = lin ? lane - 3 : lane - 9, h0 = lin ? 3 : 9;
        const int r1 = (r + 1) % 3, r2 = (r + 2) % 3;
        const double cross = omv[r1] * x[h0 + r2] - omv[r2] * x[h0 + r1];   // (omega x h)[r]
        double f = -cross;
        if (lin) f += alpha * m * (R[6 + r] * (-9.81));                     // alpha m R^T g, g = (0,0,-9.81)
        for (int j = 0; j < 4; ++j) f += Aq[4 * (lin ? r : 3 + r) + j] * x[12 + j];
        if (dist)
            f += lin ? R[r] * p[VSMPC_PP_DIST_F] + R[3 + r] * p[VSMPC_PP_DIST_F + 1] + R[6 + r] * p[VSMPC_PP_DIST_F + 2]
                     : p[VSMPC_PP_DIST_TAU + r];
        d = f;
    } else if (lane < 9) {                            // rpy' = W^-1 omega (systemDynamicsVSMPC.cpp:140-147)
        const double tp = a.sp / a.cp;
        d = lane == 6 ? omv[0] + a.sr * tp * omv[1] + a.cr * tp * omv[2]
          : lane == 7 ? a.cr * omv[1] - a.sr * omv[2]
                      : (a.sr * omv[1] + a.cr * omv[2]) / a.cp;
    } else if (jet_nn) {                              // thrusts follow the NN, not an ODE
        d = 0.0;
    } else if (lane < 16) {                           // T' = Tdot
        d = x[lane + 4];
    } else if (lane < 20) {                           // T'' = sigma_T (f + g v(u))  (JetModel.cpp:29-64)
        const int j = lane - 16;
        const double Tb = Jet::stdT(x[12 + j]), Tdb = Jet::stdTd(x[16 + j]);
        d = Jet::sgT * (Jet::f(Tb, Tdb) + Jet::g(Tb, Tdb) * vthr[j]);
    }
    return d;
}

}  // namespace vsmpc
