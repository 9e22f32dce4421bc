// Closed-loop batched rollout: the reference's hidden per-tick "advance" on the device.
//
//   record_kernel   builds the per-tick input record of every instance from its plant state, i.e. what
//                   IMPCProblem::update pulls out of Robot/QPInput plus the tick state machine, with the reference's own
//                   call-count semantics (k = number of update() calls before this one; configure() made call 0 of every
//                   plugin, IMPCProblem.cpp:94-96):
//                     measured state X0, RPY unwrapped with      constraintsVSMPC.cpp:206-247
//                       per-instance turn counters
//                     20-tick throttle hold: v0 free on ticks    constraintsVSMPC.cpp:335,351-372
//                       k % 20 == 19
//                     reference window = FIFO of 11 columns,     costsVSMPC.cpp:103-113,121-165
//                       initially all trajectory sample 0; a
//                       new sample enters the LAST column in
//                       configure and on ticks k % 20 == 19 (the
//                       throttle-release tick); its h_lin entry
//                       R^T m v is frozen with the R of the push
//                     alpha-gravity cursor: tick k uses sample   systemDynamicsVSMPC.cpp:308-311,
//                       k + 1 of the x20 linearly up-sampled       TrajectoryManager.cpp:23-39,142-153
//                       track (configure consumed sample 0)
//                     joint posture error                        costsVSMPC.cpp:574-589
//   solve_kernel    (vsmpc_kernels.hip) the MPC solve
//   advance_kernel  consumes the first move only if the status is Solved (variableSamplingMPC.cpp:91-108):
//                   q += dq, throttle / thrust references latched; then integrates a centroidal + jet plant over one
//                   MPC period in 1 ms sub-steps (the harness steps MuJoCo 5 x 1 ms per tick,
//                   src/mujoco_lib/ironcub_mujoco_simulator.py:122-139).
//
// The plant is this repo's synthetic stand-in for the MuJoCo/LSTM simulation (out of scope): the
// same centroidal-momentum model the MPC linearises, but with the non-linear rotation kinematics, the joint-dependent
// (bilinear) jet map A_mom(q) T and the non-linear polynomial jet model (utils/src/JetModel.cpp:29-64), integrated
// explicitly.
#include <type_traits>

#include "vsmpc_device.hpp"
#include "vsmpc_jet_device.hpp"
#include "vsmpc_launch.hpp"
#include "vsmpc_noise_device.hpp"
#include "vsmpc_rollout_device.hpp"

namespace vsmpc {

// Per-instance tick state that survives between ticks, VSMPC tick-state record in HBM:
//   [0, 12 n_ref)   reference window, column-major: col * 12 + (p 0:3 | h_lin 3:6 | rpy 6:9 | h_ang 9:12)
//   + 0..2          m_rpyOld (last measured, wrapped RPY)      constraintsVSMPC.cpp:246
//   + 3..5          m_nTurns                                    constraintsVSMPC.cpp:236-243
VS_HD constexpr int tick_state_doubles(int n_ref) { return 12 * n_ref + 8; }

VS_DEV double wrap_pi(double a) {  // what Rotation::asRPY() returns for an angle the plant integrates continuously
    const double two_pi = 6.283185307179586476925286766559;
    return a - two_pi * rint(a / two_pi);
}

// TrajectoryManager semantics for alpha-gravity: linear up-sampling by `up` (TrajectoryManager.cpp:23-39: the last
// original sample is dropped), cursor advanced once per dynamics evaluation and clamped at the last up-sampled sample
// (:142-153); configure consumed sample 0, so tick k reads sample k + 1.
VS_DEV double alpha_of_tick(const double* __restrict__ tr, int n, int up, int tk) {
    // (a track already at the requested rate is NOT resampled and keeps all n samples, TrajectoryManager.cpp:121-126)
    const int last = up == 1 ? n - 1 : up * (n - 1) - 1;
    int idx = tk + 1;
    idx = idx < last ? idx : last;
    idx = idx > 0 ? idx : 0;
    const int i = idx / up, j = idx - up * i;
    const double v0 = tr[i], v1 = tr[i + 1 < n ? i + 1 : n - 1];
    return v0 + (v1 - v0) * (double(j) / double(up));
}

// Record of tick `tk` from the plant state `s`, the parameters `p` and the tick state `ts` (all in LDS), assembled into
// `r` (LDS) by the 64 lanes of the workgroup; `ts` is advanced to "after update() number tk".  `first` builds the tick
// state itself: what configure() leaves behind, fast-forwarded to tick `tk` for loops that start mid-trajectory (window
// columns frozen with the current R, as if the attitude had been constant before).  Ends with a barrier.
// Tree plant (rd.tree): IB = I_B(q) and amom = A_mom,body(q) of the kinematic tree (LDS copies of the provider's outputs for
// this instance) take the place of the plant parameters; Lambda_lin / Lambda_ang are left to the kinematics kernel, which
// patches them into the finished record from the tree's Jacobians and the thrusts the advance kernel measured.
VS_DEV void assemble_record(const RolloutDev& rd, const double* __restrict__ s, const double* __restrict__ p, int tk,
                            const double* __restrict__ traj_pos, const double* __restrict__ traj_vel,
                            const double* __restrict__ traj_alpha, double* __restrict__ R, double* __restrict__ om,
                            double* __restrict__ ts, double* __restrict__ r, int lane, bool first,
                            const double* __restrict__ IB, const double* __restrict__ amom) {
    const double m = p[VSMPC_PP_MASS];
    const int nref = rd.n_ref, nwin = 12 * rd.n_ref;
    double* rpy_old = ts + nwin;
    double* n_turns = ts + nwin + 3;
    const double two_pi = 6.283185307179586476925286766559;
    if (lane == 0) {
        rot_from_rpy(s + VSMPC_PS_RPY, R);
    } else if (lane == 1) {
        double IBi[9];
        inv3(IB, IBi);
        for (int i = 0; i < 3; ++i)
            om[i] = IBi[3 * i] * s[VSMPC_PS_HANG] + IBi[3 * i + 1] * s[VSMPC_PS_HANG + 1] + IBi[3 * i + 2] * s[VSMPC_PS_HANG + 2];
    } else if (lane >= 2 && lane < 5) {
        // ConstraintInitialState::unwrapRPY (constraintsVSMPC.cpp:232-247) on the wrapped measurement
        const int i = lane - 2;
        const double meas = wrap_pi(s[VSMPC_PS_RPY + i]);
        if (first) {
            n_turns[i] = rint((s[VSMPC_PS_RPY + i] - meas) / two_pi);   // m_rpyOld = initial RPY, turns as flown so far
        } else {
            const double d = meas - rpy_old[i];
            if (d > 3.14159265358979323846) n_turns[i] -= 1.0;
            else if (d < -3.14159265358979323846) n_turns[i] += 1.0;
        }
        rpy_old[i] = meas;
    }
    __syncthreads();
    // window column from trajectory sample `idx` (window_fill_sample / window_push_sample) with the CURRENT attitude and
    // mass (costsVSMPC.cpp:103-113,127-146)
    auto column_entry = [&](int idx, int i) -> double {
        if (i < 3) return p[VSMPC_PP_PINIT + i] + traj_pos[3 * idx + i];   // m_initialCoMPos + positionCoM
        if (i < 6) {                                                        // R^T m v_ref
            const int c = i - 3;
            return R[c] * (m * traj_vel[3 * idx]) + R[3 + c] * (m * traj_vel[3 * idx + 1]) + R[6 + c] * (m * traj_vel[3 * idx + 2]);
        }
        if (i < 9)                                                          // m_initialRPY + RPY trajectory
            return p[VSMPC_PP_RPYINIT + i - 6] + (rd.traj_rpy != nullptr ? rd.traj_rpy[3 * idx + i - 6] : 0.0);
        if (rd.traj_rpyd == nullptr) return 0.0;                            // the shipped RPYDot track is all zero (A.6)
        // m_inertia * m_W * RPYDot with the CURRENT attitude (costsVSMPC.cpp:111-112,143-146,266-286); the locked inertia
        // of this plant is R I_B R^T
        const double r0 = s[VSMPC_PS_RPY], p0 = s[VSMPC_PS_RPY + 1];
        const double d0 = rd.traj_rpyd[3 * idx], d1 = rd.traj_rpyd[3 * idx + 1], d2 = rd.traj_rpyd[3 * idx + 2];
        const double wd[3] = {d0 - sin(p0) * d2, cos(r0) * d1 + cos(p0) * sin(r0) * d2, -sin(r0) * d1 + cos(r0) * cos(p0) * d2};
        double acc = 0.0;
        const int row = i - 9;
        for (int a = 0; a < 3; ++a)
            for (int c = 0; c < 3; ++c) {
                double rw = 0.0;
                for (int j = 0; j < 3; ++j) rw += R[3 * j + c] * wd[j];     // (R^T wd)[c]
                acc += R[3 * row + a] * IB[3 * a + c] * rw;
            }
        return acc;
    };
    if (first) {
        for (int e = lane; e < nwin; e += RO_BLOCK) {
            const int j = e / 12, i = e - 12 * j;
            ts[e] = column_entry(window_fill_sample(rd, tk, j), i);
        }
        __syncthreads();
    }
    if (release_tick(rd, tk)) {   // ReferenceTrackingCost::computeHessianAndGradient, m_counter == ratio - 1
        const int ns = window_push_sample(rd, tk);
        constexpr int KMAX = (12 * MAX_STAGES + RO_BLOCK - 1) / RO_BLOCK;
        double keep[KMAX];
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
            const int e = lane + k * RO_BLOCK;
            const int j = e / 12, i = e - 12 * j;
            keep[k] = e < nwin ? (j + 1 < nref ? ts[e + 12] : column_entry(ns, i)) : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
            const int e = lane + k * RO_BLOCK;
            if (e < nwin) ts[e] = keep[k];
        }
        __syncthreads();
    }
    for (int e = lane; e < nwin; e += RO_BLOCK) r[VSMPC_IN_XREF + e] = ts[e];
    // A_mom(q); Lambda column j = DJ[j] T at the measured thrust
    // (the reference recomputes both from the kinematics each tick, systemDynamicsVSMPC.cpp:159-206,304,321-350)
    if (lane < 24) {
        const double acc = amom_entry(p, s + VSMPC_PS_Q, lane);
        r[VSMPC_IN_AMOM + lane] = rd.tree ? amom[lane] : acc;
    }
    // thrusts and thrust rates as the controller sees them: the plant's own with the polynomial jet plant, the EKF
    // estimates with the NN jet plant (the harness hands the estimate to Robot::setJetThrusts)
    auto meas_T = [&](int i) { return rd.jet_nn ? s[VSMPC_PS_EST + 2 * i] : s[VSMPC_PS_T + i]; };
    auto meas_Td = [&](int i) { return rd.jet_nn ? s[VSMPC_PS_EST + 2 * i + 1] : s[VSMPC_PS_TD + i]; };
    if (lane < 48) {
        const int row = lane >> 3, j = lane & 7;   // row 0..5 of DJ[j] T
        double acc = 0.0;
        for (int c = 0; c < 4; ++c) acc += p[VSMPC_PP_DJ + 24 * j + 4 * row + c] * meas_T(c);
        if (rd.tree) acc = 0.0;   // (patched in afterwards by the kinematics kernel)
        if (row < 3) r[VSMPC_IN_LLIN + 8 * row + j] = acc;
        else r[VSMPC_IN_LANG + 8 * (row - 3) + j] = acc;
    }
    if (lane >= 48 && lane < 57) {                  // I_G = R I_B R^T (world-oriented locked inertia)
        const int i = (lane - 48) / 3, j = (lane - 48) % 3;
        double acc = 0.0;
        for (int a = 0; a < 3; ++a)
            for (int c = 0; c < 3; ++c) acc += R[3 * i + a] * IB[3 * a + c] * R[3 * j + c];
        r[VSMPC_IN_INERTIA + 3 * i + j] = acc;
    }
    // X0 (constraintsVSMPC.cpp:206-230): RPY enters unwrapped
    if (lane < 20)
        r[VSMPC_IN_X0 + lane] = (lane >= 6 && lane < 9) ? rpy_old[lane - 6] + two_pi * n_turns[lane - 6]
                                : (lane >= 16 ? meas_Td(lane - 16) : (lane >= 12 ? meas_T(lane - 12) : s[lane]));
    if (lane >= 20 && lane < 29) r[VSMPC_IN_WRB + lane - 20] = R[lane - 20];
    if (lane >= 32 && lane < 36) {
        const int i = lane - 32;
        r[VSMPC_IN_T0 + i] = meas_T(i);                  // useEstimatedThrust = true (systemDynamicsVSMPC.cpp:401-404)
        r[VSMPC_IN_TD0 + i] = meas_Td(i);
        r[VSMPC_IN_UPREV + i] = s[VSMPC_PS_U + i];
        r[VSMPC_IN_TDES + i] = s[VSMPC_PS_TDES + i];
        r[VSMPC_IN_TDDES + i] = s[VSMPC_PS_TDDES + i];
    }
    if (lane >= 36 && lane < 44) r[VSMPC_IN_QERR + lane - 36] = s[VSMPC_PS_Q + lane - 36] - p[VSMPC_PP_QREF0 + lane - 36];
    if (lane >= 44 && lane < 47) {
        const int i = lane - 44;
        r[VSMPC_IN_OMEGA + i] = om[i];
        r[VSMPC_IN_RPY + i] = rpy_old[i];                // Rotation::asRPY() of the measurement (systemDynamicsVSMPC.cpp:132)
        r[VSMPC_IN_RPYINIT + i] = p[VSMPC_PP_RPYINIT + i];
        r[VSMPC_IN_GRAV + i] = i == 2 ? -9.81 : 0.0;
    }
    if (lane == 47) {
        r[VSMPC_IN_MASS] = m;
        r[VSMPC_IN_ALPHA] = alpha_of_tick(traj_alpha, rd.n_alpha, rd.alpha_up, tk);
        r[VSMPC_IN_HOLD] = release_tick(rd, tk) ? 0.0 : 1.0;   // constraintsVSMPC.cpp:351,366-372
    }
    __syncthreads();
    if (lane < 3) {                                  // QPInput::getPosCoMReference / getRPYReference = column 0 (costsVSMPC.cpp:155-156)
        r[VSMPC_IN_X0 + 20 + lane] = s[VSMPC_PS_P + lane] - r[VSMPC_IN_XREF + lane];
        r[VSMPC_IN_X0 + 23 + lane] = r[VSMPC_IN_X0 + 6 + lane] - r[VSMPC_IN_XREF + 6 + lane];
        r[VSMPC_IN_PREF + lane] = r[VSMPC_IN_XREF + lane];
    }
    __syncthreads();
}

// The rollout's two kernels have a NOISE instantiation each (vsmpc_rollout_set_noise): the record is assembled from the measured
// state (measure_state, with the draws of the tick the record belongs to) and the gust of the tick acts beside the push; the
// plant state in HBM, the log row and the integration stay the true ones.  Without NOISE the last argument is an empty struct
// and the kernels are instruction for instruction what they were before they became templates.
struct NoNoise {};
template <bool NOISE> using NoiseArg = std::conditional_t<NOISE, RolloutNoise, NoNoise>;
template <bool NOISE>
VS_DEV double* noise_lds() {   // the draws of one tick in LDS; no LDS without NOISE
    if constexpr (NOISE) {
        __shared__ double zn[NOISE_LDS];
        return zn;
    } else {
        return nullptr;
    }
}
template <bool NOISE>
__global__ __launch_bounds__(RO_BLOCK) void record_kernel(RolloutDev rd, int batch, const double* __restrict__ state,
                                                           const double* __restrict__ params, const int* __restrict__ tick,
                                                           const double* __restrict__ traj_pos, const double* __restrict__ traj_vel,
                                                           const double* __restrict__ traj_alpha, double* __restrict__ tstate,
                                                           double* __restrict__ rec, NoiseArg<NOISE> nz) {
    __shared__ double s[VSMPC_PLANT_STATE], p[VSMPC_PLANT_PARAMS + 1], R[9], om[3], tIB[9], tAm[24];
    __shared__ double r[VSMPC_IN_XREF + 12 * MAX_STAGES], ts[12 * MAX_STAGES + 8];
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b >= batch) return;
    stage_in<VSMPC_PLANT_STATE>(state + size_t(b) * VSMPC_PLANT_STATE, s, lane);
    stage_in<VSMPC_PLANT_PARAMS>(params + size_t(b) * VSMPC_PLANT_PARAMS, p, lane);
    if (rd.tree) {
        if (lane < 9) tIB[lane] = rd.tree_kout[size_t(b) * VSMPC_KIN_OUT + 48 + lane];
        if (lane >= 32 && lane < 56) tAm[lane - 32] = rd.tree_ro[size_t(b) * VSMPC_RO_SIZE + VSMPC_RO_AMOMB + lane - 32];
    }
    __syncthreads();
    if constexpr (NOISE) {
        double* const zn = noise_lds<true>();
        draw_measurement(nz, b, tick[b], zn, lane);
        measure_state(nz, zn, p[VSMPC_PP_MASS], rd.tree ? tIB : p + VSMPC_PP_INERTIA_B, s, lane);
    }
    assemble_record(rd, s, p, tick[b] + int(p[VSMPC_PP_TICK0]), traj_pos, traj_vel, traj_alpha, R, om, ts, r, lane, true,
                    rd.tree ? tIB : p + VSMPC_PP_INERTIA_B, tAm);
    double* out = rec + size_t(b) * rd.n_in;
    for (int e = lane; e < rd.n_in; e += RO_BLOCK) out[e] = r[e];
    double* tso = tstate + size_t(b) * rd.n_ts;
    for (int e = lane; e < rd.n_ts; e += RO_BLOCK) tso[e] = ts[e];
}

// One wavefront per instance: staging and the joint-dependent jet map in parallel, the short ODE integration in lane 0
// on registers, coalesced write-back.  With `rec_next` the record of the NEXT tick is assembled from the advanced state
// while it is still in LDS (one launch and one staging less per tick than a separate record_kernel).
template <bool NOISE>
__global__ __launch_bounds__(RO_BLOCK) void advance_kernel(RolloutDev rd, int batch, double* __restrict__ state,
                                                            const double* __restrict__ params, int* __restrict__ tick,
                                                            const double* __restrict__ fm, const int* __restrict__ status,
                                                            const int* __restrict__ iters, const double* __restrict__ traj_alpha,
                                                            const RolloutCtl* __restrict__ ctl, int substeps,
                                                            const double* __restrict__ traj_pos,
                                                            const double* __restrict__ traj_vel, double* __restrict__ tstate,
                                                            double* __restrict__ rec_next, NoiseArg<NOISE> nz) {
    __shared__ double s[VSMPC_PLANT_STATE], p[VSMPC_PLANT_PARAMS + 1], f[VSMPC_FM_SIZE], Aq[24], IBi[9], R[9], om[3], tIB[9];
    __shared__ double r[VSMPC_IN_XREF + 12 * MAX_STAGES], ts[12 * MAX_STAGES + 8];
    __shared__ float jw[17 * JET_HMAX + 1];   // LSTM weights of the jet plant option
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b >= batch) return;
    if (rd.jet_nn)
        for (int e = lane; e < 17 * rd.jet_hidden + 1; e += RO_BLOCK) jw[e] = rd.jet_w[e];
    for (int e = lane; e < rd.n_ts; e += RO_BLOCK) ts[e] = tstate[size_t(b) * rd.n_ts + e];
    stage_in<VSMPC_PLANT_STATE>(state + size_t(b) * VSMPC_PLANT_STATE, s, lane);
    stage_in<VSMPC_PLANT_PARAMS>(params + size_t(b) * VSMPC_PLANT_PARAMS, p, lane);
    stage_in<VSMPC_FM_SIZE>(fm + size_t(b) * VSMPC_FM_SIZE, f, lane);
    if (rd.tree && lane < 9) tIB[lane] = rd.tree_kout[size_t(b) * VSMPC_KIN_OUT + 48 + lane];   // I_B(q) of the tree, q = the joints
    double tree_amom = 0.0;                                                                     // AFTER this tick's move
    if (rd.tree && lane < 24) tree_amom = rd.tree_ro[size_t(b) * VSMPC_RO_SIZE + VSMPC_RO_AMOMB + lane];
    const int st = status[b];
    const int tick_before = tick[b];
    // every global load of this kernel is requested as early as possible: each dependent round trip costs ~1.5 us
    double* const log = ctl->log;
    const int tick_base = ctl->tick_base, log_rows = ctl->log_rows;
    double* const zn = noise_lds<NOISE>();   // NOISE: the gust of this tick, the measurement of the next
    if constexpr (NOISE) draw_tick(nz, b, tick_before, zn, lane);
    __syncthreads();
    __shared__ double alpha_s[16];   // alpha-gravity of every sub-step (one round trip instead of one per sub-step)
    if (lane >= 32 && lane < 32 + substeps && lane < 48) {
        const int ss = lane - 32;
        const double t = (double(tick_before + int(p[VSMPC_PP_TICK0])) + double(ss) / double(substeps)) * rd.period_mpc;
        alpha_s[ss] = interp_clamped(traj_alpha, rd.n_alpha, t / rd.alpha_dt);
    }
    if (st == VSMPC_STATUS_SOLVED) consume_move<true>(s, f, lane);
    __syncthreads();
    if (lane < 24) {  // A_mom(q): the joints only move at the tick boundary
        const double acc = amom_entry(p, s + VSMPC_PS_Q, lane);
        Aq[lane] = rd.tree ? tree_amom : acc;
    } else if (lane == 24) {
        inv3(rd.tree ? tIB : p + VSMPC_PP_INERTIA_B, IBi);
    }
    __syncthreads();
    // explicit Euler sub-steps, one state component per lane (20 lanes): substep_preamble, substep_rate
    {
        __shared__ double x[20], Rm[9], omv[3], sc[6], vthr[4];
        const int tk = tick_before + int(p[VSMPC_PP_TICK0]);
        const double m = p[VSMPC_PP_MASS];
        if (lane < 20) x[lane] = s[lane];
        if (lane < 4) vthr[lane] = Jet::v_of_throttle(s[VSMPC_PS_U + lane]);
        __syncthreads();
        const double h = rd.period_mpc / double(substeps);
        for (int ss = 0; ss < substeps; ++ss) {
            const double t = substep_time(rd, tk, ss, substeps);
            const double alpha = alpha_s[ss];
            const bool dist = push_active(p, t);
            if (rd.jet_nn) {
                // jet plant option, one plant step in the order of MujocoSim.step (ironcub_mujoco_simulator.py:128-133,
                // 393-396): the NN advances every jet's thrust from its own previous output (hidden units over the lanes),
                // the jet's EKF takes the NN's (T, Tdot) as measurement, set_thrust(estimated_thrust) -- and only then the
                // body is stepped: the force of THIS sub-step is the EKF estimate of this sub-step.
                const JetNorm nm{rd.jet_norm[0], rd.jet_norm[1], rd.jet_norm[2], rd.jet_norm[3]};
                float Tn_mine = 0.0f, Tdn_mine = 0.0f;
                for (int j = 0; j < 4; ++j) {
                    float x0, x1;
                    jet_normalize(nm, float(s[VSMPC_PS_TNN + j]), float(s[VSMPC_PS_U + j]), x0, x1);
                    const float out = lstm_step_from_zero_wave(jw, rd.jet_hidden, x0, x1, lane);
                    const float Tn = (x0 + out * float(h)) * float(nm.thrust_std) + float(nm.thrust_mean);
                    const float Tdn = out * float(nm.thrust_std);
                    if (lane == j) { Tn_mine = Tn; Tdn_mine = Tdn; }
                }
                __syncthreads();                              // every lane has read s[TNN] before lanes 0..3 update it
                if (lane < 4) {
                    Ekf2 cv;
                    for (int k = 0; k < 4; ++k) { cv.q[k] = rd.ekf_q[k]; cv.r[k] = rd.ekf_r[k]; }
                    double T = s[VSMPC_PS_EST + 2 * lane], Td = s[VSMPC_PS_EST + 2 * lane + 1];
                    double Pm[4] = {s[VSMPC_PS_EKFP + 4 * lane], s[VSMPC_PS_EKFP + 4 * lane + 1],
                                    s[VSMPC_PS_EKFP + 4 * lane + 2], s[VSMPC_PS_EKFP + 4 * lane + 3]};
                    ekf_update_dev(T, Td, Pm, s[VSMPC_PS_U + lane], double(Tn_mine), double(Tdn_mine), h, cv);
                    s[VSMPC_PS_EST + 2 * lane] = T;
                    s[VSMPC_PS_EST + 2 * lane + 1] = Td;
                    for (int k = 0; k < 4; ++k) s[VSMPC_PS_EKFP + 4 * lane + k] = Pm[k];
                    s[VSMPC_PS_TNN + lane] = double(Tn_mine);   // the NN's own feedback state
                    x[12 + lane] = T;                           // set_thrust(self._estimated_thrust)
                    x[16 + lane] = Td;
                }
                __syncthreads();
            }
            substep_preamble(x, IBi, sc, omv, lane);
            __syncthreads();
            const SinCos a = sincos_of(sc);
            if (lane == 0) rot_from_sincos(a, Rm);
            __syncthreads();
            double d = substep_rate(x, Rm, omv, a, Aq, vthr, p, m, alpha, dist, rd.jet_nn, lane);
            if constexpr (NOISE) d += gust_rate(nz, zn, Rm, lane);
            __syncthreads();                                  // every lane has read x before anyone updates it
            if (lane < 20) x[lane] += h * d;
            __syncthreads();
        }
        if (lane < 20) s[lane] = x[lane];
        if (lane == 0) tick[b] = tick_before + 1;
    }
    __syncthreads();
    double* so = state + size_t(b) * VSMPC_PLANT_STATE;
    for (int i = lane; i < VSMPC_PLANT_STATE; i += RO_BLOCK) so[i] = s[i];
    // the log destination comes from a device-side control block, so the launch arguments are the same for every
    // tick and a captured graph of ticks can be replayed
    if (log != nullptr && lane < VSMPC_ROLLOUT_LOG) {
        const int row = tick_before - tick_base;   // ticks since the start of this run
        double v;
        if (lane < 3) v = s[lane];
        else if (lane < 6) v = s[6 + lane - 3];
        else if (lane < 10) v = s[12 + lane - 6];
        else if (lane < 14) v = s[VSMPC_PS_U + lane - 10];
        else if (lane == 14) v = double(st);
        else v = iters ? double(iters[b]) : 0.0;
        // a run that failed half-way leaves the counters ahead: never write outside the log (and never leave the
        // workgroup here: the record of the next tick is assembled below, with barriers)
        if (row >= 0 && row < log_rows) log[(size_t(row) * batch + b) * VSMPC_ROLLOUT_LOG + lane] = v;
    }
    if (rd.tree && lane < 4)   // the thrusts the next tick's Lambda terms are formed with (kinematics kernel, next launch)
        rd.tree_kin[size_t(b) * VSMPC_KIN_SIZE + VSMPC_KIN_THRUST + lane] = rd.jet_nn ? s[VSMPC_PS_EST + 2 * lane] : s[VSMPC_PS_T + lane];
    if (rec_next != nullptr) {
        if constexpr (NOISE) measure_state(nz, zn, p[VSMPC_PP_MASS], rd.tree ? tIB : p + VSMPC_PP_INERTIA_B, s, lane);
        assemble_record(rd, s, p, tick_before + 1 + int(p[VSMPC_PP_TICK0]), traj_pos, traj_vel, traj_alpha, R, om, ts, r, lane, false,
                        rd.tree ? tIB : p + VSMPC_PP_INERTIA_B, Aq);
        double* out = rec_next + size_t(b) * rd.n_in;
        for (int e = lane; e < rd.n_in; e += RO_BLOCK) out[e] = r[e];
        double* tso = tstate + size_t(b) * rd.n_ts;
        for (int e = lane; e < rd.n_ts; e += RO_BLOCK) tso[e] = ts[e];
    }
}

// One Philox block per thread, t = (tick, loop, block) in the order of the outputs: vsmpc_rollout_noise_draws
__global__ __launch_bounds__(RO_BLOCK) void noise_draws_kernel(RolloutNoise nz, int batch, int tick0, long long n,
                                                                double* __restrict__ z, unsigned* __restrict__ words) {
    const long long t = static_cast<long long>(blockIdx.x) * RO_BLOCK + threadIdx.x;
    if (t >= n) return;
    const int j = int(t % NOISE_BLOCKS);
    const long long tb = t / NOISE_BLOCKS;
    unsigned w[4];
    double za, zb;
    noise_block(nz, int(tb % batch), tick0 + int(tb / batch), j, w, za, zb);
    z[2 * t] = za;
    z[2 * t + 1] = zb;
    if (words != nullptr)
        for (int i = 0; i < 4; ++i) words[4 * t + i] = w[i];
}

hipError_t launch_noise_draws(const RolloutNoise& nz, int batch, int tick0, int ticks, double* z, unsigned* words, hipStream_t stream) {
    const long long n = static_cast<long long>(ticks) * batch * NOISE_BLOCKS;
    hipLaunchKernelGGL(noise_draws_kernel, dim3(unsigned((n + RO_BLOCK - 1) / RO_BLOCK)), dim3(RO_BLOCK), 0, stream, nz, batch, tick0, n,
                       z, words);
    return hipGetLastError();
}

// Provider state of the tree plant, one thread per instance: the base frame is the body frame (origin, identity attitude,
// at rest), so that every output of the provider is a body-frame quantity of the joints alone -- A_mom,body(q), the
// Jacobians behind Lambda_lin,B / Lambda_ang,B (systemDynamicsVSMPC.cpp:159-226,321-350 are body-frame expressions) and
// I_B(q).  The joints are the plant's, plus this tick's increments when the solve succeeded (variableSamplingMPC.cpp:
// 104-108): the advance kernel applies the same move and integrates with the A_mom and I_B of the moved joints.
__global__ void tree_state_kernel(RolloutDev rd, int batch, const double* __restrict__ state, const double* __restrict__ fm,
                                  const int* __restrict__ status, double* __restrict__ rs) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    const double* s = state + size_t(b) * VSMPC_PLANT_STATE;
    double* o = rs + size_t(b) * VSMPC_RS_SIZE;
    for (int i = 0; i < VSMPC_RS_SIZE; ++i) o[i] = 0.0;
    o[VSMPC_RS_R + 0] = 1.0; o[VSMPC_RS_R + 4] = 1.0; o[VSMPC_RS_R + 8] = 1.0;
    const bool move = fm != nullptr && status[b] == VSMPC_STATUS_SOLVED;
    for (int j = 0; j < 8; ++j) o[VSMPC_RS_Q + j] = s[VSMPC_PS_Q + j] + (move ? fm[size_t(b) * VSMPC_FM_SIZE + VSMPC_FM_DQ + j] : 0.0);
    for (int i = 0; i < 4; ++i) o[VSMPC_RS_T + i] = rd.jet_nn ? s[VSMPC_PS_EST + 2 * i] : s[VSMPC_PS_T + i];
}

hipError_t launch_tree_state(const RolloutDev& rd, int batch, const double* state, const double* fm, const int* status,
                             double* rs, hipStream_t stream) {
    hipLaunchKernelGGL(tree_state_kernel, dim3((batch + 63) / 64), dim3(64), 0, stream, rd, batch, state, fm, status, rs);
    return hipGetLastError();
}

hipError_t launch_record(const RolloutDev& rd, const RolloutTick& k, hipStream_t stream, const RolloutNoise* nz) {
    if (nz != nullptr)
        hipLaunchKernelGGL(record_kernel<true>, dim3(k.batch), dim3(RO_BLOCK), 0, stream, rd, k.batch, k.state, k.params, k.tick,
                           k.traj_pos, k.traj_vel, k.traj_alpha, k.tstate, k.rec, *nz);
    else
        hipLaunchKernelGGL(record_kernel<false>, dim3(k.batch), dim3(RO_BLOCK), 0, stream, rd, k.batch, k.state, k.params, k.tick,
                           k.traj_pos, k.traj_vel, k.traj_alpha, k.tstate, k.rec, NoNoise{});
    return hipGetLastError();
}

hipError_t launch_advance(const RolloutDev& rd, const RolloutTick& k, hipStream_t stream, const RolloutNoise* nz) {
    if (nz != nullptr)
        hipLaunchKernelGGL(advance_kernel<true>, dim3(k.batch), dim3(RO_BLOCK), 0, stream, rd, k.batch, k.state, k.params, k.tick,
                           k.fm, k.status, k.iters, k.traj_alpha, k.ctl, k.substeps, k.traj_pos, k.traj_vel, k.tstate, k.rec, *nz);
    else
        hipLaunchKernelGGL(advance_kernel<false>, dim3(k.batch), dim3(RO_BLOCK), 0, stream, rd, k.batch, k.state, k.params, k.tick, k.fm,
                           k.status, k.iters, k.traj_alpha, k.ctl, k.substeps, k.traj_pos, k.traj_vel, k.tstate, k.rec, NoNoise{});
    return hipGetLastError();
}

}  // namespace vsmpc
