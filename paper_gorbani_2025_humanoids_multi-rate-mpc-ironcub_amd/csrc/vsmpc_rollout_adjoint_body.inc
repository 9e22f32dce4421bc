// Device code of the rollout's backward sweep: the helpers and the body of advance_adjoint_kernel, compiled once per plant.
// The including unit names the kernel (VS_ADJ_KERNEL) and says whether it is the kinematic-tree plant's (VS_ADJ_TREE, false /
// true): vsmpc_rollout_adjoint.hip the parametric plant's, vsmpc_rollout_tree_adjoint.hip the tree's.  Two units, because a
// second kernel family in one code object moves the first one's code (LDS and address arithmetic are laid out per module).
// R(rpy) of rot_from_sincos, and its partials to roll, pitch, yaw: dR + 9 a, row-major
VS_DEV void rot_partials(const SinCos& a, double* R, double* dR) {
    const double sr = a.sr, cr = a.cr, sp = a.sp, cp = a.cp, sy = a.sy, cy = a.cy;
    rot_from_sincos(a, R);
    dR[0] = 0.0; dR[1] = cy * sp * cr + sy * sr; dR[2] = -cy * sp * sr + sy * cr;
    dR[3] = 0.0; dR[4] = sy * sp * cr - cy * sr; dR[5] = -sy * sp * sr - cy * cr;
    dR[6] = 0.0; dR[7] = cp * cr;                dR[8] = -cp * sr;
    dR[9] = -cy * sp;  dR[10] = cy * cp * sr; dR[11] = cy * cp * cr;
    dR[12] = -sy * sp; dR[13] = sy * cp * sr; dR[14] = sy * cp * cr;
    dR[15] = -cp;      dR[16] = -sp * sr;     dR[17] = -sp * cr;
    dR[18] = -sy * cp; dR[19] = -sy * sp * sr - cy * cr; dR[20] = -sy * sp * cr + cy * sr;
    dR[21] = cy * cp;  dR[22] = cy * sp * sr - sy * cr;  dR[23] = cy * sp * cr + sy * sr;
    dR[24] = 0.0;      dR[25] = 0.0;                     dR[26] = 0.0;
}

// (dR_a w) . (m v): what a window column's h_lin entry R^T m v_ref, with cotangent w, hands to rpy component a
VS_DEV double hlin_to_rpy(const double* __restrict__ dRa, const double* __restrict__ w, const double* __restrict__ v, double m) {
    double acc = 0.0;
    for (int r = 0; r < 3; ++r) acc += (dRa[3 * r] * w[0] + dRa[3 * r + 1] * w[1] + dRa[3 * r + 2] * w[2]) * (m * v[r]);
    return acc;
}

// w . (R^T v): what a window column's h_lin entry R^T m v_ref, with cotangent w, hands to the mass
VS_DEV double hlin_to_mass(const double* __restrict__ R, const double* __restrict__ w, const double* __restrict__ v) {
    double acc = 0.0;
    for (int c = 0; c < 3; ++c) acc += w[c] * (R[c] * v[0] + R[3 + c] * v[1] + R[6 + c] * v[2]);
    return acc;
}
// (R w)[r] of a row-major R
VS_DEV double rot_row(const double* __restrict__ R, const double* __restrict__ w, int r) {
    return R[3 * r] * w[0] + R[3 * r + 1] * w[1] + R[3 * r + 2] * w[2];
}

// ---- the track rows of the PT instantiation --------------------------------------------------------------------------------
// One launch touches few samples of grad_traj: those of the window columns whose cotangent becomes complete in its record half
// (slots 0 .. n_ref - 1: the columns of the `first` fill; slot n_ref: the column a release tick pushed) and those the two
// alpha-gravity look-ups read (elements 0, 1: alpha_of_tick of the record half; 2 .. 4: the three samples the sub-steps of the
// plant half can reach, since one tick never spans more than one sample interval).  Clamped ends put several slots on one
// sample: the first of them owns it.  The owner loads the sample's running sum in front of the first barrier and, at the end,
// adds the slots of that sample in slot order and stores it -- one lane, a fixed order, no atomics.
VS_DEV int slot_sample(const RolloutDev& rd, int tk, bool first, int ws) {   // -1: the slot is not live in this launch
    if (ws < rd.n_ref) return first ? window_fill_sample(rd, tk, ws) : -1;
    return release_tick(rd, tk) ? window_push_sample(rd, tk) : -1;
}
VS_DEV bool slot_owner(const RolloutDev& rd, int tk, bool first, int ws, int idx) {
    for (int w2 = 0; w2 < ws; ++w2)
        if (slot_sample(rd, tk, first, w2) == idx) return false;
    return true;
}
constexpr int ALPHA_ELEMS = 5;
// tkr, tkp: the launch's record and plant ticks with PP_TICK0 added, or -1; ai0: the lower sample of the plant tick's first sub-step
VS_DEV int alpha_elem_sample(const RolloutDev& rd, int tkr, int tkp, int ai0, int e) {
    if (e < 2) {
        if (tkr < 0) return -1;
        const Lerp l = alpha_tick_lerp(rd.n_alpha, rd.alpha_up, tkr);
        return e == 0 ? l.i0 : l.i1;
    }
    if (tkp < 0) return -1;
    const int i = ai0 + e - 2;
    return i < rd.n_alpha ? i : rd.n_alpha - 1;
}
VS_DEV bool alpha_elem_owner(const RolloutDev& rd, int tkr, int tkp, int ai0, int e, int idx) {
    for (int e2 = 0; e2 < e; ++e2)
        if (alpha_elem_sample(rd, tkr, tkp, ai0, e2) == idx) return false;
    return true;
}
// where component c (0..2 position, 3..5 velocity) of trajectory sample idx lives in a row of grad_traj
VS_DEV size_t traj_entry(const RolloutDev& rd, int idx, int c) { return size_t(c < 3 ? 0 : 3 * rd.n_traj) + size_t(3 * idx + (c < 3 ? c : c - 3)); }

// One wavefront per instance, as advance_kernel.  Every global load is requested in front of the first barrier.
// PT (vsmpc_rollout_backward_full) also accumulates dL/d(plant parameters) and dL/d(tracks) of the instance: the parameter row
// lives in LDS for the launch, the touched track samples as described above.  Without PT nothing of that is compiled in.
// TREE (the kinematic-tree plant, vsmpc_rollout_set_tree_ex with VSMPC_TREE_ADJOINT): A_mom, Lambda and I_B of both halves
// are tau = terms(q, T) at the state between them (a.tree_terms) instead of the parameter record's, and their cotangents --
// the record half's (A_mom, Lambda, I_B through I_G and omega), then the sub-steps' (A_mom, I_B through omega) -- are pulled
// back through J = d tau / d(q | T) (a.tree_jac): Lambda's to the thrusts in front of the sub-steps, everything to the joints,
// where the move shares it when the tick was Solved.  The parameter blocks the tree plant does not read get nothing.
// Without TREE nothing of that is compiled in.
template <bool PT>
__global__ __launch_bounds__(RO_BLOCK) void VS_ADJ_KERNEL(RolloutDev rd, RolloutAdj a) {
    constexpr bool TREE = VS_ADJ_TREE;
    __shared__ double s[VSMPC_PLANT_STATE], p[VSMPC_PLANT_PARAMS + 1], f[VSMPC_FM_SIZE], sb[VSMPC_PLANT_STATE];
    __shared__ double gi[VSMPC_IN_XREF + 12 * MAX_STAGES], wb[12 * MAX_STAGES];
    __shared__ double R[9], dR[27], IBi[9], Aq[24], Ab[24], vb[4], vthr[4], alpha_s[16];
    __shared__ double xs[16 * 20], lam[20], sc[6], omv[3], omb[3];
    // PT: cotangent of the parameters; of the window slots' trajectory samples (6 per slot); of the alpha elements
    __shared__ double gp[PT ? VSMPC_PLANT_PARAMS + 1 : 1], tc[PT ? 6 * (MAX_STAGES + 1) : 1], ac[PT ? ALPHA_ELEMS + 1 : 1];
    // TREE: tau, J, and the sub-steps' cotangent of I_B
    __shared__ double tt[TREE ? VSMPC_TT_SIZE + 1 : 1], tj[TREE ? VSMPC_TT_SIZE * VSMPC_TT_NDIR : 1], tib[TREE ? 9 : 1];
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b >= a.batch) return;
    const bool rec = a.tick_rec >= 0, plant = a.tick_plant >= 0;
    const int nref = rd.n_ref, nwin = 12 * rd.n_ref;
    constexpr int KT = (6 * (MAX_STAGES + 1) + RO_BLOCK - 1) / RO_BLOCK;
    double tpre[KT], apre = 0.0;   // PT: the running sums of the samples this lane owns
    int tkr = -1, tkp = -1, ai0 = 0;
    if constexpr (PT) {
        stage_in<VSMPC_PLANT_PARAMS>(a.gpar + size_t(b) * VSMPC_PLANT_PARAMS, gp, lane);
        // which samples the launch touches hangs on the instance's own PP_TICK0: one dependent round trip, still in front of
        // the first barrier
        const int tick0 = int(a.params[size_t(b) * VSMPC_PLANT_PARAMS + VSMPC_PP_TICK0]);
        const double* gt = a.gtraj + size_t(b) * size_t(6 * rd.n_traj + rd.n_alpha);
        if (rec) tkr = a.tick_rec + tick0;
        if (plant) {
            tkp = a.tick_plant + tick0;
            ai0 = interp_lerp(rd.n_alpha, substep_time(rd, tkp, 0, a.substeps) / rd.alpha_dt).i0;
        }
#pragma unroll
        for (int k = 0; k < KT; ++k) {
            const int e = lane + k * RO_BLOCK, ws = e / 6, c = e - 6 * ws;
            tpre[k] = 0.0;
            if (rec && ws <= nref) {
                const int idx = slot_sample(rd, tkr, a.first, ws);
                if (idx >= 0 && slot_owner(rd, tkr, a.first, ws, idx)) tpre[k] = gt[traj_entry(rd, idx, c)];
            }
        }
        if (lane < ALPHA_ELEMS) {
            const int idx = alpha_elem_sample(rd, tkr, tkp, ai0, lane);
            if (idx >= 0 && alpha_elem_owner(rd, tkr, tkp, ai0, lane, idx)) apre = gt[6 * rd.n_traj + idx];
        }
    }
    if constexpr (TREE) {
        stage_in<VSMPC_TT_SIZE>(a.tree_terms + size_t(b) * VSMPC_TT_SIZE, tt, lane);
        stage_in<VSMPC_TT_SIZE * VSMPC_TT_NDIR>(a.tree_jac + size_t(b) * (VSMPC_TT_SIZE * VSMPC_TT_NDIR), tj, lane);
    }
    stage_in<VSMPC_PLANT_STATE>(a.sbar + size_t(b) * VSMPC_PLANT_STATE, sb, lane);
    stage_in<VSMPC_PLANT_PARAMS>(a.params + size_t(b) * VSMPC_PLANT_PARAMS, p, lane);
    for (int e = lane; e < nwin; e += RO_BLOCK) wb[e] = a.wbar[size_t(b) * nwin + e];
    if (rec) {
        stage_in<VSMPC_PLANT_STATE>(a.s_rec + size_t(b) * VSMPC_PLANT_STATE, s, lane);
        for (int e = lane; e < rd.n_in; e += RO_BLOCK) gi[e] = a.gin[size_t(b) * rd.n_in + e];
        if (lane < VSMPC_GRAD_SIZE) a.gcfg[size_t(b) * VSMPC_GRAD_SIZE + lane] += a.gcfg_t[size_t(b) * VSMPC_GRAD_SIZE + lane];
        if (lane == VSMPC_GRAD_SIZE) a.flags[b] |= a.flags_t[b];
    }
    // the plant half's rows wait in registers until the record half is through with `s`
    double sp0 = 0.0, sp1 = 0.0, fm = 0.0, lbar = 0.0;
    int st = 0;
    if (plant) {
        sp0 = a.s_plant[size_t(b) * VSMPC_PLANT_STATE + lane];
        if (lane + RO_BLOCK < VSMPC_PLANT_STATE) sp1 = a.s_plant[size_t(b) * VSMPC_PLANT_STATE + lane + RO_BLOCK];
        if (lane < VSMPC_FM_SIZE) fm = a.fm[size_t(b) * VSMPC_FM_SIZE + lane];
        st = a.status[b];
        if (a.log_bar != nullptr && lane < 14) lbar = a.log_bar[size_t(b) * VSMPC_ROLLOUT_LOG + lane];
    }
    __syncthreads();
    const double m = p[VSMPC_PP_MASS];
    const double* DJ = p + VSMPC_PP_DJ;

    if (rec) {
        const int tk = a.tick_rec + int(p[VSMPC_PP_TICK0]);
        if (lane == 0) {
            double sr, cr, sp, cp, sy, cy;
            sincos(s[VSMPC_PS_RPY], &sr, &cr); sincos(s[VSMPC_PS_RPY + 1], &sp, &cp); sincos(s[VSMPC_PS_RPY + 2], &sy, &cy);
            rot_partials({sr, cr, sp, cp, sy, cy}, R, dR);
        } else if (lane == 1) {
            if constexpr (TREE) inv3(tt + VSMPC_TT_IB, IBi);
            else inv3(p + VSMPC_PP_INERTIA_B, IBi);
        }
        for (int e = lane; e < nwin; e += RO_BLOCK) wb[e] += gi[VSMPC_IN_XREF + e];
        __syncthreads();
        if (lane < 3) {   // X0[20:26] and PREF read column 0 of the window
            wb[lane] += gi[VSMPC_IN_PREF + lane] - gi[VSMPC_IN_X0 + 20 + lane];
            wb[6 + lane] -= gi[VSMPC_IN_X0 + 23 + lane];
        }
        __syncthreads();
        double add = 0.0;
        if (lane < 20) add = gi[VSMPC_IN_X0 + lane];               // X0: identity (the unwrapped RPY has derivative 1)
        if (lane < 3) {
            add += gi[VSMPC_IN_X0 + 20 + lane];
        } else if (lane >= 6 && lane < 9) {
            const int c = lane - 6;
            const double* dRa = dR + 9 * c;
            const double* IB = TREE ? tt + VSMPC_TT_IB : p + VSMPC_PP_INERTIA_B;
            add += gi[VSMPC_IN_X0 + 23 + c] + gi[VSMPC_IN_RPY + c];
            for (int k = 0; k < 9; ++k) add += gi[VSMPC_IN_WRB + k] * dRa[k];
            // I_G = R I_B R^T: sum_ij G_ij (dR_a I_B R^T + R I_B dR_a^T)_ij
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) {
                    double t = 0.0;
                    for (int u = 0; u < 3; ++u)
                        for (int v = 0; v < 3; ++v)
                            t += (dRa[3 * i + u] * R[3 * j + v] + R[3 * i + u] * dRa[3 * j + v]) * IB[3 * u + v];
                    add += gi[VSMPC_IN_INERTIA + 3 * i + j] * t;
                }
            if (release_tick(rd, tk)) {   // the column this tick pushed, at this tick's R
                const int idx = window_push_sample(rd, tk);
                add += hlin_to_rpy(dRa, wb + 12 * (nref - 1) + 3, a.traj_vel + 3 * idx, m);
            }
        } else if (lane >= 9 && lane < 12) {
            const int c = lane - 9;
            add += IBi[c] * gi[VSMPC_IN_OMEGA] + IBi[3 + c] * gi[VSMPC_IN_OMEGA + 1] + IBi[6 + c] * gi[VSMPC_IN_OMEGA + 2];
        } else if (lane >= 12 && lane < 16) {                       // T: T0 and Lambda column j = DJ[j] T
            const int c = lane - 12;
            add += gi[VSMPC_IN_T0 + c];
            if constexpr (TREE) {                                   // Lambda(q, T) is linear in T: its thrust columns of J
                for (int e = 0; e < 24; ++e)
                    add += tj[(VSMPC_TT_LLIN + e) * VSMPC_TT_NDIR + 8 + c] * gi[VSMPC_IN_LLIN + e]
                         + tj[(VSMPC_TT_LANG + e) * VSMPC_TT_NDIR + 8 + c] * gi[VSMPC_IN_LANG + e];
            } else {
            for (int j = 0; j < 8; ++j)
                for (int row = 0; row < 6; ++row)
                    add += DJ[24 * j + 4 * row + c] * (row < 3 ? gi[VSMPC_IN_LLIN + 8 * row + j] : gi[VSMPC_IN_LANG + 8 * (row - 3) + j]);
            }
        } else if (lane >= 16 && lane < 20) {
            add += gi[VSMPC_IN_TD0 + lane - 16];
        } else if (lane >= 20 && lane < 28) {                       // q: A_mom(q) and the posture error
            const int j = lane - 20;
            add = gi[VSMPC_IN_QERR + j];
            if constexpr (TREE) {   // the record's share of tau_bar through column j of J: A_mom, Lambda, and I_B (I_G, omega)
                for (int l = 0; l < 24; ++l)
                    add += tj[(VSMPC_TT_AMOM + l) * VSMPC_TT_NDIR + j] * gi[VSMPC_IN_AMOM + l]
                         + tj[(VSMPC_TT_LLIN + l) * VSMPC_TT_NDIR + j] * gi[VSMPC_IN_LLIN + l]
                         + tj[(VSMPC_TT_LANG + l) * VSMPC_TT_NDIR + j] * gi[VSMPC_IN_LANG + l];
                for (int u = 0; u < 3; ++u)
                    for (int v = 0; v < 3; ++v) {
                        double g = 0.0;
                        for (int i = 0; i < 3; ++i)
                            for (int k = 0; k < 3; ++k) g += R[3 * i + u] * gi[VSMPC_IN_INERTIA + 3 * i + k] * R[3 * k + v];
                        const double om = IBi[3 * v] * s[VSMPC_PS_HANG] + IBi[3 * v + 1] * s[VSMPC_PS_HANG + 1] + IBi[3 * v + 2] * s[VSMPC_PS_HANG + 2];
                        g -= (IBi[u] * gi[VSMPC_IN_OMEGA] + IBi[3 + u] * gi[VSMPC_IN_OMEGA + 1] + IBi[6 + u] * gi[VSMPC_IN_OMEGA + 2]) * om;
                        add += tj[(VSMPC_TT_IB + 3 * u + v) * VSMPC_TT_NDIR + j] * g;
                    }
            } else {
            for (int l = 0; l < 24; ++l) add += DJ[24 * j + l] * gi[VSMPC_IN_AMOM + l];
            }
        } else if (lane >= 28 && lane < 32) {
            add = gi[VSMPC_IN_UPREV + lane - 28];
        } else if (lane >= 32 && lane < 36) {
            add = gi[VSMPC_IN_TDES + lane - 32];
        } else if (lane >= 36 && lane < 40) {
            add = gi[VSMPC_IN_TDDES + lane - 36];
        }
        if constexpr (PT) {
            // The record's entries that are parameters or are built from them, at the taped state; and the column this tick
            // pushed, whose cotangent is complete here, in front of the shift: its position, attitude and h_lin entries
            const bool rel = release_tick(rd, tk);
            const double* wp = wb + 12 * (nref - 1);
            const double* vp = a.traj_vel + 3 * (rel ? window_push_sample(rd, tk) : 0);
            for (int e = lane; e < VSMPC_PP_DIST_F; e += RO_BLOCK) {
                double g = 0.0;
                if constexpr (TREE) {   // not read by the tree plant: I_B, A_mom0, DJ stay +0.0; q_ref0 keeps the posture error
                    if (e >= VSMPC_PP_INERTIA_B && e < VSMPC_PP_QREF0) continue;
                    if (e >= VSMPC_PP_QREF0 && e < VSMPC_PP_PINIT) { gp[e] -= gi[VSMPC_IN_QERR + e - VSMPC_PP_QREF0]; continue; }
                }
                if (e == VSMPC_PP_MASS) {
                    g = gi[VSMPC_IN_MASS];
                    if (rel) g += hlin_to_mass(R, wp + 3, vp);
                } else if (e < VSMPC_PP_AMOM0) {                 // I_G = R I_B R^T, and omega = I_B^-1 h_ang
                    const int u = (e - VSMPC_PP_INERTIA_B) / 3, v = (e - VSMPC_PP_INERTIA_B) % 3;
                    for (int i = 0; i < 3; ++i)
                        for (int j = 0; j < 3; ++j) g += R[3 * i + u] * gi[VSMPC_IN_INERTIA + 3 * i + j] * R[3 * j + v];
                    const double om = IBi[3 * v] * s[VSMPC_PS_HANG] + IBi[3 * v + 1] * s[VSMPC_PS_HANG + 1] + IBi[3 * v + 2] * s[VSMPC_PS_HANG + 2];
                    g -= (IBi[u] * gi[VSMPC_IN_OMEGA] + IBi[3 + u] * gi[VSMPC_IN_OMEGA + 1] + IBi[6 + u] * gi[VSMPC_IN_OMEGA + 2]) * om;
                } else if (e < VSMPC_PP_DJ) {
                    g = gi[VSMPC_IN_AMOM + e - VSMPC_PP_AMOM0];
                } else if (e < VSMPC_PP_QREF0) {                 // A_mom(q), and Lambda column j = DJ[j] T
                    const int d = e - VSMPC_PP_DJ, j = d / 24, l = d - 24 * j, row = l >> 2, c = l & 3;
                    g = gi[VSMPC_IN_AMOM + l] * (s[VSMPC_PS_Q + j] - p[VSMPC_PP_QREF0 + j])
                      + (row < 3 ? gi[VSMPC_IN_LLIN + 8 * row + j] : gi[VSMPC_IN_LANG + 8 * (row - 3) + j]) * s[VSMPC_PS_T + c];
                } else if (e < VSMPC_PP_PINIT) {                 // the posture error, and A_mom(q)
                    const int j = e - VSMPC_PP_QREF0;
                    for (int l = 0; l < 24; ++l) g += DJ[24 * j + l] * gi[VSMPC_IN_AMOM + l];
                    g = -gi[VSMPC_IN_QERR + j] - g;
                } else if (e < VSMPC_PP_RPYINIT) {
                    if (rel) g = wp[e - VSMPC_PP_PINIT];
                } else {
                    g = gi[VSMPC_IN_RPYINIT + e - VSMPC_PP_RPYINIT];
                    if (rel) g += wp[6 + e - VSMPC_PP_RPYINIT];
                }
                gp[e] += g;
            }
            if (lane >= 40 && lane < 46) {                       // the pushed column's trajectory sample
                const int c = lane - 40;
                tc[6 * nref + c] = !rel ? 0.0 : c < 3 ? wp[c] : m * rot_row(R, wp + 3, c - 3);
            } else if (lane == 46) {
                const Lerp l = alpha_tick_lerp(rd.n_alpha, rd.alpha_up, tk);
                ac[0] = gi[VSMPC_IN_ALPHA] * (1.0 - l.f);
                ac[1] = gi[VSMPC_IN_ALPHA] * l.f;
            }
        }
        __syncthreads();
        if (release_tick(rd, tk)) {   // the FIFO shifted at this tick: the cotangent shifts back, column 0 was new to it
            constexpr int KMAX = (12 * MAX_STAGES + RO_BLOCK - 1) / RO_BLOCK;
            double keep[KMAX];
#pragma unroll
            for (int k = 0; k < KMAX; ++k) {
                const int e = lane + k * RO_BLOCK;
                keep[k] = (e < nwin && e >= 12) ? wb[e - 12] : 0.0;
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < KMAX; ++k) {
                const int e = lane + k * RO_BLOCK;
                if (e < nwin) wb[e] = keep[k];
            }
            __syncthreads();
        }
        if (a.first) {   // this tick filled the window: every column was frozen with this tick's R
            if (lane >= 6 && lane < 9)
                for (int j = 0; j < nref; ++j) {
                    const int idx = window_fill_sample(rd, tk, j);
                    add += hlin_to_rpy(dR + 9 * (lane - 6), wb + 12 * j + 3, a.traj_vel + 3 * idx, m);
                }
            if constexpr (PT) {   // every column's cotangent is complete: its sample, and PINIT, RPYINIT and the mass, column by column
                for (int e = lane; e < 6 * nref; e += RO_BLOCK) {
                    const int j = e / 6, c = e - 6 * j;
                    tc[e] = c < 3 ? wb[12 * j + c] : m * rot_row(R, wb + 12 * j + 3, c - 3);
                }
                if (lane >= 32 && lane < 39) {
                    const int k = lane - 32;
                    double acc = 0.0;
                    for (int j = 0; j < nref; ++j) {
                        const double* cw = wb + 12 * j;
                        acc += k < 3 ? cw[k] : k < 6 ? cw[6 + k - 3]
                                     : hlin_to_mass(R, cw + 3, a.traj_vel + 3 * window_fill_sample(rd, tk, j));
                    }
                    gp[k < 3 ? VSMPC_PP_PINIT + k : k < 6 ? VSMPC_PP_RPYINIT + k - 3 : VSMPC_PP_MASS] += acc;
                }
            }
            __syncthreads();
            for (int e = lane; e < nwin; e += RO_BLOCK) wb[e] = 0.0;
        }
        if (lane < 40) sb[lane] += add;
        __syncthreads();
    }

    double out0 = lane < 40 ? sb[lane] : 0.0;   // the new sbar of this lane's entry (the jet-plant slots carry nothing)
    if (plant) {
        __syncthreads();
        if (lane < 14)   // the log row of this tick reads the state after it: p, rpy, T, throttle
            sb[lane < 3 ? lane : lane < 6 ? 6 + lane - 3 : lane < 10 ? 12 + lane - 6 : VSMPC_PS_U + lane - 10] += lbar;
        s[lane] = sp0;
        if (lane + RO_BLOCK < VSMPC_PLANT_STATE) s[lane + RO_BLOCK] = sp1;
        if (lane < VSMPC_FM_SIZE) f[lane] = fm;
        __syncthreads();
        const bool solved = st == VSMPC_STATUS_SOLVED;
        const int tk = a.tick_plant + int(p[VSMPC_PP_TICK0]);
        const int substeps = a.substeps;
        if (lane >= 32 && lane < 32 + substeps && lane < 48)
            alpha_s[lane - 32] = interp_clamped(a.traj_alpha, rd.n_alpha, substep_time(rd, tk, lane - 32, substeps) / rd.alpha_dt);
        if (solved) consume_move<false>(s, f, lane);   // the move the forward tick consumed
        __syncthreads();
        if (lane < 24) {
            if constexpr (TREE) Aq[lane] = tt[VSMPC_TT_AMOM + lane];
            else Aq[lane] = amom_entry(p, s + VSMPC_PS_Q, lane);
        } else if (lane == 24) {
            if constexpr (TREE) inv3(tt + VSMPC_TT_IB, IBi);
            else inv3(p + VSMPC_PP_INERTIA_B, IBi);
        } else if (lane >= 28 && lane < 32) {
            vthr[lane - 28] = Jet::v_of_throttle(s[VSMPC_PS_U + lane - 28]);
        }
        if (lane < 20) xs[lane] = s[lane];
        __syncthreads();
        const double h = rd.period_mpc / double(substeps);
        // forward: the sub-steps of advance_kernel, every one's 20-vector kept (xs + 20 ss is the state IN FRONT of sub-step ss)
        for (int ss = 0; ss + 1 < substeps; ++ss) {
            const double* x = xs + 20 * ss;
            const double t = substep_time(rd, tk, ss, substeps);
            const double alpha = alpha_s[ss];
            const bool dist = push_active(p, t);
            substep_preamble(x, IBi, sc, omv, lane);
            __syncthreads();
            const SinCos w = sincos_of(sc);
            if (lane == 0) rot_from_sincos(w, R);
            __syncthreads();
            const double d = substep_rate(x, R, omv, w, Aq, vthr, p, m, alpha, dist, false, lane);
            if (lane < 20) xs[20 * (ss + 1) + lane] = x[lane] + h * d;
            __syncthreads();
        }
        // backward: lam = dL/d(the 20-vector behind sub-step ss); lanes 32..55 collect the cotangent of A_mom(q), 56..59 of v(u)
        if (lane < 20) lam[lane] = sb[lane];
        double abar = 0.0;
        double pacc = 0.0, al0 = 0.0, al1 = 0.0, al2 = 0.0;   // PT: this lane's parameter entry; lane 20: the three alpha elements
        __syncthreads();
        for (int ss = substeps - 1; ss >= 0; --ss) {
            const double* x = xs + 20 * ss;
            const double t = substep_time(rd, tk, ss, substeps);
            const double alpha = alpha_s[ss];
            const bool dist = push_active(p, t);
            substep_preamble(x, IBi, sc, omv, lane);
            __syncthreads();
            const SinCos w = sincos_of(sc);
            const double sr = w.sr, cr = w.cr, sp = w.sp, cp = w.cp, tp = sp / cp;
            if (lane == 0) {
                rot_partials(w, R, dR);
            } else if (lane >= 1 && lane < 4) {
                // cotangent of omega: -omega x h in both momenta, and rpy' = W^-1(rpy) omega
                const int i = lane - 1, i1 = (i + 1) % 3, i2 = (i + 2) % 3;
                double o = (lam[3 + i1] * x[3 + i2] - lam[3 + i2] * x[3 + i1]) + (lam[9 + i1] * x[9 + i2] - lam[9 + i2] * x[9 + i1]);
                o += i == 0 ? lam[6]
                   : i == 1 ? sr * tp * lam[6] + cr * lam[7] + sr / cp * lam[8]
                            : cr * tp * lam[6] - sr * lam[7] + cr / cp * lam[8];
                omb[i] = o;
            }
            __syncthreads();
            double g = 0.0;
            if (lane >= 3 && lane < 6) {           // h_lin: p' = R h_lin / m, -omega x h_lin
                const int c = lane - 3, c1 = (c + 1) % 3, c2 = (c + 2) % 3;
                g = (R[c] * lam[0] + R[3 + c] * lam[1] + R[6 + c] * lam[2]) / m + (omv[c1] * lam[3 + c2] - omv[c2] * lam[3 + c1]);
            } else if (lane >= 6 && lane < 9) {    // rpy: R in p' and in R^T (alpha m g + push), W^-1
                const double* dRa = dR + 9 * (lane - 6);
                double fw[3] = {0.0, 0.0, alpha * m * (-9.81)};
                if (dist) { fw[0] += p[VSMPC_PP_DIST_F]; fw[1] += p[VSMPC_PP_DIST_F + 1]; fw[2] += p[VSMPC_PP_DIST_F + 2]; }
                for (int r = 0; r < 3; ++r) {
                    g += lam[r] * (dRa[3 * r] * x[3] + dRa[3 * r + 1] * x[4] + dRa[3 * r + 2] * x[5]) / m;
                    g += (dRa[3 * r] * lam[3] + dRa[3 * r + 1] * lam[4] + dRa[3 * r + 2] * lam[5]) * fw[r];
                }
                if (lane == 6)
                    g += lam[6] * (cr * tp * omv[1] - sr * tp * omv[2]) + lam[7] * (-sr * omv[1] - cr * omv[2])
                       + lam[8] * (cr * omv[1] - sr * omv[2]) / cp;
                else if (lane == 7)
                    g += lam[6] * (sr * omv[1] + cr * omv[2]) / (cp * cp) + lam[8] * (sr * omv[1] + cr * omv[2]) * tp / cp;
            } else if (lane >= 9 && lane < 12) {   // h_ang: -omega x h_ang, and omega = I_B^-1 h_ang
                const int c = lane - 9, c1 = (c + 1) % 3, c2 = (c + 2) % 3;
                g = (omv[c1] * lam[9 + c2] - omv[c2] * lam[9 + c1]) + IBi[c] * omb[0] + IBi[3 + c] * omb[1] + IBi[6 + c] * omb[2];
            } else if (lane >= 12 && lane < 20) {  // T, Tdot: A_mom(q) T, T' = Tdot, the jet polynomial
                const int j = (lane - 12) & 3;
                const double Tb = Jet::stdT(x[12 + j]), Tdb = Jet::stdTd(x[16 + j]);
                if (lane < 16) {
                    for (int r = 0; r < 3; ++r) g += lam[3 + r] * Aq[4 * r + j] + lam[9 + r] * Aq[4 * (3 + r) + j];
                    g += lam[16 + j] * (Jet::df_dT(Tb, Tdb) + Jet::dg_dT(Tb, Tdb) * vthr[j]);
                } else {
                    g = lam[12 + j] + lam[16 + j] * (Jet::df_dTd(Tb, Tdb) + Jet::dg_dTd(Tb, Tdb) * vthr[j]);
                }
            } else if (lane >= 32 && lane < 56) {  // A_mom(q) T is bilinear: row (lane - 32) / 4 of the momenta, thrust column
                const int l = lane - 32, row = l >> 2;
                abar += h * lam[row < 3 ? 3 + row : 9 + row - 3] * x[12 + (l & 3)];
            } else if (lane >= 56 && lane < 60) {
                const int j = lane - 56;
                abar += h * lam[16 + j] * Jet::sgT * Jet::g(Jet::stdT(x[12 + j]), Jet::stdTd(x[16 + j]));
            }
            if constexpr (PT) {   // the parameters of this sub-step, in the lanes the state leaves idle
                if (lane == 20) {                      // mass: alpha m R^T g and p' = R h_lin / m; alpha: its two samples
                    const double rg = -9.81 * (R[6] * lam[3] + R[7] * lam[4] + R[8] * lam[5]);
                    const double rh = lam[0] * rot_row(R, x + 3, 0) + lam[1] * rot_row(R, x + 3, 1) + lam[2] * rot_row(R, x + 3, 2);
                    pacc += h * (alpha * rg - rh / (m * m));
                    const Lerp l = interp_lerp(rd.n_alpha, t / rd.alpha_dt);
                    const double ga = h * m * rg, g0 = ga * (1.0 - l.f), g1 = ga * l.f;
                    const int k0 = l.i0 - ai0, k1 = l.i1 - ai0;
                    al0 += (k0 == 0 ? g0 : 0.0) + (k1 == 0 ? g1 : 0.0);
                    al1 += (k0 == 1 ? g0 : 0.0) + (k1 == 1 ? g1 : 0.0);
                    al2 += (k0 >= 2 ? g0 : 0.0) + (k1 >= 2 ? g1 : 0.0);
                } else if (lane >= 21 && lane < 30) {  // I_B through omega = I_B^-1 h_ang: -(I_B^-T omega_bar) omega^T
                    const int u = (lane - 21) / 3, v = (lane - 21) % 3;
                    pacc -= h * (IBi[u] * omb[0] + IBi[3 + u] * omb[1] + IBi[6 + u] * omb[2]) * omv[v];
                } else if (dist && (lane == 30 || lane == 31 || lane == 60)) {   // the push force enters as R^T F
                    pacc += h * rot_row(R, lam + 3, lane == 60 ? 2 : lane - 30);
                } else if (dist && lane >= 61) {       // and the torque directly
                    pacc += h * lam[9 + lane - 61];
                }
            }
            if constexpr (TREE && !PT) {   // (PT has it above) I_B through omega = I_B^-1 h_ang: -(I_B^-T omega_bar) omega^T
                if (lane >= 21 && lane < 30) {
                    const int u = (lane - 21) / 3, v = (lane - 21) % 3;
                    pacc -= h * (IBi[u] * omb[0] + IBi[3 + u] * omb[1] + IBi[6 + u] * omb[2]) * omv[v];
                }
            }
            __syncthreads();
            if (lane < 20) lam[lane] += h * g;
            __syncthreads();
        }
        if constexpr (TREE)
            if (lane >= 21 && lane < 30) tib[lane - 21] = pacc;
        if (lane >= 32 && lane < 56) Ab[lane - 32] = abar;
        if (lane >= 56 && lane < 60) vb[lane - 56] = abar;
        __syncthreads();
        if constexpr (PT && TREE) {   // I_B, q_ref0, A_mom0 and DJ are not read: what they get on the parametric plant goes through J
            if (lane == 20) {
                gp[VSMPC_PP_MASS] += pacc;
                ac[2] = al0; ac[3] = al1; ac[4] = al2;
            } else if (lane == 30 || lane == 31 || lane == 60) {
                gp[VSMPC_PP_DIST_F + (lane == 60 ? 2 : lane - 30)] += pacc;
            } else if (lane >= 61) {
                gp[VSMPC_PP_DIST_TAU + lane - 61] += pacc;
            }
        } else if constexpr (PT) {
            if (lane == 20) {
                gp[VSMPC_PP_MASS] += pacc;
                ac[2] = al0; ac[3] = al1; ac[4] = al2;
            } else if (lane >= 21 && lane < 30) {
                gp[VSMPC_PP_INERTIA_B + lane - 21] += pacc;
            } else if (lane == 30 || lane == 31 || lane == 60) {
                gp[VSMPC_PP_DIST_F + (lane == 60 ? 2 : lane - 30)] += pacc;
            } else if (lane >= 61) {
                gp[VSMPC_PP_DIST_TAU + lane - 61] += pacc;
            } else if (lane >= 40 && lane < 48) {      // q_ref0 through A_mom(q)
                const int j = lane - 40;
                double t = 0.0;
                for (int l = 0; l < 24; ++l) t += DJ[24 * j + l] * Ab[l];
                gp[VSMPC_PP_QREF0 + j] -= t;
            }
            // A_mom0 and DJ[j] (behind it in the row) from the cotangent of A_mom(q), q the joints after the move
            for (int e = lane; e < 24 + 192; e += RO_BLOCK) {
                const int j = e / 24 - 1, l = e - 24 * (j + 1);
                gp[VSMPC_PP_AMOM0 + e] += j < 0 ? Ab[l] : Ab[l] * (s[VSMPC_PS_Q + j] - p[VSMPC_PP_QREF0 + j]);
            }
        }
        double fmb = 0.0;
        if (lane < 20) {
            out0 = lam[lane];
        } else if (lane < 28) {                    // q through A_mom(q); the move added dq to it
            const int j = lane - 20;
            double q = sb[lane];
            if constexpr (TREE) {                  // the sub-steps' share of tau_bar (A_mom, I_B) through column j of J
                for (int l = 0; l < 24; ++l) q += tj[(VSMPC_TT_AMOM + l) * VSMPC_TT_NDIR + j] * Ab[l];
                for (int l = 0; l < 9; ++l) q += tj[(VSMPC_TT_IB + l) * VSMPC_TT_NDIR + j] * tib[l];
            } else {
            for (int l = 0; l < 24; ++l) q += DJ[24 * j + l] * Ab[l];
            }
            out0 = q;
        } else if (lane < 32) {                    // the latched throttle through v(u)
            const int j = lane - 28;
            out0 = sb[lane] + vb[j] * Jet::dv_du(Jet::stdU(s[VSMPC_PS_U + j])) * Jet::isgU;
        } else if (lane < 40) {
            out0 = sb[lane];
        }
        // Solved: the move overwrote the latched entries and was added to q; otherwise it was not consumed
        if (solved && lane >= 20 && lane < 40) {
            fmb = out0;
            if (lane >= 28) out0 = 0.0;
        }
        if (lane >= 20 && lane < 40) sb[lane] = fmb;
        __syncthreads();
        if (lane < VSMPC_FM_SIZE) {
            // first move: DQ 0:8 | V0 8:12 | THROTTLE 12:16 | THRUST 16:20 | THRUSTDOT 20:24; state: Q 20 | U 28 | TDES 32 | TDDES 36
            const double v = lane < 8 ? sb[VSMPC_PS_Q + lane] : lane < 12 ? 0.0 : sb[VSMPC_PS_U + lane - 12];
            a.fmbar[size_t(b) * VSMPC_FM_SIZE + lane] = v;
        }
    }
    a.sbar[size_t(b) * VSMPC_PLANT_STATE + lane] = out0;
    if (lane + RO_BLOCK < VSMPC_PLANT_STATE) a.sbar[size_t(b) * VSMPC_PLANT_STATE + lane + RO_BLOCK] = 0.0;
    for (int e = lane; e < nwin; e += RO_BLOCK) a.wbar[size_t(b) * nwin + e] = wb[e];
    if constexpr (PT) {
        __syncthreads();
        for (int e = lane; e < VSMPC_PLANT_PARAMS; e += RO_BLOCK) a.gpar[size_t(b) * VSMPC_PLANT_PARAMS + e] = gp[e];
        double* gt = a.gtraj + size_t(b) * size_t(6 * rd.n_traj + rd.n_alpha);
#pragma unroll
        for (int k = 0; k < KT; ++k) {
            const int e = lane + k * RO_BLOCK, ws = e / 6, c = e - 6 * ws;
            if (rec && ws <= nref) {
                const int idx = slot_sample(rd, tkr, a.first, ws);
                if (idx >= 0 && slot_owner(rd, tkr, a.first, ws, idx)) {
                    double sum = tpre[k];
                    for (int w2 = ws; w2 <= nref; ++w2)
                        if (slot_sample(rd, tkr, a.first, w2) == idx) sum += tc[6 * w2 + c];
                    gt[traj_entry(rd, idx, c)] = sum;
                }
            }
        }
        if (lane < ALPHA_ELEMS) {
            const int idx = alpha_elem_sample(rd, tkr, tkp, ai0, lane);
            if (idx >= 0 && alpha_elem_owner(rd, tkr, tkp, ai0, lane, idx)) {
                double sum = apre;
                for (int e2 = lane; e2 < ALPHA_ELEMS; ++e2)
                    if (alpha_elem_sample(rd, tkr, tkp, ai0, e2) == idx) sum += ac[e2];
                gt[6 * rd.n_traj + idx] = sum;
            }
        }
    }
}

