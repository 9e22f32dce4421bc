// Device code of the rollout's backward sweep: advance_adjoint_body<PT, TREE, ATT>, the body of advance_adjoint_kernel<PT>
// (vsmpc_rollout_adjoint.hip, TREE off: the parametric plant), of advance_tree_adjoint_kernel<PT>
// (vsmpc_rollout_tree_adjoint.hip, TREE on: the kinematic-tree plant) and, with ATT on, of advance_attitude_adjoint_kernel<PT>
// and advance_attitude_tree_adjoint_kernel<PT> (vsmpc_rollout_attitude_adjoint.hip, vsmpc_rollout_attitude_tree_adjoint.hip),
// as a driver over one function per phase.  One unit per family, because a second kernel family in one code object moves the
// first one's code (LDS and address arithmetic are laid out per module).
//
// One wavefront per instance, as advance_kernel.  Every global load is requested in front of the first barrier.
// PT (vsmpc_rollout_backward_full) also accumulates dL/d(plant parameters) and dL/d(tracks) of the instance: the parameter row
// lives in LDS for the launch, the touched track samples as described at slot_sample.  Without PT nothing of that is compiled in.
// TREE (vsmpc_rollout_set_tree_ex with VSMPC_TREE_ADJOINT): A_mom, Lambda and I_B of both halves are tau = terms(q, T) at the
// state between them (a.tree_terms) instead of the parameter record's, and their cotangents -- the record half's (A_mom,
// Lambda, I_B through I_G and omega), then the sub-steps' (A_mom, I_B through omega) -- are pulled back through
// J = d tau / d(q | T) (a.tree_jac): Lambda's to the thrusts in front of the sub-steps, everything to the joints, where the
// move shares it when the tick was Solved.  The parameter blocks the tree plant does not read get nothing.  Without TREE
// nothing of that is compiled in.
// ATT (vsmpc_rollout_set_attitude_tracks_ex with VSMPC_ATTITUDE_ADJOINT): rows 9..11 of a window column, the angular-momentum
// reference R I_B R^T W(roll, pitch) RPYDot[idx] frozen at the tick that pushed it, are pulled back too (att_column) -- to rpy
// through R and W, to I_B (PT: the parameter block; TREE: tau_bar's I_B rows and on through J to the joints) and, PT, to the
// RPYDot sample; rows 6..8 go to the RPY sample.  The attitude samples ride the slots of slot_sample, six more doubles each.
// Without ATT nothing of that is compiled in.
//
// The phases share the instance's LDS (AdjLds, which each of them forms itself with adj_lds) and, in registers, what the
// stage-in parked (AdjTracks, AdjPlantRows).  Above each phase: what it reads, what it leaves, the barriers it contains.
#pragma once
#include "vsmpc_device.hpp"
#include "vsmpc_launch.hpp"
#include "vsmpc_rollout_device.hpp"

namespace vsmpc {

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

// The state entry that entry `e` of a tick's log row reads, at the state after the tick: p, rpy, T, throttle
VS_DEV int log_entry_state(int e) { return e < 3 ? e : e < 6 ? 6 + e - 3 : e < 10 ? 12 + e - 6 : VSMPC_PS_U + e - 10; }

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

// PT, in registers from the stage-in to the write-out: the launch's ticks as alpha_elem_sample takes them, and the running sums
// of the samples this lane owns (slot entry lane + k RO_BLOCK; alpha element `lane`)
constexpr int ADJ_KT = (6 * (MAX_STAGES + 1) + RO_BLOCK - 1) / RO_BLOCK;
struct AdjTracks {
    int tkr = -1, tkp = -1, ai0 = 0;
    double tpre[ADJ_KT] = {}, apre = 0.0;
    double qpre[ADJ_KT] = {};   // ATT: the running sums of grad_att's samples, the slot entries as tpre
};
// The one walk over what this lane owns of grad_traj: on_slot(k, ws, c, idx) for component c of slot ws, the lane's k-th slot
// entry, where slot ws owns its sample idx; on_alpha(idx) where alpha element `lane` owns its sample idx
template <class OnSlot, class OnAlpha>
VS_DEV void for_owned_samples(const RolloutDev& rd, const RolloutAdj& a, const AdjTracks& tr, int lane, OnSlot&& on_slot, OnAlpha&& on_alpha) {
    const bool rec = a.tick_rec >= 0;
#pragma unroll
    for (int k = 0; k < ADJ_KT; ++k) {
        const int e = lane + k * RO_BLOCK, ws = e / 6, c = e - 6 * ws;
        if (rec && ws <= rd.n_ref) {
            const int idx = slot_sample(rd, tr.tkr, a.first, ws);
            if (idx >= 0 && slot_owner(rd, tr.tkr, a.first, ws, idx)) on_slot(k, ws, c, idx);
        }
    }
    if (lane < ALPHA_ELEMS) {
        const int idx = alpha_elem_sample(rd, tr.tkr, tr.tkp, tr.ai0, lane);
        if (idx >= 0 && alpha_elem_owner(rd, tr.tkr, tr.tkp, tr.ai0, lane, idx)) on_alpha(idx);
    }
}

// ---- the tree plant's pull-backs through J ----------------------------------------------------------------------------------
// acc + sum_l sum_k tj[row_k + l][c] bar_k[l], l < n: n rows of each listed block of tau_bar (row: its VSMPC_TT_* offset, bar:
// its cotangent) contracted with column c of J, the blocks side by side within every l
struct TauBlock { int row; const double* bar; };
template <int NB>
VS_DEV double tau_bar_col(double acc, const double* tj, int c, int n, const TauBlock (&blk)[NB]) {
    for (int l = 0; l < n; ++l) {
        double t = tj[(blk[0].row + l) * VSMPC_TT_NDIR + c] * blk[0].bar[l];
#pragma unroll
        for (int k = 1; k < NB; ++k) t += tj[(blk[k].row + l) * VSMPC_TT_NDIR + c] * blk[k].bar[l];
        acc += t;
    }
    return acc;
}

// ---- LDS of one instance ----------------------------------------------------------------------------------------------------
struct AdjLds {
    double *s, *p, *f, *sb, *gi, *wb, *R, *dR, *IBi, *Aq, *Ab, *vb, *vthr, *alpha_s, *xs, *lam, *sc, *omv, *omb;
    double *gp, *tc, *ac;     // PT: cotangent of the parameters; of the window slots' trajectory samples (6 per slot); of the alpha elements
    double *tt, *tj, *tib;    // TREE: tau, J, and the sub-steps' cotangent of I_B
    // ATT: cotangent of the window slots' attitude samples (rpy | rpy_dot, 6 per slot); per slot what att_column leaves for the
    // reductions over the columns: the shares of roll, pitch, yaw | ybar | v
    double *atc, *acs;
};
constexpr int ATT_COL = 9;   // doubles per slot of acs
// Every phase forms the carve-up itself: the arrays are one set per instantiation, their addresses constants wherever they
// are used; an array of an option that the instantiation does not have is never named and takes no LDS.
template <bool PT, bool TREE, bool ATT>
VS_DEV AdjLds adj_lds() {
    __shared__ double s[VSMPC_PLANT_STATE], p[VSMPC_PLANT_PARAMS + 1], f[VSMPC_FM_SIZE], sb[VSMPC_PLANT_STATE];
    __shared__ double gi[VSMPC_IN_XREF + 12 * MAX_STAGES], wb[12 * MAX_STAGES];
    __shared__ double R[9], dR[27], IBi[9], Aq[24], Ab[24], vb[4], vthr[4], alpha_s[16];
    __shared__ double xs[16 * 20], lam[20], sc[6], omv[3], omb[3];
    __shared__ double gp[PT ? VSMPC_PLANT_PARAMS + 1 : 1], tc[PT ? 6 * (MAX_STAGES + 1) : 1], ac[PT ? ALPHA_ELEMS + 1 : 1];
    __shared__ double tt[TREE ? VSMPC_TT_SIZE + 1 : 1], tj[TREE ? VSMPC_TT_SIZE * VSMPC_TT_NDIR : 1], tib[TREE ? 9 : 1];
    __shared__ double atc[ATT && PT ? 6 * (MAX_STAGES + 1) : 1], acs[ATT ? ATT_COL * (MAX_STAGES + 1) : 1];
    return {s, p, f, sb, gi, wb, R, dR, IBi, Aq, Ab, vb, vthr, alpha_s, xs, lam, sc, omv, omb, gp, tc, ac, tt, tj, tib, atc, acs};
}

// ---- ATT: the h_ang entry of a window column ----------------------------------------------------------------------------------
// Rows 9..11 of a column built from sample idx at the taped state: d = RPYDot[idx] (zeros without a track), u = W(roll, pitch) d,
// v = R^T u, y = I_B v, h = R y (assemble_record's column_entry).  With their cotangent w: ybar = R^T w, vbar = I_B^T ybar,
// ubar = R vbar; dbar = W^T ubar; I_B_bar = ybar v^T; rpy_a gets <dR_a, w y^T + u vbar^T>, roll and pitch ubar . (dW d) besides.
// Reads R, dR, sc (sin, cos of roll | pitch, as adj_record_setup leaves them) and I_B.  Leaves in acs + ATT_COL k the three
// shares of rpy | ybar | v; PT: in atc + 6 k the column's attitude samples, rows 6..8 of cw | dbar.  One lane, no barrier.
template <bool PT, bool TREE>
VS_DEV void att_column(const AdjLds& L, const double* __restrict__ cw, const double* __restrict__ traj_rpyd, int idx, int k) {
    const double* R = L.R;
    const double* IB;
    if constexpr (TREE) IB = L.tt + VSMPC_TT_IB;
    else IB = L.p + VSMPC_PP_INERTIA_B;
    const double sr = L.sc[0], cr = L.sc[1], sp = L.sc[2], cp = L.sc[3];
    const double* w = cw + 9;
    double d[3] = {0.0, 0.0, 0.0};
    if (traj_rpyd != nullptr) { d[0] = traj_rpyd[3 * idx]; d[1] = traj_rpyd[3 * idx + 1]; d[2] = traj_rpyd[3 * idx + 2]; }
    const double u[3] = {d[0] - sp * d[2], cr * d[1] + cp * sr * d[2], -sr * d[1] + cr * cp * d[2]};
    double v[3], y[3], yb[3], vb[3], ub[3];
    for (int c = 0; c < 3; ++c) v[c] = R[c] * u[0] + R[3 + c] * u[1] + R[6 + c] * u[2];
    for (int r = 0; r < 3; ++r) y[r] = rot_row(IB, v, r);
    for (int c = 0; c < 3; ++c) yb[c] = R[c] * w[0] + R[3 + c] * w[1] + R[6 + c] * w[2];
    for (int c = 0; c < 3; ++c) vb[c] = IB[c] * yb[0] + IB[3 + c] * yb[1] + IB[6 + c] * yb[2];
    for (int r = 0; r < 3; ++r) ub[r] = rot_row(R, vb, r);
    double* o = L.acs + ATT_COL * k;
    for (int a = 0; a < 3; ++a) {
        const double* dRa = L.dR + 9 * a;
        double g = 0.0;
        for (int r = 0; r < 3; ++r) g += rot_row(dRa, y, r) * w[r] + rot_row(dRa, vb, r) * u[r];
        o[a] = g;
    }
    o[0] += ub[1] * (-sr * d[1] + cp * cr * d[2]) + ub[2] * (-cr * d[1] - sr * cp * d[2]);   // ubar . (dW/droll d)
    o[1] -= (cp * ub[0] + sp * sr * ub[1] + cr * sp * ub[2]) * d[2];                           // ubar . (dW/dpitch d)
    for (int c = 0; c < 3; ++c) { o[3 + c] = yb[c]; o[6 + c] = v[c]; }
    if constexpr (PT) {
        double* t = L.atc + 6 * k;
        t[0] = cw[6]; t[1] = cw[7]; t[2] = cw[8];
        t[3] = ub[0];
        t[4] = cr * ub[1] - sr * ub[2];
        t[5] = -sp * ub[0] + cp * sr * ub[1] + cr * cp * ub[2];
    }
}
// cotangent of I_B[u][v] from slot k's column: (ybar v^T)[u][v]
VS_DEV double att_ib_bar(const AdjLds& L, int k, int u, int v) { return L.acs[ATT_COL * k + 3 + u] * L.acs[ATT_COL * k + 6 + v]; }
// TREE: acc + that cotangent, as tau_bar's I_B rows, contracted with column c of J
VS_DEV double att_tau_bar_col(const AdjLds& L, double acc, int c, int k) {
    for (int u = 0; u < 3; ++u)
        for (int v = 0; v < 3; ++v) acc += L.tj[(VSMPC_TT_IB + 3 * u + v) * VSMPC_TT_NDIR + c] * att_ib_bar(L, k, u, v);
    return acc;
}

// the plant half's rows, in registers until the record half is through with `s`
struct AdjPlantRows {
    double sp0 = 0.0, sp1 = 0.0, fm = 0.0, lbar = 0.0;
    int st = 0;
};

// ---- stage-in ---------------------------------------------------------------------------------------------------------------
// Reads: every global row of instance b that the launch needs.  Leaves: sb, p, wb (and gp, tt, tj) in LDS; with a record half
// s, gi, and the tick's grad_cfg and flags accumulated; tr (PT: ticks and the running sums of the owned samples) and pr (the
// plant half's rows) in registers.  Ends with the launch's first barrier.
template <bool PT, bool TREE, bool ATT>
VS_DEV void adj_stage_in(const RolloutDev& rd, const RolloutAdj& a, int b, int lane, AdjTracks& tr, AdjPlantRows& pr) {
    const AdjLds L = adj_lds<PT, TREE, ATT>();
    const bool rec = a.tick_rec >= 0, plant = a.tick_plant >= 0;
    const int nwin = 12 * rd.n_ref;
    if constexpr (PT) {
        stage_in<VSMPC_PLANT_PARAMS>(a.gpar + size_t(b) * VSMPC_PLANT_PARAMS, L.gp, lane);
        // which samples the launch touches hangs on the instance's own PP_TICK0: one dependent round trip, still in front of
        // the first barrier
        const int tick0 = int(a.params[size_t(b) * VSMPC_PLANT_PARAMS + VSMPC_PP_TICK0]);
        const double* gt = a.gtraj + size_t(b) * size_t(6 * rd.n_traj + rd.n_alpha);
        if (rec) tr.tkr = a.tick_rec + tick0;
        if (plant) {
            tr.tkp = a.tick_plant + tick0;
            tr.ai0 = interp_lerp(rd.n_alpha, substep_time(rd, tr.tkp, 0, a.substeps) / rd.alpha_dt).i0;
        }
        for_owned_samples(rd, a, tr, lane,
                          [&](int k, int, int c, int idx) {
                              tr.tpre[k] = gt[traj_entry(rd, idx, c)];
                              if constexpr (ATT)   // grad_att's rows are laid out as grad_traj's first two blocks
                                  if (a.gatt != nullptr) tr.qpre[k] = a.gatt[size_t(b) * size_t(6 * rd.n_traj) + traj_entry(rd, idx, c)];
                          },
                          [&](int idx) { tr.apre = gt[6 * rd.n_traj + idx]; });
    }
    if constexpr (TREE) {
        stage_in<VSMPC_TT_SIZE>(a.tree_terms + size_t(b) * VSMPC_TT_SIZE, L.tt, lane);
        stage_in<VSMPC_TT_SIZE * VSMPC_TT_NDIR>(a.tree_jac + size_t(b) * (VSMPC_TT_SIZE * VSMPC_TT_NDIR), L.tj, lane);
    }
    stage_in<VSMPC_PLANT_STATE>(a.sbar + size_t(b) * VSMPC_PLANT_STATE, L.sb, lane);
    stage_in<VSMPC_PLANT_PARAMS>(a.params + size_t(b) * VSMPC_PLANT_PARAMS, L.p, lane);
    for (int e = lane; e < nwin; e += RO_BLOCK) L.wb[e] = a.wbar[size_t(b) * nwin + e];
    if (rec) {
        stage_in<VSMPC_PLANT_STATE>(a.s_rec + size_t(b) * VSMPC_PLANT_STATE, L.s, lane);
        for (int e = lane; e < rd.n_in; e += RO_BLOCK) L.gi[e] = a.gin[size_t(b) * rd.n_in + e];
        if (lane < VSMPC_GRAD_SIZE) a.gcfg[size_t(b) * VSMPC_GRAD_SIZE + lane] += a.gcfg_t[size_t(b) * VSMPC_GRAD_SIZE + lane];
        if (lane == VSMPC_GRAD_SIZE) a.flags[b] |= a.flags_t[b];
    }
    if (plant) {
        pr.sp0 = a.s_plant[size_t(b) * VSMPC_PLANT_STATE + lane];
        if (lane + RO_BLOCK < VSMPC_PLANT_STATE) pr.sp1 = a.s_plant[size_t(b) * VSMPC_PLANT_STATE + lane + RO_BLOCK];
        if (lane < VSMPC_FM_SIZE) pr.fm = a.fm[size_t(b) * VSMPC_FM_SIZE + lane];
        pr.st = a.status[b];
        if (a.log_bar != nullptr && lane < 14) pr.lbar = a.log_bar[size_t(b) * VSMPC_ROLLOUT_LOG + lane];
    }
    __syncthreads();
}

// ---- record half ------------------------------------------------------------------------------------------------------------
// cotangent of I_B[u][v] from the record: I_G = R I_B R^T and omega = I_B^-1 h_ang give R^T G R - (I_B^-T omega_bar) omega^T
VS_DEV double ib_bar(const AdjLds& L, int u, int v) {
    double g = 0.0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) g += L.R[3 * i + u] * L.gi[VSMPC_IN_INERTIA + 3 * i + j] * L.R[3 * j + v];
    const double om = L.IBi[3 * v] * L.s[VSMPC_PS_HANG] + L.IBi[3 * v + 1] * L.s[VSMPC_PS_HANG + 1] + L.IBi[3 * v + 2] * L.s[VSMPC_PS_HANG + 2];
    g -= (L.IBi[u] * L.gi[VSMPC_IN_OMEGA] + L.IBi[3 + u] * L.gi[VSMPC_IN_OMEGA + 1] + L.IBi[6 + u] * L.gi[VSMPC_IN_OMEGA + 2]) * om;
    return g;
}

// Reads: s, p (tt), gi, wb.  Leaves: R, dR of the taped attitude and IBi; in wb the window's cotangent with grad_in's share
// (XREF, and what X0[20:26] and PREF read of column 0).  Two barriers, the second behind its last write.
// ATT: also sc (sin, cos of the taped roll | pitch | yaw) and, on a release tick, slot n_ref of acs (atc): the column this tick
// pushed, complete in front of the shift (att_column), behind a third barrier.
template <bool PT, bool TREE, bool ATT>
VS_DEV void adj_record_setup(const RolloutDev& rd, int tk, int lane) {
    const AdjLds L = adj_lds<PT, TREE, ATT>();
    const int nwin = 12 * rd.n_ref;
    if (lane == 0) {
        double sr, cr, sp, cp, sy, cy;
        sincos(L.s[VSMPC_PS_RPY], &sr, &cr); sincos(L.s[VSMPC_PS_RPY + 1], &sp, &cp); sincos(L.s[VSMPC_PS_RPY + 2], &sy, &cy);
        rot_partials({sr, cr, sp, cp, sy, cy}, L.R, L.dR);
        if constexpr (ATT) { L.sc[0] = sr; L.sc[1] = cr; L.sc[2] = sp; L.sc[3] = cp; L.sc[4] = sy; L.sc[5] = cy; }
    } else if (lane == 1) {
        if constexpr (TREE) inv3(L.tt + VSMPC_TT_IB, L.IBi);
        else inv3(L.p + VSMPC_PP_INERTIA_B, L.IBi);
    }
    for (int e = lane; e < nwin; e += RO_BLOCK) L.wb[e] += L.gi[VSMPC_IN_XREF + e];
    __syncthreads();
    if (lane < 3) {   // X0[20:26] and PREF read column 0 of the window
        L.wb[lane] += L.gi[VSMPC_IN_PREF + lane] - L.gi[VSMPC_IN_X0 + 20 + lane];
        L.wb[6 + lane] -= L.gi[VSMPC_IN_X0 + 23 + lane];
    }
    __syncthreads();
    if constexpr (ATT)
        if (release_tick(rd, tk)) {
            if (lane == 0) att_column<PT, TREE>(L, L.wb + 12 * (rd.n_ref - 1), rd.traj_rpyd, window_push_sample(rd, tk), rd.n_ref);
            __syncthreads();
        }
}

// Reads: what adj_record_setup left, and s, p (tt, tj), gi.  Returns what the record hands to state entry `lane` (< 40), the
// column a release tick pushed included (ATT: its h_ang entry too, from slot n_ref of acs).  No barrier, no write.
template <bool PT, bool TREE, bool ATT>
VS_DEV double adj_record_to_state(const RolloutDev& rd, const RolloutAdj& a, int tk, double m, int lane) {
    const AdjLds L = adj_lds<PT, TREE, ATT>();
    const double* gi = L.gi;
    const double* DJ = L.p + VSMPC_PP_DJ;
    double add = 0.0;
    if (lane < 20) add = gi[VSMPC_IN_X0 + lane];               // X0: identity (the unwrapped RPY has derivative 1)
    if (lane < 3) {
        add += gi[VSMPC_IN_X0 + 20 + lane];
    } else if (lane >= 6 && lane < 9) {
        const int c = lane - 6;
        const double* dRa = L.dR + 9 * c;
        const double* R = L.R;
        const double* IB;
        if constexpr (TREE) IB = L.tt + VSMPC_TT_IB;
        else IB = L.p + VSMPC_PP_INERTIA_B;
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
            add += hlin_to_rpy(dRa, L.wb + 12 * (rd.n_ref - 1) + 3, a.traj_vel + 3 * idx, m);
            if constexpr (ATT) add += L.acs[ATT_COL * rd.n_ref + c];   // and its h_ang entry
        }
    } else if (lane >= 9 && lane < 12) {
        const int c = lane - 9;
        add += L.IBi[c] * gi[VSMPC_IN_OMEGA] + L.IBi[3 + c] * gi[VSMPC_IN_OMEGA + 1] + L.IBi[6 + c] * gi[VSMPC_IN_OMEGA + 2];
    } else if (lane >= 12 && lane < 16) {                       // T: T0 and Lambda column j = DJ[j] T
        const int c = lane - 12;
        add += gi[VSMPC_IN_T0 + c];
        if constexpr (TREE) {                                   // Lambda(q, T) is linear in T: its thrust columns of J
            add = tau_bar_col(add, L.tj, 8 + c, 24, {{VSMPC_TT_LLIN, gi + VSMPC_IN_LLIN}, {VSMPC_TT_LANG, gi + VSMPC_IN_LANG}});
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
            add = tau_bar_col(add, L.tj, j, 24, {{VSMPC_TT_AMOM, gi + VSMPC_IN_AMOM}, {VSMPC_TT_LLIN, gi + VSMPC_IN_LLIN},
                                                 {VSMPC_TT_LANG, gi + VSMPC_IN_LANG}});
            for (int u = 0; u < 3; ++u)
                for (int v = 0; v < 3; ++v) add += L.tj[(VSMPC_TT_IB + 3 * u + v) * VSMPC_TT_NDIR + j] * ib_bar(L, u, v);
            if constexpr (ATT)      // and I_B's of the pushed column's h_ang entry
                if (release_tick(rd, tk)) add = att_tau_bar_col(L, add, j, rd.n_ref);
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
    return add;
}

// PT.  Reads: as adj_record_to_state.  Adds to gp the record's entries that are parameters or are built from them, at the
// taped state, and the share of the column this tick pushed, whose cotangent is complete here, in front of the shift: its
// position, attitude and h_lin entries (ATT, parametric plant: and what its h_ang entry hands to I_B, as adj_record_setup left
// it in slot n_ref of acs); leaves that column's trajectory sample in tc[6 n_ref ..] and alpha of the tick in ac[0..1].  No
// barrier.
template <bool TREE, bool ATT>
VS_DEV void adj_record_to_params(const RolloutDev& rd, const RolloutAdj& a, int tk, double m, int lane) {
    const AdjLds L = adj_lds<true, TREE, ATT>();
    const double* gi = L.gi;
    const double* DJ = L.p + VSMPC_PP_DJ;
    const int nref = rd.n_ref;
    const bool rel = release_tick(rd, tk);
    const double* wp = L.wb + 12 * (nref - 1);
    const double* vp = a.traj_vel + 3 * (rel ? window_push_sample(rd, tk) : 0);
    for (int e = lane; e < VSMPC_PP_DIST_F; e += RO_BLOCK) {
        double g = 0.0;
        if constexpr (TREE) {   // not read by the tree plant: I_B, A_mom0, DJ stay +0.0; q_ref0 keeps the posture error
            if (e >= VSMPC_PP_INERTIA_B && e < VSMPC_PP_QREF0) continue;
            if (e >= VSMPC_PP_QREF0 && e < VSMPC_PP_PINIT) { L.gp[e] -= gi[VSMPC_IN_QERR + e - VSMPC_PP_QREF0]; continue; }
        }
        if (e == VSMPC_PP_MASS) {
            g = gi[VSMPC_IN_MASS];
            if (rel) g += hlin_to_mass(L.R, wp + 3, vp);
        } else if (e < VSMPC_PP_AMOM0) {                 // I_G = R I_B R^T, and omega = I_B^-1 h_ang
            g = ib_bar(L, (e - VSMPC_PP_INERTIA_B) / 3, (e - VSMPC_PP_INERTIA_B) % 3);
            if constexpr (ATT)                           // and the pushed column's h_ang entry R I_B R^T W d
                if (rel) g += att_ib_bar(L, nref, (e - VSMPC_PP_INERTIA_B) / 3, (e - VSMPC_PP_INERTIA_B) % 3);
        } else if (e < VSMPC_PP_DJ) {
            g = gi[VSMPC_IN_AMOM + e - VSMPC_PP_AMOM0];
        } else if (e < VSMPC_PP_QREF0) {                 // A_mom(q), and Lambda column j = DJ[j] T
            const int d = e - VSMPC_PP_DJ, j = d / 24, l = d - 24 * j, row = l >> 2, c = l & 3;
            g = gi[VSMPC_IN_AMOM + l] * (L.s[VSMPC_PS_Q + j] - L.p[VSMPC_PP_QREF0 + j])
              + (row < 3 ? gi[VSMPC_IN_LLIN + 8 * row + j] : gi[VSMPC_IN_LANG + 8 * (row - 3) + j]) * L.s[VSMPC_PS_T + c];
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
        L.gp[e] += g;
    }
    if (lane >= 40 && lane < 46) {                       // the pushed column's trajectory sample
        const int c = lane - 40;
        L.tc[6 * nref + c] = !rel ? 0.0 : c < 3 ? wp[c] : m * rot_row(L.R, wp + 3, c - 3);
    } else if (lane == 46) {
        const Lerp l = alpha_tick_lerp(rd.n_alpha, rd.alpha_up, tk);
        L.ac[0] = gi[VSMPC_IN_ALPHA] * (1.0 - l.f);
        L.ac[1] = gi[VSMPC_IN_ALPHA] * l.f;
    }
}

// The transpose of the window FIFO's shift at a release tick: wb shifts back one column, column 0 was new to the shift.
// Called behind a barrier; two barriers, the second behind its last write.
template <bool PT, bool TREE, bool ATT>
VS_DEV void adj_window_shift_back(const RolloutDev& rd, int lane) {
    const AdjLds L = adj_lds<PT, TREE, ATT>();
    const int nwin = 12 * rd.n_ref;
    constexpr int KMAX = (12 * MAX_STAGES + RO_BLOCK - 1) / RO_BLOCK;
    double keep[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
        const int e = lane + k * RO_BLOCK;
        keep[k] = (e < nwin && e >= 12) ? L.wb[e - 12] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
        const int e = lane + k * RO_BLOCK;
        if (e < nwin) L.wb[e] = keep[k];
    }
    __syncthreads();
}

// The tick that filled the window froze every column with its R.  Reads: wb, R, dR (PT: gp).  Returns `add` with the columns'
// h_lin entries handed to rpy; PT: every column's cotangent is complete, so its sample goes to tc and its share of PINIT,
// RPYINIT and the mass to gp, column by column.  Leaves wb zero.  One barrier, in front of that.
// ATT: in front of all that lane j runs att_column on column j, and behind one more barrier the columns' h_ang entries are
// summed in column order: to rpy, and I_B's to gp (PT) or, as tau_bar's rows, through J to the joints (TREE).
template <bool PT, bool TREE, bool ATT>
VS_DEV double adj_window_first_fill(const RolloutDev& rd, const RolloutAdj& a, int tk, double m, int lane, double add) {
    const AdjLds L = adj_lds<PT, TREE, ATT>();
    const int nref = rd.n_ref, nwin = 12 * rd.n_ref;
    if constexpr (ATT) {
        if (lane < nref) att_column<PT, TREE>(L, L.wb + 12 * lane, rd.traj_rpyd, window_fill_sample(rd, tk, lane), lane);
        __syncthreads();
        if (lane >= 6 && lane < 9)
            for (int j = 0; j < nref; ++j) add += L.acs[ATT_COL * j + lane - 6];
        if constexpr (TREE) {
            if (lane >= 20 && lane < 28)
                for (int j = 0; j < nref; ++j) add = att_tau_bar_col(L, add, lane - 20, j);
        } else if constexpr (PT) {
            if (lane >= 48 && lane < 57) {
                double acc = 0.0;
                for (int j = 0; j < nref; ++j) acc += att_ib_bar(L, j, (lane - 48) / 3, (lane - 48) % 3);
                L.gp[VSMPC_PP_INERTIA_B + lane - 48] += acc;
            }
        }
    }
    if (lane >= 6 && lane < 9)
        for (int j = 0; j < nref; ++j) {
            const int idx = window_fill_sample(rd, tk, j);
            add += hlin_to_rpy(L.dR + 9 * (lane - 6), L.wb + 12 * j + 3, a.traj_vel + 3 * idx, m);
        }
    if constexpr (PT) {
        for (int e = lane; e < 6 * nref; e += RO_BLOCK) {
            const int j = e / 6, c = e - 6 * j;
            L.tc[e] = c < 3 ? L.wb[12 * j + c] : m * rot_row(L.R, L.wb + 12 * j + 3, c - 3);
        }
        if (lane >= 32 && lane < 39) {
            const int k = lane - 32;
            double acc = 0.0;
            for (int j = 0; j < nref; ++j) {
                const double* cw = L.wb + 12 * j;
                acc += k < 3 ? cw[k] : k < 6 ? cw[6 + k - 3]
                             : hlin_to_mass(L.R, cw + 3, a.traj_vel + 3 * window_fill_sample(rd, tk, j));
            }
            L.gp[k < 3 ? VSMPC_PP_PINIT + k : k < 6 ? VSMPC_PP_RPYINIT + k - 3 : VSMPC_PP_MASS] += acc;
        }
    }
    __syncthreads();
    for (int e = lane; e < nwin; e += RO_BLOCK) L.wb[e] = 0.0;
    return add;
}

// Transpose of assemble_record at the taped state, then of the window FIFO.  Reads: s, p, gi, wb, sb (tt, tj) as staged.
// Leaves: sb with the record's share added, wb as the tick in front of this one left the window (PT: gp, tc, ac).  Barriers:
// those of its pieces, one between the pull-backs and the FIFO, one at its end.
template <bool PT, bool TREE, bool ATT>
VS_DEV void adj_record_half(const RolloutDev& rd, const RolloutAdj& a, double m, int lane) {
    const AdjLds L = adj_lds<PT, TREE, ATT>();
    const int tk = a.tick_rec + int(L.p[VSMPC_PP_TICK0]);
    adj_record_setup<PT, TREE, ATT>(rd, tk, lane);
    double add = adj_record_to_state<PT, TREE, ATT>(rd, a, tk, m, lane);
    if constexpr (PT) adj_record_to_params<TREE, ATT>(rd, a, tk, m, lane);
    __syncthreads();
    if (release_tick(rd, tk)) adj_window_shift_back<PT, TREE, ATT>(rd, lane);
    if (a.first) add = adj_window_first_fill<PT, TREE, ATT>(rd, a, tk, m, lane, add);
    if (lane < 40) L.sb[lane] += add;
    __syncthreads();
}

// ---- plant half -------------------------------------------------------------------------------------------------------------
// Reads: pr, sb, p (tt).  Leaves: the log row's cotangent added to sb; in s the taped state with the move consumed when the
// tick was Solved, f the move; alpha_s, Aq, IBi, vthr of the tick; xs[0..20) the 20-vector in front of sub-step 0.  Four
// barriers, the first in front of its first write, the last behind its last.
template <bool PT, bool TREE, bool ATT>
VS_DEV void adj_plant_setup(const RolloutDev& rd, const RolloutAdj& a, const AdjPlantRows& pr, int tk, bool solved, int lane) {
    const AdjLds L = adj_lds<PT, TREE, ATT>();
    const int substeps = a.substeps;
    __syncthreads();
    if (lane < 14) L.sb[log_entry_state(lane)] += pr.lbar;
    L.s[lane] = pr.sp0;
    if (lane + RO_BLOCK < VSMPC_PLANT_STATE) L.s[lane + RO_BLOCK] = pr.sp1;
    if (lane < VSMPC_FM_SIZE) L.f[lane] = pr.fm;
    __syncthreads();
    if (lane >= 32 && lane < 32 + substeps && lane < 48)
        L.alpha_s[lane - 32] = interp_clamped(a.traj_alpha, rd.n_alpha, substep_time(rd, tk, lane - 32, substeps) / rd.alpha_dt);
    if (solved) consume_move<false>(L.s, L.f, lane);   // the move the forward tick consumed
    __syncthreads();
    if (lane < 24) {
        if constexpr (TREE) L.Aq[lane] = L.tt[VSMPC_TT_AMOM + lane];
        else L.Aq[lane] = amom_entry(L.p, L.s + VSMPC_PS_Q, lane);
    } else if (lane == 24) {
        if constexpr (TREE) inv3(L.tt + VSMPC_TT_IB, L.IBi);
        else inv3(L.p + VSMPC_PP_INERTIA_B, L.IBi);
    } else if (lane >= 28 && lane < 32) {
        L.vthr[lane - 28] = Jet::v_of_throttle(L.s[VSMPC_PS_U + lane - 28]);
    }
    if (lane < 20) L.xs[lane] = L.s[lane];
    __syncthreads();
}

// The sub-steps of advance_kernel but the last, every one's 20-vector kept: xs + 20 ss is the state IN FRONT of sub-step ss.
// Reads: what adj_plant_setup left.  Uses sc, omv, R.  Three barriers per sub-step, the last behind its write.
template <bool PT, bool TREE, bool ATT>
VS_DEV void adj_plant_forward(const RolloutDev& rd, int substeps, int tk, double m, int lane) {
    const AdjLds L = adj_lds<PT, TREE, ATT>();
    const double h = rd.period_mpc / double(substeps);
    for (int ss = 0; ss + 1 < substeps; ++ss) {
        const double* x = L.xs + 20 * ss;
        const double t = substep_time(rd, tk, ss, substeps);
        const double alpha = L.alpha_s[ss];
        const bool dist = push_active(L.p, t);
        substep_preamble(x, L.IBi, L.sc, L.omv, lane);
        __syncthreads();
        const SinCos w = sincos_of(L.sc);
        if (lane == 0) rot_from_sincos(w, L.R);
        __syncthreads();
        const double d = substep_rate(x, L.R, L.omv, w, L.Aq, L.vthr, L.p, m, alpha, dist, false, lane);
        if (lane < 20) L.xs[20 * (ss + 1) + lane] = x[lane] + h * d;
        __syncthreads();
    }
}

// what the lanes collect over the backward sub-steps: lanes 32..55 the cotangent of A_mom(q), 56..59 of v(u) (abar); PT: this
// lane's parameter entry (pacc; TREE: lanes 21..29 the cotangent of I_B) and, in lane 20, the three alpha elements
struct AdjSubstepSums { double abar = 0.0, pacc = 0.0, al0 = 0.0, al1 = 0.0, al2 = 0.0; };

// The sub-steps backwards: lam = dL/d(the 20-vector behind sub-step ss), one component per lane.  Reads: xs, sb, and what
// adj_plant_setup left; ai0 (PT): the lower alpha sample of sub-step 0.  Leaves: lam in front of sub-step 0, the lanes' sums in
// `sum`.  Uses sc, omv, omb, R, dR.  One barrier in front of the loop, four per sub-step, the last behind its write.
template <bool PT, bool TREE, bool ATT>
VS_DEV void adj_plant_backward(const RolloutDev& rd, int substeps, int tk, int ai0, double m, int lane, AdjSubstepSums& sum) {
    const AdjLds L = adj_lds<PT, TREE, ATT>();
    const double* lam = L.lam;
    const double* R = L.R;
    const double* omv = L.omv;
    const double* IBi = L.IBi;
    const double h = rd.period_mpc / double(substeps);
    if (lane < 20) L.lam[lane] = L.sb[lane];
    __syncthreads();
    for (int ss = substeps - 1; ss >= 0; --ss) {
        const double* x = L.xs + 20 * ss;
        const double t = substep_time(rd, tk, ss, substeps);
        const double alpha = L.alpha_s[ss];
        const bool dist = push_active(L.p, t);
        substep_preamble(x, L.IBi, L.sc, L.omv, lane);
        __syncthreads();
        const SinCos w = sincos_of(L.sc);
        const double sr = w.sr, cr = w.cr, sp = w.sp, cp = w.cp, tp = sp / cp;
        if (lane == 0) {
            rot_partials(w, L.R, L.dR);
        } else if (lane >= 1 && lane < 4) {
            // cotangent of omega: -omega x h in both momenta, and rpy' = W^-1(rpy) omega
            const int i = lane - 1, i1 = (i + 1) % 3, i2 = (i + 2) % 3;
            double o = (lam[3 + i1] * x[3 + i2] - lam[3 + i2] * x[3 + i1]) + (lam[9 + i1] * x[9 + i2] - lam[9 + i2] * x[9 + i1]);
            o += i == 0 ? lam[6]
               : i == 1 ? sr * tp * lam[6] + cr * lam[7] + sr / cp * lam[8]
                        : cr * tp * lam[6] - sr * lam[7] + cr / cp * lam[8];
            L.omb[i] = o;
        }
        __syncthreads();
        const double* omb = L.omb;
        double g = 0.0;
        if (lane >= 3 && lane < 6) {           // h_lin: p' = R h_lin / m, -omega x h_lin
            const int c = lane - 3, c1 = (c + 1) % 3, c2 = (c + 2) % 3;
            g = (R[c] * lam[0] + R[3 + c] * lam[1] + R[6 + c] * lam[2]) / m + (omv[c1] * lam[3 + c2] - omv[c2] * lam[3 + c1]);
        } else if (lane >= 6 && lane < 9) {    // rpy: R in p' and in R^T (alpha m g + push), W^-1
            const double* dRa = L.dR + 9 * (lane - 6);
            double fw[3] = {0.0, 0.0, alpha * m * (-9.81)};
            if (dist) { fw[0] += L.p[VSMPC_PP_DIST_F]; fw[1] += L.p[VSMPC_PP_DIST_F + 1]; fw[2] += L.p[VSMPC_PP_DIST_F + 2]; }
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
                for (int r = 0; r < 3; ++r) g += lam[3 + r] * L.Aq[4 * r + j] + lam[9 + r] * L.Aq[4 * (3 + r) + j];
                g += lam[16 + j] * (Jet::df_dT(Tb, Tdb) + Jet::dg_dT(Tb, Tdb) * L.vthr[j]);
            } else {
                g = lam[12 + j] + lam[16 + j] * (Jet::df_dTd(Tb, Tdb) + Jet::dg_dTd(Tb, Tdb) * L.vthr[j]);
            }
        } else if (lane >= 32 && lane < 56) {  // A_mom(q) T is bilinear: row (lane - 32) / 4 of the momenta, thrust column
            const int l = lane - 32, row = l >> 2;
            sum.abar += h * lam[row < 3 ? 3 + row : 9 + row - 3] * x[12 + (l & 3)];
        } else if (lane >= 56 && lane < 60) {
            const int j = lane - 56;
            sum.abar += h * lam[16 + j] * Jet::sgT * Jet::g(Jet::stdT(x[12 + j]), Jet::stdTd(x[16 + j]));
        }
        if constexpr (PT) {   // the parameters of this sub-step, in the lanes the state leaves idle
            if (lane == 20) {                      // mass: alpha m R^T g and p' = R h_lin / m; alpha: its two samples
                const double rg = -9.81 * (R[6] * lam[3] + R[7] * lam[4] + R[8] * lam[5]);
                const double rh = lam[0] * rot_row(R, x + 3, 0) + lam[1] * rot_row(R, x + 3, 1) + lam[2] * rot_row(R, x + 3, 2);
                sum.pacc += h * (alpha * rg - rh / (m * m));
                const Lerp l = interp_lerp(rd.n_alpha, t / rd.alpha_dt);
                const double ga = h * m * rg, g0 = ga * (1.0 - l.f), g1 = ga * l.f;
                const int k0 = l.i0 - ai0, k1 = l.i1 - ai0;
                sum.al0 += (k0 == 0 ? g0 : 0.0) + (k1 == 0 ? g1 : 0.0);
                sum.al1 += (k0 == 1 ? g0 : 0.0) + (k1 == 1 ? g1 : 0.0);
                sum.al2 += (k0 >= 2 ? g0 : 0.0) + (k1 >= 2 ? g1 : 0.0);
            } else if (dist && (lane == 30 || lane == 31 || lane == 60)) {   // the push force enters as R^T F
                sum.pacc += h * rot_row(R, lam + 3, lane == 60 ? 2 : lane - 30);
            } else if (dist && lane >= 61) {       // and the torque directly
                sum.pacc += h * lam[9 + lane - 61];
            }
        }
        if constexpr (PT || TREE) {   // I_B through omega = I_B^-1 h_ang: -(I_B^-T omega_bar) omega^T
            if (lane >= 21 && lane < 30) {
                const int u = (lane - 21) / 3, v = (lane - 21) % 3;
                sum.pacc -= h * (IBi[u] * omb[0] + IBi[3 + u] * omb[1] + IBi[6 + u] * omb[2]) * omv[v];
            }
        }
        __syncthreads();
        if (lane < 20) L.lam[lane] += h * g;
        __syncthreads();
    }
}

// Behind the sub-steps.  Reads: lam, sb, s, p (tj), the lanes' sums.  PT: the sub-steps' parameter shares to gp (the tree
// leaves out the blocks it does not read), the alpha elements to ac[2..4].  Returns the new sbar of entry `lane` (0 behind the
// 40) and writes the first move's cotangent; Solved: the move overwrote the latched entries and was added to q, otherwise it was
// not consumed.  Leaves Ab, vb (tib), and sb[20..40) the move's cotangent.  Two barriers, the second in front of the write of fmbar.
template <bool PT, bool TREE, bool ATT>
VS_DEV double adj_plant_tail(const RolloutAdj& a, int b, bool solved, int lane, const AdjSubstepSums& sum) {
    const AdjLds L = adj_lds<PT, TREE, ATT>();
    const double* DJ = L.p + VSMPC_PP_DJ;
    if constexpr (TREE)
        if (lane >= 21 && lane < 30) L.tib[lane - 21] = sum.pacc;
    if (lane >= 32 && lane < 56) L.Ab[lane - 32] = sum.abar;
    if (lane >= 56 && lane < 60) L.vb[lane - 56] = sum.abar;
    __syncthreads();
    if constexpr (PT) {   // TREE: I_B, q_ref0, A_mom0 and DJ are not read: what they get on the parametric plant goes through J
        if (lane == 20) {
            L.gp[VSMPC_PP_MASS] += sum.pacc;
            L.ac[2] = sum.al0; L.ac[3] = sum.al1; L.ac[4] = sum.al2;
        } else if (lane >= 21 && lane < 30) {
            if constexpr (!TREE) L.gp[VSMPC_PP_INERTIA_B + lane - 21] += sum.pacc;
        } else if (lane == 30 || lane == 31 || lane == 60) {
            L.gp[VSMPC_PP_DIST_F + (lane == 60 ? 2 : lane - 30)] += sum.pacc;
        } else if (lane >= 61) {
            L.gp[VSMPC_PP_DIST_TAU + lane - 61] += sum.pacc;
        } else if (!TREE && lane >= 40 && lane < 48) {      // q_ref0 through A_mom(q)
            const int j = lane - 40;
            double t = 0.0;
            for (int l = 0; l < 24; ++l) t += DJ[24 * j + l] * L.Ab[l];
            L.gp[VSMPC_PP_QREF0 + j] -= t;
        }
        // A_mom0 and DJ[j] (behind it in the row) from the cotangent of A_mom(q), q the joints after the move
        if constexpr (!TREE)
            for (int e = lane; e < 24 + 192; e += RO_BLOCK) {
                const int j = e / 24 - 1, l = e - 24 * (j + 1);
                L.gp[VSMPC_PP_AMOM0 + e] += j < 0 ? L.Ab[l] : L.Ab[l] * (L.s[VSMPC_PS_Q + j] - L.p[VSMPC_PP_QREF0 + j]);
            }
    }
    double out0 = 0.0, fmb = 0.0;
    if (lane < 20) {
        out0 = L.lam[lane];
    } else if (lane < 28) {                    // q through A_mom(q); the move added dq to it
        const int j = lane - 20;
        double q = L.sb[lane];
        if constexpr (TREE) {                  // the sub-steps' share of tau_bar (A_mom, I_B) through column j of J
            q = tau_bar_col(q, L.tj, j, 24, {{VSMPC_TT_AMOM, L.Ab}});
            q = tau_bar_col(q, L.tj, j, 9, {{VSMPC_TT_IB, L.tib}});
        } else {
            for (int l = 0; l < 24; ++l) q += DJ[24 * j + l] * L.Ab[l];
        }
        out0 = q;
    } else if (lane < 32) {                    // the latched throttle through v(u)
        const int j = lane - 28;
        out0 = L.sb[lane] + L.vb[j] * Jet::dv_du(Jet::stdU(L.s[VSMPC_PS_U + j])) * Jet::isgU;
    } else if (lane < 40) {
        out0 = L.sb[lane];
    }
    if (solved && lane >= 20 && lane < 40) {
        fmb = out0;
        if (lane >= 28) out0 = 0.0;
    }
    if (lane >= 20 && lane < 40) L.sb[lane] = fmb;
    __syncthreads();
    if (lane < VSMPC_FM_SIZE) {
        // first move: DQ 0:8 | V0 8:12 | THROTTLE 12:16 | THRUST 16:20 | THRUSTDOT 20:24; state: Q 20 | U 28 | TDES 32 | TDDES 36
        const double v = lane < 8 ? L.sb[VSMPC_PS_Q + lane] : lane < 12 ? 0.0 : L.sb[VSMPC_PS_U + lane - 12];
        a.fmbar[size_t(b) * VSMPC_FM_SIZE + lane] = v;
    }
    return out0;
}

// Transpose of advance_kernel at the taped (state, first move, status) of tick_plant.  Reads: pr, tr.ai0, sb, p (tt, tj).
// Returns the new sbar of entry `lane`; writes fmbar (PT: gp, ac[2..4]).  Barriers: those of its four pieces.
template <bool PT, bool TREE, bool ATT>
VS_DEV double adj_plant_half(const RolloutDev& rd, const RolloutAdj& a, const AdjTracks& tr, const AdjPlantRows& pr, double m, int b, int lane) {
    const AdjLds L = adj_lds<PT, TREE, ATT>();
    const bool solved = pr.st == VSMPC_STATUS_SOLVED;
    const int tk = a.tick_plant + int(L.p[VSMPC_PP_TICK0]);
    AdjSubstepSums sum;
    adj_plant_setup<PT, TREE, ATT>(rd, a, pr, tk, solved, lane);
    adj_plant_forward<PT, TREE, ATT>(rd, a.substeps, tk, m, lane);
    adj_plant_backward<PT, TREE, ATT>(rd, a.substeps, tk, tr.ai0, m, lane, sum);
    return adj_plant_tail<PT, TREE, ATT>(a, b, solved, lane, sum);
}

// ---- write-out --------------------------------------------------------------------------------------------------------------
// Reads: out0, wb (PT: gp, tc, ac, tr).  Writes sbar (the jet-plant slots carry nothing) and wbar; PT: behind one barrier, gpar
// and the owned samples of gtraj, each its running sum plus the slots (elements) of that sample in order; ATT: the same lane,
// the same order for the attitude samples of gatt (when the caller asked for it).
template <bool PT, bool TREE, bool ATT>
VS_DEV void adj_write_out(const RolloutDev& rd, const RolloutAdj& a, const AdjTracks& tr, double out0, int b, int lane) {
    const AdjLds L = adj_lds<PT, TREE, ATT>();
    const int nwin = 12 * rd.n_ref;
    a.sbar[size_t(b) * VSMPC_PLANT_STATE + lane] = out0;
    if (lane + RO_BLOCK < VSMPC_PLANT_STATE) a.sbar[size_t(b) * VSMPC_PLANT_STATE + lane + RO_BLOCK] = 0.0;
    for (int e = lane; e < nwin; e += RO_BLOCK) a.wbar[size_t(b) * nwin + e] = L.wb[e];
    if constexpr (PT) {
        __syncthreads();
        for (int e = lane; e < VSMPC_PLANT_PARAMS; e += RO_BLOCK) a.gpar[size_t(b) * VSMPC_PLANT_PARAMS + e] = L.gp[e];
        double* gt = a.gtraj + size_t(b) * size_t(6 * rd.n_traj + rd.n_alpha);
        for_owned_samples(rd, a, tr, lane,
                          [&](int k, int ws, int c, int idx) {
                              double sum = tr.tpre[k], asum = 0.0;
                              if constexpr (ATT) asum = tr.qpre[k];
                              for (int w2 = ws; w2 <= rd.n_ref; ++w2)
                                  if (slot_sample(rd, tr.tkr, a.first, w2) == idx) {
                                      sum += L.tc[6 * w2 + c];
                                      if constexpr (ATT) asum += L.atc[6 * w2 + c];
                                  }
                              gt[traj_entry(rd, idx, c)] = sum;
                              if constexpr (ATT)
                                  if (a.gatt != nullptr) a.gatt[size_t(b) * size_t(6 * rd.n_traj) + traj_entry(rd, idx, c)] = asum;
                          },
                          [&](int idx) {
                              double sum = tr.apre;
                              for (int e2 = lane; e2 < ALPHA_ELEMS; ++e2)
                                  if (alpha_elem_sample(rd, tr.tkr, tr.tkp, tr.ai0, e2) == idx) sum += L.ac[e2];
                              gt[6 * rd.n_traj + idx] = sum;
                          });
    }
}

// ---- the driver -------------------------------------------------------------------------------------------------------------
// second half of tick a.tick_rec, then first half of tick a.tick_plant (either may be absent)
template <bool PT, bool TREE, bool ATT = false>
VS_DEV void advance_adjoint_body(const RolloutDev& rd, const RolloutAdj& a) {
    const AdjLds L = adj_lds<PT, TREE, ATT>();
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b >= a.batch) return;
    AdjTracks tr;
    AdjPlantRows pr;
    adj_stage_in<PT, TREE, ATT>(rd, a, b, lane, tr, pr);
    const double m = L.p[VSMPC_PP_MASS];
    if (a.tick_rec >= 0) adj_record_half<PT, TREE, ATT>(rd, a, m, lane);
    double out0 = lane < 40 ? L.sb[lane] : 0.0;   // the new sbar of this lane's entry
    if (a.tick_plant >= 0) out0 = adj_plant_half<PT, TREE, ATT>(rd, a, tr, pr, m, b, lane);
    adj_write_out<PT, TREE, ATT>(rd, a, tr, out0, b, lane);
}

}  // namespace vsmpc
