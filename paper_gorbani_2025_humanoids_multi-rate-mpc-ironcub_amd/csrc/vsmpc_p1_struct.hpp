// P1s, structured condensing (FORM 1 of solve_kernel, horizons with Dims::STRUCT_P1): the chains, the contraction and
// the tile entries.
#pragma once
#include "vsmpc_smem.hpp"

namespace vsmpc {

// ------------------------------------------------------------------------------------------------
// P1s: structured condensing (Dims::STRUCT_P1; executable model: tests/condense_model.py).
//
// The model (systemDynamicsVSMPC.cpp:79-103,288-319,384-429) is a cascade throttles -> jets -> momenta -> CoM / RPY ->
// error integrators whose linear half (p, h_lin, e_pos) and angular half (rpy, h_ang, e_rpy) do not talk to each other,
// and every input reaches a half only as a 3-vector forcing of its momentum rows:  phi_i = Lambda U_{jb(i)} + A_mom T_i.
// Per half, with xi = (x, h, e), Abar_m = I + dt_m K, the condensed Hessian (what constraintsVSMPC.cpp:76-131 and
// costsVSMPC.cpp:166-200 imply once the states are eliminated) is
//     C[r, c] = sum_half sum_i pi_r(i)^T W_c(i),      W_c(i) = dt_i E_h^T nu_c(i + 1),
//     nu_c(m) = Q xi^c_m + Abar_m^T nu_c(m + 1)       (adjoint of column c's own forward trajectory xi^c),
// pi_c(i) the column's forcing profile: Lambda[:, q] while jb(i) = b for the joint column (b, q), A_mom[:, q] tau_i for a
// throttle column (tau = its jet's thrust trajectory from P1a).  A joint block only ever enters through the three momentum
// directions, so 3 generator columns per block (unit forcing e_d) stand for its 8 joint columns: one lane per
// (generator | throttle column | affine column) and half runs the forward recursion with the momentum part of the
// trajectory held in REGISTERS (3 N doubles; x and e are rolled back in the adjoint pass), then the adjoint recursion
// backwards, and leaves in LDS
//     sH [half][pair(bc <= br)][a][d]  = sum_{i in br} W_gen(bc, d)(i)[a]          (KIND 0, generator lanes)
//     sRb[half][c][b][a]               = sum_{i in b} W_c(i)[a]                     (KIND 1, throttle / affine lanes)
//     sW3[half][c][i - 1][a]           = W_c(i)[a],  i >= 1  (tau_0 = 0; short horizons: p1s_contract sums
//                                        sAc[c][i - 1][q] = sum_half A_mom[:, q]^T W_c(i) from it; long horizons add
//                                        their half of sAc straight from the chain with LDS atomics and have no sW3)
// from which p1s_entries forms every entry of C directly in the accumulator layout of the owning wavefront:
//     joint x joint        Lambda[:, qr]^T sH Lambda[:, qc]                               (summed over the halves)
//     throttle x joint     Lambda[:, qc]^T sRb[cr][bc]
//     throttle x throttle  sum_i tau^cc_i sAc[cr][i][q_cc]      (row = affine column: the condensed gradient)
// O(N^2) small 3x3 work (~0.3 MFLOP at the paper horizon) instead of the SYRK over the 18 N weighted sensitivity rows
// (3.8 MFLOP executed).  The affine column carries x0, c and the reference: W_aff(i) = gamma_i.
// ------------------------------------------------------------------------------------------------
// a wave-uniform double moved into scalar registers (v_fma_f64 takes one scalar operand pair): the coefficient matrices of
// a chain cost no vector registers, which is what lets the trajectory stay in them
VS_DEV double uniform_f64(double x) {
    const int lo = __builtin_amdgcn_readfirstlane(__double2loint(x));
    const int hi = __builtin_amdgcn_readfirstlane(__double2hiint(x));
    return __hiloint2double(hi, lo);
}

template <class D, int KIND, bool SMALL = false>
VS_DEV void p1s_chain(const DevCfg& cfg, int half, int lane, double* __restrict__ sm) {
    using S = Smem<D, SMALL>;
    constexpr int N = D::N, HC = D::HC, NV = D::NV;
    const double* sA = sm + S::oA;
    const double* sCfg = sm + S::oCfg;
    double* sH = sm + S::oSH;
    double* sRb = sm + S::oSRb;
    double* sW3 = sm + S::oSW3;
    const int xr0 = half ? 6 : 0, hr0 = half ? 9 : 3, er0 = half ? 23 : 20;   // state rows of this half
    const int yx0 = half ? 6 : 0, yh0 = half ? 9 : 3, ye0 = half ? 15 : 12;   // weighted-row slots (CFG_SQ, reference rows)
    // wave-uniform coefficients, in scalar registers.  A[h, h] = -S(omega) (systemDynamicsVSMPC.cpp:90-91,301-302) is
    // skew-symmetric with a zero diagonal: three numbers, and its transpose is its negative
    double M1[9], qx[3], qh[3], qe[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) M1[3 * r + c] = uniform_f64(sA[(xr0 + r) * NX + hr0 + c]);
        const double sx = sCfg[CFG_SQ + yx0 + r], sh = sCfg[CFG_SQ + yh0 + r], se = sCfg[CFG_SQ + ye0 + r];
        qx[r] = uniform_f64(sx * sx);
        qh[r] = uniform_f64(sh * sh);
        qe[r] = uniform_f64(se * se);
    }
    const double s01 = uniform_f64(sA[(hr0 + 0) * NX + hr0 + 1]), s02 = uniform_f64(sA[(hr0 + 0) * NX + hr0 + 2]),
                 s12 = uniform_f64(sA[(hr0 + 1) * NX + hr0 + 2]);
    // lane -> column.  Long horizons (Dims::NGX > 0): the generator columns 64 .. 3 HC - 1 ride in the lanes behind the
    // affine column of the KIND 1 wavefront of their half (unit forcing while their block is active: the activity takes
    // the place of the thrust trajectory, everything else reads the zeros)
    constexpr int NGX = D::NGX;
    constexpr bool LONG = D::STRUCT_LONG;
    constexpr int NLIVE = KIND == 0 ? (3 * HC < 64 ? 3 * HC : 64) : NV + 1 + NGX;
    const bool live = lane < NLIVE;
    const int col = live ? lane : NLIVE - 1;        // idle lanes shadow the last column and store nothing
    const bool isgen = KIND == 0 || (NGX > 0 && col > NV);
    const int gi = KIND == 0 ? col : (isgen ? 64 + col - (NV + 1) : 0);
    const int gb = gi / 3, gd = gi - 3 * gb;        // generator: joint block, momentum direction
    const bool affl = KIND == 1 && col == NV;       // KIND 1: the affine column
    // x carries x + c_e throughout (e' = x + c_e; the offset is folded into the reference the affine column reads)
    double dir[3];
    double x[3], h[3], e[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        if constexpr (KIND == 0) {
            dir[r] = gd == r ? 1.0 : 0.0;
            x[r] = 0.0; h[r] = 0.0; e[r] = 0.0;
        } else {
            const double a_q = sA[(hr0 + r) * NX + 12 + (col & 3)];
            dir[r] = affl ? 0.0 : (isgen ? (gd == r ? 1.0 : 0.0) : a_q);
            const double x0 = sm[S::oIn + VSMPC_IN_X0 + xr0 + r], h0 = sm[S::oIn + VSMPC_IN_X0 + hr0 + r],
                         e0 = sm[S::oIn + VSMPC_IN_X0 + er0 + r];
            const double ce0 = sm[S::oC + er0 + r];
            x[r] = affl ? x0 + ce0 : 0.0;
            h[r] = affl ? h0 : 0.0;
            e[r] = affl ? e0 : 0.0;
        }
    }
    // per-lane operand rows (KIND 1), as offsets into the workgroup's LDS: the jet's thrust trajectory; the affine column
    // reads its forcing A_mom Tbar_k + c_h and the reference where every other column reads zeros (no select in the chain)
    const int tauOff = (KIND == 1 && !affl && !isgen) ? S::oJetT + col * N : S::oSZero;
    const int gaOff = affl ? S::oGA + half * 3 * N : S::oSZero;
    const int refOff = affl ? S::oSRefC : S::oSZero;
    const double* tauRow = sm + tauOff;
    const double* gaRow = sm + gaOff;
    const double* refRow = sm + refOff;
    // long horizons: this half's thrust map and the row of sAc this lane adds to (see Smem::ac_off; the
    // stored stage i' lies at (i' - ac_first) * 4 behind it, so the offset of stage 0 is folded in)
    double Am[3][NTH];
    int acFirst = 0, acOff = 0;
    if constexpr (KIND == 1 && LONG) {
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int q = 0; q < NTH; ++q) Am[a][q] = sA[(hr0 + a) * NX + 12 + q];   // vector registers: the scalar file is full
        const int cr = col <= NV ? col : NV;
        acFirst = S::ac_first(cr);
        acOff = S::ac_off(cr) - 4 * acFirst;
    }
    // ---- forward: xi_{k+1} = xi_k + dt_k (K xi_k + forcing).  Only the momentum part of the trajectory is kept (3 N
    // doubles; the whole trajectory would be 18 N registers): x and e are rolled BACK in the adjoint pass, which explicit
    // Euler allows exactly up to rounding (x_m = x_{m+1} - dt_m M1 h_m, e_m = e_{m+1} - dt_m (x_m + c_e)).
    // Operands of stage k + 1 are requested at the top of stage k behind an offset the compiler cannot see through:
    // otherwise the loads of ALL stages are hoisted to the top of the unrolled chain and the trajectory gets spilled.
    double hk[N][3];
    double tk_n = 0.0, ga_n[3] = {0.0, 0.0, 0.0};
    if constexpr (KIND == 1) {
        tk_n = tauRow[0];
#pragma unroll
        for (int r = 0; r < 3; ++r) ga_n[r] = gaRow[r];
    }
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const double dt = cfg.dt[k];   // kernel argument: a scalar load
        double f[3];
        if constexpr (KIND == 0) {
            const double act = joint_block_of_stage<D>(k) == gb ? 1.0 : 0.0;
#pragma unroll
            for (int r = 0; r < 3; ++r) f[r] = act * dir[r];
        } else {
            double tk = tk_n;
            if constexpr (NGX > 0) tk = isgen ? (joint_block_of_stage<D>(k) == gb ? 1.0 : 0.0) : tk;
#pragma unroll
            for (int r = 0; r < 3; ++r) f[r] = fma(tk, dir[r], ga_n[r]);
            if (k + 1 < N) {
                int zo = 0;
                asm volatile("" : "+v"(zo));
                tk_n = tauRow[k + 1 + zo];
#pragma unroll
                for (int r = 0; r < 3; ++r) ga_n[r] = gaRow[3 * (k + 1) + r + zo];
            }
        }
        double dx[3], dh[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            dx[r] = fma(M1[3 * r + 2], h[2], fma(M1[3 * r + 1], h[1], M1[3 * r] * h[0]));
        }
        dh[0] = fma(s02, h[2], fma(s01, h[1], f[0]));
        dh[1] = fma(s12, h[2], fma(-s01, h[0], f[1]));
        dh[2] = fma(-s12, h[1], fma(-s02, h[0], f[2]));
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            e[r] = fma(dt, x[r], e[r]);           // explicit Euler: the old x (+ c_e)
            x[r] = fma(dt, dx[r], x[r]);
            h[r] = fma(dt, dh[r], h[r]);
        }
        // The state passes through an (empty) volatile statement at every stage boundary: volatile statements keep their
        // order, so stage k + 1 cannot start before stage k is complete.  Without it the instruction selector emits the
        // h chain of all stages first and the x and e chains afterwards, with every intermediate x_k alive in between.
        asm volatile("" : "+v"(x[0]), "+v"(x[1]), "+v"(x[2]), "+v"(h[0]), "+v"(h[1]), "+v"(h[2]), "+v"(e[0]), "+v"(e[1]), "+v"(e[2]));
#pragma unroll
        for (int r = 0; r < 3; ++r) hk[k][r] = h[r];   // h of node k + 1
        __builtin_amdgcn_sched_barrier(0);
    }
    // ---- backward: nu(m) = Q w_m + Abar_m^T nu(m + 1), m = N .. 1, w_m = xi_m (minus the reference on the affine column);
    // W(i) = dt_i nu(i + 1)[h].  (x, e) hold node m at the top of step m.
    double nx[3] = {0.0, 0.0, 0.0}, nh[3] = {0.0, 0.0, 0.0}, ne[3] = {0.0, 0.0, 0.0}, bs[3] = {0.0, 0.0, 0.0};
    double rf_n[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if constexpr (KIND == 1) {
        constexpr int rcN = N - 1 < D::NS ? 0 : N - 1 - D::NS;   // reference column of node N (costsVSMPC.cpp:191-200)
#pragma unroll
        for (int r = 0; r < 3; ++r) { rf_n[r] = refRow[rcN * 12 + yx0 + r]; rf_n[3 + r] = refRow[rcN * 12 + yh0 + r]; }
    }
#pragma unroll
    for (int m = N; m >= 1; --m) {
        const int i = m - 1;
        double rf[6];
#pragma unroll
        for (int r = 0; r < 6; ++r) rf[r] = rf_n[r];
        if constexpr (KIND == 1) {
            // reference column of node m - 1; the window only moves at the slow rate, so the fast nodes share column 0
            // and need no reload (costsVSMPC.cpp:191-200)
            const int rc = m - 2 < D::NS ? 0 : m - 2 - D::NS;
            const int rc_cur = m - 1 < D::NS ? 0 : m - 1 - D::NS;
            if (m >= 2 && rc != rc_cur) {
                int zo = 0;
                asm volatile("" : "+v"(zo));
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    rf_n[r] = refRow[rc * 12 + yx0 + r + zo];
                    rf_n[3 + r] = refRow[rc * 12 + yh0 + r + zo];
                }
            }
        }
        if (m < N) {
            const double dtm = cfg.dt[m];
            double t[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) t[r] = fma(M1[6 + r], nx[2], fma(M1[3 + r], nx[1], M1[r] * nx[0]));
            t[0] = fma(-s02, nh[2], fma(-s01, nh[1], t[0]));   // + Sk^T nu_h = - Sk nu_h
            t[1] = fma(-s12, nh[2], fma(s01, nh[0], t[1]));
            t[2] = fma(s12, nh[1], fma(s02, nh[0], t[2]));
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                nx[r] = fma(dtm, ne[r], nx[r]);   // K^T: the x rows of the adjoint collect the e rows (A[e, x] = I)
                nh[r] = fma(dtm, t[r], nh[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            nx[r] = fma(qx[r], KIND == 1 ? x[r] - rf[r] : x[r], nx[r]);
            nh[r] = fma(qh[r], KIND == 1 ? hk[i][r] - rf[3 + r] : hk[i][r], nh[r]);
            ne[r] = fma(qe[r], e[r], ne[r]);
        }
        const double dti = cfg.dt[i];
        if (m >= 2) {   // roll (x, e) back to node m - 1 with h of node m - 1
            // (opaque copies: otherwise the compiler recognises M1 h of the forward pass and keeps all N of them alive
            // -- in scratch -- instead of recomputing, which is the whole point of keeping only h)
            double hp[3] = {hk[i - 1][0], hk[i - 1][1], hk[i - 1][2]};
            asm volatile("" : "+v"(hp[0]), "+v"(hp[1]), "+v"(hp[2]));
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const double dxr = fma(M1[3 * r + 2], hp[2], fma(M1[3 * r + 1], hp[1], M1[3 * r] * hp[0]));
                x[r] = fma(-dti, dxr, x[r]);
                e[r] = fma(-dti, x[r], e[r]);
            }
        }
        double w[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) { w[a] = dti * nh[a]; bs[a] += w[a]; }
        if constexpr (KIND == 1 && !LONG) {
            if (i >= 1 && live) {
                double* Wp = sW3 + ((half * (NV + 1) + col) * (N - 1) + (i - 1)) * 3;
#pragma unroll
                for (int a = 0; a < 3; ++a) Wp[a] = w[a];
            }
        }
        if constexpr (KIND == 1 && LONG) {
            // A_mom[:, q]^T W_c(i), added to what the other half leaves in the same word (two addends on a zeroed word:
            // the sum does not depend on which arrives first)
            if (i >= 1) {
                if (live && !isgen && i - 1 >= acFirst) {
                    typedef __attribute__((address_space(3))) double lds_double;
                    double* Ap = sm + S::oSAc + acOff + (i - 1) * 4;
#pragma unroll
                    for (int q = 0; q < NTH; ++q) {
                        const double v = fma(Am[2][q], w[2], fma(Am[1][q], w[1], Am[0][q] * w[0]));
                        __builtin_amdgcn_ds_atomic_fadd_f64((lds_double*)(Ap + q), v, 0, 0, false);
                    }
                }
            }
        }
        if (i < HC) {   // i is the first stage of joint block jb(i) = i (the last block spans stages HC-1 .. N-1)
            if (isgen) {
                if (live && i >= gb) {
                    double* Hp = sH + (half * D::NJPAIR + i * (i + 1) / 2 + gb) * 9 + gd;
#pragma unroll
                    for (int a = 0; a < 3; ++a) Hp[3 * a] = bs[a];
                }
            } else {
                if (live) {
                    double* Rp = sRb + ((half * (NV + 1) + col) * HC + i) * 3;
#pragma unroll
                    for (int a = 0; a < 3; ++a) Rp[a] = bs[a];
                }
            }
#pragma unroll
            for (int a = 0; a < 3; ++a) bs[a] = 0.0;
        }
        asm volatile("" : "+v"(nx[0]), "+v"(nx[1]), "+v"(nx[2]), "+v"(nh[0]), "+v"(nh[1]), "+v"(nh[2]), "+v"(ne[0]), "+v"(ne[1]), "+v"(ne[2]));
        asm volatile("" : "+v"(x[0]), "+v"(x[1]), "+v"(x[2]), "+v"(e[0]), "+v"(e[1]), "+v"(e[2]), "+v"(bs[0]), "+v"(bs[1]), "+v"(bs[2]));
        __builtin_amdgcn_sched_barrier(0);
    }
}

// sAc[c][i - 1][q] = sum over the halves of A_mom,half[:, q]^T W_c(i): the throttle x throttle tiles read it as a matrix-core
// operand.  All wavefronts, between the chains and the entries: one (c, i) pair and its four q per thread and round.
// (The small-batch kind runs it off that path: p1s_contract_beside.)
template <class D>
VS_DEV void p1s_contract(double* __restrict__ sm, int tid) {
    using S = Smem<D>;
    constexpr int NI = (D::NV + 1) * (D::N - 1);
    constexpr int ROUNDS = (NI + D::BLOCK - 1) / D::BLOCK;
    const double* sA = sm + S::oA;
    const double* sW3 = sm + S::oSW3;
    double* sAc = sm + S::oSAc;
    double w[ROUNDS][6];
#pragma unroll
    for (int rd = 0; rd < ROUNDS; ++rd) {
        const int ci = tid + rd * D::BLOCK, cic = ci < NI ? ci : NI - 1;
#pragma unroll
        for (int a = 0; a < 3; ++a) { w[rd][a] = sW3[cic * 3 + a]; w[rd][3 + a] = sW3[(NI + cic) * 3 + a]; }
    }
    double Am[6][NTH];   // uniform addresses: LDS broadcasts
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int q = 0; q < NTH; ++q) { Am[a][q] = sA[(3 + a) * NX + 12 + q]; Am[3 + a][q] = sA[(9 + a) * NX + 12 + q]; }
#pragma unroll
    for (int rd = 0; rd < ROUNDS; ++rd) {
        const int ci = tid + rd * D::BLOCK;
        double v[NTH];
#pragma unroll
        for (int q = 0; q < NTH; ++q) {
            v[q] = Am[0][q] * w[rd][0];
#pragma unroll
            for (int a = 1; a < 6; ++a) v[q] = fma(Am[a][q], w[rd][a], v[q]);
        }
        if (ci < NI) {
#pragma unroll
            for (int q = 0; q < NTH; ++q) sAc[ci * 4 + q] = v[q];
        }
    }
}

// The same contraction as the small-batch kind runs it: by wavefronts 1..3 (t = 0 .. 191) beside panel stream 0, at the head of
// their instalment 1 (small_form) -- nothing reads sAc before instalment 2, and the barrier that closes stream 0 publishes it.
// One round at a time (the column-0 tiles are live in registers here); every item's expression and summation order are those
// of p1s_contract, so the values are bit for bit the same.
template <class D>
VS_DEV void p1s_contract_beside(double* __restrict__ sm, int t) {
    using S = Smem<D, true>;
    constexpr int NI = (D::NV + 1) * (D::N - 1);
    constexpr int NTHR = (D::NWAVES - 1) * 64;
    constexpr int ROUNDS = (NI + NTHR - 1) / NTHR;
    const double* sA = sm + S::oA;
    const double* sW3 = sm + S::oSW3;
    double* sAc = sm + S::oSAc;
    double Am[6][NTH];   // uniform addresses: LDS broadcasts
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int q = 0; q < NTH; ++q) { Am[a][q] = sA[(3 + a) * NX + 12 + q]; Am[3 + a][q] = sA[(9 + a) * NX + 12 + q]; }
#pragma unroll
    for (int rd = 0; rd < ROUNDS; ++rd) {
        const int ci = t + rd * NTHR, cic = ci < NI ? ci : NI - 1;
        double w[6];
#pragma unroll
        for (int a = 0; a < 3; ++a) { w[a] = sW3[cic * 3 + a]; w[3 + a] = sW3[(NI + cic) * 3 + a]; }
        double v[NTH];
#pragma unroll
        for (int q = 0; q < NTH; ++q) {
            v[q] = Am[0][q] * w[0];
#pragma unroll
            for (int a = 1; a < 6; ++a) v[q] = fma(Am[a][q], w[a], v[q]);
        }
        if (ci < NI) {
#pragma unroll
            for (int q = 0; q < NTH; ++q) sAc[ci * 4 + q] = v[q];
        }
        __builtin_amdgcn_sched_barrier(0);   // (a round's operands are dead before the next round asks for its own)
    }
}

// Entries of C = sum_k Y_k^T Y_k for the accumulator tiles wavefront W owns, formed ON THE MATRIX CORES from the small LDS
// arrays the chains leave behind, so that they arrive in the accumulator layout (lane (g, j) holds rows g + 4 r, column j)
// with a handful of LDS reads per tile.  With L = R^T (6 x 6, rows = (half, a), the input matrix of the reduced joint
// unknowns; p0_joint_reduction) a tile row t holds the joint rows 16 t .. 16 t + 15 = unknown (16 t + j) % 6 of block
// (16 t + j) / 6: at most FOUR blocks, the first one blk0(t) = 16 t / 6.  The k index of a product is split as
// k = 4 ks + g  ->  (a6, kb) = (ks, g)   (a6 = (half, a), kb = block within the tile row):
//   joint x joint        D = A B,  A[m][k] = [blk(ti, m) == blk0(ti) + kb] L[a6][unknown(ti, m)],
//                        B[k][n] = (H^(blk0(ti) + kb, blk(tj, n)) L)[a6][unknown(tj, n)]                  6 k-steps
//   throttle x joint     A[m][k] = sRb[half(a6)][row m][blk0(tj) + kb][a],
//                        B[k][n] = [blk(tj, n) == blk0(tj) + kb] L[a6][unknown(tj, n)]                    6 k-steps
//   throttle x throttle  k = (i', q): A[m][k] = sAc[row m][i'][q],  B[k][n] = [q == q_n] tau^n_{i' + 1}    N - 1 k-steps
// Rows / columns of the dummy unknowns (16 t + j >= NUY) get zero operands.  Operands first, matrix instructions
// afterwards: with the loads of a tile right in front of its instructions every tile pays LDS round trips; the
// accumulators are not live yet, so there are registers for the raw operands of a group of tiles at once (the loads are
// pinned in front of the arithmetic).
// PLAN says which slots this call forms: slot(a), a < count, in the order they are formed (groups of G), and forms(q).  The
// shipped kernels form every slot at once (AllSlots); the small-batch kind forms a wavefront's tiles in three instalments
// (SmallPlan in vsmpc_p3.hpp) from the arrays its carve-up keeps intact (Smem<D, true>).  A slot outside the plan is left alone.
template <class D, int TPW, int W, bool PIPE>
struct AllSlots {
    static constexpr bool SMALL = false;
    static constexpr int count = TPW;
    static constexpr int slot(int a) { return a; }
    static constexpr bool forms(int q) { return TileTab<D, PIPE>{}.forms(q * D::NWAVES + W, W); }
};
template <class D, int TPW, int W, bool PIPE = false, class PLAN = AllSlots<D, TPW, W, PIPE>>
VS_DEV void p1s_entries(d4 (&acc)[TPW], const double* __restrict__ sm, int lane) {
    using S = Smem<D, PLAN::SMALL>;
    constexpr int PVT = D::PVT, N = D::N, HC = D::HC, NV = D::NV;
    static_assert(D::NU % 16 == 0, "joint rows are tile aligned");
    const double* sBj = sm + S::oBj;
    const double* sH = sm + S::oSH;
    const double* sRb = sm + S::oSRb;
    const double* sAc = sm + S::oSAc;
    const double* sJetT = sm + S::oJetT;
    // (opaque: the four wave-specialised copies of this function start with the same table loads, which the compiler would
    // otherwise hoist in front of the wave dispatch and, at the 2x horizon, spill across it -- 100 registers of scratch)
    lane = fresh_lane();
    const int j = lane & 15, g = lane >> 4;
    // per lane and tile-row pattern (16 t mod 6 = 0, 4, 2 for t mod 3 = 0, 1, 2): the unknown and the block within the tile
    // row of row / column j, and the six entries L[a6][unknown]
    // LqM: the same entries masked to the k block of this lane ([blk(t, j) == blk0(t) + g]: the A operand of a joint x joint
    // tile, the B operand of a throttle x joint tile), formed once instead of with six selects per tile
    double Lq[3][NJC], LqM[3][NJC];
    int bin[3];
#pragma unroll
    for (int pat = 0; pat < 3; ++pat) {
        const int o = ((16 * pat) % NJC) + j;
        bin[pat] = o / NJC;
        const int un = o - NJC * bin[pat];
#pragma unroll
        for (int a6 = 0; a6 < NJC; ++a6) {
            Lq[pat][a6] = sBj[((a6 < 3 ? 3 : 6) + a6) * NJ + un];
            LqM[pat][a6] = bin[pat] == g ? Lq[pat][a6] : 0.0;
        }
    }
    // tiles in groups of G (the raw operands of a group are all requested before its arithmetic starts)
    // 18 G + 12 G operand registers (doubles) beside the 18 of Lq; long horizons keep finished tiles in registers meanwhile
    constexpr int G = 3;
    constexpr int NSLOT = PLAN::count;
    constexpr int NGRP = (NSLOT + G - 1) / G;
    static_for<0, NGRP>([&](auto gcst) __attribute__((always_inline)) {
    constexpr int q0 = decltype(gcst)::value * G;
    constexpr int q1 = q0 + G < NSLOT ? q0 + G : NSLOT;
    double raw[G][NJC][3];
    static_for<q0, q1>([&](auto qcst) __attribute__((always_inline)) {
        constexpr TileTab<D, PIPE> tab{};
        constexpr int qi = decltype(qcst)::value;   // position in the plan; q: the slot
        constexpr int q = PLAN::slot(qi);
        constexpr int t = q * D::NWAVES + W;
        if constexpr (PLAN::forms(q)) {
            constexpr int ti = tab.ti[t], tj = tab.tj[t];
            if constexpr (ti < PVT) {
                // H^(br, bc), br = blk0(ti) + g (this lane's k block), bc = the block of column j of tile column tj; stored
                // for br >= bc, transposed otherwise (diagonal tiles only).  Blocks beyond the horizon belong to dummy rows /
                // columns whose other operand is zero: clamped into the array.
                constexpr int b0r = (16 * ti) / NJC, b0c = (16 * tj) / NJC;
                const int brr = b0r + g, bcc = b0c + bin[tj % 3];
                const int br = brr < HC ? brr : HC - 1, bc = bcc < HC ? bcc : HC - 1;
                const bool sw = ti == tj && br < bc;
                const int hi = sw ? bc : br, lo = sw ? br : bc;
                const int st = sw ? 3 : 1, sa = sw ? 1 : 3;
                const double* Hp = sH + (hi * (hi + 1) / 2 + lo) * 9;
#pragma unroll
                for (int ks = 0; ks < NJC; ++ks) {
                    const double* Hk = Hp + (ks / 3) * D::NJPAIR * 9 + sa * (ks % 3);
#pragma unroll
                    for (int d = 0; d < 3; ++d) raw[qi - q0][ks][d] = Hk[d * st];
                }
            } else if constexpr (tj < PVT) {
                constexpr int b0c = (16 * tj) / NJC;
                const int cr = 16 * (ti - PVT) + j;
                const int crc = cr <= NV ? cr : NV;
                const int bcc = b0c + g, bc = bcc < HC ? bcc : HC - 1;
#pragma unroll
                for (int ks = 0; ks < NJC; ++ks)
                    raw[qi - q0][ks][0] = sRb[(((ks / 3) * (NV + 1) + crc) * HC + bc) * 3 + (ks % 3)];
            }
        }
    });
    __builtin_amdgcn_sched_barrier(0);
    double opa[G][NJC], opb[G][NJC];
    static_for<q0, q1>([&](auto qcst) __attribute__((always_inline)) {
        constexpr TileTab<D, PIPE> tab{};
        constexpr int qi = decltype(qcst)::value;
        constexpr int q = PLAN::slot(qi);
        constexpr int t = q * D::NWAVES + W;
#pragma unroll
        for (int ks = 0; ks < NJC; ++ks) { opa[qi - q0][ks] = 0.0; opb[qi - q0][ks] = 0.0; }
        if constexpr (PLAN::forms(q)) {
            constexpr int ti = tab.ti[t], tj = tab.tj[t];
            // rows / columns of the dummy unknowns exist in the last joint tile row / column only (compile time)
            constexpr bool DUMMY_ROWS = 16 * ti + 16 > D::NUY, DUMMY_COLS = 16 * tj + 16 > D::NUY;
            if constexpr (ti < PVT) {
                const bool okm = 16 * ti + j < D::NUY, okn = 16 * tj + j < D::NUY;
#pragma unroll
                for (int ks = 0; ks < NJC; ++ks) {
                    const int h3 = 3 * (ks / 3);
                    const double hl = fma(raw[qi - q0][ks][2], Lq[tj % 3][h3 + 2],
                                          fma(raw[qi - q0][ks][1], Lq[tj % 3][h3 + 1], raw[qi - q0][ks][0] * Lq[tj % 3][h3]));
                    opa[qi - q0][ks] = (!DUMMY_ROWS || okm) ? LqM[ti % 3][ks] : 0.0;   // A: row j of tile row ti sits in k block g
                    opb[qi - q0][ks] = (!DUMMY_COLS || okn) ? hl : 0.0;
                }
            } else if constexpr (tj < PVT) {
                const bool okr = 16 * (ti - PVT) + j <= NV;
                const bool okn = 16 * tj + j < D::NUY;
#pragma unroll
                for (int ks = 0; ks < NJC; ++ks) {
                    opa[qi - q0][ks] = okr ? raw[qi - q0][ks][0] : 0.0;
                    opb[qi - q0][ks] = (!DUMMY_COLS || okn) ? LqM[tj % 3][ks] : 0.0;
                }
            }
        }
    });
    __builtin_amdgcn_sched_barrier(0);
    static_for<q0, q1>([&](auto qcst) __attribute__((always_inline)) {
        constexpr TileTab<D, PIPE> tab{};
        constexpr int qi = decltype(qcst)::value;
        constexpr int q = PLAN::slot(qi);
        constexpr int t = q * D::NWAVES + W;
        d4 c = d4{0.0, 0.0, 0.0, 0.0}, c2 = d4{0.0, 0.0, 0.0, 0.0};
        if constexpr (PLAN::forms(q)) {
            constexpr int ti = tab.ti[t], tj = tab.tj[t];
            if constexpr (tj < PVT) {
#pragma unroll
                for (int ks = 0; ks < NJC; ks += 2) {   // two accumulators (a dependent FP64 matrix instruction issues every ~95 cycles)
                    c = __builtin_amdgcn_mfma_f64_16x16x4f64(opa[qi - q0][ks], opb[qi - q0][ks], c, 0, 0, 0);
                    c2 = __builtin_amdgcn_mfma_f64_16x16x4f64(opa[qi - q0][ks + 1], opb[qi - q0][ks + 1], c2, 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) c[r] += c2[r];
            }
        }
        acc[q] = c;
    });
    __builtin_amdgcn_sched_barrier(0);
    });
    // throttle x throttle tiles: all operand pairs of a tile are requested before its chain starts.  The k-steps start at
    // the first stage any column of the tile can see (tau_i = 0 up to a column's first stage); a row that does not store
    // an earlier stage (Smem::ac_first) meets only such columns in the lower triangle and reads a zero there.
    static_for<0, NSLOT>([&](auto qcst) __attribute__((always_inline)) {
        constexpr TileTab<D, PIPE> tab{};
        constexpr int q = PLAN::slot(decltype(qcst)::value);
        constexpr int t = q * D::NWAVES + W;
        if constexpr (PLAN::forms(q)) {
            constexpr int ti = tab.ti[t], tj = tab.tj[t];
            if constexpr (ti >= PVT && tj >= PVT) {
                constexpr int K0 = tile_first_stage<D>(tj);   // first k-step (stage i' = i - 1)
                constexpr int NK = N - 1 - K0;
                // (lane-derived values are formed afresh here: carried across the joint tiles above they were spilled)
                const int ln = fresh_lane(), j = ln & 15, g = ln >> 4;
                const int cr = 16 * (ti - PVT) + j, cc = 16 * (tj - PVT) + j;
                const bool okr = cr <= NV, okc = cc < NV && g == (cc & 3);
                const int crc = okr ? cr : NV;
                const int rfirst = S::ac_first(crc);
                const double* Ap = sAc + S::ac_off(crc) - 4 * rfirst + g;
                const double* Tp = sJetT + (cc < NV ? cc : 0) * N + 1;
                // operand pairs in chunks of CH k-steps (all of them at short horizons): at the 2x horizon a tile has up to 33
                // k-steps, and 66 operand registers requested at once were spilled to scratch as they arrived
                constexpr int CH = D::STRUCT_LONG ? 8 : NK;
                // two accumulators: a dependent v_mfma_f64_16x16x4_f64 issues every ~95 cycles, independent ones every 64
                // (tools/microbench/lat_probe.hip)
                d4 c = d4{0.0, 0.0, 0.0, 0.0}, c2 = d4{0.0, 0.0, 0.0, 0.0};
                static_for<0, (NK + CH - 1) / CH>([&](auto ccst) __attribute__((always_inline)) {
                    constexpr int k0 = decltype(ccst)::value * CH;
                    constexpr int kn = k0 + CH < NK ? CH : NK - k0;
                    double av[kn], bv[kn];
#pragma unroll
                    for (int ks = 0; ks < kn; ++ks) {
                        const int ip = K0 + k0 + ks;
                        // (a short row does not store the stages before rfirst: the load then hits the row in front of it --
                        // always inside the workgroup's LDS -- and is discarded below; a conditional load would be a branch)
                        av[ks] = Ap[4 * ip];
                        bv[ks] = Tp[ip];
                    }
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int ks = 0; ks < kn; ++ks) {
                        const int ip = K0 + k0 + ks;
                        const bool stored = !(D::STRUCT_LONG && ip < S::AC_NSH) || ip >= rfirst;
                        av[ks] = (okr && stored) ? av[ks] : 0.0;
                        bv[ks] = okc ? bv[ks] : 0.0;
                    }
#pragma unroll
                    for (int ks = 0; ks < kn; ++ks) {
                        if ((k0 + ks) & 1) c2 = __builtin_amdgcn_mfma_f64_16x16x4f64(av[ks], bv[ks], c2, 0, 0, 0);
                        else c = __builtin_amdgcn_mfma_f64_16x16x4f64(av[ks], bv[ks], c, 0, 0, 0);
                    }
                });
#pragma unroll
                for (int r = 0; r < 4; ++r) c[r] += c2[r];
                acc[q] = c;
            }
        }
    });
}

}  // namespace vsmpc
