// The record adjoint of the runtime-sized kernels: what adjoint_record_kernel_rt[_tuned] add to the adjoint entry (included
// by vsmpc_runtime.hip after vsmpc_rt_adjoint.hpp).
//
// adjoint_record_kernel_rt / adjoint_record_kernel_rt_tuned (vsmpc_adjoint_record_batch) are rt_solve<RT_ADJOINT_REC>: every
// phase of rt_solve<RT_ADJOINT>, its outputs included, then, on a Solved exit, two phases that turn what the adjoint phases
// left in LDS -- the solution (X in s.x, z = [U | V] in s.z), the primal part a of the adjoint (a_X in s.big, [a_U | a_V] in
// s.col) and its multipliers b (s.big, the throttle rows' b_t in s.vec0) -- into dL/d(every entry of the record) (DESIGN.md,
// "Adjoint of the record"; executable model: tests/adjoint_record_model.py condensed_record_adjoint).  With nu the
// multipliers of the solve itself and the rows of the dynamics written as the reference-ordered dense QP writes them
// (constraintsVSMPC.cpp:76-131), (I + dt_k A) X_k - X_{k+1} + dt_k Bj U_jb(k) + dt_k Bt V_tb(k) = -dt_k c:
//   rt_adj_model   nu_{N-1} = Q (X_N - xref_N), nu_{k-1} = Q (X_k - xref_k) + (I + dt_k A)^T nu_k (certify_kernel's costates)
//                  fused with G = dL/d(A | Bj | Bt | c):
//                  G_A = -sum_k dt_k (nu_k a_Xk^T + b_k X_k^T), G_Bj, G_Bt likewise with (a_U, U)[jb(k)] and (a_V, V)[tb(k)],
//                  G_c = -sum_k dt_k b_k
//   rt_adj_record  the transpose of p0_linearize applied to G, plus the entries that reach the QP directly (the window, the
//                  posture error, the previous throttle through the initial-throttle cost and the hold pin, X0), one record
//                  entry per thread; grad_in [n_in] and grad_model [1014] out
#pragma once
#include "vsmpc_rt_adjoint.hpp"

namespace vsmpc {

namespace {

// outputs of the record adjoint, per batch; each may be null
struct RtAdjRecOut {
    double* gin = nullptr;      // [n_in]: dL/d record
    double* gmodel = nullptr;   // [VSMPC_GRAD_MODEL_SIZE]: dL/d(A | Bj | Bt | c), vsmpc_linearize_batch's layout
};

constexpr int RT_GMODEL = VSMPC_GRAD_MODEL_SIZE;                 // 1014 entries of G
constexpr int RT_GMODEL_CPT = (RT_GMODEL + RT_BLOCK - 1) / RT_BLOCK;   // entries per thread: 4
static_assert(VSMPC_GRAD_MODEL_A == 0 && VSMPC_GRAD_MODEL_BJ == NX * NX && VSMPC_GRAD_MODEL_BT == NX * NX + NX * NJ &&
              VSMPC_GRAD_MODEL_C == NX * NX + NX * NJ + NX * NTH && RT_GMODEL == VSMPC_GRAD_MODEL_C + NX,
              "grad_model is p0_linearize's block without its padding");

// the record adjoint's carve-up of s.big: the adjoint's a_X | b, then G [1014] (an even count in front of whatever follows)
VS_HD int rt_big_adjoint_record(const RtDims& d) { return rt_big_adjoint(d) + ((RT_GMODEL + 1) & ~1); }
VS_DEV double* rt_adj_g(const RtCtx& c) { return c.lds().big + rt_big_adjoint(c.d); }

// the window entry that node i >= 1 tracks in state row r (0 on the rows without a reference)
VS_DEV double rt_xref(const RtDims& d, const double* in, int i, int r) {
    const int col = (i - 1) < d.ns ? 0 : (i - 1) - d.ns;
    return r < 12 ? in[VSMPC_IN_XREF + col * 12 + r] : 0.0;
}

// ---- record adjoint 1: the solve's costates nu_k fused with G = dL/d(A | Bj | Bt | c)
// Reads X (s.x), z (s.z), a_X and b (s.big), a_z (s.col), the window (s.in), the linearisation, s.dt, cfg.sq.  Leaves G in
// s.big behind b.  Uses s.red for nu_k | nu_{k-1} (free: rt_adj_reduce_write's partial sums have been read behind the
// barrier this phase opens with).  Thread t owns entries t, t + 256, .. of G and adds stage N - 1 first and stage 0 last,
// two fused multiply-adds per entry and stage: an order the sizes alone fix.
template <class Cfg>
VS_DEV void rt_adj_model(const RtCtx& c, const Cfg& cfg) {
    const RtSmem s = c.lds();
    const RtDims& d = c.d;
    const int tid = c.tid, N = d.n, NU = d.nu;
    const double* aX = rt_adj_ax(c);
    const double* b = rt_adj_b(c);
    const double* X = s.x;
    double* nu = s.red;   // nu_k at nu + (k & 1) * NX
    const double qd = tid < NX ? q_diag(cfg.sq, tid) : 0.0;
    // what entry e = tid + u * 256 multiplies: row r of (nu_k, b_k) and entry `col` of (left, right), where (left, right) is
    // (a_Xk, X_k) for A, (a_U, U)[jb(k)] for Bj, (a_V, V)[tb(k)] for Bt, and (0, 1) for c
    int kind[RT_GMODEL_CPT], row[RT_GMODEL_CPT], col[RT_GMODEL_CPT];   // kind: 0 A, 1 Bj, 2 Bt, 3 c, 4 none
    double acc[RT_GMODEL_CPT];
#pragma unroll
    for (int u = 0; u < RT_GMODEL_CPT; ++u) {
        const int e = tid + u * RT_BLOCK;
        kind[u] = e < VSMPC_GRAD_MODEL_BJ ? 0 : (e < VSMPC_GRAD_MODEL_BT ? 1 : (e < VSMPC_GRAD_MODEL_C ? 2 : (e < RT_GMODEL ? 3 : 4)));
        const int f = e - (kind[u] == 0 ? 0 : (kind[u] == 1 ? VSMPC_GRAD_MODEL_BJ : (kind[u] == 2 ? VSMPC_GRAD_MODEL_BT : VSMPC_GRAD_MODEL_C)));
        const int w = kind[u] == 0 ? NX : (kind[u] == 1 ? NJ : (kind[u] == 2 ? NTH : 1));
        row[u] = kind[u] == 4 ? 0 : f / w;
        col[u] = kind[u] == 4 ? 0 : f - row[u] * w;
        acc[u] = 0.0;
    }
    __syncthreads();
    if (tid < NX) nu[((N - 1) & 1) * NX + tid] = qd * (X[N * NX + tid] - rt_xref(d, s.in, N, tid));
    __syncthreads();
    for (int k = N - 1; k >= 0; --k) {
        const double* cur = nu + (k & 1) * NX;   // nu_k
        double* nxt = nu + ((k + 1) & 1) * NX;    // nu_{k-1}
        const double dt = s.dt[k];
        const int offJ = NJ * joint_block(d, k), offV = NU + NTH * throttle_block(d, k);
#pragma unroll
        for (int u = 0; u < RT_GMODEL_CPT; ++u) {
            if (kind[u] == 4) continue;
            const double bk = -dt * b[k * NX + row[u]];
            if (kind[u] == 3) { acc[u] += bk; continue; }
            const int at = (kind[u] == 0 ? k * NX : (kind[u] == 1 ? offJ : offV)) + col[u];
            const double left = kind[u] == 0 ? aX[at] : s.col[at];
            const double right = kind[u] == 0 ? X[at] : s.z[at];
            acc[u] = fma(-dt * cur[row[u]], left, acc[u]);
            acc[u] = fma(bk, right, acc[u]);
        }
        if (k > 0 && tid < NX) {
            double t = 0.0;
            for (int q = 0; q < NX; ++q) t = fma(s.sA[q * NX + tid], cur[q], t);
            nxt[tid] = qd * (X[k * NX + tid] - rt_xref(d, s.in, k, tid)) + fma(dt, t, cur[tid]);
        }
        __syncthreads();
    }
    double* G = rt_adj_g(c);
#pragma unroll
    for (int u = 0; u < RT_GMODEL_CPT; ++u)
        if (kind[u] != 4) G[tid + u * RT_BLOCK] = acc[u];
    __syncthreads();
}

// ---- record adjoint 2: one entry of dL/d record, by the thread that stores it
// Reads G, a_X, b_init (s.big), a_z (s.col), b_t (s.vec0), the record (s.in), the linearisation (A[rpy, angMom] = W^-1 I^-1
// as p0_linearize left it), cfg.sq, cfg.w_reg, cfg.w_init.  The entries nothing reads (the yaw of IN_RPY, the last window
// column) and the hold flag, a switch, get +0.0.
template <class Cfg>
VS_DEV double rt_adj_record_entry(const RtCtx& c, const Cfg& cfg, bool hold, int use_jet, int e) {
    const RtSmem s = c.lds();
    const RtDims& d = c.d;
    const int N = d.n, NU = d.nu;
    const double* in = s.in;
    const double* G = rt_adj_g(c);
    const double* GA = G + VSMPC_GRAD_MODEL_A;
    const double* GBj = G + VSMPC_GRAD_MODEL_BJ;
    const double* GBt = G + VSMPC_GRAD_MODEL_BT;
    const double* Gc = G + VSMPC_GRAD_MODEL_C;
    const double* aX = rt_adj_ax(c);
    const double* aU = s.col;
    const double* aV = s.col + NU;
    if (e < VSMPC_IN_MASS) return rt_adj_b(c)[N * NX + e];                                    // X0: b_init
    if (e >= VSMPC_IN_XREF) {
        // window column `col`, row r: q_r times the sum of a_X over the nodes that track it -- nodes 1 .. ns + 1 for column
        // 0, node ns + 1 + col for the others, none for the last column
        const int f = e - VSMPC_IN_XREF, wc = f / 12, r = f - 12 * wc;
        const int first = wc == 0 ? 1 : d.ns + 1 + wc, last = d.ns + 1 + wc < N ? d.ns + 1 + wc : N;
        double acc = 0.0;
        for (int i = first; i <= last; ++i) acc += aX[i * NX + r];
        return first <= last ? q_diag(cfg.sq, r) * acc : 0.0;
    }
    if (e >= VSMPC_IN_HOLD) return 0.0;
    if (e >= VSMPC_IN_QERR) {
        double acc = 0.0;
        for (int blk = 0; blk < d.hc; ++blk) acc += aU[blk * NJ + (e - VSMPC_IN_QERR)];
        return -cfg.w_reg * acc;
    }
    if (e >= VSMPC_IN_T0) {
        // the jets (p0_linearize, tid 64..67): A[16+i, 12+i] = dh/dT, A[16+i, 16+i] = dh/dTdot, Bt[16+i, i] = G(Tdes, Tdotdes),
        // c[16+i] = F - dh/dT T0 - dh/dTdot Tdot0 with dh/d. = df/d. + dg/d. v(u_prev); f and g are quadratics
        const int fld = (e - VSMPC_IN_T0) >> 2, i = (e - VSMPC_IN_T0) & 3;   // 0 T0, 1 TD0, 2 UPREV, 3 TDES, 4 TDDES
        const double gBt = GBt[(16 + i) * NTH + i];
        if (fld >= 3) {
            if (!use_jet) return 0.0;
            const double ta = Jet::stdT(in[VSMPC_IN_TDES + i]), tb = Jet::stdTd(in[VSMPC_IN_TDDES + i]);
            return gBt * (fld == 3 ? Jet::dg_dT(ta, tb) : Jet::dg_dTd(ta, tb));      // d(G sigma_T)/dT = dg/dTbar
        }
        const double ub = Jet::stdU(in[VSMPC_IN_UPREV + i]);
        const double dvdu = Jet::dv_du(ub) * Jet::isgU;                              // d v(u_prev) / d u_prev (percent)
        double direct = 0.0;
        if (fld == 2) direct = dvdu * (cfg.w_init * aV[i] + (hold ? s.vec0[i] : 0.0));   // initial-throttle cost, hold pin
        if (!use_jet) return direct;
        const double T0 = in[VSMPC_IN_T0 + i], Td0 = in[VSMPC_IN_TD0 + i];
        const double ta = Jet::stdT(T0), tb = Jet::stdTd(Td0), vv = Jet::v(ub);
        const double gc = Gc[16 + i];
        const double wT = fma(-gc, T0, GA[(16 + i) * NX + 12 + i]);      // on dh/dT, through A and through c
        const double wTd = fma(-gc, Td0, GA[(16 + i) * NX + 16 + i]);    // on dh/dTdot
        if (fld == 2) return direct + (wT * Jet::dg_dT(ta, tb) + wTd * Jet::dg_dTd(ta, tb)) * dvdu;
        const double hTTd = (Jet::d2f_dTdTd + Jet::d2g_dTdTd * vv) * Jet::isgT;
        if (fld == 0) {
            const double hTT = (Jet::d2f_dT2 + Jet::d2g_dT2 * vv) * Jet::isgT;
            return wT * hTT + wTd * hTTd + gc * (Jet::df_dT(ta, tb) - Jet::dh_dT(T0, Td0, in[VSMPC_IN_UPREV + i]));
        }
        const double hTdTd = (Jet::d2f_dTd2 + Jet::d2g_dTd2 * vv) * Jet::isgT;
        return wT * hTTd + wTd * hTdTd + gc * (Jet::df_dTd(ta, tb) - Jet::dh_dTd(T0, Td0, in[VSMPC_IN_UPREV + i]));
    }
    if (e >= VSMPC_IN_RPYINIT) return -Gc[23 + e - VSMPC_IN_RPYINIT];
    if (e >= VSMPC_IN_PREF) return -Gc[20 + e - VSMPC_IN_PREF];
    if (e >= VSMPC_IN_INERTIA) {
        // A[rpy, angMom] = M = W^-1(rpy) I^-1 (p0_linearize, tid < 64).  With Gm the block of G_A on it and Nm = Gm I^-T:
        // dL/dI = -M^T Nm (from dM = -M dI I^-1), dL/d roll | pitch = sum dW^-1/d. o Nm
        if (e == VSMPC_IN_RPY + 2) return 0.0;
        const double* I = in + VSMPC_IN_INERTIA;
        const double a = I[0], b = I[1], cc = I[2], dd = I[3], ee = I[4], f = I[5], g = I[6], h = I[7], k = I[8];
        const double A00 = ee * k - f * h, A01 = cc * h - b * k, A02 = b * f - cc * ee;     // the adjugate, as in P0
        const double A10 = f * g - dd * k, A11 = a * k - cc * g, A12 = cc * dd - a * f;
        const double A20 = dd * h - ee * g, A21 = b * g - a * h, A22 = a * ee - b * dd;
        const double idet = fast_rcp(a * A00 + b * A10 + cc * A20);
        const double Iinv[9] = {A00 * idet, A01 * idet, A02 * idet, A10 * idet, A11 * idet, A12 * idet,
                                A20 * idet, A21 * idet, A22 * idet};
        double Nm[9];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int l = 0; l < 3; ++l) {
                double t = 0.0;
#pragma unroll
                for (int j = 0; j < 3; ++j) t = fma(GA[(6 + i) * NX + 9 + j], Iinv[3 * l + j], t);
                Nm[3 * i + l] = t;
            }
        if (e < VSMPC_IN_RPY) {
            const int p = (e - VSMPC_IN_INERTIA) / 3, q = (e - VSMPC_IN_INERTIA) - 3 * p;
            double t = 0.0;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const double nq = q == 0 ? Nm[3 * i] : (q == 1 ? Nm[3 * i + 1] : Nm[3 * i + 2]);
                t = fma(s.sA[(6 + i) * NX + 9 + p], nq, t);
            }
            return -t;
        }
        double sr, cr, sp, cp;
        sincos(in[VSMPC_IN_RPY], &sr, &cr);
        sincos(in[VSMPC_IN_RPY + 1], &sp, &cp);
        const double icp = fast_rcp(cp), tp = sp * icp;
        // W^-1 = [1, sr tp, cr tp; 0, cr, -sr; 0, sr / cp, cr / cp]
        if (e == VSMPC_IN_RPY)
            return (cr * tp * Nm[1] - sr * tp * Nm[2]) + (-sr * Nm[4] - cr * Nm[5]) + (cr * icp * Nm[7] - sr * icp * Nm[8]);
        return (sr * Nm[1] + cr * Nm[2]) * (icp * icp) + (sr * Nm[7] + cr * Nm[8]) * (tp * icp);
    }
    if (e >= VSMPC_IN_LANG) { const int f = e - VSMPC_IN_LANG; return GBj[(9 + (f >> 3)) * NJ + (f & 7)]; }
    if (e >= VSMPC_IN_LLIN) { const int f = e - VSMPC_IN_LLIN; return GBj[(3 + (f >> 3)) * NJ + (f & 7)]; }
    if (e >= VSMPC_IN_AMOM) {
        const int f = e - VSMPC_IN_AMOM, r = f >> 2;
        return GA[(r < 3 ? 3 + r : 6 + r) * NX + 12 + (f & 3)];
    }
    // the CoM block and the gravity term (p0_linearize, tid 128): A[i, 3+j] = R_ij / m, c[3+i] = alpha m (R^T g)_i; the two
    // -S(omega) blocks A[3+i, 3+j] and A[9+i, 9+j]
    const double m = in[VSMPC_IN_MASS], alpha = in[VSMPC_IN_ALPHA];
    const double* R = in + VSMPC_IN_WRB;
    const double* gr = in + VSMPC_IN_GRAV;
    if (e >= VSMPC_IN_GRAV) {
        const int l = e - VSMPC_IN_GRAV;
        return alpha * m * (R[3 * l] * Gc[3] + R[3 * l + 1] * Gc[4] + R[3 * l + 2] * Gc[5]);
    }
    if (e >= VSMPC_IN_OMEGA && e < VSMPC_IN_ALPHA) {
        const int w = e - VSMPC_IN_OMEGA, p = (w + 1) % 3, q = (w + 2) % 3;   // -S: entry (p, q) = +omega_w, (q, p) = -omega_w
        return (GA[(3 + p) * NX + 3 + q] + GA[(9 + p) * NX + 9 + q]) - (GA[(3 + q) * NX + 3 + p] + GA[(9 + q) * NX + 9 + p]);
    }
    if (e >= VSMPC_IN_WRB && e < VSMPC_IN_OMEGA) {
        const int i = (e - VSMPC_IN_WRB) / 3, j = (e - VSMPC_IN_WRB) - 3 * i;
        return fma(GA[i * NX + 3 + j], fast_rcp(m), alpha * m * gr[i] * Gc[3 + j]);
    }
    // MASS, ALPHA: sum_i G_c[3+i] (R^T g)_i, and for the mass the CoM block too
    double rg = 0.0;
    for (int i = 0; i < 3; ++i) rg = fma(Gc[3 + i], R[i] * gr[0] + R[3 + i] * gr[1] + R[6 + i] * gr[2], rg);
    if (e == VSMPC_IN_ALPHA) return m * rg;
    double gr_a = 0.0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) gr_a = fma(GA[i * NX + 3 + j], R[3 * i + j], gr_a);
    const double im = fast_rcp(m);
    return fma(alpha, rg, -gr_a * im * im);
}

// Writes grad_in [n_in] and grad_model [1014] of this instance: the gradients when adj_ok, NaN in every entry when the
// cotangent was not finite, zero in every entry when the status is not Solved.  Plain vector stores, every entry once.
template <class Cfg>
VS_DEV void rt_adj_record(const RtCtx& c, const Cfg& cfg, const RtBox box, bool adj_ok, bool nonfinite, const RtAdjRecOut& out) {
    const RtDims& d = c.d;
    const double nan = __builtin_nan("");
    if (out.gin != nullptr) {
        double* g = out.gin + size_t(c.inst) * d.nin;
        for (int e = c.tid; e < d.nin; e += RT_BLOCK) {
            double v = 0.0;
            if (adj_ok) v = nonfinite ? nan : rt_adj_record_entry(c, cfg, box.hold, cfg.use_jet, e);
            g[e] = v;
        }
    }
    if (out.gmodel != nullptr) {
        double* g = out.gmodel + size_t(c.inst) * RT_GMODEL;
        const double* G = rt_adj_g(c);
        for (int e = c.tid; e < RT_GMODEL; e += RT_BLOCK) g[e] = !adj_ok ? 0.0 : (nonfinite ? nan : G[e]);
    }
}

}  // namespace

}  // namespace vsmpc
