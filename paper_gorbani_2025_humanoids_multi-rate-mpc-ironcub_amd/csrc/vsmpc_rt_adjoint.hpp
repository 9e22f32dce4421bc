// The adjoint entry of the runtime-sized kernels: what adjoint_kernel_rt[_tuned] add to the solve (included by
// vsmpc_runtime.hip after vsmpc_rt_core.hpp).
//
// adjoint_kernel_rt / adjoint_kernel_rt_tuned (vsmpc_adjoint_batch) are rt_solve<RT_ADJOINT>: P0 .. P6 and rt_write_solution
// exactly as in solve_kernel_rt, then, on a Solved exit, five phases that turn a cotangent xbar = dL/dx (and fmbar = dL/d
// first_move, folded into xbar) into dL/dX0 and dL/d(weights, throttle box) with one more solve against the factor the
// solver holds ("Adjoint"; executable model: tests/adjoint_model.py condensed_adjoint).  With K [a; b] = [xbar; 0]
// the KKT system of the final active set:
//   rt_adj_rhs           r = Z^T xbar by the costate form: lambda_N = xbar_XN, lambda_k = xbar_Xk + (I + dt_k A)^T lambda_{k+1},
//                        r_U[j] = xbar_U[j] + sum_{jb(k) = j} dt_k Bj^T lambda_{k+1}, r_V likewise with Bt
//   rt_adj_solve         w = L_jj^-1 r_U, t = r_V - L_vj w, S_FF dv_F = t_F (dv = 0 on bound and pinned throttles),
//                        L_jj^T du = w - L_vj^T dv: a_U = du, a_V = dv
//   rt_adj_states        a_X0 = 0, a_X{k+1} = a_Xk + dt_k (A a_Xk + Bj a_U[jb(k)] + Bt a_V[tb(k)])
//   rt_adj_costates      b_{N-1} = Q a_XN - xbar_XN, b_{i-1} = Q a_Xi - xbar_Xi + (I + dt_i A)^T b_i,
//                        b_init = xbar_X0 - (I + dt_0 A)^T b_0, b_t = xbar_Vt - (H a)_Vt - sum_{tb(i) = t} dt_i Bt^T b_i
//   rt_adj_reduce_write  dL/dX0 = b_init, dL/dvmin|vmax = sum of b_t over the lower | upper active non-pinned throttles,
//                        dL/dw = -a^T (dH/dw x + dg/dw) for every weight: 31 sums in a fixed order
#pragma once
#include "vsmpc_rt_core.hpp"

namespace vsmpc {

namespace {

// ---- the adjoint entry (rt_solve<RT_ADJOINT>): inputs and outputs, per batch; every output may be null
struct RtAdjIO {
    const double* xbar = nullptr;    // [nVar] per instance: dL/dx, reference variable order
    const double* fmbar = nullptr;   // [24] per instance or null: dL/d first_move
    double* gx0 = nullptr;           // [26]: dL/dX0
    double* gcfg = nullptr;          // [VSMPC_GRAD_SIZE]: dL/d(weights, throttle limits in percent), VSMPC_GRAD_* order
    int* active = nullptr;           // [NV]
    int* flags = nullptr;            // VSMPC_ADJ_*
};

// The cotangent of one instance with the first-move cotangent folded in (read from global memory where it is used): joint
// increments onto U_0, v0 and throttle percent (through d throttle / d v at the solution) onto V_0, thrust and thrust rate
// onto rows 12..19 of X_1.
struct RtAdjIn {
    const double* xb;    // this instance's xbar
    const double* fm;    // this instance's fmbar or null
    const double* zv;    // the throttles of the solution (LDS)
    int nxs, nu;
    VS_DEV double x(int node, int r) const {
        double v = xb[node * NX + r];
        if (fm != nullptr && node == 1 && r >= 12 && r < 20) v += fm[VSMPC_FM_THRUST + r - 12];
        return v;
    }
    VS_DEV double u(int e) const {
        double v = xb[nxs + e];
        if (fm != nullptr && e < NJ) v += fm[VSMPC_FM_DQ + e];
        return v;
    }
    VS_DEV double v(int e) const {
        double v = xb[nxs + nu + e];
        if (fm != nullptr && e < NTH) v += fm[VSMPC_FM_V0 + e] + Jet::dthrottle_dv(zv[e]) * fm[VSMPC_FM_THROTTLE + e];
        return v;
    }
};
VS_DEV RtAdjIn rt_adj_in(const RtCtx& c, const RtAdjIO& io) {
    return RtAdjIn{io.xbar + size_t(c.inst) * c.d.nvar,
                   io.fmbar != nullptr ? io.fmbar + size_t(c.inst) * VSMPC_FM_SIZE : nullptr, c.zv(), c.d.nxs, c.d.nu};
}

// ---- adjoint 1: right-hand side r = Z^T xbar in s.col[0 .. NZ), joints then throttles
// Reads xbar / fmbar (global), the linearisation, s.dt and zv.  Leaves r in s.col (free since P5).  Uses s.red for lambda_k |
// lambda_{k+1} and the wavefronts' non-finite flags.  Returns whether xbar or fmbar holds a non-finite entry (the same value in every thread).
VS_DEV bool rt_adj_rhs(const RtCtx& c, const RtAdjIn& a) {
    const RtSmem s = c.lds();
    const RtDims& d = c.d;
    const int tid = c.tid, N = d.n, NU = d.nu, NZ = d.nz;
    double* r = s.col;
    double* lam = s.red;   // lambda_k at lam + (k & 1) * NX
    int bad = 0;
    for (int e = tid; e < d.nvar; e += RT_BLOCK) bad |= isfinite(a.xb[e]) ? 0 : 1;
    if (a.fm != nullptr && tid < VSMPC_FM_SIZE) bad |= isfinite(a.fm[tid]) ? 0 : 1;
    for (int e = tid; e < NZ; e += RT_BLOCK) r[e] = e < NU ? a.u(e) : a.v(e - NU);
    if (tid < NX) lam[(N & 1) * NX + tid] = a.x(N, tid);
    const bool wave_bad = __any(bad) != 0;   // the flag of the wavefront, then of the workgroup through s.red behind lambda
    if ((tid & 63) == 0) lam[2 * NX + (tid >> 6)] = wave_bad ? 1.0 : 0.0;
    __syncthreads();
    const bool nonfinite = fmax(fmax(lam[2 * NX], lam[2 * NX + 1]), fmax(lam[2 * NX + 2], lam[2 * NX + 3])) != 0.0;
    for (int k = N - 1; k >= 0; --k) {
        const double* cur = lam + ((k + 1) & 1) * NX;   // lambda_{k+1}
        double* nxt = lam + (k & 1) * NX;
        const double dt = s.dt[k];
        if (tid < NX) {
            if (k > 0) {
                double acc = 0.0;
                for (int q = 0; q < NX; ++q) acc = fma(s.sA[q * NX + tid], cur[q], acc);
                nxt[tid] = a.x(k, tid) + fma(dt, acc, cur[tid]);
            }
        } else if (tid >= 64 && tid < 64 + NJ) {
            const int j = tid - 64;
            double acc = 0.0;
            for (int q = 0; q < NX; ++q) acc = fma(s.sBj[q * NJ + j], cur[q], acc);
            double* e = r + NJ * joint_block(d, k) + j;
            *e = fma(dt, acc, *e);
        } else if (tid >= 128 && tid < 128 + NTH) {
            const int t = tid - 128;
            double acc = 0.0;
            for (int q = 0; q < NX; ++q) acc = fma(s.sBt[q * NTH + t], cur[q], acc);
            double* e = r + NU + NTH * throttle_block(d, k) + t;
            *e = fma(dt, acc, *e);
        }
        __syncthreads();
    }
    return nonfinite;
}

// ---- adjoint 2: [C_jj C_jF; C_Fj C_FF] [du; dv_F] = [r_U; r_F] with the factors of P3 and of the box QP's last iteration
// Reads r in s.col, L (joint columns of M, all rows), the factor of S_FF in K = s.big with its free list s.idx / F_NF.
// Leaves a_z = [du | dv] in s.col[0 .. NZ), dv = 0 on bound and pinned throttles.  Uses s.vec0, s.vec1.  K is dead afterwards.
VS_DEV void rt_adj_solve(const RtCtx& c) {
    const RtSmem s = c.lds();
    const int tid = c.tid, NU = c.d.nu, NV = c.d.nv, NZ = c.d.nz;
    const double* M = c.M;
    double* r = s.col;
    // forward through the joint columns, over the throttle rows too: r_V becomes t = r_V - L_vj w.  Entry j keeps w_j L_jj
    // (the division is repeated where w_j is read), so that no thread writes what another one reads in the same step: NZ
    // rows under NU columns and nothing stored per column, which is why this is not rt_solve_forward.
    for (int j = 0; j < NU; ++j) {
        const double wj = r[j] / M[tri(j) + j];
        for (int i = j + 1 + tid; i < NZ; i += RT_BLOCK) r[i] = fma(-M[tri(i) + j], wj, r[i]);
        __syncthreads();
    }
    // S_FF dv_F = t_F
    const int nf = s.flags[F_NF];
    const double* K = s.big;
    double* rhs = s.vec0;
    double* y = s.vec1;
    for (int a = tid; a < nf; a += RT_BLOCK) rhs[a] = r[NU + s.idx[a]];
    __syncthreads();
    for (int p = tid; p < NV; p += RT_BLOCK) r[NU + p] = 0.0;
    rt_solve_forward(tid, K, nf, rhs, y);
    rt_solve_backward(tid, K, nf, y, r + NU, RtAtFree{s.idx});
    // L_jj^T du = w - L_vj^T dv
    for (int j = tid; j < NU; j += RT_BLOCK) {
        double acc = r[j] / M[tri(j) + j];
        for (int p = 0; p < NV; ++p) acc = fma(-M[tri(NU + p) + j], r[NU + p], acc);
        r[j] = acc;
    }
    __syncthreads();
    rt_solve_backward(tid, M, NU, r, r, RtAtSelf{});   // (in place)
}

// the adjoint's carve-up of s.big (the factor of S_FF is dead): a_X [N + 1][26] | b_0 .. b_{N-1}, b_init [N + 1][26]
VS_HD int rt_big_adjoint(const RtDims& d) { return 2 * NX * (d.n + 1); }
VS_DEV double* rt_adj_ax(const RtCtx& c) { return c.lds().big; }
VS_DEV double* rt_adj_b(const RtCtx& c) { return c.lds().big + NX * (c.d.n + 1); }

// ---- adjoint 3: state part of a: a_X0 = 0, a_X{k+1} = a_Xk + dt_k (A a_Xk + Bj a_U[jb(k)] + Bt a_V[tb(k)])
// Reads a_z in s.col, the linearisation, s.dt.  Leaves a_X in s.big.
VS_DEV void rt_adj_states(const RtCtx& c) {
    double* aX = rt_adj_ax(c);
    if (c.tid < NX) aX[c.tid] = 0.0;
    rt_recur_states<false>(c, aX, c.lds().col);
}

// ---- adjoint 4: costates b (the multipliers of K [a; b] = [xbar; 0]): certify_kernel's recursion with Q a_Xi - xbar_Xi
// Reads a_X, a_z, xbar, the linearisation, s.dt, cfg.sq, cfg.w_thr, cfg.w_init.  Leaves b_i and b_init in s.big behind a_X
// and the throttle rows' b_t (every throttle; only the active ones mean anything) in s.vec0.
template <class Cfg>
VS_DEV void rt_adj_costates(const RtCtx& c, const Cfg& cfg, const RtAdjIn& a) {
    const RtSmem s = c.lds();
    const RtDims& d = c.d;
    const int tid = c.tid, N = d.n, NV = d.nv;
    const double* aX = rt_adj_ax(c);
    double* b = rt_adj_b(c);
    const double qd = tid < NX ? q_diag(cfg.sq, tid) : 0.0;
    if (tid < NX) b[(N - 1) * NX + tid] = qd * aX[N * NX + tid] - a.x(N, tid);
    __syncthreads();
    for (int i = N - 1; i >= 0; --i) {
        if (tid < NX) {
            const double* bi = b + i * NX;
            double acc = 0.0;
            for (int q = 0; q < NX; ++q) acc = fma(s.sA[q * NX + tid], bi[q], acc);
            const double prop = fma(s.dt[i], acc, bi[tid]);                       // ((I + dt_i A)^T b_i)
            if (i > 0) b[(i - 1) * NX + tid] = (qd * aX[i * NX + tid] - a.x(i, tid)) + prop;
            else b[N * NX + tid] = a.x(0, tid) - prop;                            // b_init
        }
        __syncthreads();
    }
    const double* aV = s.col + d.nu;
    const double w_thr = cfg.w_thr, w_init = cfg.w_init;
    for (int f = tid; f < NV; f += RT_BLOCK) {
        const int t = f >> 2, k = f & 3;
        double sum = 0.0;
        for (int i = 0; i < N; ++i) {
            if (throttle_block(d, i) != t) continue;
            const double* bi = b + i * NX;
            double acc = 0.0;
            for (int q = 0; q < NX; ++q) acc = fma(s.sBt[q * NTH + k], bi[q], acc);
            sum = fma(s.dt[i], acc, sum);
        }
        const double v = aV[f];
        const double vm = aV[t > 0 ? f - NTH : f], vp = aV[t < d.nvb - 1 ? f + NTH : f];   // neighbours (or v: difference 0)
        const double hx = fma(w_thr, (v - vm) + (v - vp), t == 0 ? w_init * v : 0.0);
        s.vec0[f] = (a.v(f) - hx) - sum;
    }
    __syncthreads();
}

// ---- adjoint 5: the 31 contractions and the outputs
// Reads a_X, b (s.big), a_z (s.col), b_t (s.vec0), the solution (s.x, s.z), s.in (reference window, q_err), s.vprev,
// s.state, the reduced gradients (row NZ of M, s.vec2) for the degeneracy flag.  Every sum: per-lane partial over the items
// e = tid, tid + 256, .., a butterfly inside the wavefront, the four partials in wavefront order through s.red -- an order
// the sizes alone fix.  Writes dL/dX0, dL/dcfg (all zero unless adj_ok, all NaN with a non-finite cotangent; entry 31 is 0),
// the active set and the VSMPC_ADJ_* flags.  The active-set output and the degeneracy rule are rt_write_active and rt_degenerate
// (vsmpc_rt_core.hpp) written out: called here, with their loops kept from unrolling, they made adjoint_kernel_rt 0.5 % (batch
// 256) to 1.0 % (batch 4096) slower, outside the parent's spread (profiles/runtime_shared_bench.txt).
template <class Cfg>
VS_DEV void rt_adj_reduce_write(const RtCtx& c, const Cfg& cfg, const RtBox box, bool factored, bool adj_ok, bool nonfinite,
                                const RtAdjIO& out) {
    const RtDims& d = c.d;
    const RtSmem s = c.lds();
    const int tid = c.tid, inst = c.inst, N = d.n, NU = d.nu, NV = d.nv;
    const bool hold = box.hold;
    const double vmin = box.vmin, vmax = box.vmax;
    if (adj_ok) {
        const double* aX = rt_adj_ax(c);
        const double* aU = s.col;
        const double* aV = s.col + NU;
        const double* U = s.z;
        const double* V = s.z + NU;
        for (int g = 0; g < VSMPC_GRAD_THROTTLE_MAX + 1; ++g) {
            double acc = 0.0;
            if (g < VSMPC_GRAD_W_DELTA_JOINT) {
                // state weights in the order of the vsmpc_config fields: w_com_pos, w_com_pos_err, w_lin_mom, w_rpy,
                // w_rpy_err, w_ang_mom -> state rows 0, 20, 3, 6, 23, 9
                const int f = g / 3, r = (f == 0 ? 0 : f == 1 ? 20 : f == 2 ? 3 : f == 3 ? 6 : f == 4 ? 23 : 9) + g % 3;
                for (int e = tid; e < N; e += RT_BLOCK) {
                    const int i = e + 1;
                    const int col = (i - 1) < d.ns ? 0 : (i - 1) - d.ns;
                    const double ref = r < 12 ? s.in[VSMPC_IN_XREF + col * 12 + r] : 0.0;
                    acc = fma(-aX[i * NX + r], s.x[i * NX + r] - ref, acc);
                }
            } else if (g < VSMPC_GRAD_W_THROTTLE) {
                const int j = g - VSMPC_GRAD_W_DELTA_JOINT;
                for (int e = tid; e < d.hc; e += RT_BLOCK) acc = fma(-aU[e * NJ + j], U[e * NJ + j], acc);
            } else if (g == VSMPC_GRAD_W_THROTTLE) {
                for (int e = tid; e < NV - NTH; e += RT_BLOCK) acc = fma(-(aV[e] - aV[e + NTH]), V[e] - V[e + NTH], acc);
            } else if (g == VSMPC_GRAD_W_INITIAL_THROTTLE) {
                for (int e = tid; e < NTH; e += RT_BLOCK) acc = fma(-aV[e], V[e] - s.vprev[e], acc);
            } else if (g == VSMPC_GRAD_W_REG_JOINT_POS) {
                for (int e = tid; e < NU; e += RT_BLOCK) acc = fma(-aU[e], U[e] + s.in[VSMPC_IN_QERR + (e & 7)], acc);
            } else {
                const int want = g == VSMPC_GRAD_THROTTLE_MIN ? -1 : 1;
                for (int e = tid; e < NV; e += RT_BLOCK)
                    if (s.state[e] == want && !(hold && e < NTH)) acc += s.vec0[e];
            }
            acc = wave_sum(acc);
            if ((tid & 63) == 0) s.red[g * RT_NWAVES + (tid >> 6)] = acc;
        }
    }
    __syncthreads();
    if (out.gcfg != nullptr && tid < VSMPC_GRAD_SIZE) {
        double v = 0.0;
        if (adj_ok && tid <= VSMPC_GRAD_THROTTLE_MAX) {
            const double* p = s.red + tid * RT_NWAVES;
            v = ((p[0] + p[1]) + p[2]) + p[3];
            // percent, not warped throttle: d v_of_throttle / du at the limit = sqrt(1 + 4 c12 v) / sigma_U
            if (tid == VSMPC_GRAD_THROTTLE_MIN) v *= sqrt(1.0 + 4.0 * Jet::c12 * vmin) * Jet::isgU;
            if (tid == VSMPC_GRAD_THROTTLE_MAX) v *= sqrt(1.0 + 4.0 * Jet::c12 * vmax) * Jet::isgU;
            if (nonfinite) v = __builtin_nan("");
        }
        out.gcfg[size_t(inst) * VSMPC_GRAD_SIZE + tid] = v;
    }
    if (out.gx0 != nullptr && tid >= 64 && tid < 64 + NX) {
        const int q = tid - 64;
        double v = adj_ok ? rt_adj_b(c)[N * NX + q] : 0.0;
        if (adj_ok && nonfinite) v = __builtin_nan("");
        out.gx0[size_t(inst) * NX + q] = v;
    }
    if (out.active != nullptr)
        for (int p = tid; p < NV; p += RT_BLOCK)
            out.active[size_t(inst) * NV + p] = !factored ? 0 : ((hold && p < NTH) ? 2 : s.state[p]);
    if (tid == 0 && out.flags != nullptr) {
        int fl = VSMPC_ADJ_UNSOLVED;
        if (adj_ok) {   // weakly or nearly active non-pinned throttles: the gradient is one-sided there
            fl = 0;
            const double* sS = c.sS();
            const double* zv = c.zv();
            double smax = 0.0;
            for (int p = 0; p < NV; ++p) smax = fmax(smax, fabs(sS[p]));
            const double gt = VSMPC_SENS_GRAD_TOL * (1.0 + smax);
            for (int p = 0; p < NV; ++p) {
                if (hold && p < NTH) continue;
                const int st = s.state[p];
                const double v = zv[p], bt = VSMPC_SENS_BOUND_TOL * (1.0 + fabs(v));
                if ((st != 0 && fabs(s.vec2[p]) <= gt) || (st == 0 && (v - vmin <= bt || vmax - v <= bt)))
                    fl |= VSMPC_ADJ_DEGENERATE;
            }
        }
        out.flags[inst] = fl;
    }
}

}  // namespace

}  // namespace vsmpc
