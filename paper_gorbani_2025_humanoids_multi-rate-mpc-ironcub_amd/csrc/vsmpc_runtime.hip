// Runtime-sized solve kernel (gfx950): any horizon config_valid() accepts, sized by kernel arguments instead of template
// parameters, so that a configuration outside csrc/vsmpc_horizons.def runs without a rebuild
// (variableSamplingMPC.cpp:24-45 sizes the reference from its XML at run time).
//
// One workgroup of 256 threads per instance computes what solve_kernel computes -- same input record, primal in the
// reference variable order, first-move block, status and active-set iterations -- by the plainest route:
//
//   P0 linearise   p0_linearize (vsmpc_p0.hpp, the tuned kernels' own P0) into LDS
//   P1 condense    full joint blocks, no reduction.  Unknowns: 8 HC joint increments, then the 4 NVB throttles in the
//                  reference order, then the affine column (value 1).  Thread t carries columns t and t + 256: the forward
//                  sensitivity recursion X_{k+1} = X_k + dt_k (A X_k + b_k) with b_k the column's input (Bj e_j / Bt e_t
//                  where the move-blocking maps put it, constraintsVSMPC.cpp:89-128; dt_k c and X_0 = x0 for the affine
//                  column), Y_k = sqrt(Q) (X_k - xref_k) on the 18 weighted rows in LDS, then C += Y_k^T Y_k entry by
//                  entry                                      (constraintsVSMPC.cpp:76-131, costsVSMPC.cpp:166-200)
//   P2 augment     input costs on C, gradient row            (costsVSMPC.cpp:375-409,468-487,558-592)
//   P3 cholesky    right-looking over the joint columns only: the trailing block is then the throttle Schur complement
//                  S and the gradient row holds its reduced gradient s
//   P4 box QP      block principal pivoting on (S, s) with the oracle's rule: every iteration factors S_FF of the free
//                  throttles (compacted into LDS) and solves; iteration 1 holds only the hold pin (constraintsVSMPC.cpp:
//                  338-365)
//   P5 back-subst  joints from L_jj^T u = -(L_vj^T v + l_j)
//   P6 simulate    state trajectory, primal in the reference order, first-move block (variableSamplingMPC.cpp:93-108,
//                  138-151)
//
// Storage: the augmented condensed matrix (NP = NZ + 1 rows) lives in a per-instance global workspace, packed lower
// triangle row by row (element (i, j), j <= i, at i (i + 1) / 2 + j): NP (NP + 1) / 2 doubles, allocated at create.
// LDS holds the record, the linearisation, one stage of Y, the compacted S_FF of the box QP and the vectors.
// No private array is indexed by a runtime value: the two columns of a thread are unrolled at compile time.
#include <atomic>

#include "vsmpc_launch.hpp"
#include "vsmpc_p0.hpp"

namespace vsmpc {

namespace {

constexpr int RT_BLOCK = 256;
constexpr int RT_CPT = 2;                              // columns per thread: NP <= 8 * 40 + 4 * 39 + 1 = 477 < 512
constexpr int RT_LIN = NX * NX + NX * NJ + NX * NTH + 28;   // A | Bj | Bt | c (p0_linearize's contiguous block)
struct RtTag {};                                       // p0_linearize does not use its dimension parameter
constexpr int AS_PATIENCE_RT = 10;                     // the oracle's patience (vsmpc_kernels.hip: AS_PATIENCE)
enum { F_STATUS = 0, F_ITERS, F_NF, F_BEST, F_PATIENCE };   // LDS flag slots

// Entries of A that p0_linearize can make non-zero (vsmpc_p0.hpp; systemDynamicsVSMPC.cpp:79-103,288-319,384-429), by
// row block: the recursion reads only these 142 of the 676 (a dense read keeps A in registers and spills).
constexpr bool a_nz(int r, int q) {
    if (r < 3) return q >= 3 && q < 6;                          // CoM       <- h_lin
    if (r < 6) return (q >= 3 && q < 6) || (q >= 12 && q < 16);  // h_lin     <- h_lin, T
    if (r < 9) return q >= 9 && q < 12;                          // RPY       <- h_ang
    if (r < 12) return q >= 9 && q < 16;                         // h_ang     <- h_ang, T
    if (r < 20) return q >= 12 && q < 20;                        // T, Tdot   <- T, Tdot
    if (r < 23) return q < 3;                                    // e_pos     <- CoM
    return q >= 6 && q < 9;                                      // e_rpy     <- RPY
}

VS_DEV int rt_joint_block(const RtDims& d, int k) { return k < d.hc ? k : d.hc - 1; }
VS_DEV int rt_throttle_block(const RtDims& d, int k) {
    return k < d.ns ? 0 : (k < d.hc ? k - (d.ns - 1) : d.hc - d.ns);
}
VS_DEV size_t tri(int i) { return size_t(i) * size_t(i + 1) / 2; }

// next packed entry (i, j) after advancing the flat index by `step` (j <= i)
VS_DEV void tri_advance(int& i, int& j, int step) {
    j += step;
    while (j > i) { j -= i + 1; ++i; }
}

// LDS carve-up (doubles), in the order of RtDims::lds_doubles()
struct RtSmem {
    double *in, *lin, *vprev, *dt, *sq, *x, *z, *col, *red, *vec0, *vec1, *vec2, *big;
    int *state, *idx, *flags;
};
VS_DEV RtSmem rt_smem(const RtDims& d, double* base) {
    RtSmem s;
    double* p = base;
    s.in = p;    p += (d.nin + 1) & ~1;
    s.lin = p;   p += RT_LIN;
    s.vprev = p; p += 4;
    s.dt = p;    p += MAX_STAGES;
    s.sq = p;    p += NWROWS + 2;
    s.x = p;     p += NX * (d.n + 1);
    s.z = p;     p += (d.nz + 1) & ~1;
    s.col = p;   p += (d.np + 1) & ~1;
    s.red = p;   p += RT_BLOCK;
    s.vec0 = p;  p += (d.nv + 1) & ~1;
    s.vec1 = p;  p += (d.nv + 1) & ~1;
    s.vec2 = p;  p += (d.nv + 1) & ~1;
    s.state = reinterpret_cast<int*>(p); p += (d.nv + 1) / 2 + 1;
    s.idx = reinterpret_cast<int*>(p);   p += (d.nv + 1) / 2 + 1;
    s.flags = reinterpret_cast<int*>(p); p += 4;   // F_* slots
    s.big = p;   // max(18 NP, NV (NV + 1) / 2)
    return s;
}

// symmetric access to the Schur complement S (trailing block of the workspace) by throttle indices
VS_DEV double rt_S(const double* __restrict__ M, int nu, int p, int q) {
    return p >= q ? M[tri(nu + p) + nu + q] : M[tri(nu + q) + nu + p];
}

}  // namespace

__global__ __launch_bounds__(RT_BLOCK) void solve_kernel_rt(DevCfg cfg, RtDims d, const double* __restrict__ in,
                                                            double* __restrict__ ws, double* __restrict__ xout,
                                                            double* __restrict__ fmout, int* __restrict__ status_out,
                                                            int* __restrict__ iters_out) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const RtSmem s = rt_smem(d, smem);
    const int tid = threadIdx.x, inst = blockIdx.x;
    double* __restrict__ M = ws + size_t(inst) * size_t(d.ws_doubles);
    const int NP = d.np, NZ = d.nz, NU = d.nu, NV = d.nv;

    // ---- P0: record, configuration, linearisation
    for (int i = tid; i < d.nin; i += RT_BLOCK) s.in[i] = in[size_t(inst) * d.nin + i];
    if (tid < d.n) s.dt[tid] = cfg.dt[tid];
    if (tid >= 64 && tid < 64 + NWROWS) s.sq[tid - 64] = cfg.sq[tid - 64];
    if (tid == 0) { s.flags[F_STATUS] = VSMPC_STATUS_MAX_ITER; s.flags[F_ITERS] = 0; }
    __syncthreads();
    double* sA = s.lin;
    double* sBj = sA + NX * NX;
    double* sBt = sBj + NX * NJ;
    double* sC = sBt + NX * NTH;
    p0_linearize<RtTag>(cfg.use_jet, s.in, sA, sBj, sBt, sC, s.vprev, tid, RT_BLOCK);

    // ---- P1: sensitivity recursion of every condensed column, C = sum_k Y_k^T Y_k
    {
        double X[RT_CPT][NX];
        const double* src[RT_CPT];
        int stride[RT_CPT], kind[RT_CPT], blk[RT_CPT];   // kind: 0 joint, 1 throttle, 2 affine, 3 none
#pragma unroll
        for (int u = 0; u < RT_CPT; ++u) {
            const int c = tid + u * RT_BLOCK;
            kind[u] = c < NU ? 0 : (c < NZ ? 1 : (c == NZ ? 2 : 3));
            blk[u] = kind[u] == 0 ? c >> 3 : (kind[u] == 1 ? (c - NU) >> 2 : 0);
            src[u] = kind[u] == 0 ? sBj + (c & 7) : (kind[u] == 1 ? sBt + ((c - NU) & 3) : sC);
            stride[u] = kind[u] == 0 ? NJ : (kind[u] == 1 ? NTH : 1);
#pragma unroll
            for (int r = 0; r < NX; ++r) X[u][r] = kind[u] == 2 ? s.in[VSMPC_IN_X0 + r] : 0.0;
        }
        double* Y = s.big;   // Y[w * NP + c]
        for (int k = 0; k < d.n; ++k) {
            const double dt = s.dt[k];
            const int jb = rt_joint_block(d, k), tb = rt_throttle_block(d, k);
            const int i = k + 1;                                        // node of X_{k+1}
            const int col = (i - 1) < d.ns ? 0 : (i - 1) - d.ns;      // reference window column (costsVSMPC.cpp:191-200)
#pragma unroll
            for (int u = 0; u < RT_CPT; ++u) {
                if (kind[u] == 3) continue;
                const bool on = kind[u] == 2 || (kind[u] == 0 && blk[u] == jb) || (kind[u] == 1 && blk[u] == tb);
                double nx[NX];
#pragma unroll
                for (int r = 0; r < NX; ++r) {
                    double a = on ? src[u][r * stride[u]] : 0.0;
#pragma unroll
                    for (int q = 0; q < NX; ++q)
                        if (a_nz(r, q)) a = fma(sA[r * NX + q], X[u][q], a);
                    nx[r] = fma(dt, a, X[u][r]);
                }
#pragma unroll
                for (int r = 0; r < NX; ++r) X[u][r] = nx[r];
                const int c = tid + u * RT_BLOCK;
#pragma unroll
                for (int w = 0; w < NWROWS; ++w) {
                    const int r = wrow(w);
                    const double ref = (kind[u] == 2 && r < 12) ? s.in[VSMPC_IN_XREF + col * 12 + r] : 0.0;
                    Y[w * NP + c] = s.sq[w] * (X[u][r] - ref);
                }
            }
            __syncthreads();
            int ei = 0, ej = 0;
            tri_advance(ei, ej, tid);
            for (size_t e = tid; e < size_t(d.ntri); e += RT_BLOCK) {
                double acc = 0.0;
#pragma unroll
                for (int w = 0; w < NWROWS; ++w) acc = fma(Y[w * NP + ei], Y[w * NP + ej], acc);
                M[e] = k == 0 ? acc : M[e] + acc;
                tri_advance(ei, ej, RT_BLOCK);
            }
            __syncthreads();
        }
    }

    // ---- P2: input costs (every entry touched by exactly one thread), max |gradient| for the release tolerance
    {
        const double w_thr = cfg.w_thr;
        for (int c = tid; c < NZ; c += RT_BLOCK) {
            if (c < NU) {
                const int j = c & 7;
                M[tri(c) + c] += cfg.wj[j];                                   // costsVSMPC.cpp:375-381,564-571
                M[tri(NZ) + c] += cfg.w_reg * s.in[VSMPC_IN_QERR + j];        // :574-589
            } else {
                const int q = c - NU, b = q >> 2, r = q & 3;
                const int npairs = (b < d.nvb - 1 ? 1 : 0) + (b > 0 ? 1 : 0);  // first differences (:383-409)
                double diag = M[tri(c) + c];
                for (int p = 0; p < npairs; ++p) diag += w_thr;
                if (b == 0) diag += cfg.w_init;                                // ThrottleInitialValueCost (:468-487)
                M[tri(c) + c] = diag;
                if (b > 0) M[tri(c) + c - 4] -= w_thr;
                if (b == 0) M[tri(NZ) + c] += -cfg.w_init * s.vprev[r];
            }
        }
        __syncthreads();
        double gm = 0.0;
        for (int c = tid; c < NZ; c += RT_BLOCK) gm = fmax(gm, fabs(M[tri(NZ) + c]));
        s.red[tid] = gm;
        __syncthreads();
        for (int h = RT_BLOCK / 2; h > 0; h >>= 1) {
            if (tid < h) s.red[tid] = fmax(s.red[tid], s.red[tid + h]);
            __syncthreads();
        }
    }
    const double gtol = 1e-10 * (1.0 + s.red[0]);

    // ---- P3: Cholesky of the joint columns; the trailing block becomes (S, s)
    bool bad = false;
    for (int j = 0; j < NU; ++j) {
        const double piv = M[tri(j) + j];
        if (!(piv > 0.0)) { bad = true; break; }   // (every thread reads the same value: a uniform exit)
        const double l = sqrt(piv), il = 1.0 / l;
        for (int i = j + 1 + tid; i < NP; i += RT_BLOCK) {
            const double v = M[tri(i) + j] * il;
            M[tri(i) + j] = v;
            s.col[i] = v;
        }
        __syncthreads();
        if (tid == 0) M[tri(j) + j] = l;           // (after the barrier: every thread has read the pivot)
        const int m = NP - 1 - j;                  // trailing rows / columns j + 1 .. NP - 1
        const size_t nt = size_t(m) * (m + 1) / 2;
        int ei = 0, ej = 0;
        tri_advance(ei, ej, tid);
        for (size_t e = tid; e < nt; e += RT_BLOCK) {
            const int gi = j + 1 + ei, gj = j + 1 + ej;
            M[tri(gi) + gj] -= s.col[gi] * s.col[gj];
            tri_advance(ei, ej, RT_BLOCK);
        }
        __syncthreads();
    }

    // ---- P4: box QP on the throttles, block principal pivoting (executable model: tests/runtime_model.py box_qp)
    const bool hold = s.in[VSMPC_IN_HOLD] != 0.0;
    const double vmin = cfg.vmin, vmax = cfg.vmax;
    double* z = s.z;              // z[0..NU) joints, z[NU..NZ) throttles
    double* zv = z + NU;
    double* sS = M + tri(NZ) + NU;  // reduced gradient s
    if (!bad) {
        for (int p = tid; p < NV; p += RT_BLOCK) s.state[p] = (hold && p < NTH) ? -1 : 0;  // the hold pins v0 at v_prev
        if (tid == 0) { s.flags[F_BEST] = NV + 1; s.flags[F_PATIENCE] = AS_PATIENCE_RT; }
        __syncthreads();
        for (int it = 0; it < cfg.max_as_iter; ++it) {
            // bound values, free list
            for (int p = tid; p < NV; p += RT_BLOCK) {
                const bool fixed = hold && p < NTH;
                const int st = s.state[p];
                if (st != 0) zv[p] = fixed ? s.vprev[p] : (st < 0 ? vmin : vmax);
            }
            if (tid == 0) {
                int nf = 0;
                for (int p = 0; p < NV; ++p)
                    if (s.state[p] == 0) s.idx[nf++] = p;
                s.flags[F_NF] = nf;
            }
            __syncthreads();
            const int nf = s.flags[F_NF];
            double* K = s.big;
            double* rhs = s.vec0;
            double* y = s.vec1;
            // rhs_F = -(s_F + S_FB z_B); K = S_FF (packed lower)
            for (int a = tid; a < nf; a += RT_BLOCK) {
                const int p = s.idx[a];
                double acc = sS[p];
                for (int q = 0; q < NV; ++q)
                    if (s.state[q] != 0) acc = fma(rt_S(M, NU, p, q), zv[q], acc);
                rhs[a] = -acc;
            }
            {
                const size_t nk = size_t(nf) * (nf + 1) / 2;
                int ei = 0, ej = 0;
                tri_advance(ei, ej, tid);
                for (size_t e = tid; e < nk; e += RT_BLOCK) {
                    K[e] = rt_S(M, NU, s.idx[ei], s.idx[ej]);
                    tri_advance(ei, ej, RT_BLOCK);
                }
            }
            __syncthreads();
            // Cholesky of K
            for (int j = 0; j < nf; ++j) {
                const double piv = K[tri(j) + j];
                if (!(piv > 0.0)) { bad = true; break; }
                const double l = sqrt(piv), il = 1.0 / l;
                __syncthreads();   // everyone has read the pivot before it is overwritten
                for (int i = j + 1 + tid; i < nf; i += RT_BLOCK) K[tri(i) + j] *= il;
                if (tid == 0) K[tri(j) + j] = l;
                __syncthreads();
                const int m = nf - 1 - j;
                const size_t nt = size_t(m) * (m + 1) / 2;
                int ei = 0, ej = 0;
                tri_advance(ei, ej, tid);
                for (size_t e = tid; e < nt; e += RT_BLOCK) {
                    const int gi = j + 1 + ei, gj = j + 1 + ej;
                    K[tri(gi) + gj] -= K[tri(gi) + j] * K[tri(gj) + j];
                    tri_advance(ei, ej, RT_BLOCK);
                }
                __syncthreads();
            }
            if (bad) break;
            // L y = rhs, then L^T v = y (v into y)
            for (int j = 0; j < nf; ++j) {
                const double yj = rhs[j] / K[tri(j) + j];
                for (int i = j + 1 + tid; i < nf; i += RT_BLOCK) rhs[i] = fma(-K[tri(i) + j], yj, rhs[i]);
                if (tid == 0) y[j] = yj;
                __syncthreads();
            }
            for (int j = nf - 1; j >= 0; --j) {
                const double vj = y[j] / K[tri(j) + j];
                for (int i = tid; i < j; i += RT_BLOCK) y[i] = fma(-K[tri(j) + i], vj, y[i]);
                __syncthreads();
                if (tid == 0) zv[s.idx[j]] = vj;
            }
            __syncthreads();
            // gradient of the reduced problem at z
            double* grad = s.vec2;
            for (int p = tid; p < NV; p += RT_BLOCK) {
                double acc = sS[p];
                for (int q = 0; q < NV; ++q) acc = fma(rt_S(M, NU, p, q), zv[q], acc);
                grad[p] = acc;
            }
            __syncthreads();
            if (tid == 0) {
                int ninf = 0, last = -1;
                for (int p = 0; p < NV; ++p) {
                    const bool fixed = hold && p < NTH;
                    const int st = s.state[p];
                    const double tol = 1e-12 * (1.0 + fabs(zv[p]));
                    const bool vlo = st == 0 && zv[p] < vmin - tol;
                    const bool vhi = st == 0 && zv[p] > vmax + tol;
                    const bool rel = !fixed && ((st == -1 && grad[p] < -gtol) || (st == 1 && grad[p] > gtol));
                    if (vlo || vhi || rel) { ++ninf; last = p; }
                }
                s.flags[F_ITERS] = it + 1;
                if (ninf == 0) {
                    s.flags[F_STATUS] = VSMPC_STATUS_SOLVED;
                } else {
                    bool all = true;
                    if (ninf < s.flags[F_BEST]) { s.flags[F_BEST] = ninf; s.flags[F_PATIENCE] = AS_PATIENCE_RT; }
                    else if (s.flags[F_PATIENCE] > 0) { --s.flags[F_PATIENCE]; }
                    else all = false;   // single pivot on the largest infeasible index
                    for (int p = 0; p < NV; ++p) {
                        if (!all && p != last) continue;
                        const bool fixed = hold && p < NTH;
                        const int st = s.state[p];
                        const double tol = 1e-12 * (1.0 + fabs(zv[p]));
                        if (st == 0 && zv[p] < vmin - tol) s.state[p] = -1;
                        else if (st == 0 && zv[p] > vmax + tol) s.state[p] = 1;
                        else if (!fixed && ((st == -1 && grad[p] < -gtol) || (st == 1 && grad[p] > gtol))) s.state[p] = 0;
                    }
                }
            }
            __syncthreads();
            if (s.flags[F_STATUS] == VSMPC_STATUS_SOLVED) break;
        }
        __syncthreads();
        // the final point: bound throttles exactly on their bound
        for (int p = tid; p < NV; p += RT_BLOCK) {
            const bool fixed = hold && p < NTH;
            const int st = s.state[p];
            if (st != 0) zv[p] = fixed ? s.vprev[p] : (st < 0 ? vmin : vmax);
        }
        __syncthreads();
    }

    // ---- P5: joints, L_jj^T u = -(L_vj^T v + l_j)
    if (!bad) {
        double* r = s.col;
        for (int j = tid; j < NU; j += RT_BLOCK) {
            double acc = M[tri(NZ) + j];
            for (int p = 0; p < NV; ++p) acc = fma(M[tri(NU + p) + j], zv[p], acc);
            r[j] = -acc;
        }
        __syncthreads();
        for (int j = NU - 1; j >= 0; --j) {
            const double uj = r[j] / M[tri(j) + j];
            for (int i = tid; i < j; i += RT_BLOCK) r[i] = fma(-M[tri(j) + i], uj, r[i]);
            __syncthreads();
            if (tid == 0) z[j] = uj;
        }
        __syncthreads();
    }

    // ---- P6: state trajectory X_{k+1} = X_k + dt_k (A X_k + Bj U_jb + Bt v_tb + c), outputs
    double* sX = s.x;
    if (tid < NX) sX[tid] = s.in[VSMPC_IN_X0 + tid];
    __syncthreads();
    for (int k = 0; k < d.n; ++k) {
        if (tid < NX) {
            const int r = tid;
            const double* U = z + NJ * rt_joint_block(d, k);
            const double* V = zv + NTH * rt_throttle_block(d, k);
            double a = sC[r];
            for (int q = 0; q < NJ; ++q) a = fma(sBj[r * NJ + q], U[q], a);
            for (int q = 0; q < NTH; ++q) a = fma(sBt[r * NTH + q], V[q], a);
            for (int q = 0; q < NX; ++q) a = fma(sA[r * NX + q], sX[k * NX + q], a);
            sX[(k + 1) * NX + r] = fma(s.dt[k], a, sX[k * NX + r]);
        }
        __syncthreads();
    }
    const int iters = s.flags[F_ITERS];
    const int status = bad ? VSMPC_STATUS_NUMERICAL : s.flags[F_STATUS];
    if (xout != nullptr) {
        double* xo = xout + size_t(inst) * d.nvar;
        for (int i = tid; i < d.nxs; i += RT_BLOCK) xo[i] = sX[i];
        for (int i = tid; i < NZ; i += RT_BLOCK) xo[d.nxs + i] = bad ? 0.0 : z[i];
    }
    if (fmout != nullptr && tid < VSMPC_FM_SIZE) {
        double v;
        if (tid < 8) v = z[tid];                                      // delta q           (variableSamplingMPC.cpp:99)
        else if (tid < 12) v = zv[tid - 8];                           // v0                (:100)
        else if (tid < 16) v = Jet::throttle_of_v(zv[tid - 12]);      // throttle %        (:146-149)
        else if (tid < 20) v = sX[NX + 12 + (tid - 16)];              // thrust, node 1    (:101)
        else v = sX[NX + 16 + (tid - 20)];                            // thrust rate, node 1 (:102)
        fmout[size_t(inst) * VSMPC_FM_SIZE + tid] = v;
    }
    if (tid == 0) {
        status_out[inst] = status;
        if (iters_out != nullptr) iters_out[inst] = bad ? 0 : iters;
    }
}

__global__ __launch_bounds__(256) void linearize_kernel_rt(DevCfg cfg, int n_in, const double* __restrict__ in,
                                                           double* __restrict__ A, double* __restrict__ Bj,
                                                           double* __restrict__ Bt, double* __restrict__ c) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    double* sIn = smem;
    double* sA = sIn + ((n_in + 1) & ~1);
    double* sBj = sA + NX * NX;
    double* sBt = sBj + NX * NJ;
    double* sC = sBt + NX * NTH;
    double* sVprev = sC + 28;
    const int tid = threadIdx.x, b = blockIdx.x;
    for (int i = tid; i < n_in; i += 256) sIn[i] = in[size_t(b) * n_in + i];
    __syncthreads();
    p0_linearize<RtTag>(cfg.use_jet, sIn, sA, sBj, sBt, sC, sVprev, tid, 256);
    for (int i = tid; i < NX * NX; i += 256) A[size_t(b) * NX * NX + i] = sA[i];
    for (int i = tid; i < NX * NJ; i += 256) Bj[size_t(b) * NX * NJ + i] = sBj[i];
    for (int i = tid; i < NX * NTH; i += 256) Bt[size_t(b) * NX * NTH + i] = sBt[i];
    for (int i = tid; i < NX; i += 256) c[size_t(b) * NX + i] = sC[i];
}

RtDims runtime_dims(int n_iter, int n_iter_small, int control_horizon) {
    RtDims d{};
    d.n = n_iter;
    d.ns = n_iter_small;
    d.hc = control_horizon;
    d.nvb = d.hc - d.ns + 1;
    d.nu = NJ * d.hc;
    d.nv = NTH * d.nvb;
    d.nz = d.nu + d.nv;
    d.np = d.nz + 1;
    d.nin = VSMPC_IN_XREF + 12 * (d.n - d.ns + 1);
    d.nxs = NX * (d.n + 1);
    d.nvar = d.nxs + d.nz;
    d.ntri = int(size_t(d.np) * (d.np + 1) / 2);
    d.ws_doubles = d.ntri;
    const int fixed = ((d.nin + 1) & ~1) + RT_LIN + 4 + MAX_STAGES + NWROWS + 2 + NX * (d.n + 1) + ((d.nz + 1) & ~1) +
                      ((d.np + 1) & ~1) + RT_BLOCK + 3 * ((d.nv + 1) & ~1) + 2 * ((d.nv + 1) / 2 + 1) + 4;
    const int ybuf = NWROWS * d.np, kbuf = d.nv * (d.nv + 1) / 2;
    d.lds_doubles = fixed + (ybuf > kbuf ? ybuf : kbuf);
    return d;
}

size_t runtime_lds_bytes(const RtDims& d) { return size_t(d.lds_doubles) * sizeof(double); }

hipError_t launch_solve_runtime(const RtDims& d, const DevCfg& cfg, const double* d_in, int batch, double* d_ws, double* d_x,
                                double* d_fm, int* d_status, int* d_iters, hipStream_t stream) {
    constexpr int MAX_DEV = 64;
    static std::atomic<bool> attr_set[MAX_DEV];
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= MAX_DEV) return hipErrorInvalidDevice;
    const size_t lds = runtime_lds_bytes(d);
    if (lds > RT_MAX_LDS) return hipErrorInvalidValue;
    if (!attr_set[dev].load(std::memory_order_acquire)) {   // the largest size once: every horizon launches under it
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(&solve_kernel_rt), hipFuncAttributeMaxDynamicSharedMemorySize,
                                int(RT_MAX_LDS));
        if (e != hipSuccess) return e;
        attr_set[dev].store(true, std::memory_order_release);
    }
    hipLaunchKernelGGL(solve_kernel_rt, dim3(batch), dim3(RT_BLOCK), lds, stream, cfg, d, d_in, d_ws, d_x, d_fm, d_status,
                       d_iters);
    return hipGetLastError();
}

hipError_t launch_linearize_runtime(const RtDims& d, const DevCfg& cfg, const double* d_in, int batch, double* A, double* Bj,
                                    double* Bt, double* c, hipStream_t stream) {
    const size_t lds = size_t(((d.nin + 1) & ~1) + RT_LIN + 4) * sizeof(double);
    hipLaunchKernelGGL(linearize_kernel_rt, dim3(batch), dim3(256), lds, stream, cfg, d.nin, d_in, A, Bj, Bt, c);
    return hipGetLastError();
}

const char* runtime_kernel_name() { return "solve_kernel_rt"; }

}  // namespace vsmpc
