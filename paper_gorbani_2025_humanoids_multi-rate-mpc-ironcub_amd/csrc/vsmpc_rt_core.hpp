// Runtime-sized solve kernels, the part every entry shares: constants, the LDS carve-up, the context, the substitution
// helpers, the phases P0 .. P6 of the solve and its outputs (included by vsmpc_runtime.hip alone, which has the overview).
//
// One workgroup of 256 threads per instance.  The solve is a list of phase functions over one context (RtCtx: sizes, LDS
// carve-up, the instance's workspace, the linearisation); rt_solve (vsmpc_runtime.hip) calls them in order, and each states
// above its definition what it reads and what it leaves behind:
//
//   P0 rt_load_and_linearize    record and configuration into LDS, p0_linearize (vsmpc_p0.hpp, the tuned kernels' own P0)
//   P1 rt_condense              full joint blocks, no reduction.  Unknowns: 8 HC joint increments, then the 4 NVB throttles
//                  in the reference order, then the affine column (value 1).  Thread t carries columns t and t + 256: the
//                  forward sensitivity recursion X_{k+1} = X_k + dt_k (A X_k + b_k) with b_k the column's input (Bj e_j /
//                  Bt e_t where the move-blocking maps put it, constraintsVSMPC.cpp:89-128; dt_k c and X_0 = x0 for the
//                  affine column), Y_k = sqrt(Q) (X_k - xref_k) on the 18 weighted rows in LDS, then C += Y_k^T Y_k entry
//                  by entry                                   (constraintsVSMPC.cpp:76-131, costsVSMPC.cpp:166-200)
//   P2 rt_input_costs           input costs on C, gradient row    (costsVSMPC.cpp:375-409,468-487,558-592)
//   P3 rt_factor_joint_columns  right-looking Cholesky over the joint columns only: the trailing block is then the
//                  throttle Schur complement S and the gradient row holds its reduced gradient s
//   P4 rt_box_qp                block principal pivoting on (S, s) with the oracle's rule: every iteration factors S_FF of
//                  the free throttles (compacted into LDS) and solves; iteration 1 holds only the hold pin
//                  (constraintsVSMPC.cpp:338-365)
//   P5 rt_joints                joints from L_jj^T u = -(L_vj^T v + l_j)
//   P6 rt_simulate              state trajectory                  (variableSamplingMPC.cpp:93-108)
//      rt_write_solution        primal in the reference order, first-move block, status, iterations (:138-151)
//
// Storage: the augmented condensed matrix (NP = NZ + 1 rows) lives in a per-instance global workspace, packed lower
// triangle row by row (element (i, j), j <= i, at i (i + 1) / 2 + j): NP (NP + 1) / 2 doubles, allocated at create.
// LDS holds the record, the linearisation, one stage of Y, the compacted S_FF of the box QP and the vectors.
// No private array is indexed by a runtime value: the two columns of a thread are unrolled at compile time.
#pragma once
#include <cstddef>

#include "vsmpc_launch.hpp"
#include "vsmpc_p0.hpp"
#include "vsmpc_structure.hpp"

namespace vsmpc {

namespace {

constexpr int RT_BLOCK = 256;
constexpr int RT_CPT = 2;    // columns per thread: NP <= 8 * 40 + 4 * 39 + 1 = 477 (+ 26 parameter columns: 503) < 512
constexpr int RT_NPAR = NX;  // parameter columns of sens_kernel_rt: one per entry of X0
constexpr int RT_NWAVES = RT_BLOCK / 64;
enum { F_STATUS = 0, F_ITERS, F_NF, F_BEST, F_PATIENCE };   // LDS flag slots

VS_DEV size_t tri(int i) { return size_t(i) * size_t(i + 1) / 2; }

// next packed entry (i, j) after advancing the flat index by `step` (j <= i)
VS_DEV void tri_advance(int& i, int& j, int step) {
    j += step;
    while (j > i) { j -= i + 1; ++i; }
}

// LDS carve-up (doubles), stated once as a walk over P: over double* in the kernels (rt_smem), and over size_t from 0 on the
// host, where runtime_dims takes the size of the fixed part -- everything in front of `big` -- from it.  `big` is shared by
// whoever needs it at the time; its sizes stand beside their users (rt_big_condense, rt_big_box_qp, RT_BIG_SENS, rt_big_adjoint,
// rt_big_adjoint_record).
template <class P>
struct RtCarve {
    P in, lin, vprev, dt, sq, x, z, col, red, vec0, vec1, vec2, big;
    P i_state, i_idx, i_flags;   // arrays of int, two to a double
};
template <class P>
VS_HD RtCarve<P> rt_carve(const RtDims& d, P p) {
    RtCarve<P> s;
    s.in = p;    p += (d.nin + 1) & ~1;
    s.lin = p;   p += LIN_DOUBLES;
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
    s.i_state = p; p += (d.nv + 1) / 2 + 1;
    s.i_idx = p;   p += (d.nv + 1) / 2 + 1;
    s.i_flags = p; p += 4;   // F_* slots
    s.big = p;
    return s;
}
struct RtSmem : RtCarve<double*> {
    double *sA, *sBj, *sBt, *sC;   // A | Bj | Bt | c: p0_linearize's block, in lin
    int *state, *idx, *flags;      // i_state, i_idx, i_flags as what they hold
};
VS_DEV RtSmem rt_smem(const RtDims& d, double* base) {
    const RtCarve<double*> c = rt_carve(d, base);
    RtSmem s;
    static_cast<RtCarve<double*>&>(s) = c;
    s.sA = s.lin;
    s.sBj = s.sA + NX * NX;
    s.sBt = s.sBj + NX * NJ;
    s.sC = s.sBt + NX * NTH;
    s.state = reinterpret_cast<int*>(c.i_state);
    s.idx = reinterpret_cast<int*>(c.i_idx);
    s.flags = reinterpret_cast<int*>(c.i_flags);
    return s;
}

// Every phase forms the carve-up itself, from the LDS base, instead of being handed the pointers (the same addresses, and
// after inlining the same values): only with the pointers' origin in sight inside the phase function does the compiler
// form addresses and unroll loops as it did for the one body these functions replace.  Handed in through the context,
// P1 alone cost 15 spilled VGPRs.
VS_DEV RtSmem rt_lds(const RtDims& d) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    return rt_smem(d, smem);
}

// What every phase works on: the sizes, the instance's workspace M (the packed matrix; its row NZ is the gradient row, rows
// NZ + 1 + j the parameter rows of sens_kernel_rt) and, through lds(), the LDS carve-up: s.in the record, (sA, sBj, sBt,
// sC) the linearisation, s.z the solution z = [joints | throttles], s.state / s.idx / s.flags the box QP's active set, free
// list and F_* slots.
struct RtCtx {
    const RtDims& d;
    double* M;
    int tid, inst;
    VS_DEV RtSmem lds() const { return rt_lds(d); }
    VS_DEV double* zv() const { return lds().z + d.nu; }                  // throttles of z
    VS_DEV double* sS() const { return M + tri(d.nz) + d.nu; }            // reduced gradient s (after P3)
    VS_DEV double* prow(int j) const { return M + tri(d.nz + 1 + j); }    // parameter row j
    // symmetric access to the Schur complement S (trailing block of the workspace) by throttle indices
    VS_DEV double S(int p, int q) const { return p >= q ? M[tri(d.nu + p) + d.nu + q] : M[tri(d.nu + q) + d.nu + p]; }
};

// the throttle box of this instance: the hold pins block 0 at v_prev whatever the limits are (constraintsVSMPC.cpp:351)
struct RtBox {
    bool hold;
    double vmin, vmax;
    VS_DEV bool pinned(int p) const { return hold && p < NTH; }
};

// Puts every throttle that is not free on its value: v_prev where pinned, else its bound.
// Reads s.state, s.vprev; writes the non-free entries of zv.  No barrier.
VS_DEV void rt_bound_values(const RtCtx& c, const RtBox box) {
    const RtSmem s = c.lds();
    double* zv = c.zv();
    for (int p = c.tid; p < c.d.nv; p += RT_BLOCK) {
        const bool fixed = box.pinned(p);
        const int st = s.state[p];
        if (st != 0) zv[p] = fixed ? s.vprev[p] : (st < 0 ? box.vmin : box.vmax);
    }
}

// 26 right-hand sides against a packed lower factor L of order n, in place in the parameter rows: right-hand side j's
// entry i lies at prow(j)[off + at(i)], with `at` one of the two maps below.  Forward: L y = rhs.  Backward: L^T x = y.
// Reads L (LDS or workspace); barriers after every scaling and every update.
struct RtAtSelf { VS_DEV int operator()(int a) const { return a; } };                       // the joints: entry a itself
struct RtAtFree { const int* idx; VS_DEV int operator()(int a) const { return idx[a]; } };   // the a-th free throttle
template <class At>
VS_DEV void rt_sweep_forward(const RtCtx& c, const double* L, int n, int off, At at) {
    for (int a = 0; a < n; ++a) {
        if (c.tid < RT_NPAR) c.prow(c.tid)[off + at(a)] /= L[tri(a) + a];
        __syncthreads();
        for (int e = c.tid; e < (n - 1 - a) * RT_NPAR; e += RT_BLOCK) {
            const int i = a + 1 + e / RT_NPAR, j = e % RT_NPAR;
            double* row = c.prow(j) + off;
            row[at(i)] = fma(-L[tri(i) + a], row[at(a)], row[at(i)]);
        }
        __syncthreads();
    }
}
template <class At>
VS_DEV void rt_sweep_backward(const RtCtx& c, const double* L, int n, int off, At at) {
    for (int a = n - 1; a >= 0; --a) {
        if (c.tid < RT_NPAR) c.prow(c.tid)[off + at(a)] /= L[tri(a) + a];
        __syncthreads();
        for (int e = c.tid; e < a * RT_NPAR; e += RT_BLOCK) {
            const int i = e / RT_NPAR, j = e % RT_NPAR;
            double* row = c.prow(j) + off;
            row[at(i)] = fma(-L[tri(a) + i], row[at(a)], row[at(i)]);
        }
        __syncthreads();
    }
}

// One right-hand side against a packed lower factor L of order n (LDS or workspace), by the whole workgroup, with the same
// `at` maps.  rt_solve_forward: L y = rhs (rhs is used up).  rt_solve_backward: L^T x = y (y is used up), entry j of the
// solution stored at x[at(j)] by thread 0; x may be y itself, since entry j is stored after its last read.  A barrier
// after every column; the backward sweep ends with one more, behind its last store.  n = 0 leaves only that barrier.
VS_DEV void rt_solve_forward(int tid, const double* L, int n, double* rhs, double* y) {
    for (int j = 0; j < n; ++j) {
        const double yj = rhs[j] / L[tri(j) + j];
        for (int i = j + 1 + tid; i < n; i += RT_BLOCK) rhs[i] = fma(-L[tri(i) + j], yj, rhs[i]);
        if (tid == 0) y[j] = yj;
        __syncthreads();
    }
}
template <class At>
VS_DEV void rt_solve_backward(int tid, const double* L, int n, double* y, double* x, At at) {
    for (int j = n - 1; j >= 0; --j) {
        const double xj = y[j] / L[tri(j) + j];
        for (int i = tid; i < j; i += RT_BLOCK) y[i] = fma(-L[tri(j) + i], xj, y[i]);
        __syncthreads();
        if (tid == 0) x[at(j)] = xj;
    }
    __syncthreads();
}

// ---- P0: record, configuration, linearisation
// Reads the record `in` (global) and cfg.dt, cfg.sq, cfg.use_jet.  Leaves in LDS: s.in, s.dt, s.sq, the flags F_STATUS =
// MAX_ITER and F_ITERS = 0, A | Bj | Bt | c in s.lin and the previous throttles (warped) in s.vprev.  Ends with
// p0_linearize's barrier.
template <class Cfg>
VS_DEV void rt_load_and_linearize(const RtCtx& c, const Cfg& cfg, const double* in) {
    const RtSmem s = c.lds();
    const int tid = c.tid;
    for (int i = tid; i < c.d.nin; i += RT_BLOCK) s.in[i] = in[size_t(c.inst) * c.d.nin + i];
    if (tid < c.d.n) s.dt[tid] = cfg.dt[tid];
    if (tid >= 64 && tid < 64 + NWROWS) s.sq[tid - 64] = cfg.sq[tid - 64];
    if (tid == 0) { s.flags[F_STATUS] = VSMPC_STATUS_MAX_ITER; s.flags[F_ITERS] = 0; }
    __syncthreads();
    p0_linearize(cfg.use_jet, s.in, s.sA, s.sBj, s.sBt, s.sC, s.vprev, tid, RT_BLOCK);
}

// ---- P1: sensitivity recursion of every condensed column, C = sum_k Y_k^T Y_k
// Reads the linearisation, s.in (x0, reference window), s.dt, s.sq.  Leaves the packed C (NP rows; with SENS the parameter
// rows too) in M.  Uses s.big for one stage of Y.  The column arrays live here and nowhere else: they are what fills the
// register file.
VS_HD int rt_big_condense(const RtDims& d) { return NWROWS * d.np; }   // s.big: one stage of Y
template <bool SENS>
VS_DEV void rt_condense(const RtCtx& c) {
    const RtDims& d = c.d;
    const RtSmem s = c.lds();
    const int tid = c.tid, NP = d.np, NZ = d.nz, NU = d.nu;
    const double* sA = s.sA;
    double* M = c.M;
    double X[RT_CPT][NX];
    const double* src[RT_CPT];
    int stride[RT_CPT], kind[RT_CPT], blk[RT_CPT];   // kind: 0 joint, 1 throttle, 2 affine, 3 none, 4 parameter
#pragma unroll
    for (int u = 0; u < RT_CPT; ++u) {
        const int col = tid + u * RT_BLOCK;
        kind[u] = col < NU ? 0 : (col < NZ ? 1 : (col == NZ ? 2 : ((SENS && col < NP) ? 4 : 3)));
        blk[u] = kind[u] == 0 ? col >> 3 : (kind[u] == 1 ? (col - NU) >> 2 : 0);
        src[u] = kind[u] == 0 ? s.sBj + (col & 7) : (kind[u] == 1 ? s.sBt + ((col - NU) & 3) : s.sC);
        stride[u] = kind[u] == 0 ? NJ : (kind[u] == 1 ? NTH : 1);
#pragma unroll
        for (int r = 0; r < NX; ++r) X[u][r] = kind[u] == 2 ? s.in[VSMPC_IN_X0 + r] : 0.0;
        if constexpr (SENS) {
#pragma unroll
            for (int r = 0; r < NX; ++r)
                if (kind[u] == 4 && r == col - NZ - 1) X[u][r] = 1.0;   // parameter column NZ + 1 + i: X_0 = e_i
        }
    }
    double* Y = s.big;   // Y[w * NP + column]
    for (int k = 0; k < d.n; ++k) {
        const double dt = s.dt[k];
        const int jb = joint_block(d, k), tb = throttle_block(d, k);
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
            const int cc = tid + u * RT_BLOCK;
#pragma unroll
            for (int w = 0; w < NWROWS; ++w) {
                const int r = wrow(w);
                const double ref = (kind[u] == 2 && r < 12) ? s.in[VSMPC_IN_XREF + col * 12 + r] : 0.0;
                Y[w * NP + cc] = s.sq[w] * (X[u][r] - ref);
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
// Reads cfg.wj, cfg.w_reg, cfg.w_thr, cfg.w_init, s.in (q_err), s.vprev.  Adds the input costs to the diagonal and the
// first sub-diagonal block of C and their gradient terms to row NZ of M.  Returns gtol, the box QP's release tolerance
// 1e-10 (1 + max |gradient|), the same value in every thread.  Uses s.red.
template <class Cfg>
VS_DEV double rt_input_costs(const RtCtx& c, const Cfg& cfg) {
    const RtDims& d = c.d;
    const RtSmem s = c.lds();
    const int tid = c.tid, NZ = d.nz, NU = d.nu;
    double* M = c.M;
    const double w_thr = cfg.w_thr;
    for (int col = tid; col < NZ; col += RT_BLOCK) {
        if (col < NU) {
            const int j = col & 7;
            M[tri(col) + col] += cfg.wj[j];                                   // costsVSMPC.cpp:375-381,564-571
            M[tri(NZ) + col] += cfg.w_reg * s.in[VSMPC_IN_QERR + j];          // :574-589
        } else {
            const int q = col - NU, b = q >> 2, r = q & 3;
            const int npairs = (b < d.nvb - 1 ? 1 : 0) + (b > 0 ? 1 : 0);  // first differences (:383-409)
            double diag = M[tri(col) + col];
            for (int p = 0; p < npairs; ++p) diag += w_thr;
            if (b == 0) diag += cfg.w_init;                                // ThrottleInitialValueCost (:468-487)
            M[tri(col) + col] = diag;
            if (b > 0) M[tri(col) + col - 4] -= w_thr;
            if (b == 0) M[tri(NZ) + col] += -cfg.w_init * s.vprev[r];
        }
    }
    __syncthreads();
    double gm = 0.0;
    for (int col = tid; col < NZ; col += RT_BLOCK) gm = fmax(gm, fabs(M[tri(NZ) + col]));
    s.red[tid] = gm;
    __syncthreads();
    for (int h = RT_BLOCK / 2; h > 0; h >>= 1) {
        if (tid < h) s.red[tid] = fmax(s.red[tid], s.red[tid + h]);
        __syncthreads();
    }
    return 1e-10 * (1.0 + s.red[0]);
}

// ---- P3: Cholesky of the joint columns; the trailing block becomes (S, s)
// Reads and overwrites M: columns 0 .. NU - 1 become L (all NP rows), the trailing rows the Schur complement -- S, the
// reduced gradient s in row NZ, and with SENS F~ and l~ in the parameter rows.  Returns bad: a pivot was not positive
// (M is then half factored and nothing after P3 may read it).  Uses s.col for the scaled column.
// This loop and the Cholesky of S_FF in rt_box_qp are not one helper: here the column is scaled first, staged in s.col, and
// the barrier follows; there the barrier comes before the scaling and the update reads the factor itself.
VS_DEV bool rt_factor_joint_columns(const RtCtx& c) {
    const RtSmem s = c.lds();
    const int tid = c.tid, NP = c.d.np, NU = c.d.nu;
    double* M = c.M;
    bool bad = false;   // (left by `break`, not by a return inside the loop: the early return rearranged this loop and
                        // the code behind it, 1.7 % more instructions in solve_kernel_rt and 0.9 % more time)
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
    return bad;
}

// ---- P4: box QP on the throttles, block principal pivoting (executable model: tests/runtime_model.py box_qp)
// Reads (S, s) in M, s.vprev, the box, gtol and cfg.max_as_iter.  Leaves the throttles in zv (bound ones exactly on their
// bound), the final active set in s.state (-1 lower / pinned, 0 free, 1 upper), F_STATUS and F_ITERS, and from the last
// iteration: the free list s.idx with its length F_NF, the factor of S_FF in K = s.big, the reduced gradient at z in
// s.vec2.  Returns bad: a pivot of S_FF was not positive.  Uses s.vec0, s.vec1.
VS_HD int rt_big_box_qp(const RtDims& d) { return d.nv * (d.nv + 1) / 2; }   // s.big: S_FF, packed
template <class Cfg>
VS_DEV bool rt_box_qp(const RtCtx& c, const Cfg& cfg, const RtBox box, double gtol) {
    const RtSmem s = c.lds();
    const int tid = c.tid, NV = c.d.nv;
    double* zv = c.zv();
    const double* sS = c.sS();
    bool bad = false;
    for (int p = tid; p < NV; p += RT_BLOCK) s.state[p] = box.pinned(p) ? -1 : 0;  // the hold pins v0 at v_prev
    if (tid == 0) { s.flags[F_BEST] = NV + 1; s.flags[F_PATIENCE] = AS_PATIENCE; }
    __syncthreads();
    for (int it = 0; it < cfg.max_as_iter; ++it) {
        // bound values, free list
        rt_bound_values(c, box);
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
                if (s.state[q] != 0) acc = fma(c.S(p, q), zv[q], acc);
            rhs[a] = -acc;
        }
        {
            const size_t nk = size_t(nf) * (nf + 1) / 2;
            int ei = 0, ej = 0;
            tri_advance(ei, ej, tid);
            for (size_t e = tid; e < nk; e += RT_BLOCK) {
                K[e] = c.S(s.idx[ei], s.idx[ej]);
                tri_advance(ei, ej, RT_BLOCK);
            }
        }
        __syncthreads();
        // Cholesky of K (see the note on rt_factor_joint_columns)
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
        // L y = rhs, then L^T v_F = y
        rt_solve_forward(tid, K, nf, rhs, y);
        rt_solve_backward(tid, K, nf, y, zv, RtAtFree{s.idx});
        // gradient of the reduced problem at z
        double* grad = s.vec2;
        for (int p = tid; p < NV; p += RT_BLOCK) {
            double acc = sS[p];
            for (int q = 0; q < NV; ++q) acc = fma(c.S(p, q), zv[q], acc);
            grad[p] = acc;
        }
        __syncthreads();
        if (tid == 0) {
            // The pivoting rule is written out in both loops, as in the one body this function came from: shared as a helper
            // it let the compiler unroll the two loops four times, 478 -> 977 instructions in this block of solve_kernel_rt.
            const bool hold = box.hold;
            const double vmin = box.vmin, vmax = box.vmax;
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
                if (ninf < s.flags[F_BEST]) { s.flags[F_BEST] = ninf; s.flags[F_PATIENCE] = AS_PATIENCE; }
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
    rt_bound_values(c, box);
    __syncthreads();
    return bad;
}

// ---- P5: joints, L_jj^T u = -(L_vj^T v + l_j)
// Reads L (joint columns of M), the gradient row's joint entries l_j and zv.  Leaves the joints in s.z[0 .. NU).  Uses s.col.
VS_DEV void rt_joints(const RtCtx& c) {
    const RtSmem s = c.lds();
    const int tid = c.tid, NZ = c.d.nz, NU = c.d.nu, NV = c.d.nv;
    const double* M = c.M;
    const double* zv = c.zv();
    double* r = s.col;
    for (int j = tid; j < NU; j += RT_BLOCK) {
        double acc = M[tri(NZ) + j];
        for (int p = 0; p < NV; ++p) acc = fma(M[tri(NU + p) + j], zv[p], acc);
        r[j] = -acc;
    }
    __syncthreads();
    rt_solve_backward(tid, M, NU, r, s.z, RtAtSelf{});
}

// The state recursion X_{k+1} = X_k + dt_k (A X_k + Bj U_jb(k) + Bt V_tb(k) [+ c with AFFINE]) on 26 lanes, X [N + 1][26] in
// LDS with X_0 written by the caller (no barrier needed in between), z = [joints | throttles] the inputs.
// Reads the linearisation and s.dt.  A barrier after every stage.
template <bool AFFINE>
VS_DEV void rt_recur_states(const RtCtx& c, double* X, const double* z) {
    const RtSmem s = c.lds();
    const RtDims& d = c.d;
    const int tid = c.tid;
    __syncthreads();
    for (int k = 0; k < d.n; ++k) {
        if (tid < NX) {
            const int r = tid;
            const double* U = z + NJ * joint_block(d, k);
            const double* V = z + d.nu + NTH * throttle_block(d, k);
            double a = AFFINE ? s.sC[r] : 0.0;
            for (int q = 0; q < NJ; ++q) a = fma(s.sBj[r * NJ + q], U[q], a);
            for (int q = 0; q < NTH; ++q) a = fma(s.sBt[r * NTH + q], V[q], a);
            for (int q = 0; q < NX; ++q) a = fma(s.sA[r * NX + q], X[k * NX + q], a);
            X[(k + 1) * NX + r] = fma(s.dt[k], a, X[k * NX + r]);
        }
        __syncthreads();
    }
}

// ---- P6: state trajectory X_{k+1} = X_k + dt_k (A X_k + Bj U_jb + Bt v_tb + c)
// Reads the linearisation, s.in (x0), s.dt and z (whatever it holds when the factorisation failed: rt_write_solution
// writes zeros for z then).  Leaves the N + 1 states in s.x.
VS_DEV void rt_simulate(const RtCtx& c) {
    const RtSmem s = c.lds();
    if (c.tid < NX) s.x[c.tid] = s.in[VSMPC_IN_X0 + c.tid];
    rt_recur_states<true>(c, s.x, s.z);
}

// ---- outputs of the solve
// Reads s.x, z, the flags.  Writes x (states, then z, or zeros for z when bad), the first-move block, the status
// (Numerical when bad) and the iterations; xout, fmout and iters_out may be null.
VS_DEV void rt_write_solution(const RtCtx& c, bool bad, double* xout, double* fmout, int* status_out, int* iters_out) {
    const RtDims& d = c.d;
    const RtSmem s = c.lds();
    const int tid = c.tid, inst = c.inst, NZ = d.nz, NU = d.nu;
    double* z = s.z;
    double* zv = z + NU;
    double* sX = s.x;
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

// ---- what the sensitivity entry says about the final active set (rt_adj_reduce_write says the same, written out: as calls
// these two made adjoint_kernel_rt slower, see there)
// The active-set output: 0 when P3 failed (the box QP never set s.state), 2 on the pinned throttles, else s.state.
VS_DEV void rt_write_active(const RtCtx& c, const RtBox box, bool factored, int* active_out) {
    const RtSmem s = c.lds();
    const int NV = c.d.nv;
    if (active_out != nullptr)
        for (int p = c.tid; p < NV; p += RT_BLOCK)
            active_out[size_t(c.inst) * NV + p] = !factored ? 0 : (box.pinned(p) ? 2 : s.state[p]);
}
// The degeneracy rule, one thread's work: whether a non-pinned throttle is weakly active (its reduced gradient, the box QP's
// s.vec2, within VSMPC_SENS_GRAD_TOL (1 + max |s|) of zero) or free and within VSMPC_SENS_BOUND_TOL (1 + |v|) of a bound.
// A derivative of the solution is one-sided there.  Reads s.state, zv, s.vec2 and the reduced gradient s of row NZ.
// (unroll 1: unrolled, these two thread-0 loops are what made the kernels longer when the rule became a function)
VS_DEV bool rt_degenerate(const RtCtx& c, const RtBox box) {
    const RtSmem s = c.lds();
    const int NV = c.d.nv;
    const double* sS = c.sS();
    const double* zv = c.zv();
    double smax = 0.0;
#pragma unroll 1
    for (int p = 0; p < NV; ++p) smax = fmax(smax, fabs(sS[p]));
    const double gt = VSMPC_SENS_GRAD_TOL * (1.0 + smax);
    bool degenerate = false;
#pragma unroll 1
    for (int p = 0; p < NV; ++p) {
        if (box.pinned(p)) continue;
        const int st = s.state[p];
        const double v = zv[p], bt = VSMPC_SENS_BOUND_TOL * (1.0 + fabs(v));
        if ((st != 0 && fabs(s.vec2[p]) <= gt) || (st == 0 && (v - box.vmin <= bt || box.vmax - v <= bt))) degenerate = true;
    }
    return degenerate;
}

}  // namespace

}  // namespace vsmpc
