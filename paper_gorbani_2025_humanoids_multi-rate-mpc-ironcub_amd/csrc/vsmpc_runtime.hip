// Runtime-sized solve kernels (gfx950): any horizon config_valid() accepts, sized by kernel arguments instead of template
// parameters, so that a configuration outside csrc/vsmpc_horizons.def runs without a rebuild
// (variableSamplingMPC.cpp:24-45 sizes the reference from its XML at run time).
//
// One workgroup of 256 threads per instance computes what solve_kernel computes -- same input record, primal in the
// reference variable order, first-move block, status and active-set iterations -- by the plainest route.  The solve is a
// list of phase functions over one context (RtCtx: sizes, LDS carve-up, the instance's workspace, the linearisation);
// rt_solve calls them in order, and each states above its definition what it reads and what it leaves behind:
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
//
// The phases that read the configuration take its type as a template parameter: DevCfg, the kernel argument
// (solve_kernel_rt, sens_kernel_rt), or RtTunCfg, the instance's row of tunables staged in LDS (solve_kernel_rt_tuned,
// vsmpc_solve_batch_tuned).
//
// sens_kernel_rt (vsmpc_sensitivity_batch) is rt_solve<RT_SENS>: the same phases and four more.  X0 enters the QP only
// through the initial-state rows, so the solution's Jacobian with respect to X0 is that of the final active set's affine
// piece ("Sensitivities"; executable model: tests/sensitivity_model.py):
//   P1  rt_condense<true>: 26 parameter columns after the affine one (NP = NZ + 27 rows): column NZ + 1 + i starts from
//       X_0 = e_i, takes no input, no c and no reference, so that C's parameter rows hold F = d(condensed gradient)/dX0
//   P2  nothing: the input costs and their gradient terms belong to the affine row
//   P3  the same Cholesky reduces the parameter rows to F~ (throttle columns) and l~ (joint columns)
//   P4  rt_sens_throttles, after the box QP, on a Solved exit, with the factor of S_FF the last iteration left in LDS (the
//       final free set): S_FF dv_F = -F~_F, dv = 0 on bound and pinned throttles
//   P5  rt_sens_joints: L_jj^T du = -(L_vj^T dv + l~)
//   P6  rt_sens_states: dX_0 = I, dX_{k+1} = dX_k + dt_k (A dX_k + Bj dU + Bt dV); rt_sens_write: the other outputs
// The 26 right-hand sides of P4 / P5 are solved in place in the parameter rows of the workspace, which then hold dz/dX0.
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
#include <atomic>
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
enum RtMode { RT_SOLVE, RT_SENS, RT_ADJOINT };   // the instantiations of rt_solve
enum { F_STATUS = 0, F_ITERS, F_NF, F_BEST, F_PATIENCE };   // LDS flag slots

VS_DEV size_t tri(int i) { return size_t(i) * size_t(i + 1) / 2; }

// next packed entry (i, j) after advancing the flat index by `step` (j <= i)
VS_DEV void tri_advance(int& i, int& j, int step) {
    j += step;
    while (j > i) { j -= i + 1; ++i; }
}

// LDS carve-up (doubles), in the order of RtDims::lds_doubles()
struct RtSmem {
    double *in, *lin, *vprev, *dt, *sq, *x, *z, *col, *red, *vec0, *vec1, *vec2, *big;
    double *sA, *sBj, *sBt, *sC;   // A | Bj | Bt | c: p0_linearize's block, in lin
    int *state, *idx, *flags;
};
VS_DEV RtSmem rt_smem(const RtDims& d, double* base) {
    RtSmem s;
    double* p = base;
    s.in = p;    p += (d.nin + 1) & ~1;
    s.lin = p;   p += LIN_DOUBLES;
    s.sA = s.lin;
    s.sBj = s.sA + NX * NX;
    s.sBt = s.sBj + NX * NJ;
    s.sC = s.sBt + NX * NTH;
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
    s.big = p;   // max(18 NP, NV (NV + 1) / 2), and 2 x 26 x 26 with SENS, 26 (2 N + 2) with the adjoint
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

// ---- P4 (SENS): S_FF dv_F = -F~_F for the 26 parameter rows, in place (row j's throttle entry p at prow(j)[NU + p])
// Reads the last iteration's factor of S_FF in K = s.big, its free list s.idx / F_NF, and s.state.  Leaves dv/dX0 in the
// throttle entries of the parameter rows.
VS_DEV void rt_sens_throttles(const RtCtx& c) {
    const RtSmem s = c.lds();
    const int NU = c.d.nu;
    const int nf = s.flags[F_NF];
    const int* idx = s.idx;
    for (int e = c.tid; e < c.d.nv * RT_NPAR; e += RT_BLOCK) {
        const int p = e / RT_NPAR, j = e % RT_NPAR;
        double* r = c.prow(j) + NU + p;
        *r = s.state[p] == 0 ? -*r : 0.0;     // bounds and the hold pin do not depend on X0
    }
    __syncthreads();
    rt_sweep_forward(c, s.big, nf, NU, RtAtFree{idx});
    rt_sweep_backward(c, s.big, nf, NU, RtAtFree{idx});
}

// ---- P5: joints, L_jj^T u = -(L_vj^T v + l_j)
// Reads L (joint columns of M), the gradient row's joint entries l_j and zv.  Leaves the joints in s.z[0 .. NU).  Uses s.col.
VS_DEV void rt_joints(const RtCtx& c) {
    const RtSmem s = c.lds();
    const int tid = c.tid, NZ = c.d.nz, NU = c.d.nu, NV = c.d.nv;
    const double* M = c.M;
    const double* zv = c.zv();
    double* z = s.z;
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

// ---- P5 (SENS): L_jj^T du = -(L_vj^T dv + l~), in place in the joint entries of the parameter rows
// Reads L and the parameter rows (dv/dX0 from rt_sens_throttles, l~ from P3).  Leaves du/dX0 in their joint entries: the
// parameter rows then hold dz/dX0.
VS_DEV void rt_sens_joints(const RtCtx& c) {
    const int NU = c.d.nu, NV = c.d.nv;
    const double* M = c.M;
    for (int e = c.tid; e < NU * RT_NPAR; e += RT_BLOCK) {
        const int jj = e / RT_NPAR, j = e % RT_NPAR;
        double* row = c.prow(j);
        double acc = row[jj];
        for (int p = 0; p < NV; ++p) acc = fma(M[tri(NU + p) + jj], row[NU + p], acc);
        row[jj] = -acc;
    }
    __syncthreads();
    rt_sweep_backward(c, M, NU, 0, RtAtSelf{});
}

// ---- P6: state trajectory X_{k+1} = X_k + dt_k (A X_k + Bj U_jb + Bt v_tb + c)
// Reads the linearisation, s.in (x0), s.dt and z (whatever it holds when the factorisation failed: rt_write_solution
// writes zeros for z then).  Leaves the N + 1 states in s.x.
VS_DEV void rt_simulate(const RtCtx& c) {
    const RtSmem s = c.lds();
    const RtDims& d = c.d;
    const int tid = c.tid;
    double* sX = s.x;
    if (tid < NX) sX[tid] = s.in[VSMPC_IN_X0 + tid];
    __syncthreads();
    for (int k = 0; k < d.n; ++k) {
        if (tid < NX) {
            const int r = tid;
            const double* U = s.z + NJ * joint_block(d, k);
            const double* V = c.zv() + NTH * throttle_block(d, k);
            double a = s.sC[r];
            for (int q = 0; q < NJ; ++q) a = fma(s.sBj[r * NJ + q], U[q], a);
            for (int q = 0; q < NTH; ++q) a = fma(s.sBt[r * NTH + q], V[q], a);
            for (int q = 0; q < NX; ++q) a = fma(s.sA[r * NX + q], sX[k * NX + q], a);
            sX[(k + 1) * NX + r] = fma(s.dt[k], a, sX[k * NX + r]);
        }
        __syncthreads();
    }
}

// the outputs of the sensitivity entry (per instance; each may be null)
struct RtSensOut {
    double* dx = nullptr;     // dx_dx0 [nVar][26]
    double* dfm = nullptr;    // dfm_dx0 [24][26]
    int* active = nullptr;    // [NV]
    int* flags = nullptr;     // VSMPC_SENS_*
};

// ---- P6 (SENS): dX_{k+1} = dX_k + dt_k (A dX_k + Bj dU_jb + Bt dV_tb), dX_0 = I
// Reads the linearisation, s.dt and dz/dX0 in the parameter rows.  Writes the state rows of nodes 1..N of dx_dx0 and the
// node-1 thrust rows of dfm_dx0 (global).  Uses s.big for dX_k | dX_{k+1}, [26][26] each (K is no longer needed).
VS_DEV void rt_sens_states(const RtCtx& c, const RtSensOut& out) {
    const RtSmem s = c.lds();
    const RtDims& d = c.d;
    const int tid = c.tid, inst = c.inst;
    double* DX = s.big;
    for (int e = tid; e < NX * RT_NPAR; e += RT_BLOCK) DX[e] = e / RT_NPAR == e % RT_NPAR ? 1.0 : 0.0;
    __syncthreads();
    for (int k = 0; k < d.n; ++k) {
        const double* cur = DX + (k & 1) * NX * RT_NPAR;
        double* nxt = DX + ((k + 1) & 1) * NX * RT_NPAR;
        const int ub = NJ * joint_block(d, k), vb = d.nu + NTH * throttle_block(d, k);
        for (int e = tid; e < NX * RT_NPAR; e += RT_BLOCK) {
            const int r = e / RT_NPAR, j = e % RT_NPAR;
            const double* dz = c.prow(j);
            double a = 0.0;
            for (int q = 0; q < NJ; ++q) a = fma(s.sBj[r * NJ + q], dz[ub + q], a);
            for (int q = 0; q < NTH; ++q) a = fma(s.sBt[r * NTH + q], dz[vb + q], a);
            for (int q = 0; q < NX; ++q) a = fma(s.sA[r * NX + q], cur[q * RT_NPAR + j], a);
            const double v = fma(s.dt[k], a, cur[e]);
            nxt[e] = v;
            if (out.dx != nullptr) out.dx[size_t(inst) * d.nvar * RT_NPAR + size_t(k + 1) * NX * RT_NPAR + e] = v;
            if (k == 0 && out.dfm != nullptr && r >= 12 && r < 20)     // thrust and thrust rate of node 1
                out.dfm[size_t(inst) * VSMPC_FM_SIZE * RT_NPAR + (VSMPC_FM_THRUST + r - 12) * RT_NPAR + j] = v;
        }
        __syncthreads();
    }
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

// ---- the outputs of the sensitivity entry that rt_sens_states did not write
// Reads dz/dX0 in the parameter rows, zv, s.state, the reduced gradient s and the gradient at z in s.vec2.  Writes dx_dx0
// (dX_0 = I and the joint / throttle rows), dfm_dx0 (joint increments, v0, throttle percent) -- all zero unless sens_ok --
// the active set (0 when P3 failed: the box QP never set s.state) and the VSMPC_SENS_* flags.
VS_DEV void rt_sens_write(const RtCtx& c, const RtBox box, bool factored, bool sens_ok, const RtSensOut& out) {
    const RtDims& d = c.d;
    const RtSmem s = c.lds();
    const int tid = c.tid, inst = c.inst, NZ = d.nz, NU = d.nu, NV = d.nv;
    double* M = c.M;
    double* zv = s.z + NU;
    double* sS = M + tri(NZ) + NU;
    const bool hold = box.hold;
    const double vmin = box.vmin, vmax = box.vmax;
    double* const dxout = out.dx;
    double* const dfmout = out.dfm;
    int* const active_out = out.active;
    int* const flags_out = out.flags;
    // dx_dx0: dX_0 = I and the joint / throttle rows (P6 wrote the state rows of nodes 1..N); zero unless Solved
    if (dxout != nullptr) {
        double* o = dxout + size_t(inst) * d.nvar * RT_NPAR;
        for (int e = tid; e < NX * RT_NPAR; e += RT_BLOCK) o[e] = sens_ok && e / RT_NPAR == e % RT_NPAR ? 1.0 : 0.0;
        if (!sens_ok)
            for (int e = NX * RT_NPAR + tid; e < d.nxs * RT_NPAR; e += RT_BLOCK) o[e] = 0.0;
        for (int e = tid; e < NZ * RT_NPAR; e += RT_BLOCK) {
            const int col = e / RT_NPAR, j = e % RT_NPAR;
            o[size_t(d.nxs) * RT_NPAR + e] = sens_ok ? M[tri(NZ + 1 + j) + col] : 0.0;
        }
    }
    // dfm_dx0: joint increments, v0 and throttle percent (P6 wrote the node-1 thrust rows)
    if (dfmout != nullptr) {
        double* o = dfmout + size_t(inst) * VSMPC_FM_SIZE * RT_NPAR;
        for (int e = tid; e < VSMPC_FM_THRUST * RT_NPAR; e += RT_BLOCK) {
            const int r = e / RT_NPAR, j = e % RT_NPAR;
            const double* dz = M + tri(NZ + 1 + j);
            double v = 0.0;
            if (sens_ok) {
                if (r < 8) v = dz[r];
                else if (r < 12) v = dz[NU + r - 8];
                else v = Jet::dthrottle_dv(zv[r - 12]) * dz[NU + r - 12];
            }
            o[e] = v;
        }
        if (!sens_ok)
            for (int e = VSMPC_FM_THRUST * RT_NPAR + tid; e < VSMPC_FM_SIZE * RT_NPAR; e += RT_BLOCK) o[e] = 0.0;
    }
    if (active_out != nullptr)
        for (int p = tid; p < NV; p += RT_BLOCK)
            active_out[size_t(inst) * NV + p] = !factored ? 0 : ((hold && p < NTH) ? 2 : s.state[p]);
    if (tid == 0 && flags_out != nullptr) {
        int fl = VSMPC_SENS_UNSOLVED;
        if (sens_ok) {   // weakly or nearly active non-pinned throttles: the Jacobian is one-sided there
            fl = 0;
            double smax = 0.0;
            for (int p = 0; p < NV; ++p) smax = fmax(smax, fabs(sS[p]));
            const double gt = VSMPC_SENS_GRAD_TOL * (1.0 + smax);
            for (int p = 0; p < NV; ++p) {
                if (hold && p < NTH) continue;
                const int st = s.state[p];
                const double v = zv[p], bt = VSMPC_SENS_BOUND_TOL * (1.0 + fabs(v));
                if ((st != 0 && fabs(s.vec2[p]) <= gt) || (st == 0 && (v - vmin <= bt || vmax - v <= bt)))
                    fl |= VSMPC_SENS_DEGENERATE;
            }
        }
        flags_out[inst] = fl;
    }
}

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

VS_DEV double rt_wave_sum(double v) {   // butterfly: every lane ends with the same sum, formed in the same order
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
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
    // (the division is repeated where w_j is read), so that no thread writes what another one reads in the same step.
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
        if (tid == 0) r[NU + s.idx[j]] = vj;
    }
    __syncthreads();
    // L_jj^T du = w - L_vj^T dv
    for (int j = tid; j < NU; j += RT_BLOCK) {
        double acc = r[j] / M[tri(j) + j];
        for (int p = 0; p < NV; ++p) acc = fma(-M[tri(NU + p) + j], r[NU + p], acc);
        r[j] = acc;
    }
    __syncthreads();
    for (int j = NU - 1; j >= 0; --j) {
        const double uj = r[j] / M[tri(j) + j];
        for (int i = tid; i < j; i += RT_BLOCK) r[i] = fma(-M[tri(j) + i], uj, r[i]);
        __syncthreads();
        if (tid == 0) r[j] = uj;
    }
    __syncthreads();
}

// the adjoint's carve-up of s.big (the factor of S_FF is dead): a_X [N + 1][26] | b_0 .. b_{N-1}, b_init [N + 1][26]
VS_DEV double* rt_adj_ax(const RtCtx& c) { return c.lds().big; }
VS_DEV double* rt_adj_b(const RtCtx& c) { return c.lds().big + NX * (c.d.n + 1); }

// ---- adjoint 3: state part of a: a_X0 = 0, a_X{k+1} = a_Xk + dt_k (A a_Xk + Bj a_U[jb(k)] + Bt a_V[tb(k)])
// Reads a_z in s.col, the linearisation, s.dt.  Leaves a_X in s.big.
VS_DEV void rt_adj_states(const RtCtx& c) {
    const RtSmem s = c.lds();
    const RtDims& d = c.d;
    const int tid = c.tid;
    double* aX = rt_adj_ax(c);
    if (tid < NX) aX[tid] = 0.0;
    __syncthreads();
    for (int k = 0; k < d.n; ++k) {
        if (tid < NX) {
            const int r = tid;
            const double* U = s.col + NJ * joint_block(d, k);
            const double* V = s.col + d.nu + NTH * throttle_block(d, k);
            double a = 0.0;
            for (int q = 0; q < NJ; ++q) a = fma(s.sBj[r * NJ + q], U[q], a);
            for (int q = 0; q < NTH; ++q) a = fma(s.sBt[r * NTH + q], V[q], a);
            for (int q = 0; q < NX; ++q) a = fma(s.sA[r * NX + q], aX[k * NX + q], a);
            aX[(k + 1) * NX + r] = fma(s.dt[k], a, aX[k * NX + r]);
        }
        __syncthreads();
    }
}

// diagonal of Q on state row r from the square-root weights (0 on thrust and thrust rate)
template <class Cfg>
VS_DEV double rt_q_diag(const Cfg& cfg, int r) {
    const double q = cfg.sq[r < 12 ? r : (r >= 20 ? r - 8 : 0)];
    return (r >= 12 && r < 20) ? 0.0 : q * q;
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
    const double qd = tid < NX ? rt_q_diag(cfg, tid) : 0.0;
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
// the active set and the VSMPC_ADJ_* flags, whose degeneracy rule is rt_sens_write's.
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
            acc = rt_wave_sum(acc);
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

// The solve of one instance: the phases in order.  cfg is a DevCfg or an RtTunCfg; `sens` is looked at with RT_SENS only,
// `adj` with RT_ADJOINT only.
template <RtMode MODE, class Cfg>
VS_DEV void rt_solve(const Cfg& cfg, const RtDims& d, const double* in, double* ws, double* xout, double* fmout,
                     int* status_out, int* iters_out, const RtSensOut& sens = {}, const RtAdjIO& adj = {}) {
    constexpr bool SENS = MODE == RT_SENS;
    const int inst = blockIdx.x;
    const RtCtx c{d, ws + size_t(inst) * size_t(d.ws_doubles), int(threadIdx.x), inst};
    const RtSmem s = c.lds();

    rt_load_and_linearize(c, cfg, in);
    rt_condense<SENS>(c);
    const double gtol = rt_input_costs(c, cfg);
    bool bad = rt_factor_joint_columns(c);
    const bool factored = !bad;   // the box QP runs (s.state is set)
    const RtBox box{s.in[VSMPC_IN_HOLD] != 0.0, cfg.vmin, cfg.vmax};
    if (!bad) bad = rt_box_qp(c, cfg, box, gtol);
    const bool sens_ok = SENS && !bad && s.flags[F_STATUS] == VSMPC_STATUS_SOLVED;
    if constexpr (SENS) {
        if (sens_ok) rt_sens_throttles(c);
    }
    if (!bad) rt_joints(c);
    if constexpr (SENS) {
        if (sens_ok) rt_sens_joints(c);
    }
    rt_simulate(c);
    if constexpr (SENS) {
        if (sens_ok) rt_sens_states(c, sens);
    }
    rt_write_solution(c, bad, xout, fmout, status_out, iters_out);
    if constexpr (SENS) rt_sens_write(c, box, factored, sens_ok, sens);
    if constexpr (MODE == RT_ADJOINT) {
        const bool adj_ok = !bad && s.flags[F_STATUS] == VSMPC_STATUS_SOLVED;   // (the same value in every thread)
        bool nonfinite = false;
        if (adj_ok) {
            const RtAdjIn a = rt_adj_in(c, adj);
            nonfinite = rt_adj_rhs(c, a);
            rt_adj_solve(c);
            rt_adj_states(c);
            rt_adj_costates(c, cfg, a);
        }
        rt_adj_reduce_write(c, cfg, box, factored, adj_ok, nonfinite, adj);
    }
}

}  // namespace

__global__ __launch_bounds__(RT_BLOCK) void solve_kernel_rt(DevCfg cfg, RtDims d, const double* __restrict__ in,
                                                            double* __restrict__ ws, double* __restrict__ xout,
                                                            double* __restrict__ fmout, int* __restrict__ status_out,
                                                            int* __restrict__ iters_out) {
    rt_solve<RT_SOLVE>(cfg, d, in, ws, xout, fmout, status_out, iters_out);
}

// solve_kernel_rt + the 26 parameter columns and the outputs dx_dx0 [nVar][26], dfm_dx0 [24][26], active [NV] and the
// sensitivity flags (per instance, each may be null)
__global__ __launch_bounds__(RT_BLOCK) void sens_kernel_rt(DevCfg cfg, RtDims d, const double* __restrict__ in,
                                                           double* __restrict__ ws, double* __restrict__ xout,
                                                           double* __restrict__ fmout, int* __restrict__ status_out,
                                                           int* __restrict__ iters_out, double* __restrict__ dxout,
                                                           double* __restrict__ dfmout, int* __restrict__ active_out,
                                                           int* __restrict__ flags_out) {
    rt_solve<RT_SENS>(cfg, d, in, ws, xout, fmout, status_out, iters_out, RtSensOut{dxout, dfmout, active_out, flags_out});
}

// solve_kernel_rt with per-instance tunables (vsmpc_solve_batch_tuned on a runtime handle): the instance's row of `tun`
// ([batch][VSMPC_TUNE_SIZE], sCfg order) is staged in LDS and is the configuration the phases read for the weights and the
// throttle box; dt, use_jet and max_as_iter are copied beside it from the handle's DevCfg.
struct RtTunCfg {   // LDS image: the row (CFG_* order), then what the phases read of the handle's DevCfg
    double sq[NWROWS], wj[NJ], w_reg, w_thr, w_init, vmin, vmax, pad_;
    double dt[MAX_STAGES];
    int use_jet, max_as_iter;
};
static_assert(offsetof(RtTunCfg, wj) == CFG_WJ * sizeof(double) && offsetof(RtTunCfg, vmax) == CFG_VMAX * sizeof(double) &&
              offsetof(RtTunCfg, dt) == CFG_SIZE * sizeof(double) && CFG_SIZE == VSMPC_TUNE_SIZE && sizeof(RtTunCfg) % 8 == 0,
              "a row of tunables is the head of RtTunCfg");
// Stages the instance's row of `tun` and what the phases read of the handle's DevCfg behind rt_solve's carve-up (the launcher
// adds sizeof(RtTunCfg)); ends with a barrier.
VS_DEV RtTunCfg& rt_stage_tunables(const DevCfg& hcfg, const RtDims& d, const double* __restrict__ tun) {
    extern __shared__ __attribute__((aligned(16))) double smem_tuned[];
    double* const sTun = smem_tuned + d.lds_doubles;
    RtTunCfg& tcfg = *reinterpret_cast<RtTunCfg*>(sTun);
    const int t = threadIdx.x;
    double2 v = make_double2(0.0, 0.0);
    if (t < CFG_SIZE / 2) {
        v = reinterpret_cast<const double2*>(tun + size_t(blockIdx.x) * CFG_SIZE)[t];
        sTun[2 * t] = v.x;
        sTun[2 * t + 1] = v.y;
    }
    if (t >= 64 && t < 64 + MAX_STAGES) tcfg.dt[t - 64] = hcfg.dt[t - 64];
    if (t == 128) { tcfg.use_jet = hcfg.use_jet; tcfg.max_as_iter = hcfg.max_as_iter; }
    // a non-finite tunable ends like a non-finite record: the first square-root weight is made NaN, so that the first pivot
    // fails and the status is Numerical (the pad entry of the row is not looked at)
    const bool fin = isfinite(v.x) && (isfinite(v.y) || t == CFG_SIZE / 2 - 1);
    __syncthreads();
    if (!fin) tcfg.sq[0] = __builtin_nan("");
    __syncthreads();
    return tcfg;
}
__global__ __launch_bounds__(RT_BLOCK) void solve_kernel_rt_tuned(DevCfg hcfg, RtDims d, const double* __restrict__ in,
                                                                  double* __restrict__ ws, double* __restrict__ xout,
                                                                  double* __restrict__ fmout, int* __restrict__ status_out,
                                                                  int* __restrict__ iters_out,
                                                                  const double* __restrict__ tun) {
    const RtTunCfg& tcfg = rt_stage_tunables(hcfg, d, tun);
    rt_solve<RT_SOLVE>(tcfg, d, in, ws, xout, fmout, status_out, iters_out);
}

// solve_kernel_rt + the adjoint phases: xbar [batch][nVar] and fmbar [batch][24] (or null) in, dL/dX0 [batch][26],
// dL/dcfg [batch][VSMPC_GRAD_SIZE], active [batch][NV] and the VSMPC_ADJ_* flags out (each may be null)
__global__ __launch_bounds__(RT_BLOCK) void adjoint_kernel_rt(DevCfg cfg, RtDims d, const double* __restrict__ in,
                                                              double* __restrict__ ws, double* __restrict__ xout,
                                                              double* __restrict__ fmout, int* __restrict__ status_out,
                                                              int* __restrict__ iters_out, const double* __restrict__ xbar,
                                                              const double* __restrict__ fmbar, double* __restrict__ gx0,
                                                              double* __restrict__ gcfg, int* __restrict__ active_out,
                                                              int* __restrict__ flags_out) {
    rt_solve<RT_ADJOINT>(cfg, d, in, ws, xout, fmout, status_out, iters_out, RtSensOut{},
                         RtAdjIO{xbar, fmbar, gx0, gcfg, active_out, flags_out});
}
// the same with per-instance tunables, staged as in solve_kernel_rt_tuned
__global__ __launch_bounds__(RT_BLOCK) void adjoint_kernel_rt_tuned(DevCfg hcfg, RtDims d, const double* __restrict__ in,
                                                                    double* __restrict__ ws, double* __restrict__ xout,
                                                                    double* __restrict__ fmout, int* __restrict__ status_out,
                                                                    int* __restrict__ iters_out, const double* __restrict__ xbar,
                                                                    const double* __restrict__ fmbar, double* __restrict__ gx0,
                                                                    double* __restrict__ gcfg, int* __restrict__ active_out,
                                                                    int* __restrict__ flags_out, const double* __restrict__ tun) {
    const RtTunCfg& tcfg = rt_stage_tunables(hcfg, d, tun);
    rt_solve<RT_ADJOINT>(tcfg, d, in, ws, xout, fmout, status_out, iters_out, RtSensOut{},
                         RtAdjIO{xbar, fmbar, gx0, gcfg, active_out, flags_out});
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
    p0_linearize(cfg.use_jet, sIn, sA, sBj, sBt, sC, sVprev, tid, 256);
    for (int i = tid; i < NX * NX; i += 256) A[size_t(b) * NX * NX + i] = sA[i];
    for (int i = tid; i < NX * NJ; i += 256) Bj[size_t(b) * NX * NJ + i] = sBj[i];
    for (int i = tid; i < NX * NTH; i += 256) Bt[size_t(b) * NX * NTH + i] = sBt[i];
    for (int i = tid; i < NX; i += 256) c[size_t(b) * NX + i] = sC[i];
}

RtDims runtime_dims(int n_iter, int n_iter_small, int control_horizon, bool sensitivity, bool adjoint) {
    RtDims d{};
    d.n = n_iter;
    d.ns = n_iter_small;
    d.hc = control_horizon;
    d.nvb = d.hc - d.ns + 1;
    d.nu = NJ * d.hc;
    d.nv = NTH * d.nvb;
    d.nz = d.nu + d.nv;
    d.np = d.nz + 1 + (sensitivity ? RT_NPAR : 0);
    d.nin = VSMPC_IN_XREF + 12 * (d.n - d.ns + 1);
    d.nxs = NX * (d.n + 1);
    d.nvar = d.nxs + d.nz;
    d.ntri = int(size_t(d.np) * (d.np + 1) / 2);
    d.ws_doubles = d.ntri;
    const int fixed = ((d.nin + 1) & ~1) + LIN_DOUBLES + 4 + MAX_STAGES + NWROWS + 2 + NX * (d.n + 1) + ((d.nz + 1) & ~1) +
                      ((d.np + 1) & ~1) + RT_BLOCK + 3 * ((d.nv + 1) & ~1) + 2 * ((d.nv + 1) / 2 + 1) + 4;
    const int ybuf = NWROWS * d.np, kbuf = d.nv * (d.nv + 1) / 2, dxbuf = sensitivity ? 2 * NX * RT_NPAR : 0;
    const int adjbuf = adjoint ? 2 * NX * (d.n + 1) : 0;   // a_X | b after the box QP's factor is dead (rt_adj_ax, rt_adj_b)
    const int big = ybuf > kbuf ? ybuf : kbuf;
    const int big2 = big > dxbuf ? big : dxbuf;
    d.lds_doubles = fixed + (big2 > adjbuf ? big2 : adjbuf);
    return d;
}

size_t runtime_lds_bytes(const RtDims& d) { return size_t(d.lds_doubles) * sizeof(double); }

size_t runtime_tuned_lds_bytes(const RtDims& d) { return runtime_lds_bytes(d) + sizeof(RtTunCfg); }

// every horizon launches under the largest dynamic LDS, allowed once per kernel and device
static hipError_t rt_allow_lds(const void* kernel, std::atomic<bool> (&attr_set)[MAX_DEVICES], const RtDims& d) {
    if (runtime_lds_bytes(d) > RT_MAX_LDS) return hipErrorInvalidValue;
    return allow_dynamic_lds(kernel, attr_set, RT_MAX_LDS);
}

hipError_t launch_solve_runtime(const RtDims& d, const DevCfg& cfg, const double* d_in, int batch, double* d_ws, double* d_x,
                                double* d_fm, int* d_status, int* d_iters, hipStream_t stream) {
    static std::atomic<bool> attr_set[MAX_DEVICES];
    const hipError_t e = rt_allow_lds(reinterpret_cast<const void*>(&solve_kernel_rt), attr_set, d);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(solve_kernel_rt, dim3(batch), dim3(RT_BLOCK), runtime_lds_bytes(d), stream, cfg, d, d_in, d_ws, d_x,
                       d_fm, d_status, d_iters);
    return hipGetLastError();
}

hipError_t launch_solve_runtime_tuned(const RtDims& d, const DevCfg& cfg, const double* d_in, const double* d_tun, int batch,
                                      double* d_ws, double* d_x, double* d_fm, int* d_status, int* d_iters,
                                      hipStream_t stream) {
    static std::atomic<bool> attr_set[MAX_DEVICES];
    const size_t lds = runtime_tuned_lds_bytes(d);                          // the staged row lies behind the body's carve-up
    if (lds > RT_MAX_LDS) return hipErrorInvalidValue;                      // (the largest valid horizon needs 129 KB)
    const hipError_t e = rt_allow_lds(reinterpret_cast<const void*>(&solve_kernel_rt_tuned), attr_set, d);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(solve_kernel_rt_tuned, dim3(batch), dim3(RT_BLOCK), lds, stream, cfg, d, d_in, d_ws,
                       d_x, d_fm, d_status, d_iters, d_tun);
    return hipGetLastError();
}

hipError_t launch_sensitivity_runtime(const RtDims& d, const DevCfg& cfg, const double* d_in, int batch, double* d_ws,
                                      double* d_x, double* d_fm, int* d_status, int* d_iters, double* d_dx, double* d_dfm,
                                      int* d_active, int* d_flags, hipStream_t stream) {
    static std::atomic<bool> attr_set[MAX_DEVICES];
    if (d.np != d.nz + 1 + RT_NPAR || d.np > RT_BLOCK * RT_CPT) return hipErrorInvalidValue;   // runtime_dims(.., true)
    const hipError_t e = rt_allow_lds(reinterpret_cast<const void*>(&sens_kernel_rt), attr_set, d);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(sens_kernel_rt, dim3(batch), dim3(RT_BLOCK), runtime_lds_bytes(d), stream, cfg, d, d_in, d_ws, d_x,
                       d_fm, d_status, d_iters, d_dx, d_dfm, d_active, d_flags);
    return hipGetLastError();
}

hipError_t launch_adjoint_runtime(const RtDims& d, const DevCfg& cfg, const double* d_in, const double* d_tun, int batch,
                                  double* d_ws, double* d_x, double* d_fm, int* d_status, int* d_iters, const double* d_xbar,
                                  const double* d_fmbar, double* d_gx0, double* d_gcfg, int* d_active, int* d_flags,
                                  hipStream_t stream) {
    static std::atomic<bool> attr_set[MAX_DEVICES], attr_set_tuned[MAX_DEVICES];
    static_assert(VSMPC_GRAD_SIZE * RT_NWAVES <= RT_BLOCK && 2 * NX + RT_NWAVES <= RT_BLOCK, "s.red holds the partial sums and lambda");
    if (d.np != d.nz + 1) return hipErrorInvalidValue;                                    // runtime_dims(.., false, true)
    const size_t lds = d_tun != nullptr ? runtime_tuned_lds_bytes(d) : runtime_lds_bytes(d);
    if (lds > RT_MAX_LDS) return hipErrorInvalidValue;
    if (d_tun != nullptr) {
        const hipError_t e = rt_allow_lds(reinterpret_cast<const void*>(&adjoint_kernel_rt_tuned), attr_set_tuned, d);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(adjoint_kernel_rt_tuned, dim3(batch), dim3(RT_BLOCK), lds, stream, cfg, d, d_in, d_ws, d_x, d_fm,
                           d_status, d_iters, d_xbar, d_fmbar, d_gx0, d_gcfg, d_active, d_flags, d_tun);
        return hipGetLastError();
    }
    const hipError_t e = rt_allow_lds(reinterpret_cast<const void*>(&adjoint_kernel_rt), attr_set, d);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(adjoint_kernel_rt, dim3(batch), dim3(RT_BLOCK), lds, stream, cfg, d, d_in, d_ws, d_x, d_fm, d_status,
                       d_iters, d_xbar, d_fmbar, d_gx0, d_gcfg, d_active, d_flags);
    return hipGetLastError();
}

hipError_t launch_linearize_runtime(const RtDims& d, const DevCfg& cfg, const double* d_in, int batch, double* A, double* Bj,
                                    double* Bt, double* c, hipStream_t stream) {
    const size_t lds = size_t(((d.nin + 1) & ~1) + LIN_DOUBLES + 4) * sizeof(double);
    hipLaunchKernelGGL(linearize_kernel_rt, dim3(batch), dim3(256), lds, stream, cfg, d.nin, d_in, A, Bj, Bt, c);
    return hipGetLastError();
}

const char* runtime_kernel_name() { return "solve_kernel_rt"; }

}  // namespace vsmpc
