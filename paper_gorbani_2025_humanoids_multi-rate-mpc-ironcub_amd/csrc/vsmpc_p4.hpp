// P4 of the tuned solve kernels: the box QP on the throttles (small SPD solvers in registers, dual and primal form).
#pragma once
#include "vsmpc_smem.hpp"

namespace vsmpc {

// Measurement build (-DVS_DIAG_QP, diagnostic instantiation only): the box QP of the dual form in four parts, cycles of
// wavefront 0 added up in qt[0..3] = set-up / columns of P / system solves / updates and checks (tools/qp_tail.py).
#ifdef VS_DIAG_QP
#define VS_QP_TIC() do { if (qt != nullptr) qt_mark = __builtin_amdgcn_s_memtime(); } while (0)
#define VS_QP_TOC(i)                                                   \
    do {                                                               \
        if (qt != nullptr) {                                           \
            const unsigned long long qt_now = __builtin_amdgcn_s_memtime(); \
            qt[i] += qt_now - qt_mark;                                 \
            qt_mark = qt_now;                                          \
        }                                                              \
    } while (0)
#else
#define VS_QP_TIC() do { } while (0)
#define VS_QP_TOC(i) do { } while (0)
#endif

// ------------------------------------------------------------------------------------------------
// K x K symmetric positive definite system (P_AA mu = rhs_A of the dual box QP, S_FF v_F = b_F of the primal), K <= 12, all lanes redundantly on
// wave-uniform values (symmetric elimination on the lower triangle).  sP[b * NVS + i] = P[i][b]; the K set bits of
// `mask` are the active indices; lane idx[q] returns mu_q, every other lane 0.
template <int K, int NVS>
VS_DEV double small_spd_solve(const double* __restrict__ sP, unsigned long long mask, double rhs, int lane, int& bad) {
    int idx[K];
#pragma unroll
    for (int q = 0; q < K; ++q) {
        idx[q] = __ffsll((long long)mask) - 1;
        mask &= mask - 1;
    }
    double A[K][K], d[K];
#pragma unroll
    for (int q = 0; q < K; ++q) {
        d[q] = readlane_f64(rhs, idx[q]);
#pragma unroll
        for (int c = 0; c <= q; ++c) A[q][c] = sP[idx[c] * NVS + idx[q]];  // uniform address: LDS broadcast
    }
    double ip[K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
        bad |= !(A[j][j] > 0.0);
        ip[j] = fast_rcp(A[j][j]);
#pragma unroll
        for (int i = j + 1; i < K; ++i) {
            const double f = A[i][j] * ip[j];
            d[i] = fma(-f, d[j], d[i]);
#pragma unroll
            for (int c = j + 1; c <= i; ++c) A[i][c] = fma(-f, A[c][j], A[i][c]);
        }
    }
    double x[K], mu = 0.0;
#pragma unroll
    for (int j = K - 1; j >= 0; --j) {
        double t = d[j];
#pragma unroll
        for (int c = j + 1; c < K; ++c) t = fma(-A[c][j], x[c], t);
        x[j] = t * ip[j];
        mu = (lane == idx[j]) ? x[j] : mu;
    }
    return mu;
}

// size dispatch for small_spd_solve (one straight-line instantiation per size)
constexpr int SMALL_SOLVE_MAX = 6;
constexpr int AS_MAX_ITER = 64;   // active-set iteration cap (status MAX_ITER beyond)
template <int NVS, int K = SMALL_SOLVE_MAX, int KLO = 1>   // sizes KLO..K
VS_DEV double small_spd_solve_n(int k, const double* __restrict__ sP, unsigned long long mask, double rhs, int lane, int& bad) {
    if constexpr (K <= KLO) {
        return small_spd_solve<KLO, NVS>(sP, mask, rhs, lane, bad);
    } else {
        if (k == K) return small_spd_solve<K, NVS>(sP, mask, rhs, lane, bad);
        return small_spd_solve_n<NVS, K - 1, KLO>(k, sP, mask, rhs, lane, bad);
    }
}

// ------------------------------------------------------------------------------------------------
// One whole pass of dual_active_set for K active bounds, 1 <= K <= SMALL_PASS_MAX, as straight-line code: the solve of
// small_spd_solve<K> (same operations, same order, same test on the pivots) AND the update v_N = v_u,N - P[:,A] mu behind
// it.  A pass of the loop is a chain of dependent round trips, and the slowest instance of a batch-256 launch runs three of
// them while 255 compute units wait; here
//   * every LDS word of the pass -- the K (K + 1) / 2 entries of P_AA and this lane's K entries P[r][idx_q] of the active
//     columns -- is requested in ONE batch in front of the arithmetic (the scheduling barrier pins the order): one LDS round
//     trip per pass, where the loop has one in front of the solve and one per active bound behind it;
//   * the update multiplies by the wave-uniform x[q] the solve holds -- the value readlane(mu, idx_q) returns -- in
//     ascending index order with the loop's multiply-subtract: the results are bit for bit the loop's.
// The columns must be complete in LDS for this wavefront (the caller orders its own stores with wave_lds_sync).  Lane
// idx_q returns mu_q, every other lane 0; vn = the updated v for the lanes in N, v_u elsewhere.
// ------------------------------------------------------------------------------------------------
constexpr int SMALL_PASS_MAX = SMALL_SOLVE_MAX;
template <int K, int NVS>
VS_DEV double small_set_pass(const double* __restrict__ sP, unsigned long long mask, double rhs, int lane, int r, bool inN,
                             double vu, double& vn, int& bad) {
    int idx[K];
#pragma unroll
    for (int q = 0; q < K; ++q) {
        idx[q] = __ffsll((long long)mask) - 1;
        mask &= mask - 1;
    }
    double A[K][K], pc[K], d[K];
#pragma unroll
    for (int q = 0; q < K; ++q) {
#pragma unroll
        for (int c = 0; c <= q; ++c) A[q][c] = sP[idx[c] * NVS + idx[q]];  // uniform address: LDS broadcast
    }
#pragma unroll
    for (int q = 0; q < K; ++q) pc[q] = sP[idx[q] * NVS + r];              // P[r][idx_q]
#pragma unroll
    for (int q = 0; q < K; ++q) d[q] = readlane_f64(rhs, idx[q]);
    __builtin_amdgcn_sched_barrier(0);
    double ip[K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
        bad |= !(A[j][j] > 0.0);
        ip[j] = fast_rcp(A[j][j]);
#pragma unroll
        for (int i = j + 1; i < K; ++i) {
            const double f = A[i][j] * ip[j];
            d[i] = fma(-f, d[j], d[i]);
#pragma unroll
            for (int c = j + 1; c <= i; ++c) A[i][c] = fma(-f, A[c][j], A[i][c]);
        }
    }
    double x[K], mu = 0.0;
#pragma unroll
    for (int j = K - 1; j >= 0; --j) {
        double t = d[j];
#pragma unroll
        for (int c = j + 1; c < K; ++c) t = fma(-A[c][j], x[c], t);
        x[j] = t * ip[j];
        mu = (lane == idx[j]) ? x[j] : mu;
    }
    double v = vu;
#pragma unroll
    for (int q = 0; q < K; ++q)
        if (inN) v -= pc[q] * x[q];
    vn = v;
    return mu;
}

// size dispatch for small_set_pass, the small sizes first (the usual one to three saturated throttles)
template <int NVS, int KS, int K = 1>
VS_DEV double small_set_pass_n(int k, const double* __restrict__ sP, unsigned long long mask, double rhs, int lane, int r,
                               bool inN, double vu, double& vn, int& bad) {
    if constexpr (K >= KS) {
        return small_set_pass<KS, NVS>(sP, mask, rhs, lane, r, inN, vu, vn, bad);
    } else {
        if (k == K) return small_set_pass<K, NVS>(sP, mask, rhs, lane, r, inN, vu, vn, bad);
        return small_set_pass_n<NVS, KS, K + 1>(k, sP, mask, rhs, lane, r, inN, vu, vn, bad);
    }
}

// s = L22 (L^-1 g)_v, whose largest entry scales the release tolerance of the box QP (row NZ of the factor holds L^-1 g)
template <class D>
VS_DEV void schur_rhs(const double* __restrict__ Lb, double* __restrict__ sSvec, int lane) {
    constexpr int PV = D::NU >> 4;
    constexpr int GR = D::NZ - 16 * (PV + 1);  // local row of NZ in tile row PV+1
    const int r = lane < D::NV ? lane : D::NV - 1;
    const double* L76 = Lb + tile_off<D>(PV + 1, PV);
    const double* L77 = Lb + tile_off<D>(PV + 1, PV + 1);
    const double* rowp = Lb + tile_off<D>(PV + (r >> 4), PV) + (r & 15) * 17;  // L22[r][c] = rowp[(c>>4)*TS + (c&15)]
    double sr = 0.0;
#pragma unroll
    for (int c = 0; c < D::NV; ++c) {
        // tile (PV, PV+1) does not exist: that load stays inside tile row PV+1 and is masked out
        const double lrc = rowp[((c >> 4) && (r >> 4)) ? D::TS + (c & 15) : (c & 15)];
        const double ellc = c < 16 ? L76[GR * 17 + c] : L77[GR * 17 + (c - 16)];
        sr = fma(c <= r ? lrc : 0.0, ellc, sr);
    }
    if (lane < D::NV) sSvec[r] = sr;
}

// ------------------------------------------------------------------------------------------------
// Accessors of X = L22^-1 (lower triangular, NV x NV) for the dual box QP.  Entries are re-read from LDS where they are
// used instead of held in 2 NV registers: with the accumulator tiles live through P4 the box QP must stay small in
// registers, or tiles get spilled for EVERY instance.
//   XTiles  two throttle tile rows (the paper horizon): rows 0..15 are the tile X6 = inverse of the first throttle
//           diagonal tile (formed in P3), rows 16.. are formed beside the throttle sweep (dual_setup_beside_sweep) and, for
//           their first sixteen columns, at the top of the box QP (sXr[a * NVS + j] = X[16 + a][j])
//   XDense  three throttle tile rows: sXd[j * NVS + i] = X[j][i], zero above the diagonal
// col(j, r, n) = X[j][r] restricted to the rows j < n of N; pcol(b, r, n) = P[r][b] = sum_{j < n} X[j][r] X[j][b].
// ------------------------------------------------------------------------------------------------
template <class D>
struct XTiles {
    static constexpr int NVS = D::NV + 1, NR2 = D::NV - 16;
    static constexpr int KMAX = SMALL_SOLVE_MAX;   // largest system solved in registers (the accumulator tiles are in VGPRs here)
    static constexpr int KPASS = SMALL_PASS_MAX;   // largest active set that takes the straight-line pass (small_set_pass)
    static constexpr int KMID = 16;                // compact row-per-lane solver for 7..16 active bounds (mid_spd_solve): it fits
                                                   // beside the accumulator tiles without a spilled register
    const double* X6;
    const double* sXr;
    VS_DEV double col(int j, int r, int n) const {
        const double t = j < 16 ? X6[j * 17 + (r & 15)] : sXr[(j - 16) * NVS + r];
        return (j < 16 ? r < 16 : j < n) ? t : 0.0;
    }
    VS_DEV double pcol(int b, int r, int n) const {
        double p0 = 0.0, p1 = 0.0;
        if (b < 16) {  // X[j][b] = 0 for j < 16 <= b
#pragma unroll
            for (int j = 0; j < 16; j += 2) {
                p0 = fma(col(j, r, n), X6[j * 17 + b], p0);            // uniform addresses: LDS broadcasts
                p1 = fma(col(j + 1, r, n), X6[(j + 1) * 17 + b], p1);
            }
        }
#pragma unroll
        for (int a2 = 0; a2 < NR2; ++a2) p0 = fma(col(16 + a2, r, n), sXr[a2 * NVS + b], p0);
        return p0 + p1;
    }
};
template <class D>
struct XDense {
    static constexpr int NVS = D::NV + 1;
    static constexpr int KMAX = 10;                // accumulator tiles live in AGPRs at these horizons: room for 10 x 10
    static constexpr int KPASS = 0;                // no straight-line pass here: the loop as it was (with it for up to six bounds
                                                   // the 2x horizon at batch 4096 measured 0.3-0.4 % slower, outside the noise)
    static constexpr int KMID = 24;                // and for the compact row-per-lane solver up to KMID x KMID (mid_spd_solve)
    const double* sXd;
    VS_DEV double col(int j, int r, int n) const { return j < n ? sXd[j * NVS + r] : 0.0; }
    VS_DEV double pcol(int b, int r, int n) const {
        double p0 = 0.0, p1 = 0.0;
        int j = b;                                   // X[j][b] = 0 for j < b
        for (; j + 1 < n; j += 2) {
            p0 = fma(sXd[j * NVS + r], sXd[j * NVS + b], p0);
            p1 = fma(sXd[(j + 1) * NVS + r], sXd[(j + 1) * NVS + b], p1);
        }
        if (j < n) p0 = fma(sXd[j * NVS + r], sXd[j * NVS + b], p0);
        return p0 + p1;
    }
};

// ------------------------------------------------------------------------------------------------
// KMAX < K <= KMID active bounds: P_AA mu = rhs_A in registers, rows where they are (lane r = throttle r keeps
// a[q] = P[r][idx_q] for the K active indices idx_0 < idx_1 < ...: compact COLUMNS, scattered rows), Gaussian elimination
// without pivoting (SPD) with the pivot rows broadcast by v_readlane from lane idx_j (a scalar).  ~5 instructions per
// update against ~12 for the elimination on an LDS copy (three LDS operations per update) and ~2.8 k instructions for one
// iteration of the primal form on all 44 throttles, which is what instances with more than 16 violated bounds ran
// before.  Lane idx_q returns mu_q, every other lane 0.
// ------------------------------------------------------------------------------------------------
template <int KMID, int NVS>
VS_DEV double mid_spd_solve(int ka, const double* __restrict__ sP, unsigned long long Amask, double bb, int lane, bool isA,
                            int& bad) {
    int idx[KMID];
    {
        unsigned long long m = Amask;
#pragma unroll
        for (int q = 0; q < KMID; ++q) {
            idx[q] = m ? __ffsll((long long)m) - 1 : 0;   // (wave uniform: scalar registers)
            m &= m - 1;
        }
    }
    const int rank = __popcll(Amask & ((1ull << lane) - 1ull));   // compact position of this lane's throttle
    double a[KMID];
#pragma unroll
    for (int q = 0; q < KMID; ++q) a[q] = sP[idx[q] * NVS + lane];   // P[lane][idx_q] (symmetric); garbage beyond ka, unused
#pragma unroll
    for (int j = 0; j < KMID; ++j) {
        if (j < ka) {   // (guards, not `break`: an early exit keeps the loops rolled and puts a[] in scratch -- measured 2.3x slower)
            const double piv = readlane_f64(a[j], idx[j]);
            bad |= !(piv > 0.0);
            const double ip = fast_rcp(piv);
            const double bj = readlane_f64(bb, idx[j]);
            const double f = (isA && rank > j) ? a[j] * ip : 0.0;
            bb = fma(-f, bj, bb);
#pragma unroll
            for (int c = j + 1; c < KMID; ++c) {
                if (c < ka) {
                    const double pc = readlane_f64(a[c], idx[j]);
                    a[c] = fma(-f, pc, a[c]);
                }
            }
        }
    }
    double mu = 0.0;
#pragma unroll
    for (int j = KMID - 1; j >= 0; --j) {
        if (j < ka) {
            const double xj = readlane_f64(bb, idx[j]) * fast_rcp(readlane_f64(a[j], idx[j]));
            mu = (lane == idx[j]) ? xj : mu;
            bb = (isA && rank < j) ? fma(-a[j], xj, bb) : bb;
        }
    }
    return mu;
}

// orders this wavefront's LDS stores before its later LDS loads of other lanes' words, for the compiler (the hardware executes a
// wavefront's LDS operations in order: no instruction)
VS_DEV void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ------------------------------------------------------------------------------------------------
// Set-up of the dual form at two throttle tile rows, by wavefronts 1..3 BESIDE wavefront 0's throttle sweep (P4a), for
// every instance: all of its inputs (the corner tiles, X66, 1/diagonal, row NZ of the factor) are final when P3 ends, its
// outputs lie in arrays that nothing else touches before P5, and the three wavefronts have nothing else to do there.
//   wavefront 1   T = L76 X66 (NR2 x 16)                    -> sT (head of sQP, dead before the copy of P_AA is used)
//   wavefront 2   X77 = L77^-1, one column per lane          -> sXr[a * NVS + 16 + c] = X[16 + a][16 + c]
//   wavefront 3   s = L22 (L^-1 g)_v -> sSvec, then max |s|  -> sSvec[0]
// No workgroup barrier (wavefront 0 must not wait) and no value crosses from one wavefront to another in here: the barrier
// behind the violation check publishes everything.  The one product that needs two of the pieces, X76 = -X77 T, is
// left to box_qp (NR2 multiply-adds per thread and one barrier, for the instances that enter): a wavefront that forms
// more than one piece outlasts the sweep, and then every instance waits for it.  Same expressions and summation orders
// as when all of this ran at the top of box_qp (through v33): the values are bit-identical.
// ------------------------------------------------------------------------------------------------
template <class D>
VS_DEV void dual_setup_beside_sweep(int wave, int lane) {
    using S = Smem<D>;
    extern __shared__ __attribute__((aligned(16))) double smem[];
    constexpr int PV = D::PVT, NVS = D::NV + 1, NR2 = D::NV - 16;
    static_assert(S::DUALQP && NR2 >= 1 && NR2 <= 16, "two throttle tile rows");
    double* Lb = smem + S::oM;
    double* sQP = smem + S::oQP;
    double* sXr = sQP + D::NV * NVS;                              // sXr[a * NVS + j] = X[16 + a][j]
    double* sT = sQP;                                             // T = L76 X66, NR2 x 16 (dead before sK is used)
    if (wave == 1) {
        const double* X6 = smem + S::oXinv + PV * D::TS;
        const double* L76 = Lb + tile_off<D>(PV + 1, PV);
        constexpr int RND = (16 * NR2 + 63) / 64;
#pragma unroll
        for (int rd = 0; rd < RND; ++rd) {
            const int e = lane + 64 * rd;
            if (e < 16 * NR2) {
                const int a2 = e >> 4, j = e & 15;
                double t0 = 0.0, t1 = 0.0;
#pragma unroll
                for (int k = 0; k < 16; k += 2) {                     // X66[k][j] = 0 for k < j (stored zeros)
                    t0 = fma(L76[a2 * 17 + k], X6[k * 17 + j], t0);
                    t1 = fma(L76[a2 * 17 + k + 1], X6[(k + 1) * 17 + j], t1);
                }
                sT[a2 * 16 + j] = t0 + t1;
            }
        }
    } else if (wave == 2) {
        const double* sInvD = smem + S::oInvD;
        const double* L77 = Lb + tile_off<D>(PV + 1, PV + 1);
        if (lane < NR2) {
            const int c = lane;                                       // column c of X77 = L77^-1
            double x[NR2];
#pragma unroll
            for (int i = 0; i < NR2; ++i) {
                double sum = 0.0;
#pragma unroll
                for (int k = 0; k < i; ++k) sum = fma(L77[i * 17 + k], (k >= c) ? x[k] : 0.0, sum);
                const double di = sInvD[D::NU + 16 + i];
                x[i] = (i == c) ? di : ((i > c) ? -di * sum : 0.0);
                sXr[i * NVS + 16 + c] = x[i];
            }
        }
    } else {
        double* sSvec = smem + S::oSvec;
        schur_rhs<D>(Lb, sSvec, lane);
        wave_lds_sync();
        double gm = 0.0;
#pragma unroll
        for (int c = 0; c < D::NV; ++c) gm = fmax(gm, fabs(sSvec[c]));  // uniform addresses: LDS broadcasts
        wave_lds_sync();
        if (lane == 0) sSvec[0] = gm;   // every lane of this wavefront has read sSvec[0] (in-order LDS)
    }
}

// ------------------------------------------------------------------------------------------------
// Dual active-set iteration of the box QP by ONE wavefront (lane = throttle).  With N = the throttles that are not
// pinned by the hold, P = S_NN^-1 = X^T X and v_u = the sweep's solution (sZ), fixing the set A at its bounds b_A gives
// mu = P_AA^-1 (v_u,A - b_A),  v_N = v_u,N - P[:,A] mu,  gradient_A = -mu.  Only the columns of P some active set needs
// are ever formed; the |A| x |A| system is tiny for the usual one to three saturated throttles.  The sequence of active
// sets is exactly the block-pivoting sequence of the primal form.  sSvec[0] = max |s| (release tolerance).
// ------------------------------------------------------------------------------------------------
template <class D, class XA>
VS_DEV void dual_active_set(const XA& xa, bool hold, int lane, double* __restrict__ sSv, double* __restrict__ sQP,
                            const double* __restrict__ sSvec, const double* __restrict__ sVprev,
                            const double* __restrict__ sCfg, double* __restrict__ sZ, int* __restrict__ sFlags,
                            unsigned long long have0 = 0ull, unsigned long long* qt = nullptr) {
    unsigned long long qt_mark = 0;
    (void)qt; (void)qt_mark;
    VS_QP_TIC();
    constexpr int NVS = D::NV + 1;          // row stride of the LDS work arrays
    constexpr int KS = XA::KPASS;           // largest set that takes small_set_pass (0: none)
    static_assert(KS <= XA::KMAX && KS <= SMALL_PASS_MAX, "the pass has an instantiation per size");
    double* sP = sSv;                       // sP[b * NVS + i] = P[i][b] for the columns b formed so far (have0: on entry)
    double* sK = sQP;                       // working copy of P_AA
    const int r = lane < D::NV ? lane : D::NV - 1;  // lanes >= NV shadow the last row (results unused)
    const bool valid = lane < D::NV;
    const bool fixed = valid && hold && (r >= D::NV - 4);  // v0 is the trailing block
    const int n = hold ? D::NV - 4 : D::NV;
    const bool inN = valid && r < n;
    const double lo = fixed ? sVprev[r & 3] : sCfg[CFG_VMIN];    // constraintsVSMPC.cpp:351-364
    const double hi = fixed ? sVprev[r & 3] : sCfg[CFG_VMAX];
    const double gtol = 1e-10 * (1.0 + sSvec[0]);   // sSvec[0] = max |s| (see above)
    const double vu = sZ[D::NU + r];
    // Iteration 1 of the block-pivoting scheme is the solve with only the hold pin enforced: that is the
    // backward sweep that just ran.  Apply its flips here; nothing is at a bound yet, so only primal
    // violations can occur.
    int state = 0;  // 0 free, -1 at lower, +1 at upper (pinned throttles are outside N altogether)
    double v = vu;
    int best, patience = AS_PATIENCE, status = VSMPC_STATUS_MAX_ITER, iters = 1, bad = 0;
    {
        const double tolv = 1e-12 * (1.0 + fabs(v));
        const bool vlo = inN && (v < lo - tolv);
        const bool vhi = inN && (v > hi + tolv);
        best = __popcll(__ballot(vlo || vhi));
        if (vlo || vhi) state = vlo ? -1 : 1;
    }
    unsigned long long have = have0;
    for (int it = 1; it < AS_MAX_ITER; ++it) {
        iters = it + 1;
        const bool isA = inN && state != 0;
        const unsigned long long Amask = __ballot(isA);
        // columns of P for the newly active throttles: P[i][b] = sum_{j < n} X[j][i] X[j][b]
        unsigned long long need = Amask & ~have;
        have |= need;
        while (need) {
            const int b = __ffsll((long long)need) - 1;
            need &= need - 1;
            const double pb = xa.pcol(b, r, n);
            if (valid) sP[b * NVS + r] = pb;
        }
        if constexpr (KS > 0) wave_lds_sync();   // the column stores above before the hoisted loads of other lanes' words (no instruction)
        VS_QP_TOC(1);
        double bb = isA ? vu - (state < 0 ? lo : hi) : 0.0;  // right-hand side v_u,A - b_A
        double mu = 0.0;
        const int ka = __popcll(Amask);
        double vn = vu;                                      // v_N = v_u,N - P[:,A] mu
        const bool small_pass = ka >= 1 && ka <= KS;
        if (ka == 0) {
            // every bound was released again: v = v_u, no multipliers
        } else if (small_pass) {
            // few active bounds: the whole pass (solve and update) straight-line on wave-uniform values, one LDS round trip
            if constexpr (KS > 0) mu = small_set_pass_n<D::NV + 1, KS>(ka, sP, Amask, bb, lane, r, inN, vu, vn, bad);
        } else if (ka <= XA::KMAX) {
            // solved redundantly in every lane on wave-uniform values
            if constexpr (XA::KMAX > KS) mu = small_spd_solve_n<D::NV + 1, XA::KMAX, KS + 1>(ka, sP, Amask, bb, lane, bad);
        } else if (XA::KMID > 0 && ka <= XA::KMID) {
            if constexpr (XA::KMID > 0) mu = mid_spd_solve<XA::KMID, D::NV + 1>(ka, sP, Amask, bb, lane, isA, bad);
        } else {
            // K = P_AA (working copy); Gaussian elimination without pivoting (SPD) over the active indices
            if (isA) {
                unsigned long long m = Amask;
                while (m) {
                    const int c = __ffsll((long long)m) - 1;
                    m &= m - 1;
                    sK[r * NVS + c] = sP[c * NVS + r];
                }
            }
            for (unsigned long long pm = Amask; pm; pm &= pm - 1) {
                const int j = __ffsll((long long)pm) - 1;
                const double piv = sK[j * NVS + j];
                bad |= !(piv > 0.0);
                const double bj = readlane_f64(bb, j);
                if (isA && lane > j) {
                    const double f = sK[r * NVS + j] * fast_rcp(piv);
                    bb -= f * bj;
                    for (unsigned long long m = pm & (pm - 1); m; m &= m - 1) {
                        const int c = __ffsll((long long)m) - 1;
                        sK[r * NVS + c] -= f * sK[j * NVS + c];
                    }
                }
            }
            for (unsigned long long pm = Amask; pm;) {
                const int j = 63 - __clzll((long long)pm);
                pm &= ~(1ull << j);
                const double xj = readlane_f64(bb, j) * fast_rcp(sK[j * NVS + j]);
                if (lane == j) mu = xj;
                if (isA && lane < j) bb -= sK[r * NVS + j] * xj;
            }
        }
        VS_QP_TOC(2);
        if (bad) { status = VSMPC_STATUS_NUMERICAL; break; }
        if (!small_pass) {
            for (unsigned long long m = Amask; m; m &= m - 1) {
                const int b = __ffsll((long long)m) - 1;
                const double mub = readlane_f64(mu, b);
                if (inN) vn -= sP[b * NVS + r] * mub;
            }
        }
        v = vn;
        const double grad = -mu;  // gradient of the QP at the throttles that sit on a bound
        const double tolv = 1e-12 * (1.0 + fabs(v));
        const bool isF = inN && state == 0;
        const bool vlo = isF && (v < lo - tolv);
        const bool vhi = isF && (v > hi + tolv);
        const bool rlo = isA && state == -1 && grad < -gtol;
        const bool rhi = isA && state == 1 && grad > gtol;
        const bool inf = vlo || vhi || rlo || rhi;
        const unsigned long long imask = __ballot(inf);
        const int ninf = __popcll(imask);
        if (ninf == 0) { status = VSMPC_STATUS_SOLVED; break; }
        bool pick = inf;
        if (ninf < best) { best = ninf; patience = AS_PATIENCE; }
        else if (patience > 0) { --patience; }
        else { pick = inf && (lane == 63 - __clzll(imask)); }  // least-index fallback (largest index)
        if (pick) state = vlo ? -1 : (vhi ? 1 : 0);
        VS_QP_TOC(3);
    }
    VS_QP_TOC(3);
    if (valid) {
        v = fixed ? lo : (state < 0 ? lo : (state > 0 ? hi : v));  // bound variables sit exactly on their bound
        sZ[D::NU + lane] = v;
    }
    if (lane == 0) { sFlags[1] = status; sFlags[2] = iters; }
}

// ------------------------------------------------------------------------------------------------
// P4b: box QP on the throttles (constraintsVSMPC.cpp:338-365), entered only by instances whose pins-only solution violates
// a bound.  Kept small in registers (K x K systems up to 6 x 6 in registers, columns of X re-read from LDS): the
// accumulator tiles are live across it, and what it cannot hold gets spilled for every instance.  (Out of line as a
// real call it costs the slowest instance of a launch ~4 us in saved / restored registers.)  Few saturated throttles (the usual case): dual
// form, cost grows with the number of active bounds; many: primal form on the Schur complement, cost grows with the
// number of free throttles.  Called by all wavefronts (it contains workgroup barriers); result in sZ[NU..NZ), sFlags.
// Two throttle tile rows (the paper horizon): the pieces of the dual form's set-up -- T = L76 X66, X77, s, max |s| -- are NOT
// formed here: wavefronts 1..3 form them beside the throttle sweep of every instance (dual_setup_beside_sweep); an instance
// that does enter has one product (X76 = -X77 T) and one barrier in front of the columns of P.  sFlags[4] = which
// throttles the sweep left outside their box (that form only): for two to four of them the columns of P are formed one
// per wavefront behind one barrier; one column is formed by wavefront 0 without a barrier; more than four take all
// columns up front.
// ------------------------------------------------------------------------------------------------
template <class D>
VS_DEV void box_qp(int n_violated, bool hold, int wave, unsigned long long* qt = nullptr) {
    unsigned long long qt_mark = 0;
    (void)qt; (void)qt_mark;
    VS_QP_TIC();
    using S = Smem<D>;
    extern __shared__ __attribute__((aligned(16))) double smem[];
    double* sVprev = smem + S::oVprev;
    double* sInvD = smem + S::oInvD;
    double* sZ = smem + S::oZ;
    double* sSv = smem + S::oSv;
    double* sSvec = smem + S::oSvec;
    double* sCfg = smem + S::oCfg;
    int* sFlags = reinterpret_cast<int*>(smem + S::oFlags);
    double* Lb = smem + S::oM;
    double* sXinv = smem + S::oXinv;
    double* sQP = smem + S::oQP;
    // (not threadIdx.x: that would keep the work-item id register alive -- in scratch -- from the first instruction to here)
    const int lane = fresh_lane(), tid = (wave << 6) | lane;
    constexpr bool DUALQP = S::DUALQP;
    constexpr int PV = D::PVT;
    constexpr int DUAL_MAX_ACTIVE = 16;   // (10 before the register solver for mid-size active sets: take-off batch -1.4 %)
    constexpr bool DUAL3 = S::DUAL3;
    constexpr int DUAL3_MAX = 24;
    const bool few = n_violated <= (DUAL3 ? DUAL3_MAX : DUAL_MAX_ACTIVE);   // few saturated throttles: dual form
    (void)sQP; (void)sXinv; (void)sInvD;
      if (few && DUALQP) {
       if constexpr (DUALQP) {
        // ---- box QP on the throttles, dual form.  With N = the throttles that are not pinned by the hold, P = S_NN^-1
        // (S = L22 L22^T, so the factor of S_NN is the leading block of L22) and v_u = the sweep's solution, fixing the
        // set A at its bounds b_A gives  mu = P_AA^-1 (v_u,A - b_A),  v_N = v_u,N - P[:,A] mu,  gradient_A = -mu.
        // P = X^T X with X = L22^-1: rows 0..15 of X are the inverse of the first throttle diagonal tile (formed by an
        // idle wavefront during P3), the remaining rows are started beside the throttle sweep and finished below; a
        // column of P then is 24 multiply-adds per lane with no chain, and only the columns some active set needs are ever formed.  The |A| x |A| system is
        // tiny for the usual one to three saturated throttles.  The sequence of active sets is exactly the
        // block-pivoting sequence of the primal form.
        {
            // what is left of the set-up: X76 = -X77 T from the two pieces wavefronts 1 and 2 formed beside the sweep
            constexpr int NVS = D::NV + 1, NR2 = D::NV - 16;
            double* sXr = sQP + D::NV * NVS;                              // sXr[a * NVS + j] = X[16 + a][j]
            const double* sT = sQP;                                       // T = L76 X66, NR2 x 16 (dead before sK is used)
            static_assert(16 * NR2 <= D::BLOCK, "one entry of X76 per thread");
            if (tid < 16 * NR2) {
                const int a2 = tid >> 4, j = tid & 15;
                double t = 0.0;
#pragma unroll
                for (int b2 = 0; b2 < NR2; ++b2) t = fma(sXr[a2 * NVS + 16 + b2], sT[b2 * 16 + j], t);  // X77[a][b] = 0, b > a
                sXr[a2 * NVS + j] = -t;
            }
            __syncthreads();
        }
        VS_QP_TOC(0);
        static_assert(D::NU % 16 == 0 && D::NV > 16 && D::NV <= 32, "throttle block: tile aligned, two tile rows");
        const XTiles<D> xa{sXinv + PV * D::TS, sQP + D::NV * (D::NV + 1)};   // rows 16.. of X behind the copy of P_AA
        // Many violated bounds (the take-off instances enter with ten to sixteen): all columns of P up front, by all four
        // wavefronts -- 2.25 of them per thread, ~1 k cycles -- instead of one by one in the wavefront that iterates (~0.43 k each:
        // profiles/r04_v27_qp_dist_paper.txt, 24.6 k cycles for a two-iteration solve).  Same expression, same sums.
        const bool all_cols = n_violated > 4;   // workgroup-uniform
        // Two to four: the columns of the first active set (sFlags[4]: the throttles the sweep left outside their box), one
        // per wavefront, instead of one after the other in wavefront 0 while the other three wait.  Same expression, same sums.
        // (A single one stays where it was: wavefront 0 forms it without a barrier.)
        const bool first_cols = !all_cols && n_violated >= 2;   // workgroup-uniform
        if (all_cols) {
            const int n = hold ? D::NV - 4 : D::NV;
            for (int e = tid; e < D::NV * D::NV; e += D::BLOCK) {
                const int b = e / D::NV, r = e - b * D::NV;
                sSv[b * (D::NV + 1) + r] = xa.pcol(b, r, n);
            }
            __syncthreads();
        } else if (first_cols) {
            const int n = hold ? D::NV - 4 : D::NV;
            unsigned m = unsigned(sFlags[4]);            // the violation check's mask (NV <= 32 bits)
            for (int q = 0; q < wave; ++q) m &= m - 1;   // wavefront w takes the w-th violated throttle
            if (m) {
                const int b = __ffs(int(m)) - 1;
                const int r = lane < D::NV ? lane : D::NV - 1;
                const double pb = xa.pcol(b, r, n);
                if (lane < D::NV) sSv[b * (D::NV + 1) + r] = pb;
            }
            __syncthreads();
        }
        VS_QP_TOC(1);
        if (wave == 0)
            dual_active_set<D>(xa, hold, lane, sSv, sQP, sSvec, sVprev, sCfg, sZ, sFlags,
                               all_cols ? ((1ull << D::NV) - 1ull) : (first_cols ? (unsigned long long)unsigned(sFlags[4]) : 0ull),
                               qt);
       }
      } else if (few && DUAL3) {
       if constexpr (DUAL3) {
        // ---- dual form, three throttle tile rows: X = L22^-1 assembled dense in LDS from tile products,
        //   X_ii = L_ii^-1 (the first one from P3, the other two here),  X10 = -X1 (L10 X0),  X21 = -X2 (L21 X1),
        //   X20 = -X2 (L20 X0 + L21 X10)  (one round on the matrix cores, below)
        constexpr int NVS = D::NV + 1, R2 = D::NV - 32;        // throttle rows in the last tile row
        double* sXd = sQP + D::NV * NVS;                        // sXd[j * NVS + i] = X[j][i]
        double* sT0 = smem + S::oDual3T0;                       // X1 on entry (from P3); L10 X0, later L20 X0 + L21 X10
        double* sT1 = smem + S::oDual3T1;                       // X2 on entry (formed beside the sweep); L21 X1
        static_assert(S::oDual3T0 == S::oQP + 2 * D::NV * NVS, "scratch tiles behind K and X");
        const double* L10 = Lb + tile_off<D>(PV + 1, PV);
        const double* L20 = Lb + tile_off<D>(PV + 2, PV);
        const double* L21 = Lb + tile_off<D>(PV + 2, PV + 1);
        const double* X0 = sXinv + PV * D::TS;                  // from P3
        auto xd = [&](int blk_r, int blk_c) { return sXd + (16 * blk_r) * NVS + 16 * blk_c; };   // block of X, row stride NVS
        for (int e = tid; e < D::NV * NVS; e += D::BLOCK) sXd[e] = 0.0;
        if (tid < 4 * D::NV) {   // s = L22 (L^-1 g)_v (its largest entry scales the release tolerance): four threads per row,
            const int i = tid >> 2, part = tid & 3;   // every fourth term each -- one thread per row was a 44-step serial loop
            double sum = 0.0;                         // (4.4 k cycles) in front of the first barrier
            for (int k = part; k <= i; k += 4)
                sum += Lb[lower_at<D>(D::NU + i, D::NU + k)] * Lb[lower_at<D>(D::NZ, D::NU + k)];
            sSv[tid] = sum;                           // partial sums: P's array is not in use before round 6
        }
        __syncthreads();
        // ONE round for the off-diagonal blocks of X, on the matrix cores, each chain in one wavefront: an accumulator
        // (lane (g, n), register r = entry [g + 4 r][n]) IS the B operand of the next product (k-step r), so a chain of
        // products needs no LDS round trip and no barrier.  Wavefront 0: T10 = L10 X0, X10 = -X1 T10, T20 = L20 X0 + L21 X10,
        // X20 = -X2 T20; wavefront 1: T21 = L21 X1, X21 = -X2 T21; wavefront 2 copies the diagonal blocks; wavefront 3 forms
        // max |s|.  (Through v22: five barrier-separated rounds of 16-term dot products, one entry per thread: the set-up
        // of the box QP cost 14.5 k cycles.)  X2 is R2 x R2: its rows and columns beyond R2 do not exist (masked operands).
        {
            const int g = lane >> 4, n = lane & 15;
            auto a_tile = [&](const double* T, int ks) { return T[n * 17 + 4 * ks + g]; };         // A[m = n][k]
            auto b_tile = [&](const double* T, int ks) { return T[(4 * ks + g) * 17 + n]; };       // B[k][n]
            auto a_x2 = [&](int ks) {                                                              // X2 restricted to R2 x R2
                const double v = sT1[n * 17 + 4 * ks + g];
                return (n < R2 && 4 * ks + g < R2) ? v : 0.0;
            };
            const d4 zero = d4{0.0, 0.0, 0.0, 0.0};
            if (wave == 0) {
                d4 t10 = zero, x10 = zero, t20 = zero, x20 = zero;
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) t10 = __builtin_amdgcn_mfma_f64_16x16x4f64(a_tile(L10, ks), b_tile(X0, ks), t10, 0, 0, 0);
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) t20 = __builtin_amdgcn_mfma_f64_16x16x4f64(a_tile(L20, ks), b_tile(X0, ks), t20, 0, 0, 0);
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) x10 = __builtin_amdgcn_mfma_f64_16x16x4f64(a_tile(sT0, ks), t10[ks], x10, 0, 0, 0);
#pragma unroll
                for (int r = 0; r < 4; ++r) { x10[r] = -x10[r]; xd(1, 0)[(g + 4 * r) * NVS + n] = x10[r]; }
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) t20 = __builtin_amdgcn_mfma_f64_16x16x4f64(a_tile(L21, ks), x10[ks], t20, 0, 0, 0);
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) x20 = __builtin_amdgcn_mfma_f64_16x16x4f64(a_x2(ks), t20[ks], x20, 0, 0, 0);
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (g + 4 * r < R2) xd(2, 0)[(g + 4 * r) * NVS + n] = -x20[r];
            } else if (wave == 1) {
                d4 t21 = zero, x21 = zero;
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) t21 = __builtin_amdgcn_mfma_f64_16x16x4f64(a_tile(L21, ks), b_tile(sT0, ks), t21, 0, 0, 0);
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) x21 = __builtin_amdgcn_mfma_f64_16x16x4f64(a_x2(ks), t21[ks], x21, 0, 0, 0);
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (g + 4 * r < R2) xd(2, 1)[(g + 4 * r) * NVS + n] = -x21[r];
            } else if (wave == 2) {
                // the three diagonal blocks into the dense X (lower triangles; rows of the last block beyond R2 stay zero)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int i = g + 4 * r;
                    const double x0 = X0[i * 17 + n], x1 = sT0[i * 17 + n], x2 = sT1[i * 17 + n];
                    if (n <= i) {
                        xd(0, 0)[i * NVS + n] = x0;
                        xd(1, 1)[i * NVS + n] = x1;
                        if (i < R2) xd(2, 2)[i * NVS + n] = x2;
                    }
                }
            } else {
                if (lane < D::NV) sSvec[lane] = (sSv[4 * lane] + sSv[4 * lane + 1]) + (sSv[4 * lane + 2] + sSv[4 * lane + 3]);
                double gm = 0.0;
                for (int c = 0; c < D::NV; ++c) gm = fmax(gm, fabs(sSvec[c]));  // uniform addresses: LDS broadcasts
                if (lane == 0) sSvec[0] = gm;   // every lane of this wavefront has read sSvec[0] (in-order LDS)
            }
        }
        __syncthreads();
        {   // round 6: ALL of P = X_N^T X_N on the matrix cores (six lower 16 x 16 tiles, twelve k-steps each, over the four
            // wavefronts): ~2 k cycles once, where a column formed on demand inside the iteration costs one wavefront ~1.3 k
            // and an instance needs eight to twelve of them.  sP[b * NVS + i] = P[i][b], both triangles.
            static_assert(D::NV <= 48, "three tile rows");
            const int n = hold ? D::NV - 4 : D::NV;
            const int g = lane >> 4, m = lane & 15;
#pragma unroll 1
            for (int t = wave; t < 6; t += D::NWAVES) {
                const int ta = t < 1 ? 0 : (t < 3 ? 1 : 2), tb = t - ta * (ta + 1) / 2;
                const int ca = 16 * ta + m, cb = 16 * tb + m;
                double xa_[12], xb_[12];
#pragma unroll
                for (int ks = 0; ks < 12; ++ks) {
                    const int j = 4 * ks + g;
                    const double va = sXd[j * NVS + ca], vb = sXd[j * NVS + cb];   // (in range of the LDS for every lane)
                    xa_[ks] = (j < n && ca < D::NV) ? va : 0.0;
                    xb_[ks] = (j < n && cb < D::NV) ? vb : 0.0;
                }
                d4 c0 = d4{0.0, 0.0, 0.0, 0.0}, c1 = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int ks = 0; ks < 12; ks += 2) {
                    c0 = __builtin_amdgcn_mfma_f64_16x16x4f64(xa_[ks], xb_[ks], c0, 0, 0, 0);
                    c1 = __builtin_amdgcn_mfma_f64_16x16x4f64(xa_[ks + 1], xb_[ks + 1], c1, 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int i = 16 * ta + g + 4 * r;
                    const double pv = c0[r] + c1[r];
                    if (i < D::NV && cb < D::NV) {
                        sSv[cb * NVS + i] = pv;
                        sSv[i * NVS + cb] = pv;
                    }
                }
            }
        }
        __syncthreads();
        if (wave == 0) {
            const XDense<D> xa{sXd};
            dual_active_set<D>(xa, hold, lane, sSv, sQP, sSvec, sVprev, sCfg, sZ, sFlags, ~0ull);
        }
       }
      } else {
        // Schur complement S = L22 L22^T, s = L22 (L^-1 g)_v
        for (int e = tid; e < D::NV * D::NV; e += D::BLOCK) {
            const int r = e / D::NV, c = e % D::NV;
            const int kmax = r < c ? r : c;
            double sum = 0.0;
            for (int k = 0; k <= kmax; ++k)
                sum += Lb[lower_at<D>(D::NU + r, D::NU + k)] * Lb[lower_at<D>(D::NU + c, D::NU + k)];
            sSv[r * (D::NV + 1) + c] = sum;
        }
        if (tid < D::NV) {
            double sum = 0.0;
            for (int k = 0; k <= tid; ++k)
                sum += Lb[lower_at<D>(D::NU + tid, D::NU + k)] * Lb[lower_at<D>(D::NZ, D::NU + k)];
            sSvec[tid] = sum;
        }
        __syncthreads();

        if (wave == 0) {
            const int r = lane < D::NV ? lane : D::NV - 1;  // lanes >= NV shadow the last row (results unused)
            const bool valid = lane < D::NV;
            double row[D::NV];
#pragma unroll
            for (int c = 0; c < D::NV; ++c) row[c] = sSv[r * (D::NV + 1) + c];
            const double svr = sSvec[r];
            const bool fixed = valid && hold && (r >= D::NV - 4);  // v0 is the trailing block
            const double lo = fixed ? sVprev[r & 3] : sCfg[CFG_VMIN];    // constraintsVSMPC.cpp:351-364
            const double hi = fixed ? sVprev[r & 3] : sCfg[CFG_VMAX];
            int state = fixed ? -1 : 0;  // 0 free, -1 at lower, +1 at upper
            double gmax = fabs(svr);
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) gmax = fmax(gmax, __shfl_xor(gmax, o));
            const double gtol = 1e-10 * (1.0 + gmax);
            // Iteration 1 of the block-pivoting scheme is the solve with only the hold pin enforced: that is the
            // backward sweep that just ran (its throttles are in sZ).  Apply its flips here instead of repeating
            // the solve; nothing is at a bound yet, so only primal violations can occur.
            double v = sZ[D::NU + r];
            int best, patience = AS_PATIENCE, status = VSMPC_STATUS_MAX_ITER, iters = 1;
            {
                const double tolv = 1e-12 * (1.0 + fabs(v));
                const bool vlo = valid && state == 0 && (v < lo - tolv);
                const bool vhi = valid && state == 0 && (v > hi + tolv);
                best = __popcll(__ballot(vlo || vhi));
                if (vlo || vhi) state = vlo ? -1 : 1;
            }
            for (int it = 1; it < AS_MAX_ITER; ++it) {
                iters = it + 1;
                const bool isF = valid && state == 0;
                const unsigned long long Fmask = __ballot(isF);
                const double vb = isF ? 0.0 : (state < 0 ? lo : hi);
                double a[D::NV];
                double b = isF ? -svr : vb;
#pragma unroll
                for (int c = 0; c < D::NV; ++c) {
                    const bool cF = (Fmask >> c) & 1ull;
                    const double vbc = readlane_f64(vb, c);
                    if (isF && !cF) b -= row[c] * vbc;
                    a[c] = (isF && cF) ? row[c] : ((c == r && !isF) ? 1.0 : 0.0);
                }
                int bad = 0;
                const int nfree = __popcll(Fmask);
                if (nfree >= 1 && nfree <= SMALL_SOLVE_MAX) {
                    // deep saturation leaves few free throttles: S_FF v_F = b_F redundantly in registers on
                    // wave-uniform values (S is symmetric: sSv[c * (NV+1) + i] = S[i][c], the layout the solver reads)
                    const double vf = small_spd_solve_n<D::NV + 1>(nfree, sSv, Fmask, b, lane, bad);
                    v = isF ? vf : vb;
                } else {
                // Gaussian elimination without pivoting (SPD), pivot rows broadcast with v_readlane.  Rows of bound
                // throttles are identity rows whose column is zero elsewhere: their pivots are no-ops and are skipped
                // (wave-uniform branch), so the cost follows the number of free throttles
#pragma unroll
                for (int j = 0; j < D::NV; ++j) {
                    if ((Fmask >> j) & 1ull) {
                        const double piv = readlane_f64(a[j], j);
                        bad |= !(piv > 0.0);
                        const double f = (lane > j) ? a[j] * fast_rcp(piv) : 0.0;
                        const double bj = readlane_f64(b, j);
                        b -= f * bj;
#pragma unroll
                        for (int c = j + 1; c < D::NV; ++c) {
                            const double pc = readlane_f64(a[c], j);
                            a[c] -= f * pc;
                        }
                    }
                }
                v = vb;  // bound throttles; free ones follow from the back-substitution
#pragma unroll
                for (int j = D::NV - 1; j >= 0; --j) {
                    if ((Fmask >> j) & 1ull) {
                        const double xj = readlane_f64(b, j) * fast_rcp(readlane_f64(a[j], j));
                        if (lane == j) v = xj;
                        if (lane < j) b -= a[j] * xj;
                    }
                }
                }
                if (bad) { status = VSMPC_STATUS_NUMERICAL; break; }
                double grad = svr;
#pragma unroll
                for (int c = 0; c < D::NV; ++c) grad += row[c] * readlane_f64(v, c);
                const double tolv = 1e-12 * (1.0 + fabs(v));
                const bool vlo = isF && (v < lo - tolv);
                const bool vhi = isF && (v > hi + tolv);
                const bool rlo = valid && state == -1 && !fixed && grad < -gtol;
                const bool rhi = valid && state == 1 && !fixed && grad > gtol;
                const bool inf = vlo || vhi || rlo || rhi;
                const unsigned long long imask = __ballot(inf);
                const int ninf = __popcll(imask);
                if (ninf == 0) { status = VSMPC_STATUS_SOLVED; break; }
                bool pick = inf;
                if (ninf < best) { best = ninf; patience = AS_PATIENCE; }
                else if (patience > 0) { --patience; }
                else { pick = inf && (lane == 63 - __clzll(imask)); }  // least-index fallback (largest index)
                if (pick) state = vlo ? -1 : (vhi ? 1 : 0);
            }
            if (valid) {
                v = state < 0 ? lo : (state > 0 ? hi : v);  // bound variables sit exactly on their bound
                sZ[D::NU + lane] = v;
            }
            if (lane == 0) { sFlags[1] = status; sFlags[2] = iters; }
        }
      }
}

#undef VS_QP_TIC
#undef VS_QP_TOC

}  // namespace vsmpc
