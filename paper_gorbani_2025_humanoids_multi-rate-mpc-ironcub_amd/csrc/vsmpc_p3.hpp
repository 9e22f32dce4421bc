// P2 + P3 of the tuned solve kernels: the input-cost terms and the blocked Cholesky factorisation (panel streams, tile
// inverses, work lists, the pipelined and the plain schedule).
#pragma once
#include "vsmpc_p1_struct.hpp"
#include "vsmpc_smem.hpp"

namespace vsmpc {

// ------------------------------------------------------------------------------------------------
// cost terms on the condensed inputs (P2)
// ------------------------------------------------------------------------------------------------
// (sGy = Q^T b of the joint reduction; the reduced joint unknowns and the dummies have unit weights)
template <class D>
VS_DEV double input_cost_term(const double* __restrict__ sCfg, const double* __restrict__ sGy,
                              const double* __restrict__ sVprev, int gr, int gc) {
    if (gr < D::NU) return (gr == gc) ? 1.0 : 0.0;   // |y|^2 / 2 = U^T W U / 2  (costsVSMPC.cpp:375-381,564-571)
    if (gr < D::NZ) {
        if (gc < D::NU) return 0.0;
        const int q1 = gr - D::NU, q2 = gc - D::NU;
        if ((q1 & 3) != (q2 & 3)) return 0.0;
        const int b1 = v_block_of_internal<D>(q1), b2 = v_block_of_internal<D>(q2);
        if (b1 == b2)  // first-difference penalty + v0 anchor  (costsVSMPC.cpp:383-409,472-476)
            return sCfg[CFG_WTHR] * double((b1 > 0) + (b1 < D::NVB - 1)) + (b1 == 0 ? sCfg[CFG_WINIT] : 0.0);
        const int db = b1 - b2;
        return (db == 1 || db == -1) ? -sCfg[CFG_WTHR] : 0.0;
    }
    if (gr == D::NZ && gc < D::NZ) {  // gradient row
        if (gc < D::NU) return gc < D::NUY ? sGy[gc % NJC] : 0.0;                   // costsVSMPC.cpp:586-590, reduced
        const int q = gc - D::NU;
        return v_block_of_internal<D>(q) == 0 ? -sCfg[CFG_WINIT] * sVprev[q & 3] : 0.0;  // costsVSMPC.cpp:479-485
    }
    return 0.0;
}

// Debug / parity dumps of the diagnostic instantiation, one accumulator slot each (C/D fragment: row (lane >> 4) + 4 r,
// column lane & 15), into the instance's NP x NP matrix.  Which slots are dumped is the caller's business (TileTab).
// The augmented condensed Hessian before factorisation: tile (ti, tj) as P1 left it + the input-cost terms P2 adds (diagonal
// tiles and the throttle rows), lower triangle
template <class D>
VS_DEV void dump_hessian_tile(double* __restrict__ Mi, int ti, int tj, d4 tile, const double* __restrict__ sCfg,
                              const double* __restrict__ sGy, const double* __restrict__ sVprev, int lane) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int gr = 16 * ti + (lane >> 4) + 4 * r, gc = 16 * tj + (lane & 15);
        if (ti == tj || ti >= D::PVT) tile[r] += input_cost_term<D>(sCfg, sGy, sVprev, gr, gc);
        if (gc <= gr) Mi[size_t(gr) * D::NP + gc] = tile[r];
    }
}
// The factor: a tile below the diagonal of a joint column, from the registers that hold it after P3 (the diagonal tiles are
// written while they are panels, the throttle corner from LDS)
template <class D>
VS_DEV void dump_factor_tile(double* __restrict__ Li, int ti, int tj, const d4& tile, int lane) {
#pragma unroll
    for (int r = 0; r < 4; ++r) Li[size_t(16 * ti + (lane >> 4) + 4 * r) * D::NP + 16 * tj + (lane & 15)] = tile[r];
}

// ------------------------------------------------------------------------------------------------
// P3 panel factorisation in C++ by ONE wavefront, branch-free: lane l owns panel row 16p + l (lanes 0..15 = the diagonal
// tile).  Pivot-column entries are broadcast with v_readlane.  The only panel it still factors is the LAST one of a horizon
// whose pivot count NPIV has no generated stream (tools/gen_panel_asm.py LAST_PANEL_PIVOTS); the remaining rows of that tile
// (gradient row, padding) are carried along as ordinary panel rows.  `Lb` is the LDS tile storage of the panel column (ring
// of two columns + throttle corner, tile_off_c).  It is also the arithmetic the generated streams reproduce operation by
// operation.  Returns non-zero if a pivot was not positive.
// ------------------------------------------------------------------------------------------------
template <class D, int NPIV>
VS_DEV int panel_factor(double* __restrict__ Lb, double* __restrict__ sInvD, int p, int lane) {
    const int r = 16 * p + lane;
    const bool ok = r < D::NP;
    double* T = Lb + tile_off<D>(ok ? (r >> 4) : p, p) + (r & 15) * 17;  // rows beyond the matrix read an in-range tile
    double a[16];                                                          // and are never stored
#pragma unroll
    for (int c = 0; c < 16; ++c) a[c] = T[c];
    double dmin = 1.0;     // all pivots positive <=> min(pivots) > 0; a NaN pivot (fmin skips it) makes every later
                           // pivot and the last reciprocal square root NaN, which is checked at the end
    double inv_mine = 1.0, inv_last = 1.0;   // lane j keeps 1/L_jj (a select per pivot, no branch on the pivot chain)
    // software-pipelined pivots: the next pivot is complete as soon as the first column of this pivot's update is
    // done, so its reciprocal square root (a ~75-cycle dependent chain) is issued there and overlaps the rest of the
    // update instead of following it
    double d = readlane_f64(a[0], 0);
    double inv = fast_rsqrt(d);
#pragma unroll
    for (int j = 0; j < NPIV; ++j) {
        dmin = fmin(dmin, d);
        inv_mine = lane == j ? inv : inv_mine;
        inv_last = inv;
        const double l = a[j] * inv;
        a[j] = l;
        if (j + 1 < 16) {
            a[j + 1] = fma(-l, readlane_f64(l, j + 1), a[j + 1]);
            if (j + 1 < NPIV) {
                d = readlane_f64(a[j + 1], j + 1);
                inv = fast_rsqrt(d);
            }
        }
#pragma unroll
        for (int c = j + 2; c < 16; ++c) a[c] = fma(-l, readlane_f64(l, c), a[c]);
    }
    if (ok) {  // above its diagonal the diagonal tile holds leftovers: readers mask it
#pragma unroll
        for (int c = 0; c < 16; ++c) T[c] = a[c];
    }
    if (lane < NPIV) sInvD[16 * p + lane] = inv_mine;
    return !(dmin > 0.0) || !(inv_last == inv_last);
}

// ------------------------------------------------------------------------------------------------
// The panel streams as hand-scheduled assembly with DPP broadcasts (kernel v26; tools/gen_panel_asm.py has the why: a lone
// wavefront issues one FP64 instruction per ~5.5 cycles whatever the dependencies, so a stream costs its instruction
// count, and v_fmac_f64 with DPP row_newbcast needs two instructions per updated column where v_readlane needs three).
// Lane 16 r + c of wavefront w carries panel row 16 p + 16 + 64 w + 16 r + c -- all 64 lanes carry rows BELOW the diagonal
// tile -- and, in a second set of registers, row c of the diagonal tile, which every 16-lane row factors redundantly
// (bit-identical in all rows and wavefronts).  Same arithmetic as panel_factor, operation by operation; in isolation
// 2.7 k cycles against 3.9 k for the C++ stream (tools/microbench/panel_probe.hip, which keeps its own copy of that
// stream; profiles/r04_microbench_panel_probe.txt).
// ------------------------------------------------------------------------------------------------
#include "vsmpc_panel_asm.inc"
VS_DEV unsigned lds_addr(const double* q) { return unsigned(reinterpret_cast<uintptr_t>(q)); }   // flat -> LDS byte address

// Panel p < NT - 1, wavefront w of those that share it, S row slots per lane: rows 16 p + 16 + 64 (S w + s) + lane of the
// panel column; the factored diagonal tile comes back in `diag` (lanes 0..15) and 1 / L_jj goes to sInvD from wavefront 0.
// `scratch` = 32 doubles of this wavefront nobody reads: rows beyond the matrix and the other wavefronts' 1 / L_jj end there.
// Returns non-zero if a pivot was not positive (its reciprocal square root is NaN, and then so is everything after it down
// to the last one).
// KB > 0: the variant with a workgroup barrier inside (s_barrier behind pivot KB of the diagonal tile, the rows below are
// loaded behind it): the caller's other wavefronts execute a matching __syncthreads().
template <class D, int S = 1, int KB = 0>
VS_DEV int panel_dpp(double* __restrict__ Lb, double* __restrict__ sInvD, int p, int lane, int w, double (&diag)[16],
                      double* scratch) {
    unsigned ld[S], st[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const int r = 16 * p + 16 + 64 * (S * w + s) + lane;
        const bool ok = r < D::NP;
        ld[s] = lds_addr(Lb + tile_off<D>(ok ? (r >> 4) : p, p) + (r & 15) * 17);
        st[s] = ok ? ld[s] : lds_addr(scratch);
    }
    const unsigned dg = lds_addr(Lb + tile_off<D>(p, p) + (lane & 15) * 17);
    const unsigned iv = lds_addr(w == 0 ? sInvD + 16 * p : scratch + 16);
    double inv_last;
    static_assert(S >= 1 && S <= 3, "tools/gen_panel_asm.py generates one, two and three row slots");
    static_assert(KB == 0 || (S == 1 && KB == 3) || (S == 2 && (KB == 3 || KB == 6)) || (S == 3 && KB == 6), "tools/gen_panel_asm.py BARRIER_VARIANTS");
    if constexpr (S == 1 && KB == 0) panel16x1_dpp(ld[0], st[0], dg, iv, diag, inv_last);
    else if constexpr (S == 2 && KB == 0) panel16x2_dpp(ld[0], st[0], ld[1], st[1], dg, iv, diag, inv_last);
    else if constexpr (S == 3 && KB == 0) panel16x3_dpp(ld[0], st[0], ld[1], st[1], ld[2], st[2], dg, iv, diag, inv_last);
    else if constexpr (S == 1) panel16x1_b3_dpp(ld[0], st[0], dg, iv, diag, inv_last);
    else if constexpr (S == 2 && KB == 3) panel16x2_b3_dpp(ld[0], st[0], ld[1], st[1], dg, iv, diag, inv_last);
    else if constexpr (S == 2) panel16x2_b6_dpp(ld[0], st[0], ld[1], st[1], dg, iv, diag, inv_last);
    else panel16x3_b6_dpp(ld[0], st[0], ld[1], st[1], ld[2], st[2], dg, iv, diag, inv_last);
    return !(inv_last == inv_last);
}
// The joint panel column whose diagonal tile ends in the eight dummy unknowns (rows NUY .. NU - 1: unit diagonal, exactly zero
// coupling -- P2 and the zero operands of p1s_entries), one wavefront, one row slot: only pivots and columns 0..7 are
// factored.  Pivots 8..15 of the full stream would be 1 - (signed zeros) = 1 with 1 / L_jj = 1, and every update they or the
// first eight pivots make to columns 8..15 subtracts a signed zero: the tile and the rows below come out as the sixteen-pivot
// stream leaves them, up to the sign of zero (the dummy block of L is the identity), in 1.2 k modelled cycles instead of 2.8 k.
template <class D, int P>
VS_DEV int panel_dummy_dpp(double* __restrict__ Lb, double* __restrict__ sInvD, int lane, double (&diag)[16],
                           double* scratch) {
    static_assert(D::NU - D::NUY == 8 && 16 * P + 16 == D::NU && D::NP - D::NU <= 64,
                  "tools/gen_panel_asm.py JOINT_DUMMY_PIVOTS: eight dummy unknowns at the end of this column, one row slot below");
    const int r = 16 * P + 16 + lane;
    const bool ok = r < D::NP;
    const unsigned ld = lds_addr(Lb + tile_off<D>(ok ? (r >> 4) : P, P) + (r & 15) * 17);
    const unsigned st = ok ? ld : lds_addr(scratch);
    double inv_last;
    panel8x1_dpp(ld, st, lds_addr(Lb + tile_off<D>(P, P) + (lane & 15) * 17), lds_addr(sInvD + 16 * P), diag, inv_last);
    if (lane >= 8 && lane < 16) sInvD[16 * P + lane] = 1.0;
    return !(inv_last == inv_last);
}

// The last panel (one wavefront): NPIV pivots, the remaining rows of the tile (gradient row, padding) are ordinary rows.
template <class D, int NPIV>
VS_DEV int panel_last_dpp(double* __restrict__ Lb, double* __restrict__ sInvD, int lane) {
    constexpr int p = D::NT - 1;
    double g[16], inv_last;
    double* T = Lb + tile_off<D>(p, p) + (lane & 15) * 17;
    static_assert(NPIV == 8 || NPIV == 12, "tools/gen_panel_asm.py LAST_PANEL_PIVOTS");
    if constexpr (NPIV == 8) panel_last8_dpp(lds_addr(T), lds_addr(sInvD + 16 * p), g, inv_last);
    else panel_last12_dpp(lds_addr(T), lds_addr(sInvD + 16 * p), g, inv_last);
    if (lane < 16) {
#pragma unroll
        for (int c = 0; c < 16; ++c) T[c] = g[c];
    }
    return !(inv_last == inv_last);
}

// Long horizons (one wavefront per SIMD, 512 registers per lane): the accumulator tiles belong in the AGPR half of the
// register file for all of P2..P5.  Left to itself the allocator parked about half of the 30 tiles of a wavefront in scratch
// and reloaded them around every trailing update (1.3 GB of scratch writes per 4096-instance launch of the 2x horizon,
// profiles/r03_v14_c4_h2x4096_summary.md).  An empty asm statement with "a" constraints on fifteen tiles at once (an asm
// statement takes thirty operands, a read-write one counts twice) says so at the phase boundaries.
template <int TPW>
VS_DEV void pin_tiles_agpr(d4 (&acc)[TPW]) {
    constexpr int G = 15;
#pragma unroll
    for (int b = 0; b + G <= TPW; b += G)
        asm volatile("" : "+a"(acc[b]), "+a"(acc[b + 1]), "+a"(acc[b + 2]), "+a"(acc[b + 3]), "+a"(acc[b + 4]), "+a"(acc[b + 5]),
                          "+a"(acc[b + 6]), "+a"(acc[b + 7]), "+a"(acc[b + 8]), "+a"(acc[b + 9]), "+a"(acc[b + 10]),
                          "+a"(acc[b + 11]), "+a"(acc[b + 12]), "+a"(acc[b + 13]), "+a"(acc[b + 14]));
#pragma unroll
    for (int q = (TPW / G) * G; q < TPW; ++q) asm volatile("" : "+a"(acc[q]));
}

// ------------------------------------------------------------------------------------------------
// P2 + P3 for wavefront W, straight-line: the panel index and the tile table are compile-time, so every
// "does this tile take part" decision folds away and every LDS offset is an immediate.
//   P2  input-cost terms (joint weights, throttle coupling, gradient row) are added to the SYRK
//       accumulators in registers;
//   P3  right-looking blocked Cholesky with a register-resident trailing matrix AND a register-resident factor:
//       a tile goes to LDS exactly once, when its tile column becomes the panel (ring of two columns, see
//       Dims); the panel is factored in LDS (panel_dpp); every wavefront updates the tiles it owns with four
//       v_mfma_f64_16x16x4_f64 per tile and takes the finished tiles of the panel column it owns BACK into the
//       accumulator registers that held them, where the back-substitution of P5 finds them.
// All instantiations execute the same number of workgroup barriers.
// ------------------------------------------------------------------------------------------------
// X = L_pp^-1 of one factored diagonal tile by one wavefront: lane j carries column j (lanes >= 16 shadow), the
// entries of L_pp and 1/L_ii are wave-uniform LDS broadcasts.  X is stored like a tile: X[i][j] at i*17 + j.
template <class D>
VS_DEV void tile_inverse(const double* __restrict__ Lpp, const double* __restrict__ invd, double* __restrict__ X,
                         int lane) {
    const int j = lane & 15;
    double x[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        double s0 = 0.0, s1 = 0.0;
#pragma unroll
        for (int k = 0; k + 1 < i; k += 2) {
            s0 = fma(Lpp[i * 17 + k], x[k], s0);
            s1 = fma(Lpp[i * 17 + k + 1], x[k + 1], s1);
        }
        if (i & 1) s0 = fma(Lpp[i * 17 + i - 1], x[i - 1], s0);
        const double di = invd[i];
        x[i] = (i == j) ? di : -di * (s0 + s1);  // rows above the diagonal come out as (signed) zeros
    }
    if (lane < 16) {
#pragma unroll
        for (int i = 0; i < 16; ++i) X[i * 17 + j] = x[i];
    }
}

// rows I0 .. I1 - 1 of tile_inverse, resumable: x carries the column of this lane between calls (rows < I0 done before)
template <int I0, int I1>
VS_DEV void tile_inverse_rows(const double* __restrict__ Lpp, const double* __restrict__ invd, double (&x)[16], int lane) {
    const int j = lane & 15;
#pragma unroll
    for (int i = I0; i < I1; ++i) {
        double s0 = 0.0, s1 = 0.0;
#pragma unroll
        for (int k = 0; k + 1 < i; k += 2) {
            s0 = fma(Lpp[i * 17 + k], x[k], s0);
            s1 = fma(Lpp[i * 17 + k + 1], x[k + 1], s1);
        }
        if (i & 1) s0 = fma(Lpp[i * 17 + i - 1], x[i - 1], s0);
        const double di = invd[i];
        x[i] = (i == j) ? di : -di * (s0 + s1);
    }
}

// Compile-time work lists of wavefront W: for every panel p the slots whose tile lies right of the panel column
// (trailing update), and for every tile row r the slots whose tile (r, q), q < min(r, PVT), is kept in registers
// after P3 (back-substitution).
template <class D, int TPW, int W, bool PIPE = false>
struct WaveLists {
    int ntrail[D::NT];
    int trail[D::NT][TPW];
    int nrow[D::NT];
    int row[D::NT][TPW];
    // PIPE: the update of panel p in two parts -- the tiles of column p + 1 (the next panel: `first`, on the critical path)
    // and everything right of it (`rest`, under the next panel's stream)
    int nfirst[D::NT];
    int first[D::NT][TPW];
    int nrest[D::NT];
    int rest[D::NT][TPW];
    constexpr WaveLists() : ntrail{}, trail{}, nrow{}, row{}, nfirst{}, first{}, nrest{}, rest{} {
        constexpr TileTab<D, PIPE> tab{};
        for (int p = 0; p < D::NT; ++p) {
            for (int q = 0; q < TPW; ++q) {
                const int t = q * D::NWAVES + W;
                if (!tab.holds(t, W)) continue;
                if (tab.tj[t] > p) trail[p][ntrail[p]++] = q;
                if (tab.tj[t] == p + 1) first[p][nfirst[p]++] = q;
                if (tab.tj[t] > p + 1) rest[p][nrest[p]++] = q;
                if (tab.ti[t] == p && tab.tj[t] < p && tab.tj[t] < D::PVT) row[p][nrow[p]++] = q;
            }
        }
    }
};

// VS_DIAG_P3 (measurement builds, with the stamps instantiation): where P3's cycles go, seen from wavefront 0 -- panel
// stream, wait at the barrier behind it, diagonal store + reloads + trailing update, wait at the barrier behind that.
// Reported by tools/gpu_phases.py in place of the P1 detail rows.
#ifdef VS_DIAG_P3
__shared__ unsigned long long vs_diag_p3[4];
#define VS_P3_MARK(i)                                                                                 \
    do {                                                                                              \
        if (DEBUG && W == 0) {                                                                        \
            const unsigned long long now_ = __builtin_amdgcn_s_memtime();                             \
            if (lane == 0) vs_diag_p3[i] += now_ - p3_mark;                                           \
            p3_mark = now_;                                                                           \
        }                                                                                             \
    } while (0)
#else
#define VS_P3_MARK(i) do { } while (0)
#endif
// PIPE: acc[q] -= L_ip L_jp^T for the slots of one work list of wavefront W (KIND 1: the tiles of column PP + 1, which are
// then handed to LDS as the next panel; KIND 2: everything right of it), panel column PP in LDS.  Two tiles at a time:
// independent v_mfma_f64_16x16x4_f64 issue every 64 cycles, a dependent one every ~95 -- since the pipelined schedule put
// these chains on the critical path (first) or beside a panel stream that is no longer than they are (rest), that matters.
// The operands of the next pair are requested before the chains of the current one.
// KIND 1: the tiles of column PP + 1 (3: only its diagonal tile, 4: all but the diagonal tile), 2: everything right of it
template <class D, int TPW, int W, int PP, int KIND>
constexpr int pipe_slot(int a) {
    constexpr WaveLists<D, TPW, W, true> wl{};
    constexpr TileTab<D, true> tab{};
    if (KIND == 2) return a < wl.nrest[PP] ? wl.rest[PP][a] : -1;
    int k = 0;
    for (int b = 0; b < wl.nfirst[PP]; ++b) {
        const int t = wl.first[PP][b] * D::NWAVES + W;
        const bool dg = tab.ti[t] == tab.tj[t];
        if (KIND == 1 || (KIND == 3 && dg) || (KIND == 4 && !dg)) {
            if (k == a) return wl.first[PP][b];
            ++k;
        }
    }
    return -1;
}
template <class D, int TPW, int W, int PP, int KIND>
constexpr int pipe_count() {
    int n = 0;
    while (n < TPW && pipe_slot<D, TPW, W, PP, KIND>(n) >= 0) ++n;
    return n;
}
// the most tiles any of the wavefronts 1..3 has to update between the barrier that says "diagonal tile of column PP + 1
// ready" and the one inside the next panel stream (decides how far into the stream that barrier sits)
template <class D, int TPW, int PP>
constexpr int pipe_max_others() {
    const int n1 = pipe_count<D, TPW, 1, PP, 4>(), n2 = pipe_count<D, TPW, 2, PP, 4>(), n3 = pipe_count<D, TPW, 3, PP, 4>();
    return n1 > n2 ? (n1 > n3 ? n1 : n3) : (n2 > n3 ? n2 : n3);
}
template <class D, int TPW, int W, int PP, int KIND>
VS_DEV void pipe_update(d4 (&acc)[TPW], double* __restrict__ sM, int lrow, int crow) {
    constexpr TileTab<D, true> tab{};
    constexpr int n = pipe_count<D, TPW, W, PP, KIND>();
    double la[2][2][4], lb[2][2][4];   // [buffer][tile of the pair][k-step]
    auto request = [&](auto acst) __attribute__((always_inline)) {
        constexpr int a = decltype(acst)::value;   // first tile of the pair
        static_for<0, 2>([&](auto ucst) __attribute__((always_inline)) {
            constexpr int u = decltype(ucst)::value;
            if constexpr (a + u < n) {
                constexpr int t = pipe_slot<D, TPW, W, PP, KIND>(a + u) * D::NWAVES + W;
                const double* Lip = sM + tile_off_c<D>(tab.ti[t], PP) + lrow;
                const double* Ljp = sM + tile_off_c<D>(tab.tj[t], PP) + lrow;
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) { la[(a >> 1) & 1][u][ks] = -Lip[4 * ks]; lb[(a >> 1) & 1][u][ks] = Ljp[4 * ks]; }
            }
        });
    };
    request(std::integral_constant<int, 0>{});
    static_for<0, (TPW + 1) / 2>([&](auto hcst) __attribute__((always_inline)) {
        constexpr int a = 2 * decltype(hcst)::value;
        if constexpr (a < n) {
            request(std::integral_constant<int, a + 2>{});
            constexpr int q0 = pipe_slot<D, TPW, W, PP, KIND>(a), q1 = pipe_slot<D, TPW, W, PP, KIND>(a + 1 < n ? a + 1 : a);
            constexpr int b = (a >> 1) & 1;
            if constexpr (a + 1 < n) {
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) {
                    acc[q0] = __builtin_amdgcn_mfma_f64_16x16x4f64(la[b][0][ks], lb[b][0][ks], acc[q0], 0, 0, 0);
                    acc[q1] = __builtin_amdgcn_mfma_f64_16x16x4f64(la[b][1][ks], lb[b][1][ks], acc[q1], 0, 0, 0);
                }
            } else if constexpr (KIND == 2 || KIND == 1) {
#pragma unroll
                for (int ks = 0; ks < 4; ++ks)
                    acc[q0] = __builtin_amdgcn_mfma_f64_16x16x4f64(la[b][0][ks], lb[b][0][ks], acc[q0], 0, 0, 0);
            } else {   // (long horizons) a lone tile on the critical path: two chains of two, summed (a dependent step costs ~95 cycles, not 64)
                d4 c2 = d4{0.0, 0.0, 0.0, 0.0};
                acc[q0] = __builtin_amdgcn_mfma_f64_16x16x4f64(la[b][0][0], lb[b][0][0], acc[q0], 0, 0, 0);
                c2 = __builtin_amdgcn_mfma_f64_16x16x4f64(la[b][0][1], lb[b][0][1], c2, 0, 0, 0);
                acc[q0] = __builtin_amdgcn_mfma_f64_16x16x4f64(la[b][0][2], lb[b][0][2], acc[q0], 0, 0, 0);
                c2 = __builtin_amdgcn_mfma_f64_16x16x4f64(la[b][0][3], lb[b][0][3], c2, 0, 0, 0);
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[q0][r] += c2[r];
            }
            if constexpr (KIND != 2) {
                static_for<0, 2>([&](auto ucst) __attribute__((always_inline)) {
                    constexpr int u = decltype(ucst)::value;
                    if constexpr (a + u < n) {
                        constexpr int q = u ? q1 : q0;
                        double* T = sM + tile_off_c<D>(tab.ti[q * D::NWAVES + W], PP + 1) + crow;
#pragma unroll
                        for (int r = 0; r < 4; ++r) T[4 * r * 17] = acc[q][r];
                    }
                });
            }
        }
    });
}

// X = L_pp^-1 by the DPP rows stream on the identity (tools/gen_panel_asm.py, stream_inverse): 234 instructions, ~1.3 k cycles
// against ~2.5 k for tile_inverse (LDS broadcast + FMA pairs)
VS_DEV void tile_inverse_dpp(const double* __restrict__ Lpp, const double* __restrict__ invd, double* __restrict__ X, int lane) {
    panel_inverse_dpp(lds_addr(Lpp + (lane & 15) * 17), lds_addr(invd), lds_addr(X + (lane & 15)), lane & 15);
}

// Which of the wavefronts 1..3 inverts the diagonal tile of panel p - 1 while panel p is streamed (PIPE): the one with the
// fewest tiles in the update that runs beside it.
template <class D, int TPW>
constexpr int pipe_inverse_wave(int p) {
    constexpr WaveLists<D, TPW, 1, true> w1{};
    constexpr WaveLists<D, TPW, 2, true> w2{};
    constexpr WaveLists<D, TPW, 3, true> w3{};
    const int n1 = w1.nrest[p - 1], n2 = w2.nrest[p - 1], n3 = w3.nrest[p - 1];
    return (n3 <= n1 && n3 <= n2) ? 3 : (n2 <= n1 ? 2 : 1);
}

// P2 for the slots of PLAN (see p1s_entries): the input-cost terms are added to the entries in registers.
template <class D, int TPW, int W, bool PIPE, class PLAN>
VS_DEV void p2_terms(const double* __restrict__ sCfg, d4 (&acc)[TPW], const double* __restrict__ sGy,
                     const double* __restrict__ sVprev, int lane) {
    constexpr TileTab<D, PIPE> tab{};
    constexpr int PVT = D::PVT;
    // ---- P2: the input-cost terms, by kind of tile (compile time).  A joint diagonal tile gets the joint weights on its
    // diagonal, a tile of throttle rows x joint columns only the regularisation term of the gradient row, and only the
    // throttle x throttle tiles go through the general (branchy) input_cost_term.  (Through v13 every element of every
    // such tile went through it: 23k instructions of control flow at the 2x horizon, whose saved execution masks were what
    // pushed scalar registers into vector lanes and accumulator tiles into scratch.)
    static_for<0, PLAN::count>([&](auto qcst) __attribute__((always_inline)) {
        constexpr int q = PLAN::slot(decltype(qcst)::value);
        constexpr int t = q * D::NWAVES + W;
        if constexpr (PLAN::forms(q)) {
            constexpr int ti = tab.ti[t], tj = tab.tj[t];
            if constexpr (ti == tj && 16 * ti + 16 <= D::NU) {
                // unit weights on the reduced joint unknowns (U^T W U / 2 = |y|^2 / 2 + |n|^2 / 2, costsVSMPC.cpp:375-381,
                // 564-571 through the joint reduction) and on the dummy unknowns behind them
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[q][r] += ((lane >> 4) + 4 * r == (lane & 15)) ? 1.0 : 0.0;
            } else if constexpr (ti >= PVT && 16 * tj + 16 <= D::NU) {
                if constexpr (ti == D::NT - 1) {   // the gradient row: Q^T b, b = w_reg W^(-1/2) q_err (costsVSMPC.cpp:586-590)
                    const int gc = 16 * tj + (lane & 15);
                    const double gv = sGy[gc % NJC];
                    const double gq = gc < D::NUY ? gv : 0.0;
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[q][r] += (16 * ti + (lane >> 4) + 4 * r == D::NZ) ? gq : 0.0;
                }
            } else if constexpr (ti == tj || ti >= PVT) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    acc[q][r] += input_cost_term<D>(sCfg, sGy, sVprev, 16 * ti + (lane >> 4) + 4 * r, 16 * tj + (lane & 15));
            }
        }
    });
}

// ------------------------------------------------------------------------------------------------
// The small-batch kind (solve_kernel_small): when a wavefront forms which of its tiles.  Nothing of P1s lies under the ring
// there (Smem<D, true>), so only what the first streams need is formed in front of them:
//   instalment 0  in front of stream 0: tile column 0, dealt over all four wavefronts -- wavefronts 1..3 form the column-0
//                 tiles they will later hold (in the slots the factors come back to), wavefront 0 takes two of wavefront 1's
//                 (wavefront 1 holds one more than the others) -- each adds its P2 term and stores the tile into ring slot 0
//   instalment 1  wavefronts 1..3 beside stream 0 (which wavefront 0 runs alone, in two row slots): first the contraction sAc
//                 (p1s_contract_beside: 192 threads, three rounds -- the shipped kernels run it on all threads behind a barrier of
//                 its own in front of the entries), then tile column 1, which the update between streams 0 and 1 needs, and
//                 the next tiles in slot order up to SMALL_BESIDE0 per wavefront.  None of them reads sAc.
//   instalment 2  wavefronts 1..3 beside stream 1, in front of rest-update(0), the first update that touches them: the rest,
//                 the three throttle x throttle tiles among them (small_ac_tiles_last), which read sAc behind the barrier
//                 that closes stream 0
// Per tile the order of operations is the shipped one: entries, P2 term, panel updates 0, 1, ...  Two barriers of the shipped
// kernel do not exist here, in any of the four wavefront copies: the one behind the contraction, and the first one of
// cholesky_wave, which would follow the barrier behind instalment 0 with nothing in between.
// SMALL_BESIDE0, measured with the contraction in instalment 1 (profiles/small_offpath_phase_cycles.txt): 3 makes instalment 2
// and rest-update(0) outlast stream 1 (P3 +1.0 k cycles), 5 takes 0.16 k off P3 but not off the launch (30.47-30.55 us against
// 30.21-30.43 in alternation).
// ------------------------------------------------------------------------------------------------
constexpr int SMALL_BESIDE0 = 4;
template <class D>
constexpr bool small_wave0_forms(int ti) {   // column-0 tiles wavefront 0 forms in place of their holder, wavefront 1
    return ti % (D::NWAVES - 1) == 0 && ti / (D::NWAVES - 1) < (D::NT + 1) / 4;
}
template <class D, int TPW, int W>
constexpr int small_instalment(int q) {      // -1: this wavefront never forms slot q
    constexpr TileTab<D, true> tab{};
    const int t = q * D::NWAVES + W;
    if (!tab.ok(t)) return -1;
    if (W == 0) return small_wave0_forms<D>(tab.ti[t]) ? 0 : -1;
    if (tab.tj[t] == 0) return (W == 1 && small_wave0_forms<D>(tab.ti[t])) ? -1 : 0;
    int n = 0;
    for (int b = 0; b < q; ++b) n += (tab.ok(b * D::NWAVES + W) && tab.tj[b * D::NWAVES + W] > 0) ? 1 : 0;
    // a throttle x throttle tile reads sAc, which is formed at the head of instalment 1: never before instalment 2 (at the paper
    // horizon the count puts them there anyway; shorter horizons have too few tiles for that).  None is in column 1, which
    // has to be formed beside stream 0: has_small_kind asks for PVT >= 2
    if (tab.ti[t] >= D::PVT && tab.tj[t] >= D::PVT) return 2;
    return (tab.tj[t] == 1 || n < SMALL_BESIDE0) ? 1 : 2;
}
template <class D, int TPW, int W, int INST>
struct SmallPlan {
    static constexpr bool SMALL = true;
    static constexpr int count_() {
        int n = 0;
        for (int q = 0; q < TPW; ++q) n += small_instalment<D, TPW, W>(q) == INST ? 1 : 0;
        return n;
    }
    static constexpr int count = count_();
    static constexpr int slot(int a) {
        for (int q = 0; q < TPW; ++q)
            if (small_instalment<D, TPW, W>(q) == INST && a-- == 0) return q;
        return 0;
    }
    static constexpr bool forms(int) { return true; }
};
// every tile is formed exactly once: column 0 by the four wavefronts together, the others by their holders
template <class D, int TPW>
constexpr bool small_plan_complete() {
    constexpr TileTab<D, true> tab{};
    int col0[D::NT] = {};
    for (int q = 0; q < TPW; ++q) {
        const int i0 = small_instalment<D, TPW, 0>(q);
        if (i0 >= 0) col0[tab.ti[q * D::NWAVES]] += 1;
        const int inst[3] = {small_instalment<D, TPW, 1>(q), small_instalment<D, TPW, 2>(q), small_instalment<D, TPW, 3>(q)};
        for (int w = 1; w < D::NWAVES; ++w) {
            const int t = q * D::NWAVES + w;
            if (!tab.ok(t)) continue;
            if (tab.tj[t] == 0) col0[tab.ti[t]] += inst[w - 1] == 0 ? 1 : 0;
            else if (inst[w - 1] < 1) return false;
        }
    }
    for (int i = 0; i < D::NT; ++i)
        if (col0[i] != 1) return false;
    return true;
}
// every tile that reads sAc (throttle x throttle) is formed in instalment 2: sAc itself is formed beside stream 0, at the head
// of instalment 1 (p1s_contract_beside), and the barrier that closes that stream is the first one behind it
template <class D, int TPW>
constexpr bool small_ac_tiles_last() {
    constexpr TileTab<D, true> tab{};
    for (int q = 0; q < TPW; ++q) {
        const int inst[D::NWAVES] = {small_instalment<D, TPW, 0>(q), small_instalment<D, TPW, 1>(q), small_instalment<D, TPW, 2>(q),
                                     small_instalment<D, TPW, 3>(q)};
        for (int w = 0; w < D::NWAVES; ++w) {
            const int t = q * D::NWAVES + w;
            if (inst[w] >= 0 && tab.ti[t] >= D::PVT && tab.tj[t] >= D::PVT && inst[w] != 2) return false;
        }
    }
    return true;
}
// one instalment of wavefront W: entries, P2 term, and (instalment 0) the tile into the first panel column
template <class D, int TPW, int W, int INST>
VS_DEV void small_form(const double* __restrict__ sCfg, d4 (&acc)[TPW], double* __restrict__ sM, const double* __restrict__ sGy,
                       const double* __restrict__ sVprev, int lane, int crow) {
    using PLAN = SmallPlan<D, TPW, W, INST>;
    static_assert(small_plan_complete<D, TPW>(), "every tile is formed exactly once");
    static_assert(small_ac_tiles_last<D, TPW>(), "the tiles that read sAc are formed behind the barrier that publishes it");
    if constexpr (INST == 1) {
        static_assert(W >= 1, "wavefront 0 runs stream 0 meanwhile");
        p1s_contract_beside<D>(sM - Smem<D>::oM, 64 * (W - 1) + lane);
    }
    if constexpr (PLAN::count > 0) {
        p1s_entries<D, TPW, W, true, PLAN>(acc, sM - Smem<D>::oM, lane);
        p2_terms<D, TPW, W, true, PLAN>(sCfg, acc, sGy, sVprev, lane);
        if constexpr (INST == 0) {
            constexpr TileTab<D, true> tab{};
            static_for<0, PLAN::count>([&](auto acst) __attribute__((always_inline)) {
                constexpr int q = PLAN::slot(decltype(acst)::value);
                double* T = sM + tile_off_c<D>(tab.ti[q * D::NWAVES + W], 0) + crow;
#pragma unroll
                for (int r = 0; r < 4; ++r) T[4 * r * 17] = acc[q][r];
            });
        }
    }
}

template <class D, int TPW, int W, bool DEBUG, bool PIPE = false, bool SMALL = false>
VS_DEV void cholesky_wave(const double* __restrict__ sCfg, d4 (&acc)[TPW], double* __restrict__ sM, double* __restrict__ sInvD,
                          const double* __restrict__ sGy, const double* __restrict__ sVprev, int* __restrict__ sFlags,
                          double* __restrict__ sXinv, double* __restrict__ sW, double* __restrict__ dbgL, int lane,
                          int crow, int lrow, double* sZ_) {
    constexpr TileTab<D, PIPE> tab{};
    constexpr WaveLists<D, TPW, W, PIPE> wl{};
    using S = Smem<D>;
    constexpr int PVT = D::PVT;
    constexpr int GL = D::NZ & 15;  // local row of the gradient row (row NZ) in the last tile row
    if constexpr (D::WG_PER_CU == 1) pin_tiles_agpr<TPW>(acc);
    // ---- P2 (the small-batch kind adds the terms where it forms the tiles: small_form)
    if constexpr (!SMALL) p2_terms<D, TPW, W, PIPE, AllSlots<D, TPW, W, PIPE>>(sCfg, acc, sGy, sVprev, lane);
    if constexpr (D::WG_PER_CU == 1) pin_tiles_agpr<TPW>(acc);
    // ---- P3: tile column 0 goes to LDS; every later column is stored by the update that completes it
#pragma unroll
    for (int q = 0; q < TPW; ++q) {
        const int t = q * D::NWAVES + W;
        if (!SMALL && tab.forms(t, W) && tab.tj[t] == 0) {
            double* T = sM + tile_off_c<D>(tab.ti[t], 0) + crow;
#pragma unroll
            for (int r = 0; r < 4; ++r) T[4 * r * 17] = acc[q][r];
        }
    }
    // (small-batch kind: column 0 went to LDS in instalment 0, and the barrier behind that -- the caller's, straight in front
    // of this call -- is this one)
    if constexpr (!SMALL) __syncthreads();
#ifdef VS_DIAG_P3
    unsigned long long p3_mark = __builtin_amdgcn_s_memtime();
    if (DEBUG && W == 0 && lane < 4) vs_diag_p3[lane] = 0;
#endif
    // ---------------------------------------------------------------- PIPE: the pipelined schedule (kernel v27)
    // Wavefront 0 factors panel p while wavefronts 1..3 -- which hold all the tiles -- apply panel p - 1 to everything right of
    // column p.  Only the update of column p + 1 itself (`first`: one or two tiles per wavefront) stands between two streams:
    //     wavefront 0                         wavefronts 1..3
    //     stream(p): pivots 0..KB of the      first-update(p - 1) of the tiles (i, p), i > p, handed to LDS
    //     diagonal tile ...
    //     ----- s_barrier inside the stream = barrier: column p complete
    //     ... the rows below join, rest of    column p - 1's finished tiles -> registers; rest-update(p - 1): tiles (i, j), j > p,
    //     the stream                          with column p - 1;  one of them: X_(p-1)
    //     ----------------------------------- barrier: column p factored, the ring slot of column p - 1 free
    //     store the diagonal tile             first-update(p) of tile (p + 1, p + 1) with column p, handed to LDS
    //     ----------------------------------- barrier: diagonal tile of column p + 1 complete
    // Panel 0 has no update beside it: it is shared like in the plain schedule (one 64-row stream per wavefront); from
    // panel 1 on wavefront 0 carries all rows below the diagonal tile in one to three row slots.
    if constexpr (PIPE) {
        // Long horizons (one workgroup per CU; panel columns up to eleven tiles high): the diagonal tile of the next column is
        // updated by wavefront 0 itself and the other tiles arrive under the first pivots of its stream (ND, below).  Measured:
        // 1,637 -> 1,596 us per 4096 instances at the 2x horizon; at the paper horizon, where a column is at most six tiles
        // and the other wavefronts are done with them in the time wavefront 0 needs for its one, 37.4 us against 37.2.
        constexpr bool ND = D::WG_PER_CU == 1;
        static_for<0, D::NT>([&](auto pcst) __attribute__((always_inline)) {
            constexpr int p = decltype(pcst)::value;
            if constexpr (D::WG_PER_CU == 1) pin_tiles_agpr<TPW>(acc);
            constexpr int below = D::NP - 16 * p - 16;
            constexpr int nshare0 = (below + 63) / 64;
            constexpr int SL = below <= 64 ? 1 : (below <= 128 ? 2 : 3);
            static_assert(p == 0 ? nshare0 <= D::NWAVES - 1 : below <= 192, "rows of a panel fit the streams");
            double* scratch = p <= PVT ? sXinv + p * D::TS + 64 * W : sZ_ + 64 * W;
            double diag[16];
            if constexpr (p == D::NT - 1) {
                constexpr int NPIV_LAST = D::NZ - 16 * (D::NT - 1);
                if constexpr (NPIV_LAST == 8 || NPIV_LAST == 12) {   // the generated streams (tools/gen_panel_asm.py LAST_PANEL_PIVOTS)
                    if (W == 0 && panel_last_dpp<D, NPIV_LAST>(sM, sInvD, lane) && lane == 0) sFlags[0] = 1;
                } else {                                              // any other horizon: the C++ stream
                    if (W == 0 && panel_factor<D, NPIV_LAST>(sM, sInvD, p, lane) && lane == 0) sFlags[0] = 1;
                }
            } else if constexpr (p == 0 && SMALL) {
                // small-batch kind: wavefront 0 takes panel 0 alone, in nshare0 row slots; the others form tiles meanwhile.
                // (Measured against wavefront 1 sharing the stream as in the shipped kernel and forming its column-1 tiles behind
                // its share: 32.4-32.8 us per 256-launch against 33.1-33.3, profiles/small_batch_bench_alternating.txt.)
                static_assert(!SMALL || nshare0 <= 3, "row slots of one stream");
                if constexpr (W == 0) {
                    if (panel_dpp<D, nshare0>(sM, sInvD, p, lane, 0, diag, scratch) && lane == 0) sFlags[0] = 1;
                } else {
                    small_form<D, TPW, W, 1>(sCfg, acc, sM, sGy, sVprev, lane, crow);
                }
            } else if constexpr (p == 0) {
                if (W < nshare0) {
                    const int bad = panel_dpp<D, 1>(sM, sInvD, p, lane, W, diag, scratch);
                    if (W == 0 && bad && lane == 0) sFlags[0] = 1;
                }
            } else if constexpr (W == 0) {
                // the stream starts on the diagonal tile alone; the barrier that says "the rows below are complete" is the
                // s_barrier INSIDE it (behind pivot KB: far enough in for the other wavefronts' one or two -- long horizons:
                // up to four -- tiles of this column), matched by the __syncthreads() behind their first-update below
                constexpr int KB = !ND ? 0 : (SL == 3 ? 6 : (SL == 1 ? 3 : (pipe_max_others<D, TPW, p - 1>() > 2 ? 6 : 3)));
                int bad;
                if constexpr (16 * p + 16 == D::NU && D::NU - D::NUY == 8 && SL == 1 && KB == 0)
                    bad = panel_dummy_dpp<D, p>(sM, sInvD, lane, diag, scratch);
                else
                    bad = panel_dpp<D, SL, KB>(sM, sInvD, p, lane, 0, diag, scratch);
                if (bad && lane == 0) sFlags[0] = 1;
            }
            // the holder of tile (p + 1, p + 1) parks it in LDS (all earlier panels applied): wavefront 0 applies panel p to it
            // itself as soon as its stream has ended, no wavefront has to be waited for (not for the last panel, which is that
            // one tile: its holder updates it as before)
            auto park_next_diag = [&]() __attribute__((always_inline)) {
                if constexpr (ND && W >= 1 && p + 1 < D::NT - 1) {
                    static_for<0, TPW>([&](auto qcst) __attribute__((always_inline)) {
                        constexpr int q = decltype(qcst)::value;
                        constexpr int t = q * D::NWAVES + W;
                        if constexpr (tab.holds(t, W)) {
                            if constexpr (tab.ti[t] == p + 1 && tab.tj[t] == p + 1) {
                                double* T = sM + (S::oNextDiag - S::oM) + crow;
#pragma unroll
                                for (int r = 0; r < 4; ++r) T[4 * r * 17] = acc[q][r];
                            }
                        }
                    });
                }
            };
            if constexpr (p == 0) park_next_diag();
            if constexpr (p >= 1 && W >= 1) {
                if constexpr (SMALL && p == 1) small_form<D, TPW, W, 2>(sCfg, acc, sM, sGy, sVprev, lane, crow);
                // the finished tiles of column p - 1 come back into the registers that held them (the factor P5 reads; the
                // gradient row -> right-hand side of the back-substitution).  Here, beside the stream, not between two streams:
                // their ring slot stays intact until the barrier that ends this stream.
                if constexpr (p - 1 < PVT) {
#pragma unroll
                    for (int q = 0; q < TPW; ++q) {
                        const int t = q * D::NWAVES + W;
                        if (tab.holds(t, W) && tab.tj[t] == p - 1 && tab.ti[t] > p - 1) {
                            const double* T = sM + tile_off_c<D>(tab.ti[t], p - 1) + crow;
#pragma unroll
                            for (int r = 0; r < 4; ++r) acc[q][r] = T[4 * r * 17];
                            if (tab.ti[t] == D::NT - 1 && (lane >> 4) == (GL & 3)) sW[16 * (p - 1) + (lane & 15)] = -acc[q][GL >> 2];
                        }
                    }
                }
                pipe_update<D, TPW, W, p - 1, 2>(acc, sM, lrow, crow);   // rest-update(p - 1)
                park_next_diag();
                if constexpr (W == pipe_inverse_wave<D, TPW>(p)) {
                    if constexpr (p - 1 < S::NXT)
                        tile_inverse_dpp(sM + tile_off_c<D>(p - 1, p - 1), sInvD + 16 * (p - 1), sXinv + (p - 1) * D::TS, lane);
                    if constexpr (S::DUAL3 && p - 1 == D::PVT + 1)
                        tile_inverse_dpp(sM + tile_off_c<D>(p - 1, p - 1), sInvD + 16 * (p - 1), sM + (S::oDual3T0 - S::oM), lane);
                }
            }
            VS_P3_MARK(0);
            __syncthreads();
            VS_P3_MARK(1);
            if constexpr (p + 1 < D::NT) {
                if (W == 0 && lane < 16) {  // nobody reads tile (p, p) before the next barrier
                    double* Tpp = sM + tile_off_c<D>(p, p) + lane * 17;
#pragma unroll
                    for (int c = 0; c < 16; ++c) Tpp[c] = diag[c];
                    if (DEBUG && dbgL != nullptr) {
#pragma unroll
                        for (int c = 0; c < 16; ++c)
                            if (c <= lane) dbgL[size_t(16 * p + lane) * D::NP + 16 * p + c] = diag[c];
                    }
                }
                if constexpr (ND && p + 1 < D::NT - 1) {
                    // first-update(p).  Wavefront 0: the diagonal tile of column p + 1, from its parked copy, written where the
                    // next stream loads it (same wavefront: LDS operations stay in order, no barrier) -- two chains of two matrix
                    // instructions.  Wavefronts 1..3: the other tiles of the column, handed to LDS, then the barrier that
                    // wavefront 0 meets INSIDE its next stream, behind the first pivots of the diagonal tile.
                    if constexpr (W == 0) {
                        const double* Ljp = sM + tile_off_c<D>(p + 1, p) + lrow;
                        const double* Cn = sM + (S::oNextDiag - S::oM) + crow;
                        double lb[4];
                        d4 c, c2 = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
                        for (int ks = 0; ks < 4; ++ks) lb[ks] = Ljp[4 * ks];
#pragma unroll
                        for (int r = 0; r < 4; ++r) c[r] = Cn[4 * r * 17];
                        c = __builtin_amdgcn_mfma_f64_16x16x4f64(-lb[0], lb[0], c, 0, 0, 0);
                        c2 = __builtin_amdgcn_mfma_f64_16x16x4f64(-lb[1], lb[1], c2, 0, 0, 0);
                        c = __builtin_amdgcn_mfma_f64_16x16x4f64(-lb[2], lb[2], c, 0, 0, 0);
                        c2 = __builtin_amdgcn_mfma_f64_16x16x4f64(-lb[3], lb[3], c2, 0, 0, 0);
                        double* T = sM + tile_off_c<D>(p + 1, p + 1) + crow;
#pragma unroll
                        for (int r = 0; r < 4; ++r) T[4 * r * 17] = c[r] + c2[r];
                        VS_P3_MARK(2);
                    } else {
                        pipe_update<D, TPW, W, p, 4>(acc, sM, lrow, crow);
                        __syncthreads();
                    }
                } else {
                    // short horizons, and the last panel (one tile) everywhere: the holders apply panel p to the whole column,
                    // a barrier, wavefront 0 factors it
                    if constexpr (W >= 1) pipe_update<D, TPW, W, p, 1>(acc, sM, lrow, crow);
                    VS_P3_MARK(2);
                    __syncthreads();
                    VS_P3_MARK(3);
                }
            }
        });
        return;
    }
    // (a compile-time loop: the work lists below are indexed with p in constant expressions)
    static_for<0, D::NT>([&](auto pcst) __attribute__((always_inline)) {
        constexpr int p = decltype(pcst)::value;
        if constexpr (D::WG_PER_CU == 1) pin_tiles_agpr<TPW>(acc);   // long horizons: the tiles stay in the AGPR half
        // rows under the diagonal tile and the wavefronts that share the panel: one 64-row stream each (panel_dpp)
        const int below = D::NP - 16 * p - 16;
        const int nshare = below <= 64 ? 1 : (below + 63) / 64;
        static_assert((D::NP - 16 + 63) / 64 <= D::NWAVES - 1, "panel 0 leaves one wavefront for the side work");
        double diag[16];  // factored diagonal tile of a shared panel (wavefront 0, lanes 0..15), stored after the barrier
        // scratch strip of this wavefront (64 doubles, see panel_dpp): the slot of X_p, which nobody writes before panel
        // p + 1; the last panels (one wavefront each) borrow the not-yet-used z vector
        double* scratch = p <= PVT ? sXinv + p * D::TS + 64 * W : sZ_ + 64 * W;
        static_assert(D::TS >= 64 * D::NWAVES && D::NP >= 64, "scratch strips");
        {
            constexpr int NPIV_LAST = D::NZ - 16 * (D::NT - 1);
            if (p == D::NT - 1) {
                if constexpr (NPIV_LAST == 8 || NPIV_LAST == 12) {   // the generated streams (tools/gen_panel_asm.py LAST_PANEL_PIVOTS)
                    if (W == 0 && panel_last_dpp<D, NPIV_LAST>(sM, sInvD, lane) && lane == 0) sFlags[0] = 1;
                } else {                                              // any other horizon: the C++ stream
                    if (W == 0 && panel_factor<D, NPIV_LAST>(sM, sInvD, p, lane) && lane == 0) sFlags[0] = 1;
                }
            } else if (W < nshare) {
                const int bad = panel_dpp<D>(sM, sInvD, p, lane, W, diag, scratch);
                if (W == 0 && bad && lane == 0) sFlags[0] = 1;
            }
        }
        // a wavefront without panel rows inverts the diagonal tile finished one panel ago (its ring slot is intact
        // until the update of THIS panel hands column p+1 over): X_0..X_PVT for P5 and the dual box QP
        if (W == (nshare > 1 ? D::NWAVES - 1 : 1) && p >= 1 && p - 1 < S::NXT)
            tile_inverse<D>(sM + tile_off_c<D>(p - 1, p - 1), sInvD + 16 * (p - 1), sXinv + (p - 1) * D::TS, lane);
        // three throttle tile rows: the box QP also wants the inverses of the other two corner diagonal tiles.  The second
        // one here, into the tile-shaped scratch the QP reads it from (that part of the ring is dead since the last joint
        // panel); the third one after P3 (solve_kernel).  ~4 k cycles each that used to sit at the top of the box QP.
        if constexpr (S::DUAL3) {
            if (W == (nshare > 1 ? D::NWAVES - 1 : 1) && p - 1 == D::PVT + 1)
                tile_inverse<D>(sM + tile_off_c<D>(p - 1, p - 1), sInvD + 16 * (p - 1), sM + (S::oDual3T0 - S::oM), lane);
        }
        VS_P3_MARK(0);
        __syncthreads();
        VS_P3_MARK(1);
        if (W == 0 && p < D::NT - 1 && lane < 16) {  // nobody reads tile (p, p) before the next barrier
            double* Tpp = sM + tile_off_c<D>(p, p) + lane * 17;
#pragma unroll
            for (int c = 0; c < 16; ++c) Tpp[c] = diag[c];
            if (DEBUG && dbgL != nullptr) {
#pragma unroll
                for (int c = 0; c < 16; ++c)
                    if (c <= lane) dbgL[size_t(16 * p + lane) * D::NP + 16 * p + c] = diag[c];
            }
        }
        if (p + 1 < D::NT) {
            // finished tiles of panel column p come back into the registers that held them (columns of the throttle
            // corner stay in LDS); the gradient row -> right-hand side y = -L^-1 g of the back-substitution.  Requested
            // first: the loads complete under the matrix-core work below.
            if (p < PVT) {
#pragma unroll
                for (int q = 0; q < TPW; ++q) {
                    const int t = q * D::NWAVES + W;
                    if (t < D::NTRI && tab.tj[t] == p && tab.ti[t] > p) {
                        const double* T = sM + tile_off_c<D>(tab.ti[t], p) + crow;
#pragma unroll
                        for (int r = 0; r < 4; ++r) acc[q][r] = T[4 * r * 17];
                        if (tab.ti[t] == D::NT - 1 && (lane >> 4) == (GL & 3)) sW[16 * p + (lane & 15)] = -acc[q][GL >> 2];
                    }
                }
            }
            // trailing update M_ij -= L_ip L_jp^T for the owned tiles right of the panel; the operands of the next
            // tile are requested before the four matrix-core instructions of the current one.  (Two tiles at a time --
            // interleaved chains, a dependent v_mfma_f64_16x16x4_f64 issues every ~95 cycles, independent ones every 64 --
            // measured no faster at either horizon: the panel streams bound P3, not these.)
            double la[2][4], lb[2][4];
            auto request = [&](auto acst) __attribute__((always_inline)) {
                constexpr int a = decltype(acst)::value;
                if constexpr (a < wl.ntrail[p]) {
                    constexpr int t = wl.trail[p][a] * D::NWAVES + W;
                    const double* Lip = sM + tile_off_c<D>(tab.ti[t], p) + lrow;
                    const double* Ljp = sM + tile_off_c<D>(tab.tj[t], p) + lrow;
#pragma unroll
                    for (int ks = 0; ks < 4; ++ks) { la[a & 1][ks] = -Lip[4 * ks]; lb[a & 1][ks] = Ljp[4 * ks]; }
                }
            };
            request(std::integral_constant<int, 0>{});
            static_for<0, TPW>([&](auto acst) __attribute__((always_inline)) {
                constexpr int a = decltype(acst)::value;
                if constexpr (a < wl.ntrail[p]) {
                    request(std::integral_constant<int, a + 1>{});
                    constexpr int q = wl.trail[p][a];
                    constexpr int t = q * D::NWAVES + W;
#pragma unroll
                    for (int ks = 0; ks < 4; ++ks)
                        acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(la[a & 1][ks], lb[a & 1][ks], acc[q], 0, 0, 0);
                    if constexpr (tab.tj[t] == p + 1) {  // this tile column is the next panel: hand it to LDS
                        double* T = sM + tile_off_c<D>(tab.ti[t], p + 1) + crow;
#pragma unroll
                        for (int r = 0; r < 4; ++r) T[4 * r * 17] = acc[q][r];
                    }
                }
            });
            VS_P3_MARK(2);
            __syncthreads();
            VS_P3_MARK(3);
        }
    });
}

}  // namespace vsmpc
