// What every phase of the tuned solve kernels shares: the compile-time tables and loops, the LDS carve-up (Smem<D>) and
// the tile addressing.  Included by the per-horizon unit (vsmpc_kernels.hip) and, for the LDS sizes of the horizon table,
// by vsmpc_dispatch.hip.
#pragma once
#include <type_traits>

#include "vsmpc_device.hpp"

namespace vsmpc {

typedef double d4 __attribute__((ext_vector_type(4)));

template <class D, bool PIPE = false>
__device__ constexpr TileTab<D, PIPE> kTileTab{};
template <class D>
__device__ constexpr NactTab<D> kNactTab{};
template <class D>
__device__ constexpr TilePack<D> kTilePack{};

// compile-time loop: f(std::integral_constant<int, I>{}) for I = I0 .. N-1
template <int I, int N, class F>
VS_DEV void static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}

// The lane id, re-derived where it is needed (two instructions) instead of carried there: a value that is live across a
// long phase is what the register allocator spills first, and at the 2x horizon every spilled dword is 4 MB of scratch
// traffic per 4096-instance launch.
VS_DEV int fresh_lane() {
    unsigned m = ~0u;
    asm volatile("" : "+s"(m));
    return int(__builtin_amdgcn_mbcnt_hi(m, __builtin_amdgcn_mbcnt_lo(m, 0u)));
}

// ------------------------------------------------------------------------------------------------
// LDS carve-up (doubles).  One region R is reused phase by phase:
//   P1      the Y buffer (two nodes x 18 weighted rows x YS)
//   P3      the ring of two panel columns + the throttle corner (Dims::L_TILES tiles, see vsmpc_device.hpp)
//   P4..P6  over the (by then dead) ring: box-QP work arrays, the per-wavefront partial sums of the register
//           back-substitution, the state trajectory and the stage forcing terms; the corner stays where it is
// Paper horizon: 71 KB in total, so two workgroups fit one CU.
// ------------------------------------------------------------------------------------------------
// SMALL: the carve-up of the small-batch kind (solve_kernel_small, one workgroup per CU, up to 160 KB): the arrays of P1a /
// P1s lie BEHIND everything P3..P6 use instead of under the X region and the ring, so that a wavefront can still form tile
// entries from them while the panel streams run.  Every other offset is the shipped one.
template <class D, bool SMALL = false>
struct Smem {
    // the dual box QP and the chain-free first pass need the throttle block to span exactly two tile rows
    static constexpr bool DUALQP = D::NT - 2 == D::PVT && D::NU % 16 == 0 && D::NV >= 20 && D::NV <= 32;
    static constexpr int oIn = 0;
    static constexpr int oA = oIn + ((D::NIN + 3) & ~3);
    static constexpr int oBj = oA + NX * NX;
    static constexpr int oBt = oBj + NX * NJ;
    static constexpr int oC = oBt + NX * NTH;
    static constexpr int oVprev = oC + 28;
    static constexpr int oInvD = oVprev + 4;
    static constexpr int oW = oInvD + D::NP;
    static constexpr int oZ = oW + D::NP;
    static constexpr int oSvec = oZ + D::NP;
    static constexpr int oV = oSvec + D::NV;
    static constexpr int oDt = oV + D::NV;           // per-stage dt (copied out of the kernel arguments once)
    static constexpr int oCfg = oDt + MAX_STAGES;    // configuration scalars (CFG_* offsets)
    static constexpr int oFlags = oCfg + CFG_SIZE;   // 4 doubles worth of int flags
    static constexpr int NFLAGS = 5;                 // [0] numerical failure, [1] status, [2] iterations, [3] bounds violated, [4] which
    static_assert(NFLAGS * sizeof(int) <= 4 * sizeof(double), "the int flags fit their four doubles (oQR follows)");
    // X_p = L_pp^-1 of the joint diagonal tiles and of the first throttle tile, produced by wavefronts that idle
    // during the panel factorisations of P3
    // joint reduction (p0_joint_reduction): the six Householder vectors, their betas, the reduced gradient Q^T b, the null
    // component n = -N^T b and W^(-1/2)
    static constexpr int oQR = (oFlags + 4 + 3) & ~3;
    static constexpr int QR_V = 0, QR_BETA = 48, QR_GY = 56, QR_NS = 62, QR_ISW = 64, QR_A = 72, QR_SIZE = 128;
    static constexpr int NXT = D::PVT + 1;
    static constexpr int oXinv = (oQR + QR_SIZE + 3) & ~3;
    static constexpr int oR = oXinv + NXT * D::TS;
    static constexpr int YROWS = 36;                 // two nodes x 18 weighted rows = 9 exact MFMA k-steps
    static constexpr int oY = oR;
    static constexpr int sizeY = YROWS * D::YS;
    static constexpr int oM = oR;                    // ring + corner tiles (Y is dead after P1)
    static constexpr int sizeM = D::L_TILES * D::TS;
    static constexpr int NVS = D::NV + 1;            // row stride of the box-QP work arrays
    static constexpr int oSv = oR;                   // Schur complement / columns of P
    // three throttle tile rows, tile aligned (the 2x horizon): dual form on a dense X assembled from tile products
    static constexpr bool DUAL3 = !DUALQP && D::NT - 3 == D::PVT && D::NU % 16 == 0 && D::NV > 32 && D::NV <= 48;
    static constexpr int oQP = oSv + D::NV * NVS;    // dual form: K | rows 16.. of X (DUALQP); K | X | two scratch tiles (DUAL3)
    static constexpr int sizeQP = DUALQP ? D::NV * NVS + (D::NV - 16) * NVS : (DUAL3 ? 2 * D::NV * NVS + 2 * D::TS : 0);
    static constexpr int oDual3T0 = oQP + 2 * D::NV * NVS;   // DUAL3: two tile-shaped scratches behind K and X
    static constexpr int oDual3T1 = oDual3T0 + D::TS;
    // per-wavefront partial sums of L^T z, NP each.  The box-QP arrays are dead by then: where the dense X would not fit
    // beside them (DUAL3) the two overlap
    static constexpr int oU = DUAL3 ? oR : oQP + sizeQP;
    static constexpr int oX = oU + D::NWAVES * D::NP;  // P6: state trajectory
    static constexpr int oF = oX + D::NXS;           // P6: per-stage input terms, NX per stage
    static constexpr int endScratch = (oF + NX * D::N > oQP + sizeQP) ? oF + NX * D::N : oQP + sizeQP;
    static_assert(endScratch <= oR + D::CORNER_TILE0 * D::TS, "P4..P6 scratch must not reach the corner tiles");
    // P1a: jet thrust trajectories [NJROW][N] and the affine column's momentum forcing [2][N][3], at the head of the X
    // region (the X tiles are not written before P3)
    static constexpr int NJROW = D::NV + NTH + 1;
    // (small-batch kind: behind the ring, the corner, the parked diagonal tile and the scratch of P4..P6)
    static constexpr int oP1Small = ((oR + D::L_TILES * D::TS + D::TS > endScratch ? oR + D::L_TILES * D::TS + D::TS : endScratch) + 3) & ~3;
    static constexpr int oJetT = SMALL ? oP1Small : oXinv;
    static constexpr int oGA = oJetT + NJROW * D::N;
    // P1s (structured condensing, Dims::STRUCT_P1): behind them, across the rest of the X region and R
    //   sH [2][NJPAIR][3][3]      block sums of H(i, i') over (row block, column block) pairs of the joint blocks
    //   sRb[2][NV + 1][HC][3]     W_c(i) of the throttle columns and of the affine column, summed over joint blocks
    //   sW3[2][NV + 1][N - 1][3]  W_c(i), i = 1 .. N - 1, of the throttle columns and of the affine column
    //   sAc[NV + 1][N - 1][4]     sum over the halves of A_mom[:, q]^T W_c(i) (formed by all wavefronts after the chains;
    //                             small-batch kind: by wavefronts 1..3 beside panel stream 0)
    //   sRefC[NREF][12]           reference window with the integrator offsets c_e folded into the x rows
    //   sZero                     zeros: what the columns without a thrust trajectory / forcing / reference read
    static constexpr int oSH = oGA + 6 * D::N;
    static constexpr int oSRb = oSH + 2 * D::NJPAIR * 9;
    static constexpr int oSW3 = oSRb + 2 * (D::NV + 1) * D::HC * 3;
    // long horizons (Dims::STRUCT_LONG) have no sW3: the chains add A_mom^T W straight into sAc (LDS atomics, two addends
    // per word: order independent).  A row of sAc keeps the stages i' = i - 1 >= ac_first(row) only: the tile columns at or
    // left of a throttle row before the v_0 block all start at stage NS or later, and tau_i = 0 up to a column's first stage
    static constexpr int oSAc = oSW3 + (D::STRUCT_LONG ? 0 : 2 * (D::NV + 1) * (D::N - 1) * 3);
    static constexpr int AC_SHORT = D::STRUCT_LONG ? D::NV - NTH : 0;   // rows [0, AC_SHORT) are short
    static constexpr int AC_NSH = D::STRUCT_LONG ? D::NS : 0;           // first stored i' of a short row
    VS_HD static constexpr int ac_first(int cr) { return cr < AC_SHORT ? AC_NSH : 0; }
    VS_HD static constexpr int ac_off(int cr) {   // offset of row cr's first stored stage (4 doubles per stage)
        // = cr < AC_SHORT ? cr (N - 1 - AC_NSH) 4 : (AC_SHORT (N - 1 - AC_NSH) + (cr - AC_SHORT) (N - 1)) 4, written without a
        // branch: as a conditional the compiler made basic blocks of it inside p1s_entries, and at their joins moved the
        // finished accumulator tiles through the vector registers (and a few values into scratch)
        return 4 * (cr * (D::N - 1) - (cr < AC_SHORT ? cr : AC_SHORT) * AC_NSH);
    }
    static constexpr int sizeAc = ac_off(D::NV + 1);
    static constexpr int oSRefC = oSAc + sizeAc;
    static constexpr int sizeZero = 3 * D::N > 12 * D::NREF ? 3 * D::N : 12 * D::NREF;
    // the zeros: long horizons borrow the (not yet used) w and z vectors of P3..P5
    static constexpr int oSZero = D::STRUCT_LONG ? oW : oSRefC + 12 * D::NREF;
    static_assert(!D::STRUCT_LONG || sizeZero <= 2 * D::NP, "zeros fit the w and z vectors");
    static constexpr int endP1s = D::STRUCT_LONG ? oSRefC + 12 * D::NREF : oSZero + sizeZero;
    // P3, pipelined schedule: one tile behind the ring and the corner -- the diagonal tile of the NEXT panel column as its holder
    // has it (updates of all earlier panels applied), parked there so that wavefront 0 can apply the current panel to it
    // itself the moment its stream ends (cholesky_wave).  The arrays of P1s that lie there are dead by then.
    static constexpr int oNextDiag = oM + sizeM;
    static constexpr int total_syrk = oR + (sizeY > sizeM ? sizeY : sizeM);
    static constexpr int total_struct = D::STRUCT_P1 ? (endP1s > oNextDiag + D::TS ? endP1s : oNextDiag + D::TS) : total_syrk;
    // both forms share one carve-up; a horizon with the structured form never launches the SYRK form unless asked to
    // (vsmpc_set_kernel_form), so each form gets its own size
    static constexpr int total = total_syrk;
    static constexpr size_t bytes = size_t(total) * sizeof(double);
    static constexpr size_t bytes_struct = size_t(total_struct) * sizeof(double);
    static_assert(bytes <= 160 * 1024 && bytes_struct <= 160 * 1024, "LDS budget of one CU");
    static_assert(SMALL || D::WG_PER_CU < 2 || (bytes <= 80 * 1024 && bytes_struct <= 80 * 1024), "two workgroups per CU");
    // small-batch kind: nothing of P1a / P1s (jet trajectories, sGA, sH, sRb, sW3, sAc, reference window, zeros) overlaps the
    // X region, the ring, the corner, the parked next diagonal tile or the scratch of P4..P6
    static_assert(!SMALL || (D::STRUCT_P1 && !D::STRUCT_LONG), "the small-batch kind exists for short structured horizons");
    static_assert(!SMALL || (oJetT >= oNextDiag + D::TS && oJetT >= endScratch && oJetT >= oXinv + NXT * D::TS && endP1s <= total_struct),
                  "small-batch kind: the arrays of P1 stay apart from everything P3..P6 write");
};

// Horizons with the small-batch kind of the solve kernel: those whose shipped kernel is the pipelined structured form at two
// workgroups per CU (when the batch does not exceed the CUs the second workgroup slot of a CU is empty anyway), and whose tile
// column 1 holds no throttle x throttle tile (PVT >= 2): column 1 is formed beside stream 0, where the contraction those
// tiles read is still being formed
template <class D>
constexpr bool has_small_kind() { return D::STRUCT_P1 && !D::STRUCT_LONG && D::WG_PER_CU == 2 && D::PVT >= 2; }

// tile (i, j), j <= i, of the factor in LDS: panel columns left of the throttle corner live in a ring of two
// (even columns at tile 0, odd ones at tile RING_A), the corner is dense behind the ring
template <class D>
VS_HD constexpr int tile_off_c(int i, int j) {
    return (j < D::PVT ? (j & 1) * D::RING_A + (i - j)
                       : D::CORNER_TILE0 + (i - D::PVT) * (i - D::PVT + 1) / 2 + (j - D::PVT)) * D::TS;
}
template <class D>
VS_DEV int tile_off(int i, int j) { return tile_off_c<D>(i, j); }

// element (gr, gc), gc <= gr, of a tile that is currently in LDS
template <class D>
VS_DEV int lower_at(int gr, int gc) {
    return tile_off<D>(gr >> 4, gc >> 4) + (gr & 15) * 17 + (gc & 15);
}

}  // namespace vsmpc
