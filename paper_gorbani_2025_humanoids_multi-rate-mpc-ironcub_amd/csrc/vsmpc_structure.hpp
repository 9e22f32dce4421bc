// What the runtime-sized kernels (vsmpc_runtime.hip, vsmpc_certify.hip) both state about the problem's structure: the
// move-blocking maps by RtDims, the size of p0_linearize's block, which entries of A the linearisation can fill, the
// diagonal of Q and the wavefront reductions.
#pragma once
#include "vsmpc_launch.hpp"

namespace vsmpc {

constexpr int LIN_DOUBLES = NX * NX + NX * NJ + NX * NTH + 28;   // A | Bj | Bt | c (p0_linearize's contiguous block)

// move blocking: the joint / throttle block that acts on stage k (constraintsVSMPC.cpp:89-103 and :104-128)
VS_DEV int joint_block(const RtDims& d, int k) { return k < d.hc ? k : d.hc - 1; }
VS_DEV int throttle_block(const RtDims& d, int k) {
    return k < d.ns ? 0 : (k < d.hc ? k - (d.ns - 1) : d.hc - d.ns);
}

// Entries of A that p0_linearize can make non-zero (vsmpc_p0.hpp; systemDynamicsVSMPC.cpp:79-103,288-319,384-429): 142 of
// the 676, stated twice -- entry by entry, for code that unrolls over (r, q) at compile time (a dense read keeps A in
// registers and spills), and as the two column ranges [a0, a1) and [b0, b1) of row r, for code that loops at run time.
VS_HD constexpr bool a_nz(int r, int q) {
    if (r < 3) return q >= 3 && q < 6;                          // CoM       <- h_lin
    if (r < 6) return (q >= 3 && q < 6) || (q >= 12 && q < 16);  // h_lin     <- h_lin, T
    if (r < 9) return q >= 9 && q < 12;                          // RPY       <- h_ang
    if (r < 12) return q >= 9 && q < 16;                         // h_ang     <- h_ang, T
    if (r < 20) return q >= 12 && q < 20;                        // T, Tdot   <- T, Tdot
    if (r < 23) return q < 3;                                    // e_pos     <- CoM
    return q >= 6 && q < 9;                                      // e_rpy     <- RPY
}
VS_HD constexpr void a_row_ranges(int r, int& a0, int& a1, int& b0, int& b1) {
    b0 = b1 = 0;
    if (r < 3) { a0 = 3; a1 = 6; }                          // CoM    <- h_lin
    else if (r < 6) { a0 = 3; a1 = 6; b0 = 12; b1 = 16; }   // h_lin  <- h_lin, T
    else if (r < 9) { a0 = 9; a1 = 12; }                    // RPY    <- h_ang
    else if (r < 12) { a0 = 9; a1 = 16; }                   // h_ang  <- h_ang, T
    else if (r < 20) { a0 = 12; a1 = 20; }                  // T, Tdot <- T, Tdot
    else if (r < 23) { a0 = 0; a1 = 3; }                    // e_pos  <- CoM
    else { a0 = 6; a1 = 9; }                                // e_rpy  <- RPY
}
constexpr bool a_sparsity_statements_agree() {
    for (int r = 0; r < NX; ++r) {
        int a0 = 0, a1 = 0, b0 = 0, b1 = 0;
        a_row_ranges(r, a0, a1, b0, b1);
        for (int q = 0; q < NX; ++q)
            if (a_nz(r, q) != ((q >= a0 && q < a1) || (q >= b0 && q < b1))) return false;
    }
    return true;
}
static_assert(a_sparsity_statements_agree(), "a_nz and a_row_ranges describe the same 26 x 26 pattern");

// diagonal of Q on state row r (costsVSMPC.cpp:78-93) from the 18 square-root weights `sq` (a row of tunables' CFG_SQ part,
// or the sq of a DevCfg): the squared weight of the weighted rows, 0 on T, Tdot
VS_DEV double q_diag(const double* __restrict__ sq, int r) {
    const double s = sq[r < 12 ? r : (r >= 20 ? r - 8 : 0)];   // loaded unconditionally, selected afterwards
    return (r >= 12 && r < 20) ? 0.0 : s * s;
}

// wavefront reductions by butterfly: every lane ends with the same value, formed in the same order
VS_DEV double wave_max(double v) {
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}
VS_DEV double wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

}  // namespace vsmpc
