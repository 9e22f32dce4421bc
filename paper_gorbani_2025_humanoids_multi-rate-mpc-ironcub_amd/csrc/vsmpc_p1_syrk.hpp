// P1, SYRK form (FORM 0 of solve_kernel, every horizon): the pass tables and the matrix-core chain of one accumulator tile.
// The sensitivity recursion that feeds it is in the kernel body (vsmpc_kernels.hip).
#pragma once
#include "vsmpc_smem.hpp"

namespace vsmpc {

// active accumulator slots of SYRK pass m, maximum over the wavefronts (see NactTab)
template <class D>
constexpr int nact_max(int m) {
    constexpr NactTab<D> t{};
    int n = 0;
    for (int w = 0; w < D::NWAVES; ++w) n = t.n[m][w] > n ? t.n[m][w] : n;
    return n;
}

// runs of consecutive SYRK passes with the same slot count and the same number of k-steps
template <class D>
struct PassGroups {
    static constexpr int NPASS = (D::N + 1) / 2;
    int start[NPASS], end[NPASS], nact[NPASS], nks[NPASS], n;
    constexpr PassGroups() : start{}, end{}, nact{}, nks{}, n(0) {
        for (int m = 0; m < NPASS; ++m) {
            const int a = nact_max<D>(m), k = (2 * m + 1 < D::N) ? 9 : 5;
            if (n > 0 && nact[n - 1] == a && nks[n - 1] == k) { end[n - 1] = m + 1; continue; }
            start[n] = m; end[n] = m + 1; nact[n] = a; nks[n] = k; ++n;
        }
    }
    static constexpr int count() { return PassGroups().n; }
};

// ------------------------------------------------------------------------------------------------
// SYRK of P1, one accumulator tile (slot) at a time: NKS k-steps of 4 rows as ONE dependent chain on the tile's
// accumulator (a dependent v_mfma_f64_16x16x4_f64 issues every 64 cycles, like independent ones).
//   * The slots a pass runs are a prefix NACT-1, ..., 0 of the stage-sorted tile table, and NACT is a COMPILE-TIME
//     constant of the pass, the same for the four wavefronts (the maximum over them; a wavefront with fewer active
//     tiles multiplies columns of Y that are still exactly zero).  The chains of a pass are therefore straight-line
//     code.  Every earlier form with control flow around the chains (an instantiation per slot count through v9, a
//     fall-through switch, a branch per slot) made the register allocator move whole accumulator tiles at the joins
//     and the loop back-edge: ~1.1k cycles per pass whatever the number of chains (38.8k cycles of matrix-core
//     section against a floor of 29.4k; now 31.6k).  Short horizons unroll the pass loop, long ones run one rolled
//     loop per distinct slot count (PassGroups).
//   * Operand loads are software-pipelined SYRK_DIST instructions ahead ACROSS slots and pinned with sched_barrier:
//     the wave's stream blocks at every MFMA issue until the pipe is free (64 cycles), an LDS read returns in ~130.
//     `ha`/`hb` carry the first SYRK_DIST operand pairs of the slot in and those of the NEXT slot (slot q - 1) out.
// The matrix instruction is the builtin; the form written as inline assembly with a tied accumulator measured no faster
// once the chains were straight-line code.
// ------------------------------------------------------------------------------------------------
constexpr int SYRK_DIST = 2;         // prefetch distance of the operand loads, in matrix instructions
constexpr int SYRK_UNROLL_TPW = 12;  // the pass loop is unrolled up to that many slots per wavefront (short horizons)

template <class D, int NKS, bool PIN = true>
VS_DEV void syrk_slot(d4& acc, const double* __restrict__ pa, const double* __restrict__ pb, double (&ha)[SYRK_DIST],
                      double (&hb)[SYRK_DIST], const double* __restrict__ pan, const double* __restrict__ pbn) {
    static_assert(NKS >= 2 * SYRK_DIST - 1, "pipeline depth");
    double av[NKS], bv[NKS], na[SYRK_DIST], nb[SYRK_DIST];
#pragma unroll
    for (int ks = 0; ks < SYRK_DIST; ++ks) { av[ks] = ha[ks]; bv[ks] = hb[ks]; }
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[ks], bv[ks], acc, 0, 0, 0);
        if constexpr (PIN) __builtin_amdgcn_sched_barrier(0);
        const int n = ks + SYRK_DIST;
        if (n < NKS) {
            av[n] = pa[n * 4 * D::YS];
            bv[n] = pb[n * 4 * D::YS];
        }
        // the head of the NEXT slot is requested behind the FIRST instructions of this chain, not the last ones: by the
        // control-flow join that follows the chain every load has long returned (the compiler drains the LDS counter at
        // a join: it cannot count outstanding loads across predecessors)
        if (ks < SYRK_DIST) {
            na[ks] = pan[ks * 4 * D::YS];
            nb[ks] = pbn[ks * 4 * D::YS];
        }
        if constexpr (PIN) __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int ks = 0; ks < SYRK_DIST; ++ks) { ha[ks] = na[ks]; hb[ks] = nb[ks]; }
}

}  // namespace vsmpc
