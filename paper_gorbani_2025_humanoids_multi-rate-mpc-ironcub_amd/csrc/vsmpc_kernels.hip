// Hand-written HIP kernels for gfx950 (MI355X): one workgroup per MPC instance.
//
// Replaces, per instance, IMPCProblem::update + IMPCProblem::solve + VariableSamplingMPC::solveMPC
// (IMPCProblem.cpp:150-298, variableSamplingMPC.cpp:88-112) with a structure-exploiting exact solve:
//
//   P0 linearise   A, Bj, Bt, c in LDS                       (systemDynamicsVSMPC.cpp:79-103,288-319,384-429)
//                  + joint reduction: a joint block acts on the dynamics through [Lambda_lin; Lambda_ang] (6 x 8) only, so
//                  SIX unknowns per block are condensed (Householder QR of (Lambda W^-1/2)^T, p0_joint_reduction); the two
//                  others have a closed form                  (constraintsVSMPC.cpp:85-103, costsVSMPC.cpp:375-381,564-591)
//   P1 condense    jet thrust sensitivities first (one two-state recursion per throttle column, four for the affine
//                  column).  Structured form (P1s, the default where Dims::STRUCT_P1): forward / adjoint recursions on
//                  three generator columns per joint block, the throttle columns and the affine column, one lane per
//                  (column, half), trajectory in registers; the tile entries of C formed on the matrix cores from the
//                  block sums the chains leave in LDS -- O(N^2) work.  SYRK form (every horizon; vsmpc_set_kernel_form):
//                  the sensitivity recursion in registers, thread (half, col) carries the linear-momentum half (p, h_lin,
//                  e_pos) or the angular half (rpy, h_ang, e_rpy) of one condensed column; two nodes (36 weighted rows =
//                  9 exact MFMA k-steps) per pass; C = sum_k Y_k^T Y_k with v_mfma_f64_16x16x4_f64, every pass a
//                  straight-line sequence of per-tile chains (compile-time slot count).  Accumulators in registers
//                  from here to P5; 256 threads, two workgroups per CU at the paper horizon
//                                                            (constraintsVSMPC.cpp:76-131, costsVSMPC.cpp:166-178)
//   P2 augment     M = C + R, gradient row                   (costsVSMPC.cpp:375-409,468-487,558-592)
//   P3 cholesky    right-looking LL^T on 16x16 tiles; the trailing matrix AND the finished factor stay in registers,
//                  LDS holds a ring of two panel columns + the throttle corner; trailing updates on MFMA.  A panel stream
//                  is generated assembly (vsmpc_panel_asm.inc <- tools/gen_panel_asm.py): every lane carries panel rows
//                  and, replicated per 16-lane row, a row of the diagonal tile; the pivot column is broadcast inside the FMA
//                  (v_fmac_f64 DPP row_newbcast).  Structured form: PIPELINED -- wavefront 0 factors panel p while
//                  wavefronts 1..3, which hold all tiles, apply panel p - 1 and invert diagonal tile p - 1 (cholesky_wave,
//                  TileTab<D, PIPE>); SYRK form: the panel shared by up to three wavefronts, all four update
//   P4 box QP      backward pass over the throttle tiles with only the hold pin; only if a bound is violated: block
//                  principal pivoting in one wavefront, dual form on P = X^T X for few violated bounds, primal form
//                  on the Schur complement otherwise, small systems in registers   (constraintsVSMPC.cpp:338-365)
//   P5 back-subst  joints from the register-resident factor, tile row by tile row: z_r = X_r^T (w_r - u_r), then every
//                  wavefront adds L_rq^T z_r of the tiles it owns to its partial sums u_q
//                  (pipelined schedule: the panel wavefront, which holds no tile, runs the jets link of P6 beside it)
//   P6 simulate    state trajectory, primal in the reference variable order, first-move block.  Pipelined schedule: the
//                  momenta link and the CoM / RPY link with its integrators are one stream in one wavefront, a state row per
//                  lane, a half of the model per 16-lane row, the 3 x 3 products as DPP row_newbcast FMAs (no barrier
//                  inside); the other wavefronts expand the joints and send the inputs and the first move meanwhile.  SYRK
//                  form: the three links in three wavefronts, a chunk of stages apart
//                                                            (variableSamplingMPC.cpp:93-108,138-151)
//
// FP64 throughout.  The un-condensed KKT system the reference hands to OSQP has condition number
// ~1e12; the condensed Hessian factored here is benign (1e2..1e3).
//
// Measured on MI355X (profiles/r01_microbench_*.txt, tools/microbench/lat_probe.hip): v_mfma_f64_16x16x4_f64 issues
// every 64 cycles per SIMD (77.7 TFLOP/s chip-wide, already with one wavefront per SIMD), a dependent one every ~95; FP64
// VALU work does not hide under it (shared FP64 datapath); a lone wavefront issues one FP64 vector instruction per ~5.7
// cycles whatever the dependencies (a serial stream costs its instruction count), a v_readlane takes ~32 cycles to land.
// Hence: every index is compile-time or scalar, LDS offsets are immediates, and the matrix-core streams carry nothing but
// operand loads.
//
// This file and vsmpc_solve_body.inc hold the kernel body (P0 to P6 in one function: the phases share the LDS pointers and
// re-derive the work-item ids on purpose), the joint reduction it calls in P0, P1 and P6, and the launchers of one horizon; what the phases are built
// from is in one header each -- vsmpc_smem.hpp (tables, LDS carve-up), vsmpc_p0.hpp, vsmpc_p1_syrk.hpp, vsmpc_p1_struct.hpp,
// vsmpc_p3.hpp (P2 + P3), vsmpc_p4.hpp, vsmpc_p5.hpp.  A change here or there is checked against the previous build with
// tools/isa_diff.py.
#include <atomic>

#include "vsmpc_launch.hpp"
#include "vsmpc_p0.hpp"
#include "vsmpc_p1_syrk.hpp"
#include "vsmpc_p1_struct.hpp"
#include "vsmpc_p3.hpp"
#include "vsmpc_p4.hpp"
#include "vsmpc_p5.hpp"

#define VS_KIND_PRODUCTION 1   // the kinds of unit (see the launchers below); another name is 0: refused at the end of the file
#define VS_KIND_DIAGNOSTIC 2
#define VS_KIND_TUNED 3
#define VS_KIND_SMALL 4
#if !defined(VS_TU_HORIZON) || !defined(VS_TU_KIND) || (VS_TU_KIND == VS_KIND_TUNED && !defined(VS_TU_FORM))
#error "one unit per horizon and kind: -DVS_TU_HORIZON=N,NS,HC -DVS_TU_KIND=VS_KIND_..., tuned kind: -DVS_TU_FORM=0|1 (build.py)"
#endif

namespace vsmpc {

// ------------------------------------------------------------------------------------------------
// Joint reduction (see NJC in vsmpc_device.hpp), by ONE wavefront.  Householder QR of A = (Lambda W^(-1/2))^T (8 x 6):
// lane c < 6 carries column c of A (= row c of [Lambda_lin; Lambda_ang], scaled), lane 6 the vector b = w_reg W^(-1/2)
// q_err that rides along; step k takes its reflector from lane k (v_readlane broadcasts) and every lane behind applies
// it to its own column.  Leaves in LDS: R^T as the joint input matrix (rows 3..5 and 9..11 of Bj, columns 0..5), the
// reflectors v_k and beta_k (for the way back in P6), Q^T b (the gradient of the reduced unknowns), n = -N^T b and
// W^(-1/2).  No inverse, no division by a pivot: a rank-deficient Lambda (no thrust) leaves zero columns in R^T.
// ------------------------------------------------------------------------------------------------
// Steps K0 .. K1 - 1 of the six; a wavefront that does not start at 0 picks the columns up from LDS where the previous
// one left them (QR_A), so that the work can be spread over the idle stretches of different wavefronts: the first half in
// wavefront 3 during P0 (which has only copies to do there), the second half in a generator wavefront while it waits for
// the throttle chains -- a lone wavefront needs ~900 cycles per step (two reductions, a reciprocal square root and a
// reciprocal in one dependent chain).
template <class D, int K0 = 0, int K1 = NJC>
VS_DEV void p0_joint_reduction(double* __restrict__ sm, int lane) {
    using S = Smem<D>;
    static_assert(VSMPC_IN_LANG == VSMPC_IN_LLIN + 24, "Lambda_lin and Lambda_ang are adjacent in the record");
    const double* sIn = sm + S::oIn;
    const double* sCfg = sm + S::oCfg;
    double* sBj = sm + S::oBj;
    double* sQR = sm + S::oQR;
    const int c = lane < 6 ? lane : 6;   // lanes beyond 6 shadow lane 6 and store nothing
    double a[8];
    if constexpr (K0 == 0) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const double isw = fast_rsqrt(sCfg[CFG_WJ + j]);                       // uniform
            const double lam = sIn[VSMPC_IN_LLIN + (c < 6 ? c : 0) * 8 + j];
            const double bq = sCfg[CFG_WREG] * sIn[VSMPC_IN_QERR + j];             // costsVSMPC.cpp:586-590
            a[j] = (c < 6 ? lam : bq) * isw;
            if (lane == 0) sQR[S::QR_ISW + j] = isw;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) a[j] = sQR[S::QR_A + 8 * c + j];
    }
#pragma unroll
    for (int k = K0; k < K1; ++k) {
        // (sums as two or three partial chains: the dependent length is what a lone wavefront pays for)
        double s0 = a[k] * a[k], s1 = 0.0;
#pragma unroll
        for (int i = k + 1; i < 8; i += 2) {
            s1 = fma(a[i], a[i], s1);
            if (i + 1 < 8) s0 = fma(a[i + 1], a[i + 1], s0);
        }
        const double s = s0 + s1;
        const double sk = readlane_f64(s, k), xk = readlane_f64(a[k], k);      // the pivot column's, wave uniform
        const bool nz = sk > 1e-300;
        const double rs = fast_rsqrt(nz ? sk : 1.0);
        const double nrm = nz ? sk * rs : 0.0;
        const double alpha = xk >= 0.0 ? -nrm : nrm;
        const double beta = nz ? rs * fast_rcp(nrm + fabs(xk)) : 0.0;          // 1 / (nrm (nrm + |x_k|))
        double v[8];
        v[k] = xk - alpha;
#pragma unroll
        for (int i = k + 1; i < 8; ++i) v[i] = readlane_f64(a[i], k);
        double w0 = v[k] * a[k], w1 = 0.0;
#pragma unroll
        for (int i = k + 1; i < 8; i += 2) {
            w1 = fma(v[i], a[i], w1);
            if (i + 1 < 8) w0 = fma(v[i + 1], a[i + 1], w0);
        }
        const double w = (w0 + w1) * beta;
        const bool behind = lane > k;
#pragma unroll
        for (int i = k; i < 8; ++i) a[i] = behind ? fma(-w, v[i], a[i]) : a[i];
        a[k] = lane == k ? alpha : a[k];                                        // R[k][k]
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < 8; ++i) sQR[S::QR_V + 8 * k + i] = i >= k ? v[i] : 0.0;
            sQR[S::QR_BETA + k] = beta;
        }
    }
    if constexpr (K1 < NJC) {
        if (lane < 7) {
#pragma unroll
            for (int j = 0; j < 8; ++j) sQR[S::QR_A + 8 * lane + j] = a[j];
        }
        return;
    }
    if (lane < 6) {   // column `lane` of R = row `lane` of the input matrix R^T: entries k <= lane
        const int row = lane < 3 ? 3 + lane : 6 + lane;                         // momentum rows 3..5, 9..11
#pragma unroll
        for (int k = 0; k < NJC; ++k) sBj[row * NJ + k] = k <= lane ? a[k] : 0.0;
    } else if (lane == 6) {
#pragma unroll
        for (int k = 0; k < NJC; ++k) sQR[S::QR_GY + k] = a[k];
        sQR[S::QR_NS + 0] = -a[6];
        sQR[S::QR_NS + 1] = -a[7];
    }
}

// U = W^(-1/2) H_1 ... H_6 [y; n] for one joint block (the way back from the reduced unknowns).  Resumable: reflectors
// K1 - 1 down to K0; K1 = NJC loads [y; n], K0 = 0 ends with the scaling (P6 runs the first half beside its input-term pass)
template <class D, int K1 = NJC, int K0 = 0>
VS_DEV void joint_expand(const double* __restrict__ sQR, const double* __restrict__ y, double (&u)[8]) {
    using S = Smem<D>;
    if constexpr (K1 == NJC) {
#pragma unroll
        for (int i = 0; i < NJC; ++i) u[i] = y[i];
        u[6] = sQR[S::QR_NS + 0];
        u[7] = sQR[S::QR_NS + 1];
    }
#pragma unroll
    for (int k = K1 - 1; k >= K0; --k) {
        double t = 0.0;
#pragma unroll
        for (int i = k; i < 8; ++i) t = fma(sQR[S::QR_V + 8 * k + i], u[i], t);   // uniform addresses: LDS broadcasts
        t *= sQR[S::QR_BETA + k];
#pragma unroll
        for (int i = k; i < 8; ++i) u[i] = fma(-t, sQR[S::QR_V + 8 * k + i], u[i]);
    }
    if constexpr (K0 == 0) {
#pragma unroll
        for (int i = 0; i < 8; ++i) u[i] *= sQR[S::QR_ISW + i];
    }
}

// ------------------------------------------------------------------------------------------------
// the solve kernel
// ------------------------------------------------------------------------------------------------
// Kernel-argument block as it lies in the kernarg segment.  Everything but `in` and `batch` is needed late (outputs) or
// rarely (debug dumps, stamps): those are re-read from the kernarg segment where they are used instead of being held in
// (and spilled from) scalar registers for the whole kernel.  late_args() returns the segment pointer behind an opaque
// barrier, so the compiler cannot hoist the loads to the top of the kernel.
struct SolveArgs {
    DevCfg cfg;
    const double* in;
    int batch;
    int pad_;
    double* xout;
    double* fmout;
    int* status_out;
    int* iters_out;
    double* dbgM;
    double* dbgL;
    unsigned long long* stamps;
};
VS_DEV const SolveArgs* late_args() {
    const SolveArgs* ka = reinterpret_cast<const SolveArgs*>(
        (const void*)__builtin_amdgcn_kernarg_segment_ptr());
    asm volatile("" : "+s"(ka));
    return ka;
}

// STAMPS = true is the diagnostic build: thread 0 records s_memtime at every phase boundary into
// `stamps` (its own buffer, never read by the kernel).  The shipped instantiation has STAMPS = false.
// FORM selects how P1 condenses: 0 = sensitivity recursion + SYRK on the matrix cores (every horizon), 1 = structured
// condensing (P1s, horizons with Dims::STRUCT_P1; the default there).  Everything from P2 on is the same code; the two
// forms agree to rounding (different summation order), which tests/test_gpu_parity.py checks on the device.
// TUNED = true is the per-instance-tunables kind (vsmpc_solve_batch_tuned): `tun` holds one row of VSMPC_TUNE_SIZE doubles
// per instance, in sCfg order (vsmpc_pack_tunables), which P0 loads beside the record and writes to sCfg where the shared
// kind copies the kernel argument.  Nothing after P0 differs.  The body (vsmpc_solve_body.inc; its head says what an includer
// declares) is included under the three kernel entries below so that the shared kind keeps its name, arguments and code.
template <class D, bool STAMPS, int FORM = 0>
__global__ __launch_bounds__(D::BLOCK, D::WG_PER_CU) void solve_kernel(DevCfg cfg, const double* __restrict__ in, int batch,
                                                         double* xout_, double* fmout_, int* status_out_,
                                                         int* iters_out_, double* dbgM_, double* dbgL_,
                                                         unsigned long long* stamps_) {
    constexpr bool TUNED = false;
    constexpr bool SMALL = false;
    const double* const tun = nullptr;
#include "vsmpc_solve_body.inc"
}

// the tuned kind: the arguments of solve_kernel (SolveArgs is their common prefix) + the rows of tunables
template <class D, int FORM = 0>
__global__ __launch_bounds__(D::BLOCK, D::WG_PER_CU) void solve_kernel_tuned(DevCfg cfg, const double* __restrict__ in, int batch,
                                                         double* xout_, double* fmout_, int* status_out_,
                                                         int* iters_out_, double* dbgM_, double* dbgL_,
                                                         unsigned long long* stamps_, const double* __restrict__ tun) {
    constexpr bool STAMPS = false;
    constexpr bool TUNED = true;
    constexpr bool SMALL = false;
#include "vsmpc_solve_body.inc"
}

// the small-batch kind (horizons with has_small_kind<D>(), structured form): launched when the batch does not exceed the
// device's CUs, where a CU runs one workgroup whatever the kernel needs -- so it takes the LDS of a whole CU (Smem<D, true>)
// and forms most Hessian tiles beside the first two panel streams (SmallPlan, vsmpc_p3.hpp).  Same arguments, same
// arithmetic per tile and same workgroup barriers as solve_kernel<D, STAMPS, 1>: bit-identical outputs.  A name of its own:
// the resource tests of the shipped kernels match on theirs.  Registers: the 256 per lane of the shipped kernel -- with 512
// (__launch_bounds__(256, 1)) the allocator moved the tiles through 80 AGPRs and the launch took 33.2-33.5 us against
// 32.4-32.8 (profiles/small_batch_bench_alternating.txt).
template <class D, bool STAMPS>
__global__ __launch_bounds__(D::BLOCK, D::WG_PER_CU) void solve_kernel_small(DevCfg cfg, const double* __restrict__ in, int batch,
                                                         double* xout_, double* fmout_, int* status_out_,
                                                         int* iters_out_, double* dbgM_, double* dbgL_,
                                                         unsigned long long* stamps_) {
    constexpr bool TUNED = false;
    constexpr bool SMALL = true;
    constexpr int FORM = 1;
    const double* const tun = nullptr;
#include "vsmpc_solve_body.inc"
}

// ------------------------------------------------------------------------------------------------
// launchers of ONE horizon.  The kernels are straight-line template instantiations over Dims<nIter, nIterSmall,
// controlHorizon>, ~10 instantiations of a 30 k-instruction kernel per horizon, so build.py compiles this file once per
// horizon of csrc/vsmpc_horizons.def (-DVS_TU_HORIZON=N,NS,HC) and kind (-DVS_TU_KIND=), in parallel:
//   VS_KIND_PRODUCTION, VS_KIND_DIAGNOSTIC   the solve kernels of that horizon, as explicit instantiations of launch_solve_dims,
//                    which the dispatchers (vsmpc_dispatch.hip) only see declared (vsmpc_launch.hpp)
//   VS_KIND_TUNED    solve_kernel_tuned of that horizon and condensing form (-DVS_TU_FORM=0|1), as launch_solve_tuned_dims
//   VS_KIND_SMALL    solve_kernel_small (production and diagnostic) of that horizon, as launch_solve_small_dims
// ------------------------------------------------------------------------------------------------
// One launch, one workgroup per instance: `lds` bytes of dynamic LDS, allowed once per kernel and device (attr_set is the
// kernel's own, one per instantiation; allow_dynamic_lds, vsmpc_launch.hpp)
template <auto Kernel, class D, class... Args>
static hipError_t solve_launch(size_t lds, int batch, hipStream_t stream, Args... args) {
    static std::atomic<bool> attr_set[MAX_DEVICES];
    const hipError_t e = allow_dynamic_lds(reinterpret_cast<const void*>(Kernel), attr_set, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(Kernel, dim3(batch), dim3(D::BLOCK), lds, stream, args...);
    return hipGetLastError();
}

template <class D, bool STAMPS, int FORM>
static hipError_t launch_solve_f(const DevCfg& cfg, const double* d_in, int batch, double* d_x, double* d_fm, int* d_status,
                                 int* d_iters, double* dbgM, double* dbgL, unsigned long long* stamps, hipStream_t stream) {
    constexpr size_t lds = FORM == 1 ? Smem<D>::bytes_struct : Smem<D>::bytes;
    return solve_launch<solve_kernel<D, STAMPS, FORM>, D>(lds, batch, stream, cfg, d_in, batch, d_x, d_fm, d_status, d_iters, dbgM,
                                                          dbgL, stamps);
}

template <int N, int NS, int HC, bool STAMPS>
hipError_t launch_solve_dims(int form, const DevCfg& cfg, const double* d_in, int batch, double* d_x, double* d_fm,
                             int* d_status, int* d_iters, double* dbgM, double* dbgL, unsigned long long* stamps,
                             hipStream_t stream) {
    using D = Dims<N, NS, HC>;
    if constexpr (D::STRUCT_P1) {
        if (form != 2) return launch_solve_f<D, STAMPS, 1>(cfg, d_in, batch, d_x, d_fm, d_status, d_iters, dbgM, dbgL, stamps, stream);
    }
    return launch_solve_f<D, STAMPS, 0>(cfg, d_in, batch, d_x, d_fm, d_status, d_iters, dbgM, dbgL, stamps, stream);
}

template <int N, int NS, int HC>
hipError_t launch_solve_small_dims(const DevCfg& cfg, const double* d_in, int batch, double* d_x, double* d_fm, int* d_status,
                                   int* d_iters, unsigned long long* stamps, hipStream_t stream) {
    using D = Dims<N, NS, HC>;
    if constexpr (!has_small_kind<D>()) {
        return hipErrorInvalidValue;   // (launch_solve asks for the kind only where variant_has_small says the horizon has it)
    } else {
        constexpr size_t lds = Smem<D, true>::bytes_struct;
        static_assert(lds <= 160 * 1024, "the small-batch kind takes the LDS of one CU");
        double* const no_dump = nullptr;
        if (stamps != nullptr)
            return solve_launch<solve_kernel_small<D, true>, D>(lds, batch, stream, cfg, d_in, batch, d_x, d_fm, d_status, d_iters,
                                                                no_dump, no_dump, stamps);
        return solve_launch<solve_kernel_small<D, false>, D>(lds, batch, stream, cfg, d_in, batch, d_x, d_fm, d_status, d_iters,
                                                             no_dump, no_dump, stamps);
    }
}

template <int N, int NS, int HC, int FORM>
hipError_t launch_solve_tuned_dims(const DevCfg& cfg, const double* d_in, const double* d_tun, int batch, double* d_x,
                                   double* d_fm, int* d_status, int* d_iters, hipStream_t stream) {
    using D = Dims<N, NS, HC>;
    if constexpr (FORM == 1 && !D::STRUCT_P1) {
        return hipErrorInvalidValue;   // (launch_solve_tuned asks for the structured form only where the horizon has it)
    } else {
        constexpr size_t lds = FORM == 1 ? Smem<D>::bytes_struct : Smem<D>::bytes;
        static_assert(D::WG_PER_CU < 2 || lds <= 80 * 1024, "the tuned kind keeps two workgroups per CU");
        double* const no_dump = nullptr;
        unsigned long long* const no_stamps = nullptr;
        return solve_launch<solve_kernel_tuned<D, FORM>, D>(lds, batch, stream, cfg, d_in, batch, d_x, d_fm, d_status, d_iters,
                                                            no_dump, no_dump, no_stamps, d_tun);
    }
}

#define VS_INSTANTIATE_SOLVE(N, NS, HC, ST)                                                                              \
    template hipError_t launch_solve_dims<N, NS, HC, ST>(int, const DevCfg&, const double*, int, double*, double*, int*, \
                                                         int*, double*, double*, unsigned long long*, hipStream_t);
#define VS_INSTANTIATE_TUNED(N, NS, HC, F)                                                                                 \
    template hipError_t launch_solve_tuned_dims<N, NS, HC, F>(const DevCfg&, const double*, const double*, int, double*, \
                                                              double*, int*, int*, hipStream_t);
#define VS_TU_APPLY(M, ...) M(__VA_ARGS__)
#define VS_INSTANTIATE_SMALL(N, NS, HC)                                                                              \
    template hipError_t launch_solve_small_dims<N, NS, HC>(const DevCfg&, const double*, int, double*, double*, int*, int*, \
                                                           unsigned long long*, hipStream_t);
#if VS_TU_KIND == VS_KIND_SMALL
VS_TU_APPLY(VS_INSTANTIATE_SMALL, VS_TU_HORIZON)
#elif VS_TU_KIND == VS_KIND_TUNED
VS_TU_APPLY(VS_INSTANTIATE_TUNED, VS_TU_HORIZON, VS_TU_FORM)
#elif VS_TU_KIND == VS_KIND_DIAGNOSTIC
VS_TU_APPLY(VS_INSTANTIATE_SOLVE, VS_TU_HORIZON, true)
#elif VS_TU_KIND == VS_KIND_PRODUCTION
VS_TU_APPLY(VS_INSTANTIATE_SOLVE, VS_TU_HORIZON, false)
#else
#error "VS_TU_KIND is none of VS_KIND_PRODUCTION, VS_KIND_DIAGNOSTIC, VS_KIND_TUNED, VS_KIND_SMALL"
#endif

}  // namespace vsmpc
