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
//
// solve_kernel_rt_tuned (vsmpc_solve_batch_tuned) is the same body with the weights and the throttle box read from the
// instance's row of tunables in LDS instead of the kernel argument.
// sens_kernel_rt (vsmpc_sensitivity_batch) is the same body (vsmpc_runtime_body.inc) with SENS = true; solve_kernel_rt's
// code is not changed by it.  X0 enters the QP only through the initial-state rows, so the solution's Jacobian with
// respect to X0 is that of the final active set's affine piece ("Sensitivities"; executable model:
// tests/sensitivity_model.py):
//   P1  26 parameter columns after the affine one (NP = NZ + 27 rows): column NZ + 1 + i starts from X_0 = e_i, takes no
//       input, no c and no reference, so that C's parameter rows hold F = d(condensed gradient)/dX0
//   P2  nothing: the input costs and their gradient terms belong to the affine row
//   P3  the same Cholesky reduces the parameter rows to F~ (throttle columns) and l~ (joint columns)
//   P4  after the box QP, on a Solved exit, with the factor of S_FF the last iteration left in LDS (the final free set):
//       S_FF dv_F = -F~_F, dv = 0 on bound and pinned throttles
//   P5  L_jj^T du = -(L_vj^T dv + l~)
//   P6  dX_0 = I, dX_{k+1} = dX_k + dt_k (A dX_k + Bj dU + Bt dV)
// The 26 right-hand sides of P4 / P5 are solved in place in the parameter rows of the workspace, which then hold dz/dX0.
#include <atomic>
#include <cstddef>

#include "vsmpc_launch.hpp"
#include "vsmpc_p0.hpp"

namespace vsmpc {

namespace {

constexpr int RT_BLOCK = 256;
constexpr int RT_CPT = 2;    // columns per thread: NP <= 8 * 40 + 4 * 39 + 1 = 477 (+ 26 parameter columns: 503) < 512
constexpr int RT_NPAR = NX;  // parameter columns of sens_kernel_rt: one per entry of X0
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
    s.big = p;   // max(18 NP, NV (NV + 1) / 2), and 2 x 26 x 26 with SENS
    return s;
}

// symmetric access to the Schur complement S (trailing block of the workspace) by throttle indices
VS_DEV double rt_S(const double* __restrict__ M, int nu, int p, int q) {
    return p >= q ? M[tri(nu + p) + nu + q] : M[tri(nu + q) + nu + p];
}

// the largest dynamic LDS once per kernel and device: every horizon launches under it
constexpr int RT_MAX_DEV = 64;
hipError_t rt_allow_lds(const void* kernel, std::atomic<bool> (&attr_set)[RT_MAX_DEV], const RtDims& d) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= RT_MAX_DEV) return hipErrorInvalidDevice;
    if (runtime_lds_bytes(d) > RT_MAX_LDS) return hipErrorInvalidValue;
    if (!attr_set[dev].load(std::memory_order_acquire)) {
        e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, int(RT_MAX_LDS));
        if (e != hipSuccess) return e;
        attr_set[dev].store(true, std::memory_order_release);
    }
    return hipSuccess;
}

}  // namespace

__global__ __launch_bounds__(RT_BLOCK) void solve_kernel_rt(DevCfg cfg, RtDims d, const double* __restrict__ in,
                                                            double* __restrict__ ws, double* __restrict__ xout,
                                                            double* __restrict__ fmout, int* __restrict__ status_out,
                                                            int* __restrict__ iters_out) {
    constexpr bool SENS = false;
    double* const dxout = nullptr;
    double* const dfmout = nullptr;
    int* const active_out = nullptr;
    int* const flags_out = nullptr;
#include "vsmpc_runtime_body.inc"
}

// solve_kernel_rt + the 26 parameter columns and the outputs dx_dx0 [nVar][26], dfm_dx0 [24][26], active [NV] and the
// sensitivity flags (per instance, each may be null)
__global__ __launch_bounds__(RT_BLOCK) void sens_kernel_rt(DevCfg cfg, RtDims d, const double* __restrict__ in,
                                                           double* __restrict__ ws, double* __restrict__ xout,
                                                           double* __restrict__ fmout, int* __restrict__ status_out,
                                                           int* __restrict__ iters_out, double* __restrict__ dxout,
                                                           double* __restrict__ dfmout, int* __restrict__ active_out,
                                                           int* __restrict__ flags_out) {
    constexpr bool SENS = true;
#include "vsmpc_runtime_body.inc"
}

// solve_kernel_rt with per-instance tunables (vsmpc_solve_batch_tuned on a runtime handle): the instance's row of `tun`
// ([batch][VSMPC_TUNE_SIZE], sCfg order) is staged in LDS and stands where the body reads the weights and the throttle box
// of the kernel argument; cfg.dt, cfg.use_jet and cfg.max_as_iter stay the handle's.
struct RtTunCfg {   // LDS image: the row (CFG_* order), then what the body reads of the handle's DevCfg
    double sq[NWROWS], wj[NJ], w_reg, w_thr, w_init, vmin, vmax, pad_;
    double dt[MAX_STAGES];
    int use_jet, max_as_iter;
};
static_assert(offsetof(RtTunCfg, wj) == CFG_WJ * sizeof(double) && offsetof(RtTunCfg, vmax) == CFG_VMAX * sizeof(double) &&
              offsetof(RtTunCfg, dt) == CFG_SIZE * sizeof(double) && CFG_SIZE == VSMPC_TUNE_SIZE && sizeof(RtTunCfg) % 8 == 0,
              "a row of tunables is the head of RtTunCfg");
__global__ __launch_bounds__(RT_BLOCK) void solve_kernel_rt_tuned(DevCfg hcfg, RtDims d, const double* __restrict__ in,
                                                                  double* __restrict__ ws, double* __restrict__ xout,
                                                                  double* __restrict__ fmout, int* __restrict__ status_out,
                                                                  int* __restrict__ iters_out,
                                                                  const double* __restrict__ tun) {
    constexpr bool SENS = false;
    double* const dxout = nullptr;
    double* const dfmout = nullptr;
    int* const active_out = nullptr;
    int* const flags_out = nullptr;
    extern __shared__ __attribute__((aligned(16))) double smem_tuned[];
    double* const sTun = smem_tuned + d.lds_doubles;   // behind the body's carve-up (the launcher adds sizeof(RtTunCfg))
    RtTunCfg& tcfg = *reinterpret_cast<RtTunCfg*>(sTun);
    {
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
    }
    const RtTunCfg& cfg = tcfg;
#include "vsmpc_runtime_body.inc"
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

RtDims runtime_dims(int n_iter, int n_iter_small, int control_horizon, bool sensitivity) {
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
    const int fixed = ((d.nin + 1) & ~1) + RT_LIN + 4 + MAX_STAGES + NWROWS + 2 + NX * (d.n + 1) + ((d.nz + 1) & ~1) +
                      ((d.np + 1) & ~1) + RT_BLOCK + 3 * ((d.nv + 1) & ~1) + 2 * ((d.nv + 1) / 2 + 1) + 4;
    const int ybuf = NWROWS * d.np, kbuf = d.nv * (d.nv + 1) / 2, dxbuf = sensitivity ? 2 * NX * RT_NPAR : 0;
    const int big = ybuf > kbuf ? ybuf : kbuf;
    d.lds_doubles = fixed + (big > dxbuf ? big : dxbuf);
    return d;
}

size_t runtime_lds_bytes(const RtDims& d) { return size_t(d.lds_doubles) * sizeof(double); }

hipError_t launch_solve_runtime(const RtDims& d, const DevCfg& cfg, const double* d_in, int batch, double* d_ws, double* d_x,
                                double* d_fm, int* d_status, int* d_iters, hipStream_t stream) {
    static std::atomic<bool> attr_set[RT_MAX_DEV];
    const hipError_t e = rt_allow_lds(reinterpret_cast<const void*>(&solve_kernel_rt), attr_set, d);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(solve_kernel_rt, dim3(batch), dim3(RT_BLOCK), runtime_lds_bytes(d), stream, cfg, d, d_in, d_ws, d_x,
                       d_fm, d_status, d_iters);
    return hipGetLastError();
}

hipError_t launch_solve_runtime_tuned(const RtDims& d, const DevCfg& cfg, const double* d_in, const double* d_tun, int batch,
                                      double* d_ws, double* d_x, double* d_fm, int* d_status, int* d_iters,
                                      hipStream_t stream) {
    static std::atomic<bool> attr_set[RT_MAX_DEV];
    const size_t lds = runtime_lds_bytes(d) + sizeof(RtTunCfg);            // the staged row lies behind the body's carve-up
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
    static std::atomic<bool> attr_set[RT_MAX_DEV];
    if (d.np != d.nz + 1 + RT_NPAR || d.np > RT_BLOCK * RT_CPT) return hipErrorInvalidValue;   // runtime_dims(.., true)
    const hipError_t e = rt_allow_lds(reinterpret_cast<const void*>(&sens_kernel_rt), attr_set, d);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(sens_kernel_rt, dim3(batch), dim3(RT_BLOCK), runtime_lds_bytes(d), stream, cfg, d, d_in, d_ws, d_x,
                       d_fm, d_status, d_iters, d_dx, d_dfm, d_active, d_flags);
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
