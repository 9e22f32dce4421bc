// Runtime-sized solve kernels (gfx950): any horizon config_valid() accepts, sized by kernel arguments instead of template
// parameters, so that a configuration outside csrc/vsmpc_horizons.def runs without a rebuild
// (variableSamplingMPC.cpp:24-45 sizes the reference from its XML at run time).
//
// One workgroup of 256 threads per instance computes what solve_kernel computes -- same input record, primal in the
// reference variable order, first-move block, status and active-set iterations -- by the plainest route: the phase
// functions P0 .. P6 of vsmpc_rt_core.hpp, which rt_solve below calls in order.  Split as the tuned kernel is:
//   vsmpc_rt_core.hpp     constants, the LDS carve-up, RtCtx, the substitution helpers, P0 .. P6, rt_write_solution
//   vsmpc_rt_sens.hpp     the four extra phases of sens_kernel_rt (vsmpc_sensitivity_batch): rt_solve<RT_SENS>
//   vsmpc_rt_adjoint.hpp  the five extra phases of adjoint_kernel_rt[_tuned] (vsmpc_adjoint_batch): rt_solve<RT_ADJOINT>
//   vsmpc_rt_adjoint_record.hpp  the two phases adjoint_record_kernel_rt[_tuned] (vsmpc_adjoint_record_batch) add to those:
//                         rt_solve<RT_ADJOINT_REC>
//   this file             RtTunCfg and its staging, rt_solve, the kernels, runtime_dims and launch_runtime: the one launcher
//                         of the family, which picks the kernel from an RtMode and unpacks an RtLaunch (vsmpc_launch.hpp:
//                         every pointer of a launch by name) into the kernel's positional arguments
//
// The phases that read the configuration take its type as a template parameter: DevCfg, the kernel argument
// (solve_kernel_rt, sens_kernel_rt), or RtTunCfg, the instance's row of tunables staged in LDS (solve_kernel_rt_tuned,
// vsmpc_solve_batch_tuned).
#include <atomic>
#include <cstddef>
#include <type_traits>

#include "vsmpc_rt_core.hpp"
#include "vsmpc_rt_sens.hpp"
#include "vsmpc_rt_adjoint.hpp"
#include "vsmpc_rt_adjoint_record.hpp"

namespace vsmpc {

namespace {

// The solve of one instance: the phases in order.  cfg is a DevCfg or an RtTunCfg; `sens` is looked at with RT_SENS only,
// `adj` with RT_ADJOINT and RT_ADJOINT_REC only, `rec` with RT_ADJOINT_REC only.
template <RtMode MODE, class Cfg>
VS_DEV void rt_solve(const Cfg& cfg, const RtDims& d, const double* in, double* ws, double* xout, double* fmout,
                     int* status_out, int* iters_out, const RtSensOut& sens = {}, const RtAdjIO& adj = {},
                     const RtAdjRecOut& rec = {}) {
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
    if constexpr (MODE == RT_ADJOINT || MODE == RT_ADJOINT_REC) {
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
        if constexpr (MODE == RT_ADJOINT_REC) {
            if (adj_ok && !nonfinite) rt_adj_model(c, cfg);
            rt_adj_record(c, cfg, box, adj_ok, nonfinite, rec);
        }
    }
}

}  // namespace

// Positional __restrict__ pointers are the kernels' ABI: in by-value structs they lose alias analysis (+86..131 instructions, measured)
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

// adjoint_kernel_rt + the record phases: dL/d record [batch][n_in] and dL/d(A | Bj | Bt | c) [batch][VSMPC_GRAD_MODEL_SIZE] out
// as well (each may be null)
__global__ __launch_bounds__(RT_BLOCK) void adjoint_record_kernel_rt(DevCfg cfg, RtDims d, const double* __restrict__ in,
                                                                     double* __restrict__ ws, double* __restrict__ xout,
                                                                     double* __restrict__ fmout, int* __restrict__ status_out,
                                                                     int* __restrict__ iters_out, const double* __restrict__ xbar,
                                                                     const double* __restrict__ fmbar, double* __restrict__ gx0,
                                                                     double* __restrict__ gcfg, int* __restrict__ active_out,
                                                                     int* __restrict__ flags_out, double* __restrict__ gin,
                                                                     double* __restrict__ gmodel) {
    rt_solve<RT_ADJOINT_REC>(cfg, d, in, ws, xout, fmout, status_out, iters_out, RtSensOut{},
                             RtAdjIO{xbar, fmbar, gx0, gcfg, active_out, flags_out}, RtAdjRecOut{gin, gmodel});
}
// the same with per-instance tunables, staged as in solve_kernel_rt_tuned
__global__ __launch_bounds__(RT_BLOCK) void adjoint_record_kernel_rt_tuned(DevCfg hcfg, RtDims d, const double* __restrict__ in,
                                                                           double* __restrict__ ws, double* __restrict__ xout,
                                                                           double* __restrict__ fmout, int* __restrict__ status_out,
                                                                           int* __restrict__ iters_out,
                                                                           const double* __restrict__ xbar,
                                                                           const double* __restrict__ fmbar, double* __restrict__ gx0,
                                                                           double* __restrict__ gcfg, int* __restrict__ active_out,
                                                                           int* __restrict__ flags_out, double* __restrict__ gin,
                                                                           double* __restrict__ gmodel,
                                                                           const double* __restrict__ tun) {
    const RtTunCfg& tcfg = rt_stage_tunables(hcfg, d, tun);
    rt_solve<RT_ADJOINT_REC>(tcfg, d, in, ws, xout, fmout, status_out, iters_out, RtSensOut{},
                             RtAdjIO{xbar, fmbar, gx0, gcfg, active_out, flags_out}, RtAdjRecOut{gin, gmodel});
}

// linearize_kernel_rt's LDS (doubles): the record, p0_linearize's block, the previous throttles
struct LinLdsOff { int lin, vprev, size; };
VS_HD LinLdsOff lin_lds_offsets(int n_in) {
    LinLdsOff o;
    o.lin = (n_in + 1) & ~1;
    o.vprev = o.lin + LIN_DOUBLES;
    o.size = o.vprev + 4;
    return o;
}
__global__ __launch_bounds__(RT_BLOCK) void linearize_kernel_rt(DevCfg cfg, int n_in, const double* __restrict__ in,
                                                                double* __restrict__ A, double* __restrict__ Bj,
                                                                double* __restrict__ Bt, double* __restrict__ c) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const LinLdsOff o = lin_lds_offsets(n_in);
    double* sIn = smem;
    double* sA = smem + o.lin;
    double* sBj = sA + NX * NX;
    double* sBt = sBj + NX * NJ;
    double* sC = sBt + NX * NTH;
    double* sVprev = smem + o.vprev;
    const int tid = threadIdx.x, b = blockIdx.x;
    for (int i = tid; i < n_in; i += RT_BLOCK) sIn[i] = in[size_t(b) * n_in + i];
    __syncthreads();
    p0_linearize(cfg.use_jet, sIn, sA, sBj, sBt, sC, sVprev, tid, RT_BLOCK);
    for (int i = tid; i < NX * NX; i += RT_BLOCK) A[size_t(b) * NX * NX + i] = sA[i];
    for (int i = tid; i < NX * NJ; i += RT_BLOCK) Bj[size_t(b) * NX * NJ + i] = sBj[i];
    for (int i = tid; i < NX * NTH; i += RT_BLOCK) Bt[size_t(b) * NX * NTH + i] = sBt[i];
    for (int i = tid; i < NX; i += RT_BLOCK) c[size_t(b) * NX + i] = sC[i];
}

RtDims runtime_dims(int n_iter, int n_iter_small, int control_horizon, bool sensitivity, bool adjoint, bool adjoint_record) {
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
    int big = rt_big_condense(d) > rt_big_box_qp(d) ? rt_big_condense(d) : rt_big_box_qp(d);   // s.big holds one at a time
    if (sensitivity && RT_BIG_SENS > big) big = RT_BIG_SENS;
    if (adjoint && rt_big_adjoint(d) > big) big = rt_big_adjoint(d);
    if (adjoint_record && rt_big_adjoint_record(d) > big) big = rt_big_adjoint_record(d);
    d.lds_doubles = int(rt_carve(d, size_t(0)).big) + big;
    return d;
}

size_t runtime_lds_bytes(const RtDims& d) { return size_t(d.lds_doubles) * sizeof(double); }

size_t runtime_tuned_lds_bytes(const RtDims& d) { return runtime_lds_bytes(d) + sizeof(RtTunCfg); }

// The one launcher: every horizon launches under the largest dynamic LDS, allowed once per kernel and device (attr_set is
// the kernel's own, one per instantiation)
template <auto Kernel, class... Args>
hipError_t rt_launch(size_t lds, int batch, hipStream_t stream, Args... args) {
    static std::atomic<bool> attr_set[MAX_DEVICES];
    if (lds > RT_MAX_LDS) return hipErrorInvalidValue;
    const hipError_t e = allow_dynamic_lds(reinterpret_cast<const void*>(Kernel), attr_set, RT_MAX_LDS);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(Kernel, dim3(batch), dim3(RT_BLOCK), lds, stream, args...);
    return hipGetLastError();
}

// One kind of the family: Kernel, or Tuned (nullptr: the kind has none) when the launch carries rows of tunables.  Here, and
// nowhere else, an RtLaunch becomes positional arguments: the eight every kernel begins with, the kind's own (`more`, in
// the order of its kernel's signature), and the rows last.  The staged row of the tuned kernel lies behind the body's
// carve-up (the largest valid horizon needs 129 KB).
template <auto Kernel, auto Tuned, class... More>
hipError_t rt_launch_kind(const RtDims& d, const DevCfg& cfg, int batch, const RtLaunch& a, hipStream_t stream, More... more) {
    if (a.tun == nullptr)
        return rt_launch<Kernel>(runtime_lds_bytes(d), batch, stream, cfg, d, a.in, a.ws, a.x, a.fm, a.status, a.iters, more...);
    if constexpr (!std::is_null_pointer_v<decltype(Tuned)>)
        return rt_launch<Tuned>(runtime_tuned_lds_bytes(d), batch, stream, cfg, d, a.in, a.ws, a.x, a.fm, a.status, a.iters,
                                more..., a.tun);
    else
        return hipErrorInvalidValue;
}

hipError_t launch_runtime(RtMode kind, const RtDims& d, const DevCfg& cfg, int batch, const RtLaunch& a, hipStream_t stream) {
    static_assert(VSMPC_GRAD_SIZE * RT_NWAVES <= RT_BLOCK && 2 * NX + RT_NWAVES <= RT_BLOCK, "s.red holds the partial sums and lambda");
    static_assert(2 * NX <= RT_BLOCK, "s.red holds nu_k and nu_{k-1}");
    switch (kind) {
        case RT_SOLVE:
            return rt_launch_kind<solve_kernel_rt, solve_kernel_rt_tuned>(d, cfg, batch, a, stream);
        case RT_SENS:
            if (d.np != d.nz + 1 + RT_NPAR || d.np > RT_BLOCK * RT_CPT) return hipErrorInvalidValue;   // runtime_dims(.., true)
            return rt_launch_kind<sens_kernel_rt, nullptr>(d, cfg, batch, a, stream, a.dx, a.dfm, a.active, a.flags);
        case RT_ADJOINT:
            if (d.np != d.nz + 1) return hipErrorInvalidValue;                                    // runtime_dims(.., false, true)
            return rt_launch_kind<adjoint_kernel_rt, adjoint_kernel_rt_tuned>(d, cfg, batch, a, stream, a.xbar, a.fmbar, a.gx0,
                                                                              a.gcfg, a.active, a.flags);
        case RT_ADJOINT_REC:
            // runtime_dims(.., false, true, true): s.big holds G behind a_X and the costates
            if (d.np != d.nz + 1 || d.lds_doubles < int(rt_carve(d, size_t(0)).big) + rt_big_adjoint_record(d)) return hipErrorInvalidValue;
            return rt_launch_kind<adjoint_record_kernel_rt, adjoint_record_kernel_rt_tuned>(
                d, cfg, batch, a, stream, a.xbar, a.fmbar, a.gx0, a.gcfg, a.active, a.flags, a.gin, a.gmodel);
    }
    return hipErrorInvalidValue;
}

hipError_t launch_linearize_runtime(const RtDims& d, const DevCfg& cfg, const double* d_in, int batch, double* A, double* Bj,
                                    double* Bt, double* c, hipStream_t stream) {
    return rt_launch<linearize_kernel_rt>(size_t(lin_lds_offsets(d.nin).size) * sizeof(double), batch, stream, cfg, d.nin, d_in,
                                          A, Bj, Bt, c);
}

const char* runtime_kernel_name() { return "solve_kernel_rt"; }

}  // namespace vsmpc
