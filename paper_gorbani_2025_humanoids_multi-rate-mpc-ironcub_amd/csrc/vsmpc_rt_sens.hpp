// The sensitivity entry of the runtime-sized kernels: what sens_kernel_rt adds to the solve (included by vsmpc_runtime.hip
// after vsmpc_rt_core.hpp).
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
#pragma once
#include "vsmpc_rt_core.hpp"

namespace vsmpc {

namespace {

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
constexpr int RT_BIG_SENS = 2 * NX * RT_NPAR;   // s.big: dX_k | dX_{k+1}
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

// ---- the outputs of the sensitivity entry that rt_sens_states did not write
// Reads dz/dX0 in the parameter rows, zv, s.state, the reduced gradient s and the gradient at z in s.vec2.  Writes dx_dx0
// (dX_0 = I and the joint / throttle rows), dfm_dx0 (joint increments, v0, throttle percent) -- all zero unless sens_ok --
// the active set and the VSMPC_SENS_* flags.
VS_DEV void rt_sens_write(const RtCtx& c, const RtBox box, bool factored, bool sens_ok, const RtSensOut& out) {
    const RtDims& d = c.d;
    const RtSmem s = c.lds();
    const int tid = c.tid, inst = c.inst, NZ = d.nz, NU = d.nu;
    double* M = c.M;
    double* zv = s.z + NU;
    double* const dxout = out.dx;
    double* const dfmout = out.dfm;
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
    rt_write_active(c, box, factored, out.active);
    if (tid == 0 && flags_out != nullptr)
        flags_out[inst] = !sens_ok ? VSMPC_SENS_UNSOLVED : (rt_degenerate(c, box) ? VSMPC_SENS_DEGENERATE : 0);
}

}  // namespace

}  // namespace vsmpc
