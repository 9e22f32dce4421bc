// Duals and KKT certificate of a given primal (gfx950): certify_kernel, behind vsmpc_certify_batch[_device].
//
// Restates, for the structure of this QP, what the oracle does with dense matrices (the module is cited in
// include/vsmpc.h): the duals of its solve_exact (OSQP's sign: y > 0 where the upper bound is active, y < 0 where the
// lower one is) and the certificate of its kkt_certificate, on the QP of its assemble_dense (IMPCProblem.cpp:150-194;
// rows: dynamics constraintsVSMPC.cpp:76-131, initial state IQPUtilsMPC.cpp:71-92, throttle box constraintsVSMPC.cpp:
// 338-365; costs costsVSMPC.cpp:166-200,375-409,468-487,558-592).  It never runs the solver's code: x is an input, from wherever.
//
// With x given, stationarity of the state columns DEFINES the equality duals (one backward costate recursion through A),
// stationarity of the throttle columns DEFINES the box multipliers, and what is left of Hx + g + Ac^T y is the joint
// columns' gradient ("Duals and certificate"; executable model: tests/certificate_model.py):
//   y_{N-1} = Q (X_N - xr_N),   y_{i-1} = Q (X_i - xr_i) + (I + dt_i A)^T y_i,   y_init = -(I + dt_0 A)^T y_0
//   mu_t    = -(gV_t + sum_{i: tb(i) = t} dt_i Bt^T y_i)
//   stat_j  = (W_dq + w_reg I) U_j + w_reg q_err + sum_{i: jb(i) = j} dt_i Bj^T y_i
//
// One workgroup of 256 threads per instance, sizes as kernel arguments (RtDims): every horizon the configuration check
// accepts, on tuned and runtime handles alike.
//   load      record, x and the row of tunables (or the handle's DevCfg) into LDS, 16 bytes per lane
//   P0        p0_linearize (vsmpc_p0.hpp, the solve kernels' own) into LDS
//   phase A   wavefront 0: the costate recursion, lane = state row, its column of A in registers, y_i broadcast from LDS;
//             wavefronts 1..3 meanwhile: one (stage, row) pair per lane and pass -- the dynamics row's residual (only the
//             structural non-zeros of the row of A, Bj, Bt), the node's share of the scale and of the objective -- and the
//             initial-state rows
//   phase B   one (block, entry) pair per lane: the contractions sum dt_i B^T y_i, joint gradient, throttle multiplier,
//             box violation and complementarity, their shares of scale and objective
//   reduce    per-lane partials -> butterfly inside the wavefront -> four partials through LDS, combined in wavefront order
// Every sum has a fixed order that depends on the sizes only (no atomics): repeated and permuted batches are bit-identical.
// max() drops a NaN, so non-finite data is carried as a flag: a non-finite record, tunable, x or dual makes STATIONARITY
// and PRIMAL NaN.
#include "vsmpc_launch.hpp"
#include "vsmpc_p0.hpp"
#include "vsmpc_structure.hpp"

namespace vsmpc {

namespace {

constexpr int CB = 256;
// running maximum that remembers a non-finite candidate (fmax drops a NaN)
VS_DEV void take_max(double& m, double v, double& bad) {
    m = fmax(m, v);
    bad = isfinite(v) ? bad : 1.0;
}

struct CertSmem {
    double *in, *lin, *vprev, *cfg, *dt, *x, *y, *red;
};
VS_DEV CertSmem cert_smem(const RtDims& d, int ncon, double* base) {
    CertSmem s;
    double* p = base;
    s.in = p;    p += (d.nin + 1) & ~1;
    s.lin = p;   p += LIN_DOUBLES;
    s.vprev = p; p += 4;
    s.cfg = p;   p += CFG_SIZE;
    s.dt = p;    p += MAX_STAGES;
    s.x = p;     p += (d.nvar + 1) & ~1;
    s.y = p;     p += (ncon + 1) & ~1;
    s.red = p;   // 4 wavefronts x VSMPC_CERT_SIZE
    return s;
}

VS_HD int cert_ncon(const RtDims& d) { return d.nxs + NTH * (d.n - d.ns + 1); }
VS_HD int cert_lds_doubles(const RtDims& d) {
    return ((d.nin + 1) & ~1) + LIN_DOUBLES + 4 + CFG_SIZE + MAX_STAGES + ((d.nvar + 1) & ~1) + ((cert_ncon(d) + 1) & ~1) +
           4 * VSMPC_CERT_SIZE;
}

}  // namespace

// in [batch][nin], x [batch][nvar] (reference variable order), tun [batch][VSMPC_TUNE_SIZE] or null (the handle's DevCfg),
// y [batch][nCon] or null, cert [batch][VSMPC_CERT_SIZE].  in, x, tun and y are 16-byte aligned (nin, nvar, nCon are even).
__global__ __launch_bounds__(CB) void certify_kernel(DevCfg cfg, RtDims d, const double* __restrict__ in,
                                                     const double* __restrict__ x, const double* __restrict__ tun,
                                                     double* __restrict__ yout, double* __restrict__ cert) {
    extern __shared__ __attribute__((aligned(16))) double smem_cert[];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int N = d.n, ncon = cert_ncon(d);
    const CertSmem s = cert_smem(d, ncon, smem_cert);
    const double* __restrict__ sA = s.lin;
    const double* __restrict__ sBj = sA + NX * NX;
    const double* __restrict__ sBt = sBj + NX * NJ;
    const double* __restrict__ sC = sBt + NX * NTH;
    const int offJ = d.nxs, offV = d.nxs + d.nu;

    double bad = 0.0;   // 1 once anything non-finite was seen by this lane
    // ---- load: 16 bytes per lane
    {
        const double2* in2 = reinterpret_cast<const double2*>(in + size_t(b) * d.nin);
        for (int i = tid; i < d.nin / 2; i += CB) {
            const double2 v = in2[i];
            reinterpret_cast<double2*>(s.in)[i] = v;
            bad = (isfinite(v.x) && isfinite(v.y)) ? bad : 1.0;
        }
        const double2* x2 = reinterpret_cast<const double2*>(x + size_t(b) * d.nvar);
        for (int i = tid; i < d.nvar / 2; i += CB) {
            const double2 v = x2[i];
            reinterpret_cast<double2*>(s.x)[i] = v;
            bad = (isfinite(v.x) && isfinite(v.y)) ? bad : 1.0;
        }
        if (tun != nullptr) {
            if (tid < CFG_SIZE / 2) {
                const double2 v = reinterpret_cast<const double2*>(tun + size_t(b) * CFG_SIZE)[tid];
                reinterpret_cast<double2*>(s.cfg)[tid] = v;
                bad = (isfinite(v.x) && (isfinite(v.y) || tid == CFG_SIZE / 2 - 1)) ? bad : 1.0;   // (the pad entry is not looked at)
            }
        } else if (tid < NWROWS) {
            s.cfg[CFG_SQ + tid] = cfg.sq[tid];
        } else if (tid >= 32 && tid < 32 + NJ) {
            s.cfg[CFG_WJ + tid - 32] = cfg.wj[tid - 32];
        } else if (tid == 64) {
            s.cfg[CFG_WREG] = cfg.w_reg;
            s.cfg[CFG_WTHR] = cfg.w_thr;
            s.cfg[CFG_WINIT] = cfg.w_init;
            s.cfg[CFG_VMIN] = cfg.vmin;
            s.cfg[CFG_VMAX] = cfg.vmax;
            s.cfg[CFG_SIZE - 1] = 0.0;
        }
        if (tid >= 128 && tid < 128 + MAX_STAGES) s.dt[tid - 128] = cfg.dt[tid - 128];
        // throttle rows of y behind the last filled block: exactly 0 (constraintsVSMPC.cpp:338-365 leaves them [0, 0])
        for (int i = (N + 1) * NX + d.nv + tid; i < ncon; i += CB) s.y[i] = 0.0;
    }
    __syncthreads();
    p0_linearize(cfg.use_jet, s.in, s.lin, s.lin + NX * NX, s.lin + NX * NX + NX * NJ,
                          s.lin + NX * NX + NX * NJ + NX * NTH, s.vprev, tid, CB);

    // per-lane partials of the certificate
    double m_stat = 0.0, m_scale = 1.0, m_prim = 0.0, m_comp = 0.0, m_dual = 0.0, obj = 0.0;

    // ---- phase A
    if (tid < 64) {
        // costate recursion, lane q = state row (lanes >= 26 repeat row 25 and store nothing)
        const int q = tid < NX ? tid : NX - 1;
        double acol[NX];   // column q of A: row q of A^T
#pragma unroll
        for (int r = 0; r < NX; ++r) acol[r] = sA[r * NX + q];
        const double qd = q_diag(s.cfg + CFG_SQ, q);
        const int qx = q < 12 ? q : 11;           // reference rows 0..11 only: loaded unconditionally, selected afterwards
        double yv;
        {
            const int col = (N - 1) < d.ns ? 0 : (N - 1) - d.ns;                  // costsVSMPC.cpp:191-200
            const double xr = s.in[VSMPC_IN_XREF + col * 12 + qx];
            yv = qd * (s.x[N * NX + q] - (q < 12 ? xr : 0.0));                    // y_{N-1} = Q (X_N - xr_N)
            if (tid < NX) s.y[(N - 1) * NX + q] = yv;
            take_max(m_dual, fabs(yv), bad);
        }
        for (int i = N - 1; i >= 0; --i) {
            // lanes of this wavefront exchange y_i through LDS: order the store above against the loads below
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            const double* __restrict__ yi = s.y + i * NX;
            double t0 = 0.0, t1 = 0.0;             // (A^T y_i)_q in two chains
#pragma unroll
            for (int r = 0; r < NX; r += 2) {
                t0 = fma(acol[r], yi[r], t0);
                t1 = fma(acol[r + 1], yi[r + 1], t1);
            }
            const double prop = fma(s.dt[i], t0 + t1, yv);                        // ((I + dt_i A)^T y_i)_q
            if (i > 0) {
                const int col = (i - 1) < d.ns ? 0 : (i - 1) - d.ns;
                const double xr = s.in[VSMPC_IN_XREF + col * 12 + qx];
                yv = fma(qd, s.x[i * NX + q] - (q < 12 ? xr : 0.0), prop);        // y_{i-1}
                if (tid < NX) s.y[(i - 1) * NX + q] = yv;
            } else {
                yv = -prop;                                                        // y_init
                if (tid < NX) s.y[N * NX + q] = yv;
            }
            take_max(m_dual, fabs(yv), bad);
        }
    } else {
        // (stage, row) pairs: residual of the dynamics row, node i + 1's share of scale and objective; then X_0 = x0
        for (int e = tid - 64; e < (N + 1) * NX; e += CB - 64) {
            const int i = e / NX, r = e - i * NX;
            if (i == N) {
                take_max(m_prim, fabs(s.x[r] - s.in[VSMPC_IN_X0 + r]), bad);
                continue;
            }
            const double* __restrict__ xi = s.x + i * NX;
            int a0, a1, b0, b1;
            a_row_ranges(r, a0, a1, b0, b1);
            double acc = sC[r];
            for (int c = a0; c < a1; ++c) acc = fma(sA[r * NX + c], xi[c], acc);
            for (int c = b0; c < b1; ++c) acc = fma(sA[r * NX + c], xi[c], acc);
            if ((r >= 3 && r < 6) || (r >= 9 && r < 12)) {                        // rows of Lambda_lin,B / Lambda_ang,B
                const double* __restrict__ u = s.x + offJ + joint_block(d, i) * NJ;
#pragma unroll
                for (int k = 0; k < NJ; ++k) acc = fma(sBj[r * NJ + k], u[k], acc);
            }
            if (r >= 12 && r < 20) {                                              // thrust or thrust-rate rows
                const double* __restrict__ v = s.x + offV + throttle_block(d, i) * NTH;
#pragma unroll
                for (int k = 0; k < NTH; ++k) acc = fma(sBt[r * NTH + k], v[k], acc);
            }
            const double xn = xi[NX + r];                                         // X_{i+1}[r]
            take_max(m_prim, fabs(fma(s.dt[i], acc, xi[r]) - xn), bad);
            const int col = i < d.ns ? 0 : i - d.ns;                              // node i + 1 reads column (i + 1) - 1 - nS
            const double xrl = s.in[VSMPC_IN_XREF + col * 12 + (r < 12 ? r : 11)];
            const double qd = q_diag(s.cfg + CFG_SQ, r), gq = qd * (r < 12 ? xrl : 0.0);   // g = -Q xr
            const double hx = qd * xn;
            take_max(m_scale, fmax(fabs(hx), fabs(gq)), bad);
            obj += xn * fma(0.5, hx, -gq);
        }
    }
    __syncthreads();

    // ---- phase B: joint entries (block j, joint k), then throttle entries (block t, jet k)
    const double w_reg = s.cfg[CFG_WREG], w_thr = s.cfg[CFG_WTHR], w_init = s.cfg[CFG_WINIT];
    for (int e = tid; e < d.nu + d.nv; e += CB) {
        if (e < d.nu) {
            const int j = e >> 3, k = e & 7;
            double sum = 0.0;
            const int iend = j == d.hc - 1 ? N : j + 1;   // jb(i) = j: stage j alone, and every stage from HC - 1 on for the last block
            for (int i = j; i < iend; ++i) {
                const double* __restrict__ yi = s.y + i * NX;
                double t = 0.0;
#pragma unroll
                for (int r = 3; r < 6; ++r) t = fma(sBj[r * NJ + k], yi[r], t);
#pragma unroll
                for (int r = 9; r < 12; ++r) t = fma(sBj[r * NJ + k], yi[r], t);
                sum = fma(s.dt[i], t, sum);
            }
            const double u = s.x[offJ + e];
            const double hx = s.cfg[CFG_WJ + k] * u, g = w_reg * s.in[VSMPC_IN_QERR + k];   // costsVSMPC.cpp:375-381,564-591
            take_max(m_stat, fabs((hx + g) + sum), bad);
            take_max(m_scale, fmax(fabs(hx), fabs(g)), bad);
            obj += u * fma(0.5, hx, g);
        } else {
            const int f = e - d.nu, t = f >> 2, k = f & 3;
            double sum = 0.0;
            for (int i = 0; i < N; ++i) {
                if (throttle_block(d, i) != t) continue;
                const double* __restrict__ yi = s.y + i * NX;
                double c = 0.0;
#pragma unroll
                for (int r = 12; r < 20; ++r) c = fma(sBt[r * NTH + k], yi[r], c);
                sum = fma(s.dt[i], c, sum);
            }
            const double* __restrict__ V = s.x + offV;
            const double v = V[f];
            const double vm = V[t > 0 ? f - NTH : f], vp = V[t < d.nvb - 1 ? f + NTH : f];   // neighbours (or v itself: difference 0)
            const double vprev = s.vprev[k];
            // RegualarizationCost first differences + ThrottleInitialValueCost (costsVSMPC.cpp:382-409,468-487)
            const double hx = fma(w_thr, (v - vm) + (v - vp), t == 0 ? w_init * v : 0.0);
            const double g = t == 0 ? -w_init * vprev : 0.0;
            const double mu = -((hx + g) + sum);
            s.y[(N + 1) * NX + f] = mu;
            take_max(m_dual, fabs(mu), bad);
            take_max(m_scale, fmax(fabs(hx), fabs(g)), bad);
            const double dv = v - vp;
            obj += 0.5 * w_thr * dv * dv + (t == 0 ? v * fma(0.5 * w_init, v, g) : 0.0);
            const bool pinned = t == 0 && s.in[VSMPC_IN_HOLD] != 0.0;              // constraintsVSMPC.cpp:351
            const double lo = pinned ? vprev : s.cfg[CFG_VMIN], hi = pinned ? vprev : s.cfg[CFG_VMAX];
            take_max(m_prim, fmax(0.0, fmax(lo - v, v - hi)), bad);
            if (!pinned) take_max(m_comp, fmax(fmax(mu, 0.0) * (hi - v), fmax(-mu, 0.0) * (v - lo)), bad);
        }
    }

    // ---- reduce
    m_stat = wave_max(m_stat);
    m_scale = wave_max(m_scale);
    m_prim = wave_max(m_prim);
    m_comp = wave_max(m_comp);
    m_dual = wave_max(m_dual);
    bad = wave_max(bad);
    obj = wave_sum(obj);
    if ((tid & 63) == 0) {
        double* r = s.red + (tid >> 6) * VSMPC_CERT_SIZE;
        r[VSMPC_CERT_STATIONARITY] = m_stat;
        r[VSMPC_CERT_STAT_SCALE] = m_scale;
        r[VSMPC_CERT_PRIMAL] = m_prim;
        r[VSMPC_CERT_COMPLEMENTARITY] = m_comp;
        r[VSMPC_CERT_OBJECTIVE] = obj;
        r[VSMPC_CERT_DUAL_MAX] = m_dual;
        r[6] = bad;
        r[7] = 0.0;
    }
    __syncthreads();
    if (tid < VSMPC_CERT_SIZE) {
        const double r0 = s.red[tid], r1 = s.red[VSMPC_CERT_SIZE + tid], r2 = s.red[2 * VSMPC_CERT_SIZE + tid],
                     r3 = s.red[3 * VSMPC_CERT_SIZE + tid];
        const bool nonfinite = fmax(fmax(s.red[6], s.red[VSMPC_CERT_SIZE + 6]),
                                    fmax(s.red[2 * VSMPC_CERT_SIZE + 6], s.red[3 * VSMPC_CERT_SIZE + 6])) != 0.0;
        double v = tid == VSMPC_CERT_OBJECTIVE ? ((r0 + r1) + r2) + r3 : fmax(fmax(r0, r1), fmax(r2, r3));
        if (tid >= 6) v = 0.0;                                                     // reserved
        if (nonfinite && (tid == VSMPC_CERT_STATIONARITY || tid == VSMPC_CERT_PRIMAL)) v = __builtin_nan("");
        cert[size_t(b) * VSMPC_CERT_SIZE + tid] = v;
    }
    if (yout != nullptr) {
        double2* y2 = reinterpret_cast<double2*>(yout + size_t(b) * ncon);
        for (int i = tid; i < ncon / 2; i += CB) y2[i] = reinterpret_cast<const double2*>(s.y)[i];
    }
}

hipError_t launch_certify(const RtDims& d, const DevCfg& cfg, const double* d_in, const double* d_x, const double* d_tun,
                          int batch, double* d_y, double* d_cert, hipStream_t stream) {
    const size_t lds = size_t(cert_lds_doubles(d)) * sizeof(double);   // 21 KB at the paper horizon, 36 KB at (40, 2, 40)
    if (lds > 64 * 1024) return hipErrorInvalidValue;                  // (not for a valid configuration)
    hipLaunchKernelGGL(certify_kernel, dim3(batch), dim3(CB), lds, stream, cfg, d, d_in, d_x, d_tun, d_y, d_cert);
    return hipGetLastError();
}

}  // namespace vsmpc
