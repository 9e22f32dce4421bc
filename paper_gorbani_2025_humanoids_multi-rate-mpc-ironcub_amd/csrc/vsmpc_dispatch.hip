// What the tuned solve kernels share across horizons, compiled once: the kinematics kernel, the table of instantiated
// horizons (csrc/vsmpc_horizons.def, one X(...) line per horizon, written by build.py; variant ids are 1-based positions in
// it) and the dispatchers onto the per-horizon launchers of vsmpc_kernels.hip.
#include <cstdlib>

#include "vsmpc_launch.hpp"
#include "vsmpc_smem.hpp"

namespace vsmpc {

// ------------------------------------------------------------------------------------------------
// kinematics-derived inputs (vsmpc_kinematics_batch): Lambda_lin,B, Lambda_ang,B, I_G per instance.
// HBM-bound (5.6 KB in, 0.46 KB out per instance): one wavefront per instance stages the record in LDS with
// 16 B/lane loads, 57 lanes compute one output element each.
//   computeLambdaLin          systemDynamicsVSMPC.cpp:321-350
//   computeLambdaAng          systemDynamicsVSMPC.cpp:159-206 ("unfiltered"), getRelativeJacobianCoM :208-226
//   locked inertia I_G        systemDynamicsVSMPC.cpp:128-130 (iDynTree adjoint X = [R, S(r)R; 0, R])
// ------------------------------------------------------------------------------------------------
// Options (vsmpc_set_kinematics_options): `sel` = robot joint index of each controlled joint for Lambda_ang, which the
// reference selects by NAME (systemDynamicsVSMPC.cpp:57-66,202-205; Lambda_lin keeps the reference's hard-coded column
// offset 3, :348); `constant_lambda` = jointsLambdaOption "constant" (:186-200,329-337): axes, arms and relative Jacobians
// are the configure-time ones, the angular term uses the relative Jacobian's own top rows (delivered in the JFRAME slot)
// instead of R^T (J_frame - J_CoM) and the thrusts of getRobot() (delivered in JCOM[0..3]).
__global__ __launch_bounds__(64) void kinematics_kernel(const double* __restrict__ kin, int batch,
                                                        double* __restrict__ out, KinOpts opts) {
    __shared__ __attribute__((aligned(16))) double s[VSMPC_KIN_SIZE + 1];
    __shared__ double sRa[12], sRr[12];  // R^T a_i, R^T r_i
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b >= batch) return;
    const double* rec = kin + size_t(b) * VSMPC_KIN_SIZE;
    // the record stride (697 doubles) is odd, so 16 B alignment alternates: peel one element where needed
    const int head = (reinterpret_cast<size_t>(rec) & 15) ? 1 : 0;
    if (lane == 0 && head) s[0] = rec[0];
    const double2* r2 = reinterpret_cast<const double2*>(rec + head);
    const int n2 = (VSMPC_KIN_SIZE - head) / 2;
    for (int i = lane; i < n2; i += 64) {
        const double2 v = r2[i];
        s[head + 2 * i] = v.x;
        s[head + 2 * i + 1] = v.y;
    }
    if (lane == 0 && ((VSMPC_KIN_SIZE - head) & 1)) s[VSMPC_KIN_SIZE - 1] = rec[VSMPC_KIN_SIZE - 1];
    __syncthreads();
    const double* R = s + VSMPC_KIN_WRB;
    if (lane < 24) {  // R^T a_i and R^T r_i
        const int which = lane / 12, e = lane % 12, i = e / 3, c = e % 3;
        const double* v = s + (which ? VSMPC_KIN_ARMS : VSMPC_KIN_AXES) + 3 * i;
        const double val = R[c] * v[0] + R[3 + c] * v[1] + R[6 + c] * v[2];
        (which ? sRr : sRa)[e] = val;
    }
    __syncthreads();
    constexpr int NJq = VSMPC_KIN_NJ, OFF = 3;  // Lambda_lin: robot joints 3..10 (systemDynamicsVSMPC.cpp:348)
    double res = 0.0;
    if (lane < 48) {
        const bool ang = lane >= 24;
        const int e = lane % 24, r = e >> 3, col = ang ? opts.sel[e & 7] : OFF + (e & 7);
        for (int i = 0; i < 4; ++i) {
            const double T = (ang && opts.constant_lambda) ? s[VSMPC_KIN_JCOM + i] : s[VSMPC_KIN_THRUST + i];
            const double* a = sRa + 3 * i;
            const double* Jrel = s + VSMPC_KIN_JREL + i * 3 * NJq;
            // w = S(a) * Jrel[:, col]  (skew: FlightControlUtils.cpp:77-85)
            const double j0 = Jrel[col], j1 = Jrel[NJq + col], j2 = Jrel[2 * NJq + col];
            const double w0 = -a[2] * j1 + a[1] * j2, w1 = a[2] * j0 - a[0] * j2, w2 = -a[1] * j0 + a[0] * j1;
            if (!ang) {
                res -= T * (r == 0 ? w0 : (r == 1 ? w1 : w2));
            } else {
                const double* Jf = s + VSMPC_KIN_JFRAME + i * 3 * NJq;
                const double* Jc = s + VSMPC_KIN_JCOM;
                const double d0 = Jf[col] - Jc[col], d1 = Jf[NJq + col] - Jc[NJq + col], d2 = Jf[2 * NJq + col] - Jc[2 * NJq + col];
                double g0 = R[0] * d0 + R[3] * d1 + R[6] * d2;  // R^T (J_frame - J_CoM)
                double g1 = R[1] * d0 + R[4] * d1 + R[7] * d2;
                double g2 = R[2] * d0 + R[5] * d1 + R[8] * d2;
                if (opts.constant_lambda) { g0 = Jf[col]; g1 = Jf[NJq + col]; g2 = Jf[2 * NJq + col]; }
                const double u0 = -a[2] * g1 + a[1] * g2, u1 = a[2] * g0 - a[0] * g2, u2 = -a[1] * g0 + a[0] * g1;
                const double* q = sRr + 3 * i;  // S(R^T r_i) * w
                const double z0 = -q[2] * w1 + q[1] * w2, z1 = q[2] * w0 - q[0] * w2, z2 = -q[1] * w0 + q[0] * w1;
                res -= T * ((r == 0 ? u0 : (r == 1 ? u1 : u2)) + (r == 0 ? z0 : (r == 1 ? z1 : z2)));
            }
        }
    } else if (lane < 57) {
        // I_G = [S(r)R; R]^T M_b [S(r)R; R], element (i, j)
        const int e = lane - 48, i = e / 3, j = e % 3;
        const double* rr = s + VSMPC_KIN_R;
        const double* M = s + VSMPC_KIN_MB;
        double Xi[6], Xj[6];  // columns i and j of the 6x3 matrix [S(r)R; R]
        for (int k = 0; k < 3; ++k) { Xi[3 + k] = R[3 * k + i]; Xj[3 + k] = R[3 * k + j]; }
        Xi[0] = -rr[2] * Xi[4] + rr[1] * Xi[5]; Xi[1] = rr[2] * Xi[3] - rr[0] * Xi[5]; Xi[2] = -rr[1] * Xi[3] + rr[0] * Xi[4];
        Xj[0] = -rr[2] * Xj[4] + rr[1] * Xj[5]; Xj[1] = rr[2] * Xj[3] - rr[0] * Xj[5]; Xj[2] = -rr[1] * Xj[3] + rr[0] * Xj[4];
        for (int a = 0; a < 6; ++a) {
            double t = 0.0;
            for (int c = 0; c < 6; ++c) t += M[6 * a + c] * Xj[c];
            res += Xi[a] * t;
        }
    }
    if (out != nullptr && lane < VSMPC_KIN_OUT) out[size_t(b) * VSMPC_KIN_OUT + lane] = res;
    if (opts.records != nullptr && lane < (opts.skip_inertia ? 48 : VSMPC_KIN_OUT)) {   // device-resident input records: LLIN | LANG | INERTIA
        double* rec = opts.records + size_t(b) * opts.n_in;
        rec[(lane < 24 ? VSMPC_IN_LLIN + lane : (lane < 48 ? VSMPC_IN_LANG + lane - 24 : VSMPC_IN_INERTIA + lane - 48))] = res;
    }
}

hipError_t launch_kinematics_patch(const double* d_kin, int batch, double* d_records, int n_in, const KinOpts& opts,
                                   hipStream_t stream) {
    KinOpts o = opts;
    o.records = d_records;
    o.n_in = n_in;
    hipLaunchKernelGGL(kinematics_kernel, dim3(batch), dim3(64), 0, stream, d_kin, batch, static_cast<double*>(nullptr), o);
    return hipGetLastError();
}

hipError_t launch_kinematics(const double* d_kin, int batch, double* d_out, const KinOpts& opts, hipStream_t stream) {
    hipLaunchKernelGGL(kinematics_kernel, dim3(batch), dim3(64), 0, stream, d_kin, batch, d_out, opts);
    return hipGetLastError();
}

// condensing form of a handle: 0 = the default of the horizon (structured where Dims::STRUCT_P1), 1 = structured,
// 2 = SYRK (vsmpc_set_kernel_form).  VSMPC_FORM=structured|syrk is what a new handle starts with, for measurements of
// unmodified programs.
int initial_kernel_form() {
    const char* v = getenv("VSMPC_FORM");
    return (v != nullptr && v[0] == 's' && v[1] == 't') ? 1 : (v != nullptr && v[0] == 's' && v[1] == 'y') ? 2 : 0;
}

// which kernel serves small batches (vsmpc_set_small_batch_kernel): 0 = the small-batch kind when the batch does not exceed
// the device's CUs, 1 = never, 2 = always where the horizon has it.  VSMPC_SMALL_BATCH=auto|never|always is what a new handle
// starts with.
int initial_small_batch_mode() {
    const char* v = getenv("VSMPC_SMALL_BATCH");
    return (v != nullptr && v[0] == 'n') ? 1 : (v != nullptr && v[0] == 'a' && v[1] == 'l') ? 2 : 0;
}

template <class D>
constexpr size_t small_lds_bytes() {
    if constexpr (has_small_kind<D>()) return Smem<D, true>::bytes_struct;
    else return 0;
}

struct HorizonEntry {
    int n_iter, n_iter_small, control_horizon, n_p;
    size_t lds_bytes;
    const char* name;
    bool structured;
    size_t small_lds_bytes;   // 0: the horizon has no small-batch kind
};
#define VSMPC_STR2(x) #x
#define VSMPC_STR(x) VSMPC_STR2(x)
static const HorizonEntry kHorizons[] = {
#define X(N, NS, HC) {N, NS, HC, Dims<N, NS, HC>::NP, Dims<N, NS, HC>::STRUCT_P1 ? Smem<Dims<N, NS, HC>>::bytes_struct : Smem<Dims<N, NS, HC>>::bytes, "solve_kernel<Dims<" VSMPC_STR(N) "," VSMPC_STR(NS) "," VSMPC_STR(HC) ">>", Dims<N, NS, HC>::STRUCT_P1, small_lds_bytes<Dims<N, NS, HC>>()},
#include "vsmpc_horizons.def"
#undef X
};
constexpr int kNumHorizons = int(sizeof(kHorizons) / sizeof(kHorizons[0]));

int select_variant(int n_iter, int n_iter_small, int control_horizon) {
    for (int i = 0; i < kNumHorizons; ++i)
        if (kHorizons[i].n_iter == n_iter && kHorizons[i].n_iter_small == n_iter_small &&
            kHorizons[i].control_horizon == control_horizon)
            return i + 1;
    return VARIANT_NONE;
}

int num_variants() { return kNumHorizons; }

void variant_horizon(int variant, int* n_iter, int* n_iter_small, int* control_horizon) {
    const HorizonEntry& h = kHorizons[variant - 1];
    *n_iter = h.n_iter;
    *n_iter_small = h.n_iter_small;
    *control_horizon = h.control_horizon;
}

const char* variant_kernel_name(int variant) {
    return (variant >= 1 && variant <= kNumHorizons) ? kHorizons[variant - 1].name : "none";
}

int variant_condensed_dim(int variant) {
    return (variant >= 1 && variant <= kNumHorizons) ? kHorizons[variant - 1].n_p : 0;
}

bool variant_has_structured(int variant) {
    return variant >= 1 && variant <= kNumHorizons && kHorizons[variant - 1].structured;
}

bool variant_has_small(int variant) { return variant_small_lds_bytes(variant) != 0; }

size_t variant_small_lds_bytes(int variant) {
    return (variant >= 1 && variant <= kNumHorizons) ? kHorizons[variant - 1].small_lds_bytes : 0;
}

hipError_t launch_solve_small(int variant, const DevCfg& cfg, const double* d_in, int batch, double* d_x, double* d_fm,
                              int* d_status, int* d_iters, unsigned long long* stamps, hipStream_t stream) {
    if (!variant_has_small(variant)) return hipErrorInvalidValue;
    int id = 0;
#define X(N, NS, HC) \
    if (variant == ++id) return launch_solve_small_dims<N, NS, HC>(cfg, d_in, batch, d_x, d_fm, d_status, d_iters, stamps, stream);
#include "vsmpc_horizons.def"
#undef X
    return hipErrorInvalidValue;
}

size_t variant_lds_bytes(int variant) {
    return (variant >= 1 && variant <= kNumHorizons) ? kHorizons[variant - 1].lds_bytes : 0;
}

hipError_t launch_solve(int variant, int form, const DevCfg& cfg, const double* d_in, int batch, double* d_x, double* d_fm,
                        int* d_status, int* d_iters, double* dbgM, double* dbgL, unsigned long long* stamps,
                        hipStream_t stream) {
    int id = 0;
#define X(N, NS, HC)                                                                                                  \
    if (variant == ++id) {                                                                                            \
        if (stamps != nullptr || dbgM != nullptr || dbgL != nullptr)                                                  \
            return launch_solve_dims<N, NS, HC, true>(form, cfg, d_in, batch, d_x, d_fm, d_status, d_iters, dbgM, dbgL,   \
                                                      stamps, stream);                                                \
        return launch_solve_dims<N, NS, HC, false>(form, cfg, d_in, batch, d_x, d_fm, d_status, d_iters, dbgM, dbgL,      \
                                                   nullptr, stream);                                                  \
    }
#include "vsmpc_horizons.def"
#undef X
    return hipErrorInvalidValue;
}

template <int N, int NS, int HC>
static hipError_t launch_solve_tuned_pick(int form, const DevCfg& cfg, const double* d_in, const double* d_tun, int batch,
                                          double* d_x, double* d_fm, int* d_status, int* d_iters, hipStream_t stream) {
    if constexpr (Dims<N, NS, HC>::STRUCT_P1) {
        if (form != 2)
            return launch_solve_tuned_dims<N, NS, HC, 1>(cfg, d_in, d_tun, batch, d_x, d_fm, d_status, d_iters, stream);
    }
    return launch_solve_tuned_dims<N, NS, HC, 0>(cfg, d_in, d_tun, batch, d_x, d_fm, d_status, d_iters, stream);
}

hipError_t launch_solve_tuned(int variant, int form, const DevCfg& cfg, const double* d_in, const double* d_tun, int batch,
                              double* d_x, double* d_fm, int* d_status, int* d_iters, hipStream_t stream) {
    int id = 0;
#define X(N, NS, HC) \
    if (variant == ++id) return launch_solve_tuned_pick<N, NS, HC>(form, cfg, d_in, d_tun, batch, d_x, d_fm, d_status, d_iters, stream);
#include "vsmpc_horizons.def"
#undef X
    return hipErrorInvalidValue;
}

}  // namespace vsmpc
