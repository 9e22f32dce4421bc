// Host-visible launch interface of the kernel units (vsmpc_dispatch.hip, vsmpc_kernels.hip, ...; internal to the library;
// the public boundary is include/vsmpc.h).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>

#include "vsmpc_device.hpp"

struct vsmpc_jet;   // include/vsmpc_jet.h

namespace vsmpc {

// Entry points that must run on the handle's device switch to it for their own duration only: the caller's current device
// is put back on every return path (a library call that silently re-targets the caller's later HIP calls is a bug).
struct DeviceScope {
    int caller = -1, target = -1;
    hipError_t err = hipSuccess;
    explicit DeviceScope(int device) : target(device) {
        err = hipGetDevice(&caller);
        if (err == hipSuccess && caller != target) err = hipSetDevice(target);
    }
    ~DeviceScope() { if (caller >= 0 && caller != target) (void)hipSetDevice(caller); }
    DeviceScope(const DeviceScope&) = delete;
    DeviceScope& operator=(const DeviceScope&) = delete;
};

// The dynamic-LDS limit of a kernel is a per-device function attribute, and one process may drive several devices: allows
// `bytes` of dynamic LDS for `kernel` on the current device, once per device.  `attr_set` is the kernel's own flag array, a
// function-local static of its launcher.  Two host threads with their own handles may arrive together: the flag is atomic,
// setting the attribute twice is harmless, and it is published only after the call has succeeded.
constexpr int MAX_DEVICES = 64;
inline hipError_t allow_dynamic_lds(const void* kernel, std::atomic<bool> (&attr_set)[MAX_DEVICES], size_t bytes) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= MAX_DEVICES) return hipErrorInvalidDevice;
    if (!attr_set[dev].load(std::memory_order_acquire)) {
        e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, int(bytes));
        if (e != hipSuccess) return e;
        attr_set[dev].store(true, std::memory_order_release);
    }
    return hipSuccess;
}

// VSMPC_ERR_INVALID_ARG for every entry but vsmpc_pack_tunables and the fields vsmpc_rollout_set_noise refuses (defined beside
// the first in vsmpc_capi.hip; the other codes that carry a text are declared in vsmpc_host.hpp): it also drops the text such a
// refusal left on this thread, so that vsmpc_strerror describes the call that failed last
int invalid_arg();

enum Variant { VARIANT_NONE = 0 };  // 1.. = position in csrc/vsmpc_horizons.def

int select_variant(int n_iter, int n_iter_small, int control_horizon);
int num_variants();
void variant_horizon(int variant, int* n_iter, int* n_iter_small, int* control_horizon);
const char* variant_kernel_name(int variant);
int variant_condensed_dim(int variant);
size_t variant_lds_bytes(int variant);  // dynamic LDS of one workgroup (<= 80 KB: two workgroups share a CU)

int initial_kernel_form();               // VSMPC_FORM: what a new handle starts with
bool variant_has_structured(int variant);

// form: 0 the horizon's default (structured condensing where available), 1 structured, 2 SYRK
hipError_t launch_solve(int variant, int form, const DevCfg& cfg, const double* d_in, int batch, double* d_x, double* d_fm,
                        int* d_status, int* d_iters, double* dbgM, double* dbgL, unsigned long long* stamps,
                        hipStream_t stream);
// the launchers of one horizon: explicit instantiations in that horizon's units of vsmpc_kernels.hip (STAMPS: the diagnostic
// one), which launch_solve (vsmpc_dispatch.hip) dispatches onto
template <int N, int NS, int HC, bool STAMPS>
hipError_t launch_solve_dims(int form, const DevCfg& cfg, const double* d_in, int batch, double* d_x, double* d_fm,
                             int* d_status, int* d_iters, double* dbgM, double* dbgL, unsigned long long* stamps,
                             hipStream_t stream);
// the small-batch kind (solve_kernel_small; one unit of vsmpc_kernels.hip per horizon): structured form, no dumps; stamps !=
// nullptr picks its diagnostic instantiation
bool variant_has_small(int variant);
hipError_t launch_solve_small(int variant, const DevCfg& cfg, const double* d_in, int batch, double* d_x, double* d_fm,
                              int* d_status, int* d_iters, unsigned long long* stamps, hipStream_t stream);
template <int N, int NS, int HC>
hipError_t launch_solve_small_dims(const DevCfg& cfg, const double* d_in, int batch, double* d_x, double* d_fm, int* d_status,
                                   int* d_iters, unsigned long long* stamps, hipStream_t stream);
size_t variant_small_lds_bytes(int variant);   // its dynamic LDS (<= 160 KB: one workgroup per CU), 0 without the kind
int initial_small_batch_mode();                // VSMPC_SMALL_BATCH: what a new handle starts with
// the per-instance-tunables kind (solve_kernel_tuned; one unit of vsmpc_kernels.hip per horizon and condensing form, FORM
// 1 = structured): d_tun [batch][VSMPC_TUNE_SIZE], rows of vsmpc_pack_tunables, 16-byte aligned
hipError_t launch_solve_tuned(int variant, int form, const DevCfg& cfg, const double* d_in, const double* d_tun, int batch,
                              double* d_x, double* d_fm, int* d_status, int* d_iters, hipStream_t stream);
template <int N, int NS, int HC, int FORM>
hipError_t launch_solve_tuned_dims(const DevCfg& cfg, const double* d_in, const double* d_tun, int batch, double* d_x,
                                   double* d_fm, int* d_status, int* d_iters, hipStream_t stream);

// Runtime-sized solve kernel (vsmpc_runtime.hip): every horizon config_valid() accepts, sizes as kernel arguments.
struct RtDims {
    int n, ns, hc;        // nIter, nIterSmall, controlHorizon
    int nvb, nu, nv;      // throttle blocks, joint unknowns 8 HC, throttle unknowns 4 NVB
    int nz, np;           // condensed unknowns, + the affine / gradient column
    int nin, nxs, nvar;   // record length, states 26 (N + 1), primal length
    int ntri;             // NP (NP + 1) / 2: packed lower triangle of the augmented condensed matrix
    int ws_doubles;       // per-instance global workspace (doubles)
    int lds_doubles;      // dynamic LDS of one workgroup (doubles)
};
constexpr size_t RT_MAX_LDS = 160 * 1024;
// sensitivity: the sizes of sens_kernel_rt (NP = NZ + 1 + 26: the parameter columns of d/dX0); adjoint: those of
// adjoint_kernel_rt[_tuned] (the solve kernel's, with room in LDS for a_X and the costates at horizons with few unknowns);
// adjoint_record (with adjoint): those of adjoint_record_kernel_rt[_tuned] (room for dL/d(A | Bj | Bt | c) behind them)
RtDims runtime_dims(int n_iter, int n_iter_small, int control_horizon, bool sensitivity = false, bool adjoint = false,
                    bool adjoint_record = false);
size_t runtime_lds_bytes(const RtDims& d);
// the same with the staged row of the per-instance-tunables kinds behind it (solve_kernel_rt_tuned, adjoint_kernel_rt_tuned)
size_t runtime_tuned_lds_bytes(const RtDims& d);
const char* runtime_kernel_name();
// The kinds of the runtime-sized kernel (the instantiations of rt_solve) and their C entries:
enum RtMode {
    RT_SOLVE,        // solve_kernel_rt[_tuned]: vsmpc_solve_batch[_tuned] on a runtime handle; d from runtime_dims(..)
    RT_SENS,         // sens_kernel_rt: vsmpc_sensitivity_batch; d from runtime_dims(.., true); no tuned kind
    RT_ADJOINT,      // adjoint_kernel_rt[_tuned]: vsmpc_adjoint_batch; d from runtime_dims(.., false, true)
    RT_ADJOINT_REC   // adjoint_record_kernel_rt[_tuned]: vsmpc_adjoint_record_batch; d from runtime_dims(.., false, true, true)
};
// Every pointer of one launch, by name (device memory, one row per instance of the launch).  A caller sets what its kind
// reads and what it wants written; of the outputs only `status` is required, and a kind ignores the fields of the others.
struct RtLaunch {
    const double* in = nullptr;    // records [n_in]
    const double* tun = nullptr;   // rows of per-instance tunables [VSMPC_TUNE_SIZE], 16-byte aligned: the kind's tuned kernel
                                   // runs; nullptr: the handle's configuration for every instance
    double* ws = nullptr;          // workspace of the launch's first instance (instance b uses ws + b * d.ws_doubles)
    double *x = nullptr, *fm = nullptr;           // primal [nVar], first move [24]
    int *status = nullptr, *iters = nullptr;
    // every kind but RT_SOLVE: final throttle states [NV] and the VSMPC_SENS_* / VSMPC_ADJ_* flags
    int *active = nullptr, *flags = nullptr;
    // RT_SENS: dx_dx0 [nVar][26], dfm_dx0 [24][26]
    double *dx = nullptr, *dfm = nullptr;
    // RT_ADJOINT, RT_ADJOINT_REC: the cotangents [nVar] (required) and [24] in, dL/dX0 [26] and dL/dcfg [VSMPC_GRAD_SIZE] out
    const double *xbar = nullptr, *fmbar = nullptr;
    double *gx0 = nullptr, *gcfg = nullptr;
    // RT_ADJOINT_REC: dL/d record [n_in], dL/d(A | Bj | Bt | c) [VSMPC_GRAD_MODEL_SIZE]
    double *gin = nullptr, *gmodel = nullptr;
};
// launches the kernel of `kind` (its tuned one when a.tun is given) over `batch` instances; hipErrorInvalidValue when `d`
// is not the kind's runtime_dims, or the kind has no tuned kernel
hipError_t launch_runtime(RtMode kind, const RtDims& d, const DevCfg& cfg, int batch, const RtLaunch& a, hipStream_t stream);
// linearize_kernel_rt (vsmpc_linearize_batch, on every handle): p0_linearize alone
hipError_t launch_linearize_runtime(const RtDims& d, const DevCfg& cfg, const double* d_in, int batch, double* A, double* Bj,
                                    double* Bt, double* c, hipStream_t stream);

// certify_kernel (vsmpc_certify.hip): duals y [batch][nCon] (or nullptr) and certificate [batch][VSMPC_CERT_SIZE] of the
// primals d_x [batch][nvar] for the records d_in; d from runtime_dims(.., false) on every handle; d_tun rows of
// per-instance tunables or nullptr (the handle's configuration).  d_in, d_x, d_tun, d_y 16-byte aligned.
hipError_t launch_certify(const RtDims& d, const DevCfg& cfg, const double* d_in, const double* d_x, const double* d_tun,
                          int batch, double* d_y, double* d_cert, hipStream_t stream);

struct KinOpts {
    int sel[VSMPC_N_JOINTS];   // robot joint index of every controlled joint (Lambda_ang columns)
    int constant_lambda;       // jointsLambdaOption "constant"
    double* records = nullptr; // when set: LLIN | LANG | INERTIA are written into these device-resident input records
    int n_in = 0;
    int skip_inertia = 0;      // patching only: leave INERTIA alone (the rollout's tree plant writes R I_B R^T itself)
};
hipError_t launch_kinematics(const double* d_kin, int batch, double* d_out, const KinOpts& opts, hipStream_t stream);

// kinematics provider on a simplified tree (vsmpc_provider.hip)
hipError_t launch_provider(const vsmpc_tree& tree, const double* d_state, int batch, double* d_kin, double* d_robot,
                           double* d_records, int n_in, hipStream_t stream);
// kinematics terms written straight into device-resident input records (LLIN, LANG, INERTIA)
hipError_t launch_kinematics_patch(const double* d_kin, int batch, double* d_records, int n_in, const KinOpts& opts,
                                   hipStream_t stream);

// tree_jacobian_kernel (vsmpc_tree_jacobian.hip): terms [batch][VSMPC_TT_SIZE] and / or their Jacobian [batch][VSMPC_TT_SIZE]
// [VSMPC_TT_NDIR] (either may be nullptr) of the tree at the joints d_q + b q_stride [8] and thrusts d_thrust + b t_stride [4]
// of instance b (rows of their own, or a row of plant states), base at the origin with identity attitude; opts.sel picks
// Lambda_ang's columns (opts.constant_lambda is the caller's to refuse)
hipError_t launch_tree_jacobian(const vsmpc_tree& tree, const KinOpts& opts, const double* d_q, int q_stride, const double* d_thrust,
                                int t_stride, int batch, double* d_terms, double* d_jac, hipStream_t stream);

// closed-loop rollout (vsmpc_rollout.hip)
struct RolloutDev {
    int n_in, n_ref, ratio, n_traj, n_alpha;
    int n_ts;         // doubles of per-instance tick state (reference window, RPY unwrap: see vsmpc_rollout.hip)
    int alpha_up;     // up-sampling factor of the alpha-gravity track (TrajectoryManager.cpp:23-39)
    double period_mpc, alpha_dt;
    const double* traj_rpy;      // device, [n_traj][3] or nullptr: RPY / RPYDot tracks of the position trajectory
    const double* traj_rpyd;     //   (vsmpc_rollout_set_attitude_tracks; the shipped ones are all zero)
    // jet plant option (vsmpc_rollout_set_jet_plant): LSTM thrust dynamics + EKF estimates instead of the polynomial model
    // kinematic-tree plant (vsmpc_rollout_set_tree): A_mom,body(q), I_B(q) and the Lambda terms come from the kinematics
    // provider evaluated on the plant's own joint state in the body frame (base at the origin, identity attitude), through
    // these per-instance arrays: Robot-level outputs [batch][VSMPC_RO_SIZE], kinematics terms [batch][VSMPC_KIN_OUT] (I_G
    // = I_B there), and the kinematics record [batch][VSMPC_KIN_SIZE] whose thrusts the advance kernel refreshes
    int tree;
    const double* tree_ro;
    const double* tree_kout;
    double* tree_kin;
    int jet_nn, jet_hidden;
    const float* jet_w;          // device: wih col 0 [4H] | wih col 1 [4H] | b_ih [4H] | b_hh [4H] | fc_w [H] | fc_b
    double jet_norm[4];          // thrust mean / std, throttle mean / std of the checkpoint
    double ekf_q[4], ekf_r[4];
};
// view of a jet handle for the rollout (vsmpc_jet.hip)
void jet_plant_view(const ::vsmpc_jet* j, const float** w, int* hidden, double norm[4], int* device);
struct RolloutCtl {   // device-resident per-run control block of the rollout
    double* log;      // [ticks of this run][batch][VSMPC_ROLLOUT_LOG] or nullptr
    int tick_base;    // tick counter at the start of the run
    int log_rows;     // rows the log buffer holds
};
// provider state of every instance at the body-frame pose: joints = plant joints (+ the first move's increments when `fm`
// is given and the status is Solved: what the advance kernel is about to apply), thrusts as the controller sees them
hipError_t launch_tree_state(const RolloutDev& rd, int batch, const double* state, const double* fm, const int* status,
                             double* rs, hipStream_t stream);
// What one tick's launches work on, the same at every tick (all device pointers, [batch][..] rows).  record_kernel builds the
// record of the tick the counters stand at; advance_kernel consumes the solve's outputs, flies the plant over one MPC period
// and leaves the record of the following tick.
struct RolloutTick {
    int batch, substeps;
    double* state;               // [VSMPC_PLANT_STATE]
    const double* params;        // [VSMPC_PLANT_PARAMS]
    int* tick;                   // ticks since the reset
    const double* traj_pos;
    const double* traj_vel;
    const double* traj_alpha;
    double* tstate;              // per-instance tick state [rd.n_ts]
    double* rec;                 // the record [rd.n_in]
    const double* fm;            // advance only: first move [VSMPC_FM_SIZE], status and iterations of the solve, control block
    const int* status;
    const int* iters;
    const RolloutCtl* ctl;
};
// Noise of the closed loop (vsmpc_rollout_set_noise; the generator and the draws: vsmpc_noise_device.hpp).  It rides behind the
// other arguments of the two kernels' NOISE instantiations and is no part of RolloutDev: the code of a rollout without noise
// stays as it is.
struct RolloutNoise {
    unsigned long long seed;
    unsigned long long first_index;   // global index of loop 0 of this rollout
    double sigma_pos, sigma_lin_vel, sigma_rpy, sigma_ang_vel;   // measurement: m, m/s, rad, rad/s
    double sigma_force, sigma_torque;                            // gust: N, Nm
};
// nz == nullptr: record_kernel<false> / advance_kernel<false>, what the kernels were before they had a second instantiation;
// given: their NOISE instantiations, with the measured state in the record and the gust beside the push
hipError_t launch_record(const RolloutDev& rd, const RolloutTick& k, hipStream_t stream, const RolloutNoise* nz = nullptr);
hipError_t launch_advance(const RolloutDev& rd, const RolloutTick& k, hipStream_t stream, const RolloutNoise* nz = nullptr);
// noise_draws_kernel: what ticks tick0 .. tick0 + ticks - 1 of `batch` loops draw, z [ticks][batch][18] and (or nullptr) the
// generator's words [ticks][batch][9][4] (device), through the device function the two noisy kernels call
hipError_t launch_noise_draws(const RolloutNoise& nz, int batch, int tick0, int ticks, double* z, unsigned* words, hipStream_t stream);

// One launch of the rollout's backward sweep (vsmpc_rollout_adjoint.hip): the record half of tick `tick_rec`, then the plant
// half of tick `tick_plant` (ticks as the rollout counts them since its reset; -1: that half is absent).  All device pointers,
// [batch][..] rows.  sbar, wbar, gcfg and flags are read and written in place.
struct RolloutAdj {
    int batch, substeps;
    int tick_rec, first;         // `first`: tick_rec built the reference window (the first tick after a reset)
    int tick_plant;
    const double* params;        // [VSMPC_PLANT_PARAMS]
    const double* traj_vel;
    const double* traj_alpha;
    const double* s_rec;         // taped plant state in front of tick_rec [VSMPC_PLANT_STATE]
    const double* gin;           // the record adjoint's outputs of tick_rec: grad_in [n_in], grad_cfg [VSMPC_GRAD_SIZE], flags
    const double* gcfg_t;
    const int* flags_t;
    const double* s_plant;       // tape of tick_plant: plant state in front of it, first move [VSMPC_FM_SIZE], status
    const double* fm;
    const int* status;
    const double* log_bar;       // cotangent of tick_plant's log row [VSMPC_ROLLOUT_LOG], or nullptr
    double* sbar;                // cotangent of the plant state [VSMPC_PLANT_STATE]
    double* wbar;                // cotangent of the reference window [12 n_ref]
    double* fmbar;               // out: cotangent of tick_plant's first move [VSMPC_FM_SIZE]
    double* gcfg;                // accumulated over the ticks [VSMPC_GRAD_SIZE]
    int* flags;
    // vsmpc_rollout_backward_full: both or neither.  Given, the launch runs the kernel's second instantiation, which also
    // accumulates over the ticks dL/d(plant parameters) [VSMPC_PLANT_PARAMS] and dL/d(traj_pos | traj_vel | traj_alpha)
    // [6 n_traj + n_alpha], one row per instance
    double* gpar;
    double* gtraj;
    // kinematic-tree plant (vsmpc_rollout_set_tree_ex with VSMPC_TREE_ADJOINT): both or neither.  Given, the launch runs the
    // kernel's tree instantiations on tau = terms(q, T) [VSMPC_TT_SIZE] of the state in front of tick_rec (= behind
    // tick_plant) and its Jacobian [VSMPC_TT_SIZE][VSMPC_TT_NDIR] (launch_tree_jacobian on that state)
    const double* tree_terms;
    const double* tree_jac;
    // attitude tracks (vsmpc_rollout_set_attitude_tracks_ex with VSMPC_ATTITUDE_ADJOINT): the launch runs the ATT kernels, which
    // also pull back rows 9..11 of the window columns (rd.traj_rpyd, nullptr: zeros); gatt, with gpar and gtraj only, or nullptr:
    // dL/d(traj_rpy | traj_rpy_dot) [6 n_traj], one row per instance, accumulated over the ticks
    int attitude;
    double* gatt;
};
hipError_t launch_advance_adjoint(const RolloutDev& rd, const RolloutAdj& a, hipStream_t stream);
// the tree instantiations (vsmpc_rollout_tree_adjoint.hip): what launch_advance_adjoint launches when a.tree_terms is given
hipError_t launch_advance_tree_adjoint(const RolloutDev& rd, const RolloutAdj& a, hipStream_t stream);
// the ATT instantiations (vsmpc_rollout_attitude_adjoint.hip, vsmpc_rollout_attitude_tree_adjoint.hip): what
// launch_advance_adjoint launches when a.attitude is set, the second when a.tree_terms is given too
hipError_t launch_advance_attitude_adjoint(const RolloutDev& rd, const RolloutAdj& a, hipStream_t stream);
hipError_t launch_advance_attitude_tree_adjoint(const RolloutDev& rd, const RolloutAdj& a, hipStream_t stream);

}  // namespace vsmpc
