// What the host units of the C-ABI share (vsmpc_capi*.hip, the host part of vsmpc_jet.hip): the standard headers, owners of
// HIP resources, the handle structs, row copies, and the way a HIP failure becomes a return code.  No kernels.
#pragma once
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <utility>
#include <vector>

#include "vsmpc_launch.hpp"
#include "../../include/vsmpc_jet.h"

namespace vsmpc {

// Move-only owner of a HIP resource that one call destroys.  The destructor runs on the CURRENT device: the destroy entries
// set up a DeviceScope of the handle's device before they delete the handle.
template <typename H, hipError_t (*Destroy)(H)>
struct Owned {
    H h = nullptr;
    Owned() = default;
    Owned(Owned&& o) noexcept : h(o.h) { o.h = nullptr; }
    Owned& operator=(Owned&& o) noexcept { std::swap(h, o.h); return *this; }
    ~Owned() { reset(); }
    void reset() { if (h) (void)Destroy(h); h = nullptr; }
    H* put() { reset(); return &h; }   // for the create call
    operator H() const { return h; }
};
using Stream = Owned<hipStream_t, hipStreamDestroy>;
using Event = Owned<hipEvent_t, hipEventDestroy>;
template <typename T> hipError_t dev_free(T* p) { return hipFree(p); }
template <typename T>
struct DevBuf : Owned<T*, dev_free<T>> {   // `n` elements of device memory
    hipError_t alloc(size_t n) {   // (whatever it held is freed first; empty after a failure)
        const hipError_t e = hipMalloc(reinterpret_cast<void**>(this->put()), n * sizeof(T));
        if (e != hipSuccess) this->h = nullptr;
        return e;
    }
    T* get() const { return this->h; }
};
// Device staging of one argument of a chunked host-pointer entry: `width` elements per instance, for one chunk of instances.
// vsmpc_create_ex states the width once; the allocation and every copy take it from here.
template <typename T>
struct StageBuf : DevBuf<T> {
    size_t width = 0;
    hipError_t alloc(size_t instances, size_t w) { width = w; return DevBuf<T>::alloc(instances * w); }
};

// Rows first .. first + n - 1 ([..][width]) between a caller's buffer and device staging, on a stream.  A null host pointer
// is an input or output the caller does not want: nothing is enqueued.  (T comes from the host pointer: a DevBuf converts.)
template <typename T> struct Same { using type = T; };
template <typename T>
hipError_t upload_rows(typename Same<T>::type* dev, const T* host, size_t first, size_t n, size_t width, hipStream_t s) {
    if (host == nullptr) return hipSuccess;
    return hipMemcpyAsync(dev + first * width, host + first * width, n * width * sizeof(T), hipMemcpyHostToDevice, s);
}
template <typename T>
hipError_t download_rows(T* host, const typename Same<T>::type* dev, size_t first, size_t n, size_t width, hipStream_t s) {
    if (host == nullptr) return hipSuccess;
    return hipMemcpyAsync(host + first * width, dev + first * width, n * width * sizeof(T), hipMemcpyDeviceToHost, s);
}

// VSMPC_ERR_UNSUPPORTED_CONFIG with the plain text, or with `why` for the entries whose refusal names a create flag
// (vsmpc_strerror describes the call that failed last on this thread).  Every return of that code in this library goes
// through here: a site that returned the bare constant would leave the text of an earlier refusal standing.
int unsupported(const char* why = nullptr);
// VSMPC_ERR_INVALID_ARG with a text that names the entry and the argument's field it refuses (vsmpc_capi.hip)
int invalid_field(const char* entry, const char* field);
int hip_fail(hipError_t e, const char* what);   // VSMPC_ERR_HIP, through vsmpc_strerror's channel
inline int hip_fail_into(char (&msg)[256], hipError_t e, const char* what) {
    snprintf(msg, sizeof(msg), "HIP error in %s: %s", what, hipGetErrorString(e));
    return VSMPC_ERR_HIP;
}

}  // namespace vsmpc

// HIP_TRY returns through vsmpc::hip_fail unless the unit named its own channel first (vsmpc_jet.hip: vsmpc_jet_last_error)
#ifndef VSMPC_HIP_FAIL
#define VSMPC_HIP_FAIL vsmpc::hip_fail
#endif
#define HIP_TRY(expr)                                           \
    do {                                                        \
        hipError_t _e = (expr);                                 \
        if (_e != hipSuccess) return VSMPC_HIP_FAIL(_e, #expr); \
    } while (0)
#define ON_DEVICE(dev) vsmpc::DeviceScope _scope(dev); HIP_TRY(_scope.err)

struct vsmpc_handle {
    vsmpc_config cfg;
    vsmpc::DevCfg dev;
    int variant;     // tuned instantiation (1..), or VARIANT_NONE on a runtime handle
    int runtime;     // solve with the runtime-sized kernel (vsmpc_create_ex)
    vsmpc::RtDims rt;               // its sizes; on every handle: the linearise and certify kernels are sized by them too
    vsmpc::DevBuf<double> d_ws;     // its per-instance workspace, max_batch x rt.ws_doubles
    // What each create flag of the runtime family owns: `on`, the sizes of its kernel (filled on every handle), its workspace
    // (max_batch x dims.ws_doubles) and the staging of its host-pointer entry, one chunk of instances at a time.
    struct RtOwned { int on; vsmpc::RtDims dims; vsmpc::DevBuf<double> ws; };
    // VSMPC_CREATE_SENSITIVITY: sens_kernel_rt; the outputs of SENS_CHUNK instances
    struct Sens : RtOwned {
        vsmpc::StageBuf<double> dx, dfm;
        vsmpc::StageBuf<int> active, flags;
    } sens;
    // VSMPC_CREATE_ADJOINT: adjoint_kernel_rt[_tuned]; `ws` where the handle is not a runtime one (there d_ws serves); the
    // cotangents, the rows of tunables and the outputs of ADJ_CHUNK instances
    struct Adjoint : RtOwned {
        vsmpc::StageBuf<double> xbar, fmbar, tun, gx0, gcfg;
        vsmpc::StageBuf<int> active, flags;
    } adjoint;
    // VSMPC_CREATE_ADJOINT_RECORD (implies `adjoint`, whose workspace and staging serve; `ws` stays empty):
    // adjoint_record_kernel_rt[_tuned]; its two further outputs of ADJ_CHUNK instances
    struct AdjointRecord : RtOwned {
        vsmpc::StageBuf<double> gin, gmodel;
    } adjoint_record;
    // VSMPC_CREATE_TUNABLES: device staging of the rows of vsmpc_solve_batch_tuned, max_batch x VSMPC_TUNE_SIZE
    int tunables;
    vsmpc::DevBuf<double> d_tun;
    // VSMPC_CREATE_CERTIFY: device staging of vsmpc_certify_batch for max_batch instances: x, y | certificate, tunables
    int certify;
    vsmpc::DevBuf<double> d_cx, d_cy, d_ccert, d_ctun;
    int form;       // condensing form of the solve kernel (vsmpc_set_kernel_form)
    int small_mode; // which kernel serves small batches (vsmpc_set_small_batch_kernel): 0 auto, 1 never, 2 always
    int cu_count;   // compute units of `device` (read once, at create): auto takes the small-batch kind up to this batch
    vsmpc::KinOpts kin;     // vsmpc_set_kinematics_options
    int device;
    int max_batch;
    int n_var, n_con, n_in, n_p;
    // device staging buffers for the host-pointer entry points
    vsmpc::DevBuf<double> d_in, d_x, d_fm;
    vsmpc::DevBuf<int> d_status, d_iters;
    vsmpc::DevBuf<double> d_lin;  // A | Bj | Bt | c for max_batch instances
    vsmpc::DevBuf<double> d_dbg;  // M | L for one instance
    vsmpc::DevBuf<double> d_kin;  // vsmpc_kinematics_batch: records in, terms out (max_batch instances)
    vsmpc::DevBuf<double> d_kout;
    vsmpc::DevBuf<unsigned long long> d_stamps;  // vsmpc_debug_phase_cycles (max_batch x 16)
    vsmpc::Event ev0, ev1;
    // host-pointer entry for larger batches: chunks alternate between two streams so that the upload of one chunk, the
    // solve of the previous one and the download of the one before overlap (full overlap needs pinned caller buffers)
    vsmpc::Stream pipe[4];
    vsmpc::Event pipe_done[4];
    vsmpc::Event pipe_start;
    // small batches through the host-pointer entry (the reference's own use: one instance per tick): pinned,
    // device-mapped staging that the kernel reads and writes directly, instead of five small copies
    vsmpc::Owned<void*, hipHostFree> stage;
    double* h_stage;      // host view (typed view of `stage`, owns nothing):  in[ZC_MAX][n_in] | x[ZC_MAX][n_var] | fm[ZC_MAX][24] |
                          //   status[ZC_MAX] | iters[ZC_MAX] | kin[ZC_MAX][VSMPC_KIN_SIZE] (vsmpc_tick) | tun[ZC_MAX][VSMPC_TUNE_SIZE]
    double* d_stage;      // device view of the same allocation (its own base pointer: the two views are unrelated addresses)
};

// resident closed-loop state of a batch (uses the handle's record / first-move / status buffers as its per-tick scratch)
struct vsmpc_rollout {
    vsmpc_handle* h;
    int batch;
    int substeps;
    vsmpc::RolloutDev rd;
    vsmpc::DevBuf<double> d_state, d_params;
    vsmpc::DevBuf<int> d_tick;
    vsmpc::DevBuf<double> d_tpos, d_tvel, d_talpha;
    vsmpc::DevBuf<double> d_trpy, d_trpyd;   // vsmpc_rollout_set_attitude_tracks (or empty)
    int attitude_adjoint;     // the tracks were set with VSMPC_ATTITUDE_ADJOINT: the sweep runs the ATT kernels
    vsmpc::DevBuf<double> d_log;
    int log_ticks;
    vsmpc::DevBuf<double> d_tstate;  // per-instance tick state: reference window FIFO, RPY unwrap (see vsmpc_rollout.hip)
    int valid;                // 0 after a run failed half-way: the device counters are ahead, reset() before the next run
    vsmpc::DevBuf<double> d_rec;     // record of the next tick ([batch][n_in]): written by reset and by every tick's advance
    vsmpc::DevBuf<vsmpc::RolloutCtl> d_ctl;   // per-run control block read by advance_kernel (log destination, tick base)
    int ticks_done;           // ticks since the last reset (the same for every instance)
    vsmpc::Stream own_stream; // used when the caller passes the null stream (which cannot be captured)
    hipGraphExec_t gexec;     // GRAPH_TICKS ticks (3 launches each) captured once, replayed per chunk
    int graph_state;          // 0 not built yet, 1 ready, -1 capture unavailable (direct launches only)
    int graph_form;           // h->form the graph was captured with (vsmpc_set_kernel_form on the handle rebuilds it)
    int graph_small;          // small_batch_kernel(h, batch) it was captured with (vsmpc_set_small_batch_kernel likewise)
    // kinematic-tree plant (vsmpc_rollout_set_tree)
    int use_tree;
    vsmpc_tree tree;
    vsmpc::DevBuf<double> d_rs;   // provider states [batch][VSMPC_RS_SIZE]
    vsmpc::DevBuf<double> d_ro;   // Robot-level outputs of the provider [batch][VSMPC_RO_SIZE]
    // VSMPC_TREE_ADJOINT (vsmpc_rollout_set_tree_ex): the sweep's rows of one launch, terms [batch][VSMPC_TT_SIZE] and their
    // Jacobian [batch][VSMPC_TT_SIZE][VSMPC_TT_NDIR] (allocated by the first call with the flag)
    int tree_adjoint;
    vsmpc::DevBuf<double> d_tt, d_tj;
    // per-instance tunables (vsmpc_rollout_set_tunables)
    int use_tun;
    vsmpc::DevBuf<double> d_tun;  // rows [batch][VSMPC_TUNE_SIZE]
    // sensor noise and gusts (vsmpc_rollout_set_noise): the record and advance launches are then of the noisy kernels
    int use_noise;
    vsmpc::RolloutNoise noise;
    // tape of the last vsmpc_rollout_run_taped and the scratch of vsmpc_rollout_backward: allocated or grown by run_taped
    struct Tape {
        int ticks = 0;        // ticks on the tape; 0: none (never taped, or invalidated by reset / set_* / an untaped run)
        int cap = 0;          // ticks the four buffers below hold
        int tick_base = 0;    // the rollout's tick counter at the start of the taped run
        vsmpc::KinOpts kin = {};   // tree plant: the handle's kinematics options (joint selector) the taped run flew with
        vsmpc::DevBuf<double> s, rec, fm;   // [cap][batch][VSMPC_PLANT_STATE | n_in | VSMPC_FM_SIZE]
        vsmpc::DevBuf<int> status;          // [cap][batch]
        // per-instance rows of the sweep: cotangents of the plant state, the window and the first move; the record adjoint's
        // xbar (zeros, [n_var]), grad_in, grad_cfg, flags and status of one tick; the sums over the ticks
        vsmpc::DevBuf<double> sbar, wbar, fmbar, xbar, gin, gcfg_t, gcfg, log_bar;
        vsmpc::DevBuf<int> flags_t, flags, bstatus;
        int log_bar_ticks = 0;              // rows of ticks the host entry's log_bar staging holds
        // vsmpc_rollout_backward_full: dL/d(plant parameters) [batch][VSMPC_PLANT_PARAMS] and dL/d(tracks) [batch][6 n_traj +
        // n_alpha], allocated by the first call that asks for either (gtraj last: its presence says that both are there)
        vsmpc::DevBuf<double> gpar, gtraj;
        // vsmpc_rollout_backward_attitude: dL/d(traj_rpy | traj_rpy_dot) [batch][6 n_traj], allocated by the first call that
        // asks for it
        vsmpc::DevBuf<double> gatt;
    } tape;
};

namespace vsmpc {

constexpr int ZC_MAX = 8;  // largest batch served through the mapped staging buffer
#ifndef VS_PIPE_CHUNK
#define VS_PIPE_CHUNK 1024
#endif
#ifndef VS_PIPE_STREAMS
#define VS_PIPE_STREAMS 2
#endif
constexpr int PIPE_CHUNK = VS_PIPE_CHUNK;   // instances per chunk of the pipelined host-pointer entry
constexpr int PIPE_STREAMS = VS_PIPE_STREAMS;
static_assert(PIPE_STREAMS >= 1 && PIPE_STREAMS <= 4, "vsmpc_handle::pipe holds four streams");
constexpr int SENS_CHUNK = 256;   // instances per chunk of vsmpc_sensitivity_batch (dx_dx0 staging: 82 MB at (40, 2, 40))
constexpr int SENS_NPAR = VSMPC_N_STATES;
constexpr int ADJ_CHUNK = 256;    // instances per chunk of vsmpc_adjoint_batch and vsmpc_adjoint_record_batch

void fill_dt(const vsmpc_config& c, double* dt);   // vsmpc_capi.hip: the dt schedule, MAX_STAGES doubles
bool tree_valid(const vsmpc_tree& tree);            // vsmpc_capi_debug.hip: parents precede children, indices in range
// vsmpc_capi_solve.hip.  The solve launch of a handle: the tuned instantiation, or the runtime-sized kernel with the
// workspace of instances `first` .. `first + batch - 1` (a chunk of a larger batch must not share workspace with a chunk
// on another stream).  d_tun: rows of per-instance tunables of these instances (the tuned kind of either kernel), or
// nullptr: the handle's configuration for all of them.
hipError_t solve_launch(const vsmpc_handle* h, const double* d_in, int batch, double* d_x, double* d_fm, int* d_status,
                        int* d_iters, size_t first, hipStream_t s, const double* d_tun = nullptr);
// does a launch of `batch` instances of the handle's configuration run on the small-batch kind (solve_kernel_small)?  The
// horizon has it, the handle's form is structured, and the mode says always, or auto with the batch within the CUs.  (The
// per-instance-tunables entries keep the shipped kernel.)
inline bool small_batch_kernel(const vsmpc_handle* h, int batch) {
    return !h->runtime && h->form != 2 && variant_has_small(h->variant) &&
           (h->small_mode == 2 || (h->small_mode == 0 && batch <= h->cu_count));
}

}  // namespace vsmpc
