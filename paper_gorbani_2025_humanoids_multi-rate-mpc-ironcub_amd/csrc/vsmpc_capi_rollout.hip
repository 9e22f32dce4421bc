// C-ABI of include/vsmpc.h and include/vsmpc_jet.h, the closed-loop rollout: everything vsmpc_rollout_*.
#include "vsmpc_host.hpp"

using namespace vsmpc;

namespace {

// Tree plant of a rollout: provider on the body-frame states (joints + this tick's move when `fm` is given), then the
// kinematics terms of those records (I_B for the plant's integration; the Lambda terms are formed again after the advance,
// with the thrusts it measured).  The handle's kinematics buffers are the rollout's scratch, like its solve buffers.
hipError_t enqueue_tree(vsmpc_rollout* r, const double* fm, const int* status, hipStream_t s) {
    vsmpc_handle* h = r->h;
    hipError_t e = launch_tree_state(r->rd, r->batch, r->d_state, fm, status, r->d_rs, s);
    if (e == hipSuccess) e = launch_provider(r->tree, r->d_rs, r->batch, h->d_kin, r->d_ro, nullptr, h->n_in, s);
    if (e == hipSuccess) {
        KinOpts o = h->kin;
        o.constant_lambda = 0;
        e = launch_kinematics(h->d_kin, r->batch, h->d_kout, o, s);
    }
    return e;
}
// Lambda_lin,B | Lambda_ang,B of the tree at the thrusts the advance kernel left in the kinematics records -> r->d_rec
hipError_t enqueue_tree_lambda(vsmpc_rollout* r, hipStream_t s) {
    KinOpts o = r->h->kin;
    o.constant_lambda = 0;
    o.skip_inertia = 1;   // the record's I_G = R I_B R^T is the advance kernel's (the tree is evaluated in the body frame)
    return launch_kinematics_patch(r->h->d_kin, r->batch, r->d_rec, r->h->n_in, o, s);
}

// drops the captured ticks and marks the rollout for vsmpc_rollout_reset before the next run
void invalidate(vsmpc_rollout* r) {
    if (r->gexec) { (void)hipGraphExecDestroy(r->gexec); r->gexec = nullptr; }
    r->graph_state = 0;
    r->valid = 0;
}

}  // namespace

extern "C" {

int vsmpc_rollout_create(vsmpc_handle* h, int batch, const double* traj_pos, const double* traj_vel, int n_traj,
                         const double* traj_alpha, int n_alpha, double alpha_dt, vsmpc_rollout** out) {
    if (h == nullptr || out == nullptr || traj_pos == nullptr || traj_vel == nullptr || traj_alpha == nullptr ||
        batch <= 0 || n_traj <= 0 || n_alpha <= 0 || !(alpha_dt > 0.0))
        return invalid_arg();
    *out = nullptr;
    if (batch > h->max_batch) return VSMPC_ERR_BATCH_TOO_LARGE;
    ON_DEVICE(h->device);
    vsmpc_rollout* r = new (std::nothrow) vsmpc_rollout();
    if (r == nullptr) return VSMPC_ERR_ALLOC;
    r->h = h;
    r->batch = batch;
    r->rd.n_in = h->n_in;
    r->rd.n_ref = h->cfg.n_iter - h->cfg.n_iter_small + 1;
    r->rd.ratio = int(std::lround(h->cfg.period_large / h->cfg.period_small));   // constraintsVSMPC.cpp:322
    r->rd.n_traj = n_traj;
    r->rd.n_alpha = n_alpha;
    r->rd.period_mpc = h->cfg.period_mpc;
    r->rd.alpha_dt = alpha_dt;
    r->rd.n_ts = 12 * r->rd.n_ref + 8;
    {   // TrajectoryManager::configure(.., 1 / periodMPC): des_fps truncated to int (systemDynamicsVSMPC.cpp:272), integer
        // up-sampling factor against the track's own rate
        const int des_fps = int(1.0 / h->cfg.period_mpc + 1e-9), fps = int(std::lround(1.0 / alpha_dt));
        if (fps <= 0 || des_fps < fps || des_fps % fps != 0) { delete r; return invalid_arg(); }
        r->rd.alpha_up = des_fps / fps;
    }
    r->substeps = std::min(16, std::max(1, int(std::lround(h->cfg.period_mpc / 1e-3))));  // 1 kHz plant, as the MuJoCo harness
    const size_t B = size_t(batch);
    hipError_t e = r->d_state.alloc(B * VSMPC_PLANT_STATE);
    if (e == hipSuccess) e = r->d_params.alloc(B * VSMPC_PLANT_PARAMS);
    if (e == hipSuccess) e = r->d_tick.alloc(B);
    if (e == hipSuccess) e = r->d_tpos.alloc(size_t(n_traj) * 3);
    if (e == hipSuccess) e = r->d_tvel.alloc(size_t(n_traj) * 3);
    if (e == hipSuccess) e = r->d_talpha.alloc(size_t(n_alpha));
    if (e == hipSuccess) e = hipMemcpy(r->d_tpos, traj_pos, size_t(n_traj) * 3 * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(r->d_tvel, traj_vel, size_t(n_traj) * 3 * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(r->d_talpha, traj_alpha, size_t(n_alpha) * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(r->d_tick, 0, B * sizeof(int));
    if (e == hipSuccess) e = r->d_ctl.alloc(1);
    if (e == hipSuccess) e = r->d_tstate.alloc(B * r->rd.n_ts);
    if (e == hipSuccess) e = hipMemset(r->d_tstate, 0, B * r->rd.n_ts * sizeof(double));
    if (e == hipSuccess) e = r->d_rec.alloc(B * h->n_in);
    if (e == hipSuccess) e = hipMemset(r->d_rec, 0, B * h->n_in * sizeof(double));
    if (e == hipSuccess) e = hipStreamCreateWithFlags(r->own_stream.put(), hipStreamNonBlocking);
    if (e != hipSuccess) {
        vsmpc_rollout_destroy(r);
        return e == hipErrorOutOfMemory ? VSMPC_ERR_ALLOC : hip_fail(e, "vsmpc_rollout_create");
    }
    *out = r;
    return VSMPC_OK;
}

void vsmpc_rollout_destroy(vsmpc_rollout* r) {
    if (r == nullptr) return;
    DeviceScope scope(r->h->device);   // the owners free on the current device
    if (r->gexec) (void)hipGraphExecDestroy(r->gexec);
    delete r;
}

int vsmpc_rollout_reset(vsmpc_rollout* r, const double* state, const double* params) {
    if (r == nullptr || state == nullptr || params == nullptr) return invalid_arg();
    ON_DEVICE(r->h->device);
    const size_t B = size_t(r->batch);
    HIP_TRY(hipMemcpy(r->d_state, state, B * VSMPC_PLANT_STATE * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(r->d_params, params, B * VSMPC_PLANT_PARAMS * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(r->d_tick, 0, B * sizeof(int)));
    r->ticks_done = 0;
    // record of tick 0; from here on every tick's advance kernel leaves the record of the following tick
    r->valid = 0;
    if (r->use_tree) HIP_TRY(enqueue_tree(r, nullptr, nullptr, nullptr));
    HIP_TRY(launch_record(r->rd, r->batch, r->d_state, r->d_params, r->d_tick, r->d_tpos, r->d_tvel, r->d_talpha,
                          r->d_tstate, r->d_rec, nullptr));
    if (r->use_tree) HIP_TRY(enqueue_tree_lambda(r, nullptr));
    HIP_TRY(hipDeviceSynchronize());
    r->valid = 1;
    return VSMPC_OK;
}

int vsmpc_rollout_set_attitude_tracks(vsmpc_rollout* r, const double* traj_rpy, const double* traj_rpy_dot) {
    if (r == nullptr) return invalid_arg();
    ON_DEVICE(r->h->device);
    const size_t bytes = size_t(r->rd.n_traj) * 3 * sizeof(double);
    // whatever happens below, the captured ticks and the record of the next tick refer to the old tracks: drop them first
    invalidate(r);
    auto set = [&](DevBuf<double>& dst, const double* src) -> hipError_t {
        if (src == nullptr) { dst.reset(); return hipSuccess; }
        const hipError_t e = dst == nullptr ? dst.alloc(bytes / sizeof(double)) : hipSuccess;   // (empty after a failure)
        if (e != hipSuccess) return e;
        return hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice);
    };
    const hipError_t e0 = set(r->d_trpy, traj_rpy);
    r->rd.traj_rpy = r->d_trpy;              // (a failed set leaves either the old, still valid buffer or nullptr)
    HIP_TRY(e0);
    const hipError_t e1 = set(r->d_trpyd, traj_rpy_dot);
    r->rd.traj_rpyd = r->d_trpyd;
    HIP_TRY(e1);
    return VSMPC_OK;
}

int vsmpc_rollout_set_tree(vsmpc_rollout* r, const vsmpc_tree* tree) {
    if (r == nullptr) return invalid_arg();
    ON_DEVICE(r->h->device);
    invalidate(r);   // the captured ticks have other launches
    r->use_tree = 0;
    r->rd.tree = 0;
    if (tree == nullptr) return VSMPC_OK;
    if (!tree_valid(*tree)) return invalid_arg();
    const size_t B = size_t(r->batch);
    if (r->d_rs == nullptr) HIP_TRY(r->d_rs.alloc(B * VSMPC_RS_SIZE));
    if (r->d_ro == nullptr) HIP_TRY(r->d_ro.alloc(B * VSMPC_RO_SIZE));
    r->tree = *tree;
    r->use_tree = 1;
    r->rd.tree = 1;
    r->rd.tree_ro = r->d_ro;
    r->rd.tree_kout = r->h->d_kout;
    r->rd.tree_kin = r->h->d_kin;
    return VSMPC_OK;
}

int vsmpc_rollout_set_tunables(vsmpc_rollout* r, const double* tunables) {
    if (r == nullptr) return invalid_arg();
    ON_DEVICE(r->h->device);
    if (tunables != nullptr) {   // first, what can fail: a refused call leaves the rollout as it was
        const size_t n = size_t(r->batch) * VSMPC_TUNE_SIZE;
        if (r->d_tun == nullptr) {
            const hipError_t e = r->d_tun.alloc(n);   // on first use, like the buffers of set_tree
            if (e != hipSuccess) return hip_fail(e, "hipMalloc(rollout tunables)");
        }
        HIP_TRY(hipMemcpy(r->d_tun, tunables, n * sizeof(double), hipMemcpyHostToDevice));
    }
    invalidate(r);   // the captured ticks hold the other solve launch
    r->use_tun = tunables != nullptr;
    return VSMPC_OK;
}

// include/vsmpc_jet.h
int vsmpc_rollout_set_jet_plant(vsmpc_rollout* r, vsmpc_jet* j, const double* Q, const double* R) {
    if (r == nullptr || (j != nullptr && (Q == nullptr || R == nullptr))) return invalid_arg();
    RolloutDev rd = r->rd;
    rd.jet_nn = 0;
    rd.jet_w = nullptr;
    if (j != nullptr) {
        int dev = -1;
        jet_plant_view(j, &rd.jet_w, &rd.jet_hidden, rd.jet_norm, &dev);
        if (dev != r->h->device) return invalid_arg();
        rd.jet_nn = 1;
        for (int k = 0; k < 4; ++k) { rd.ekf_q[k] = Q[k]; rd.ekf_r[k] = R[k]; }
    }
    r->rd = rd;
    // the captured tick graph holds the old launch arguments, and the record of the next tick was built from the other
    // set of measurements: rebuild both
    invalidate(r);
    return VSMPC_OK;
}

}  // extern "C"

namespace {

constexpr int GRAPH_TICKS = 25;  // ticks per captured graph (50 kernel nodes)

// one closed-loop tick: two launches on `s` (solve, advance + next record), the stream order is the only
// synchronisation the loop needs
hipError_t enqueue_tick(vsmpc_rollout* r, hipStream_t s) {
    vsmpc_handle* h = r->h;
    hipError_t e = solve_launch(h, r->d_rec, r->batch, h->d_x, h->d_fm, h->d_status, h->d_iters, 0, s,
                                r->use_tun ? r->d_tun : nullptr);
    if (e == hipSuccess && r->use_tree) e = enqueue_tree(r, h->d_fm, h->d_status, s);   // A_mom, I_B of the joints after the move
    if (e == hipSuccess)
        e = launch_advance(r->rd, r->batch, r->d_state, r->d_params, r->d_tick, h->d_fm, h->d_status, h->d_iters,
                           r->d_talpha, r->d_ctl, r->substeps, r->d_tpos, r->d_tvel, r->d_tstate, r->d_rec, s);
    if (e == hipSuccess && r->use_tree) e = enqueue_tree_lambda(r, s);
    return e;
}

// Captures GRAPH_TICKS ticks into a graph (every launch argument is tick-invariant: tick counters, log destination and
// tick base live in device memory).  Launch-bound loop -> one graph launch per chunk instead of 50 kernel launches.
void build_tick_graph(vsmpc_rollout* r, hipStream_t s) {
    r->graph_state = -1;
    r->graph_form = r->h->form;
    r->graph_small = small_batch_kernel(r->h, r->batch) ? 1 : 0;
    if (hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal) != hipSuccess) { (void)hipGetLastError(); return; }
    hipError_t e = hipSuccess;
    for (int t = 0; t < GRAPH_TICKS && e == hipSuccess; ++t) e = enqueue_tick(r, s);
    hipGraph_t graph = nullptr;
    const hipError_t e2 = hipStreamEndCapture(s, &graph);
    if (e == hipSuccess && e2 == hipSuccess && graph != nullptr &&
        hipGraphInstantiate(&r->gexec, graph, nullptr, nullptr, 0) == hipSuccess)
        r->graph_state = 1;
    else
        (void)hipGetLastError();
    if (graph) (void)hipGraphDestroy(graph);
}

}  // namespace

extern "C" {

int vsmpc_rollout_run(vsmpc_rollout* r, int ticks, double* log, void* stream) {
    if (r == nullptr || ticks < 0) return invalid_arg();
    if (!r->valid) return invalid_arg();   // never reset, or a previous run failed half-way: reset() first
    if (ticks == 0) return VSMPC_OK;
    vsmpc_handle* h = r->h;
    ON_DEVICE(h->device);
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : r->own_stream.h;
    const size_t row = size_t(r->batch) * VSMPC_ROLLOUT_LOG;
    if (log != nullptr && r->log_ticks < ticks) {
        r->log_ticks = 0;
        hipError_t e = r->d_log.alloc(size_t(ticks) * row);   // (frees the shorter one first)
        if (e != hipSuccess) return e == hipErrorOutOfMemory ? VSMPC_ERR_ALLOC : hip_fail(e, "vsmpc_rollout_run");
        r->log_ticks = ticks;
    }
    const RolloutCtl ctl = {log ? r->d_log : nullptr, r->ticks_done, log ? ticks : 0};
    HIP_TRY(hipMemcpyAsync(r->d_ctl, &ctl, sizeof(ctl), hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));  // `ctl` lives on this stack frame
    r->valid = 0;                       // until the whole run has completed: a failure below leaves the counters ahead
    int t = 0;
    // the captured launches are of the other condensing form, or of the other kernel for this batch size
    if (r->graph_state != 0 && (r->graph_form != h->form || r->graph_small != (small_batch_kernel(h, r->batch) ? 1 : 0))) invalidate(r);
    if (ticks >= GRAPH_TICKS && r->graph_state == 0) build_tick_graph(r, s);
    if (r->graph_state == 1)
        for (; ticks - t >= GRAPH_TICKS; t += GRAPH_TICKS) HIP_TRY(hipGraphLaunch(r->gexec, s));
    for (; t < ticks; ++t) HIP_TRY(enqueue_tick(r, s));
    HIP_TRY(download_rows(log, r->d_log, 0, size_t(ticks), row, s));
    HIP_TRY(hipStreamSynchronize(s));
    r->ticks_done += ticks;
    r->valid = 1;
    return VSMPC_OK;
}

int vsmpc_rollout_get_state(vsmpc_rollout* r, double* state) {
    if (r == nullptr || state == nullptr) return invalid_arg();
    ON_DEVICE(r->h->device);
    HIP_TRY(hipMemcpy(state, r->d_state, size_t(r->batch) * VSMPC_PLANT_STATE * sizeof(double), hipMemcpyDeviceToHost));
    return VSMPC_OK;
}

int vsmpc_rollout_get_records(vsmpc_rollout* r, double* records) {
    if (r == nullptr || records == nullptr) return invalid_arg();
    ON_DEVICE(r->h->device);
    HIP_TRY(hipMemcpy(records, r->d_rec, size_t(r->batch) * r->h->n_in * sizeof(double), hipMemcpyDeviceToHost));
    return VSMPC_OK;
}

}  // extern "C"
