// C-ABI of include/vsmpc.h and include/vsmpc_jet.h, the closed-loop rollout: everything vsmpc_rollout_*.
#include "vsmpc_host.hpp"

using namespace vsmpc;

namespace {

// the launch record of the rollout's two kernels (in RolloutTick's order): its own rows, the handle's solve outputs as scratch
RolloutTick tick_record(const vsmpc_rollout* r) {
    const vsmpc_handle* h = r->h;
    return {r->batch, r->substeps, r->d_state, r->d_params, r->d_tick, r->d_tpos, r->d_tvel, r->d_talpha, r->d_tstate, r->d_rec,
            h->d_fm, h->d_status, h->d_iters, r->d_ctl};
}

// a failed allocation is VSMPC_ERR_ALLOC, any other HIP failure of `what` VSMPC_ERR_HIP
int alloc_fail(hipError_t e, const char* what) { return e == hipErrorOutOfMemory ? VSMPC_ERR_ALLOC : hip_fail(e, what); }

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
    r->tape.ticks = 0;
}

const RolloutNoise* noise_of(const vsmpc_rollout* r) { return r->use_noise ? &r->noise : nullptr; }

const char* const NOISE_NO_ADJOINT =
    "vsmpc_rollout_run_taped / vsmpc_rollout_backward: no adjoint of a rollout with noise (vsmpc_rollout_set_noise): its derivative would need the noise's "
    "own dependence on the attitude, the mass and I_B";

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
        return alloc_fail(e, "vsmpc_rollout_create");
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
    r->tape.ticks = 0;
    // record of tick 0; from here on every tick's advance kernel leaves the record of the following tick
    r->valid = 0;
    if (r->use_tree) HIP_TRY(enqueue_tree(r, nullptr, nullptr, nullptr));
    HIP_TRY(launch_record(r->rd, tick_record(r), nullptr, noise_of(r)));
    if (r->use_tree) HIP_TRY(enqueue_tree_lambda(r, nullptr));
    HIP_TRY(hipDeviceSynchronize());
    r->valid = 1;
    return VSMPC_OK;
}

int vsmpc_rollout_set_attitude_tracks(vsmpc_rollout* r, const double* traj_rpy, const double* traj_rpy_dot) {
    return vsmpc_rollout_set_attitude_tracks_ex(r, traj_rpy, traj_rpy_dot, 0u);
}

int vsmpc_rollout_set_attitude_tracks_ex(vsmpc_rollout* r, const double* traj_rpy, const double* traj_rpy_dot, unsigned flags) {
    if (r == nullptr || (flags & ~VSMPC_ATTITUDE_ADJOINT) != 0u) return invalid_arg();
    ON_DEVICE(r->h->device);
    r->attitude_adjoint = (flags & VSMPC_ATTITUDE_ADJOINT) != 0u ? 1 : 0;
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

int vsmpc_rollout_set_tree(vsmpc_rollout* r, const vsmpc_tree* tree) { return vsmpc_rollout_set_tree_ex(r, tree, 0u); }

int vsmpc_rollout_set_tree_ex(vsmpc_rollout* r, const vsmpc_tree* tree, unsigned flags) {
    if (r == nullptr || (flags & ~VSMPC_TREE_ADJOINT) != 0u) return invalid_arg();
    ON_DEVICE(r->h->device);
    const bool adjoint = tree != nullptr && (flags & VSMPC_TREE_ADJOINT) != 0u;
    const size_t B = size_t(r->batch);
    if (adjoint) {   // first, what the flag can fail on: a refused call leaves the rollout as it was
        if (r->h->kin.constant_lambda) return unsupported();
        if (!tree_valid(*tree)) return invalid_arg();
        // every buffer of the tree plant, the forward run's two among them, in front of anything that changes the rollout
        hipError_t e = hipSuccess;
        if (r->d_rs == nullptr) e = r->d_rs.alloc(B * VSMPC_RS_SIZE);
        if (e == hipSuccess && r->d_ro == nullptr) e = r->d_ro.alloc(B * VSMPC_RO_SIZE);
        if (e == hipSuccess && r->d_tj == nullptr) {   // (d_tj last of the two: its presence says that both are there)
            e = r->d_tt.alloc(B * VSMPC_TT_SIZE);
            if (e == hipSuccess) e = r->d_tj.alloc(B * VSMPC_TT_SIZE * VSMPC_TT_NDIR);
            if (e != hipSuccess) r->d_tt.reset();
        }
        if (e != hipSuccess) return alloc_fail(e, "vsmpc_rollout_set_tree_ex");
    }
    invalidate(r);   // the captured ticks have other launches
    r->use_tree = 0;
    r->rd.tree = 0;
    r->tree_adjoint = 0;
    if (tree == nullptr) return VSMPC_OK;
    if (!tree_valid(*tree)) return invalid_arg();
    if (r->d_rs == nullptr) HIP_TRY(r->d_rs.alloc(B * VSMPC_RS_SIZE));
    if (r->d_ro == nullptr) HIP_TRY(r->d_ro.alloc(B * VSMPC_RO_SIZE));
    r->tree = *tree;
    r->use_tree = 1;
    r->rd.tree = 1;
    r->rd.tree_ro = r->d_ro;
    r->rd.tree_kout = r->h->d_kout;
    r->rd.tree_kin = r->h->d_kin;
    r->tree_adjoint = adjoint ? 1 : 0;
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

int vsmpc_rollout_set_noise(vsmpc_rollout* r, const vsmpc_noise* n) {
    if (n != nullptr) {   // first, what can be refused: a refused call leaves the rollout as it was, and touches no device
        const struct { const char* name; double v; } sig[] = {
            {"sigma_pos", n->sigma_pos}, {"sigma_lin_vel", n->sigma_lin_vel}, {"sigma_rpy", n->sigma_rpy},
            {"sigma_ang_vel", n->sigma_ang_vel}, {"sigma_force", n->sigma_force}, {"sigma_torque", n->sigma_torque}};
        for (const auto& f : sig)
            if (!(f.v >= 0.0) || !std::isfinite(f.v)) return invalid_field("vsmpc_rollout_set_noise", f.name);
        if (n->first_index < 0) return invalid_field("vsmpc_rollout_set_noise", "first_index");
    }
    if (r == nullptr) return invalid_arg();
    ON_DEVICE(r->h->device);
    invalidate(r);   // the captured ticks have the other launches, the record of the next tick the other measurement
    r->use_noise = n != nullptr;
    if (n != nullptr)
        r->noise = {n->seed, static_cast<unsigned long long>(n->first_index), n->sigma_pos, n->sigma_lin_vel, n->sigma_rpy,
                    n->sigma_ang_vel, n->sigma_force, n->sigma_torque};
    return VSMPC_OK;
}

int vsmpc_rollout_noise_draws(vsmpc_rollout* r, int tick0, int ticks, double* z, unsigned* words) {
    if (r == nullptr || z == nullptr || tick0 < 0 || ticks <= 0 || tick0 > INT_MAX - ticks) return invalid_arg();
    if (!r->use_noise) return invalid_field("vsmpc_rollout_noise_draws", "rollout: no noise set (vsmpc_rollout_set_noise)");
    ON_DEVICE(r->h->device);
    const size_t blocks = size_t(ticks) * size_t(r->batch) * 9;
    DevBuf<double> d_z;
    DevBuf<unsigned> d_w;
    hipError_t e = d_z.alloc(2 * blocks);
    if (e == hipSuccess && words != nullptr) e = d_w.alloc(4 * blocks);
    if (e != hipSuccess) return alloc_fail(e, "vsmpc_rollout_noise_draws");
    HIP_TRY(launch_noise_draws(r->noise, r->batch, tick0, ticks, d_z, d_w, nullptr));
    HIP_TRY(hipMemcpy(z, d_z, 2 * blocks * sizeof(double), hipMemcpyDeviceToHost));
    if (words != nullptr) HIP_TRY(hipMemcpy(words, d_w, 4 * blocks * sizeof(unsigned), hipMemcpyDeviceToHost));
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

// One closed-loop tick: two launches on `s` (solve, advance + next record), the stream order is the only
// synchronisation the loop needs.  With tape_row >= 0 the tape's rows of that tick of the run are copied out between the
// launches (state and record in front of the solve, first move and status behind it); -1 is the plain tick, kernels only.
hipError_t enqueue_tick(vsmpc_rollout* r, hipStream_t s, int tape_row) {
    vsmpc_handle* h = r->h;
    vsmpc_rollout::Tape& tp = r->tape;
    const bool taped = tape_row >= 0;
    const size_t B = size_t(r->batch), o = taped ? size_t(tape_row) * B : 0;
    auto keep = [&](void* dst, const void* src, size_t bytes) {
        return taped ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s) : hipSuccess;
    };
    hipError_t e = keep(tp.s + o * VSMPC_PLANT_STATE, r->d_state, B * VSMPC_PLANT_STATE * sizeof(double));
    if (e == hipSuccess) e = keep(tp.rec + o * h->n_in, r->d_rec, B * h->n_in * sizeof(double));
    if (e == hipSuccess)
        e = solve_launch(h, r->d_rec, r->batch, h->d_x, h->d_fm, h->d_status, h->d_iters, 0, s, r->use_tun ? r->d_tun : nullptr);
    if (e == hipSuccess) e = keep(tp.fm + o * VSMPC_FM_SIZE, h->d_fm, B * VSMPC_FM_SIZE * sizeof(double));
    if (e == hipSuccess) e = keep(tp.status + o, h->d_status, B * sizeof(int));
    if (e == hipSuccess && r->use_tree) e = enqueue_tree(r, h->d_fm, h->d_status, s);   // A_mom, I_B of the joints after the move
    if (e == hipSuccess) e = launch_advance(r->rd, tick_record(r), s, noise_of(r));
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
    for (int t = 0; t < GRAPH_TICKS && e == hipSuccess; ++t) e = enqueue_tick(r, s, -1);
    hipGraph_t graph = nullptr;
    const hipError_t e2 = hipStreamEndCapture(s, &graph);
    if (e == hipSuccess && e2 == hipSuccess && graph != nullptr &&
        hipGraphInstantiate(&r->gexec, graph, nullptr, nullptr, 0) == hipSuccess)
        r->graph_state = 1;
    else
        (void)hipGetLastError();
    if (graph) (void)hipGraphDestroy(graph);
}

// what a run does in front of its ticks: the device log of `ticks` rows (grown when shorter) and the control block
int begin_run(vsmpc_rollout* r, int ticks, double* log, hipStream_t s) {
    const size_t row = size_t(r->batch) * VSMPC_ROLLOUT_LOG;
    if (log != nullptr && r->log_ticks < ticks) {
        r->log_ticks = 0;
        hipError_t e = r->d_log.alloc(size_t(ticks) * row);   // (frees the shorter one first)
        if (e != hipSuccess) return alloc_fail(e, "vsmpc_rollout_run");
        r->log_ticks = ticks;
    }
    const RolloutCtl ctl = {log ? r->d_log : nullptr, r->ticks_done, log ? ticks : 0};
    HIP_TRY(hipMemcpyAsync(r->d_ctl, &ctl, sizeof(ctl), hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));  // `ctl` lives on this stack frame
    return VSMPC_OK;
}
// and behind them: the log comes back, the run has completed
int end_run(vsmpc_rollout* r, int ticks, double* log, hipStream_t s) {
    HIP_TRY(download_rows(log, r->d_log, 0, size_t(ticks), size_t(r->batch) * VSMPC_ROLLOUT_LOG, s));
    HIP_TRY(hipStreamSynchronize(s));
    r->ticks_done += ticks;
    r->valid = 1;
    return VSMPC_OK;
}

const char* const BACKWARD_NEEDS_FLAG =
    "vsmpc_rollout_backward needs a rollout on a handle created with VSMPC_CREATE_ADJOINT_RECORD (vsmpc_create_ex)";

// Tape of `ticks` ticks and the rows of the backward sweep.  A failure leaves no tape and the rollout as it was.
hipError_t grow_tape(vsmpc_rollout* r, int ticks) {
    vsmpc_rollout::Tape& tp = r->tape;
    const vsmpc_handle* h = r->h;
    const size_t B = size_t(r->batch), T = size_t(ticks);
    hipError_t e = hipSuccess;
    if (tp.cap < ticks) {
        tp.cap = 0;
        e = tp.s.alloc(T * B * VSMPC_PLANT_STATE);
        if (e == hipSuccess) e = tp.rec.alloc(T * B * h->n_in);
        if (e == hipSuccess) e = tp.fm.alloc(T * B * VSMPC_FM_SIZE);
        if (e == hipSuccess) e = tp.status.alloc(T * B);
        if (e == hipSuccess) e = tp.log_bar.alloc(T * B * VSMPC_ROLLOUT_LOG);
        if (e != hipSuccess) return e;
        tp.cap = ticks;
    }
    if (tp.bstatus == nullptr) {   // (allocated last: its presence says that all of them are there)
        e = tp.sbar.alloc(B * VSMPC_PLANT_STATE);
        if (e == hipSuccess) e = tp.wbar.alloc(B * 12 * r->rd.n_ref);
        if (e == hipSuccess) e = tp.fmbar.alloc(B * VSMPC_FM_SIZE);
        if (e == hipSuccess) e = tp.xbar.alloc(B * h->n_var);
        if (e == hipSuccess) e = hipMemset(tp.xbar, 0, B * h->n_var * sizeof(double));   // the sweep's xbar is zero
        if (e == hipSuccess) e = tp.gin.alloc(B * h->n_in);
        if (e == hipSuccess) e = tp.gcfg_t.alloc(B * VSMPC_GRAD_SIZE);
        if (e == hipSuccess) e = tp.gcfg.alloc(B * VSMPC_GRAD_SIZE);
        if (e == hipSuccess) e = tp.flags_t.alloc(B);
        if (e == hipSuccess) e = tp.flags.alloc(B);
        if (e == hipSuccess) e = tp.bstatus.alloc(B);
    }
    return e;
}

size_t traj_grad_size(const vsmpc_rollout* r) { return size_t(6) * size_t(r->rd.n_traj) + size_t(r->rd.n_alpha); }
size_t att_grad_size(const vsmpc_rollout* r) { return size_t(6) * size_t(r->rd.n_traj); }

// The two rows per instance of vsmpc_rollout_backward_full, on first request.  A failure leaves neither, and the tape as it was.
hipError_t grow_full(vsmpc_rollout* r) {
    vsmpc_rollout::Tape& tp = r->tape;
    if (tp.gtraj != nullptr) return hipSuccess;
    hipError_t e = tp.gpar.alloc(size_t(r->batch) * VSMPC_PLANT_PARAMS);
    if (e == hipSuccess) e = tp.gtraj.alloc(size_t(r->batch) * traj_grad_size(r));
    if (e != hipSuccess) { tp.gpar.reset(); tp.gtraj.reset(); }
    return e;
}

// The row per instance of vsmpc_rollout_backward_attitude, on first request.  A failure leaves the tape as it was.
hipError_t grow_att(vsmpc_rollout* r) {
    vsmpc_rollout::Tape& tp = r->tape;
    if (tp.gatt != nullptr) return hipSuccess;
    return tp.gatt.alloc(size_t(r->batch) * att_grad_size(r));
}

// The backward sweep over the tape, last tick to first, in stream order: tape.sbar holds dL/d(final state) on entry and
// dL/d(state at the start of the taped run) on exit; tape.gcfg and tape.flags receive the sums over the ticks.  Launch k of
// advance_adjoint_kernel is the record half of tick k behind the plant half of tick k - 1, with the record adjoint of tick
// k - 1 (the `_device` body of vsmpc_adjoint_record_batch: xbar = 0, fmbar = the plant half's) between launches k and k - 1.
// `full`: tape.gpar and tape.gtraj (grow_full) receive the sums over the ticks too, through the kernel's second instantiation.
// `att` (with `full`, on a rollout with VSMPC_ATTITUDE_ADJOINT): tape.gatt (grow_att) likewise; such a rollout's launches are
// of the ATT kernels whatever the entry asked for.
int enqueue_sweep(vsmpc_rollout* r, const double* d_log_bar, hipStream_t s, bool full = false, bool att = false) {
    vsmpc_handle* h = r->h;
    vsmpc_rollout::Tape& tp = r->tape;
    const size_t B = size_t(r->batch);
    const int T = tp.ticks;
    HIP_TRY(hipMemsetAsync(tp.wbar, 0, B * 12 * r->rd.n_ref * sizeof(double), s));
    HIP_TRY(hipMemsetAsync(tp.gcfg, 0, B * VSMPC_GRAD_SIZE * sizeof(double), s));
    HIP_TRY(hipMemsetAsync(tp.flags, 0, B * sizeof(int), s));
    RolloutAdj a = {};
    if (full) {
        HIP_TRY(hipMemsetAsync(tp.gpar, 0, B * VSMPC_PLANT_PARAMS * sizeof(double), s));
        HIP_TRY(hipMemsetAsync(tp.gtraj, 0, B * traj_grad_size(r) * sizeof(double), s));
        a.gpar = tp.gpar;
        a.gtraj = tp.gtraj;
    }
    a.attitude = r->attitude_adjoint;
    if (att) {
        HIP_TRY(hipMemsetAsync(tp.gatt, 0, B * att_grad_size(r) * sizeof(double), s));
        a.gatt = tp.gatt;
    }
    a.batch = r->batch;
    a.substeps = r->substeps;
    a.params = r->d_params;
    a.traj_vel = r->d_tvel;
    a.traj_alpha = r->d_talpha;
    a.gin = tp.gin; a.gcfg_t = tp.gcfg_t; a.flags_t = tp.flags_t;
    a.sbar = tp.sbar; a.wbar = tp.wbar; a.fmbar = tp.fmbar; a.gcfg = tp.gcfg; a.flags = tp.flags;
    for (int k = T; k >= 0; --k) {
        if (r->use_tree) {
            // tau and its Jacobian at the state between ticks k - 1 and k: the tape's row k, behind the last tick the state the
            // run left (an untaped run, a reset and the set_* calls all drop the tape), under the taped run's joint selector
            const double* sk = k < T ? tp.s + size_t(k) * B * VSMPC_PLANT_STATE : r->d_state.get();
            HIP_TRY(launch_tree_jacobian(r->tree, tp.kin, sk + VSMPC_PS_Q, VSMPC_PLANT_STATE, sk + VSMPC_PS_T, VSMPC_PLANT_STATE,
                                         r->batch, r->d_tt, r->d_tj, s));
            a.tree_terms = r->d_tt;
            a.tree_jac = r->d_tj;
        }
        if (k < T) {
            const int rc = vsmpc_adjoint_record_batch_device(h, tp.rec + size_t(k) * B * h->n_in, r->use_tun ? r->d_tun.get() : nullptr,
                                                             tp.xbar, tp.fmbar, r->batch, nullptr, nullptr, tp.bstatus, nullptr,
                                                             nullptr, tp.gcfg_t, nullptr, tp.flags_t, tp.gin, nullptr, s);
            if (rc != VSMPC_OK) return rc;
        }
        a.tick_rec = k < T ? tp.tick_base + k : -1;
        a.first = k < T && tp.tick_base + k == 0;
        a.s_rec = k < T ? tp.s + size_t(k) * B * VSMPC_PLANT_STATE : nullptr;
        a.tick_plant = k > 0 ? tp.tick_base + k - 1 : -1;
        if (k > 0) {
            const size_t o = size_t(k - 1) * B;
            a.s_plant = tp.s + o * VSMPC_PLANT_STATE;
            a.fm = tp.fm + o * VSMPC_FM_SIZE;
            a.status = tp.status + o;
            a.log_bar = d_log_bar ? d_log_bar + o * VSMPC_ROLLOUT_LOG : nullptr;
        }
        HIP_TRY(launch_advance_adjoint(r->rd, a, s));
    }
    return VSMPC_OK;
}

// Both run entries.  `taped` keeps the tape of the run for vsmpc_rollout_backward, with direct launches (the captured graph has
// no room for the copies between its kernels); the plain run replays the captured ticks where it can and leaves no tape.
int run(vsmpc_rollout* r, int ticks, double* log, void* stream, bool taped) {
    if (r == nullptr || ticks < 0) return invalid_arg();
    if (!r->valid) return invalid_arg();   // never reset, or a previous run failed half-way: reset() first
    if (taped) {                           // what the backward sweep has no transpose of
        if (r->use_noise) return unsupported(NOISE_NO_ADJOINT);
        if (r->use_tree && !r->tree_adjoint)
            return unsupported("vsmpc_rollout_run_taped: no adjoint of the kinematic-tree plant (vsmpc_rollout_set_tree)");
        if (r->rd.jet_nn) return unsupported("vsmpc_rollout_run_taped: no adjoint of the jet plant option (vsmpc_rollout_set_jet_plant)");
        if (r->rd.traj_rpyd != nullptr && !r->attitude_adjoint)
            return unsupported("vsmpc_rollout_run_taped: no adjoint of an RPYDot track (vsmpc_rollout_set_attitude_tracks)");
        r->tape.ticks = 0;
    }
    if (ticks == 0) return VSMPC_OK;
    vsmpc_handle* h = r->h;
    ON_DEVICE(h->device);
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : r->own_stream.h;
    if (taped)
        if (const hipError_t e = grow_tape(r, ticks); e != hipSuccess)   // (the rollout itself is untouched: still runnable)
            return alloc_fail(e, "vsmpc_rollout_run_taped");
    if (const int rc = begin_run(r, ticks, log, s); rc != VSMPC_OK) return rc;
    r->tape.ticks = 0;                  // the tape describes the run in front of this one
    r->valid = 0;                       // until the whole run has completed: a failure below leaves the counters ahead
    int t = 0;
    if (!taped) {
        // the captured launches are of the other condensing form, or of the other kernel for this batch size
        if (r->graph_state != 0 && (r->graph_form != h->form || r->graph_small != (small_batch_kernel(h, r->batch) ? 1 : 0))) invalidate(r);
        if (ticks >= GRAPH_TICKS && r->graph_state == 0) build_tick_graph(r, s);
        if (r->graph_state == 1)
            for (; ticks - t >= GRAPH_TICKS; t += GRAPH_TICKS) HIP_TRY(hipGraphLaunch(r->gexec, s));
    }
    for (; t < ticks; ++t) HIP_TRY(enqueue_tick(r, s, taped ? t : -1));
    if (const int rc = end_run(r, ticks, log, s); rc != VSMPC_OK) return rc;
    if (taped) {
        r->tape.ticks = ticks;
        r->tape.tick_base = r->ticks_done - ticks;
        r->tape.kin = h->kin;
        r->tape.kin.constant_lambda = 0;   // as enqueue_tree flies it
    }
    return VSMPC_OK;
}

// what both backward entries refuse, in this order
int backward_refusal(const vsmpc_rollout* r, const double* log_bar, const double* state_bar) {
    if (r == nullptr) return invalid_arg();
    if (r->use_noise) return unsupported(NOISE_NO_ADJOINT);   // (it has no tape either: the caller learns why)
    if ((log_bar == nullptr && state_bar == nullptr) || r->tape.ticks == 0) return invalid_arg();
    if (!r->h->adjoint_record.on) return unsupported(BACKWARD_NEEDS_FLAG);
    return VSMPC_OK;
}
// dL/d(final state) of the sweep: the caller's rows, from where `kind` says they live, or zeros
hipError_t seed_sbar(vsmpc_rollout* r, const double* state_bar, hipMemcpyKind kind, hipStream_t s) {
    const size_t bytes = size_t(r->batch) * VSMPC_PLANT_STATE * sizeof(double);
    return state_bar != nullptr ? hipMemcpyAsync(r->tape.sbar, state_bar, bytes, kind, s) : hipMemsetAsync(r->tape.sbar, 0, bytes, s);
}

// what the `_full` entries refuse in front of that, by name: a rollout of these kinds has no tape either, but the caller asked
// for derivatives of a plant that has none
int full_refusal(const vsmpc_rollout* r) {
    if (r == nullptr) return invalid_arg();
    if (r->use_tree && !r->tree_adjoint)
        return unsupported("vsmpc_rollout_backward_full: no adjoint of the kinematic-tree plant (vsmpc_rollout_set_tree)");
    if (r->rd.jet_nn) return unsupported("vsmpc_rollout_backward_full: no adjoint of the jet plant option (vsmpc_rollout_set_jet_plant)");
    if (r->rd.traj_rpyd != nullptr && !r->attitude_adjoint)
        return unsupported("vsmpc_rollout_backward_full: no adjoint of an RPYDot track (vsmpc_rollout_set_attitude_tracks)");
    return VSMPC_OK;
}

// what the `_attitude` entries refuse in front of that
int attitude_refusal(const vsmpc_rollout* r, const char* why) {
    if (r == nullptr) return invalid_arg();
    if (!r->attitude_adjoint) return unsupported(why);
    return full_refusal(r);
}

// The device entries (gpar == gtraj == gatt == nullptr: the plain one) and the host entries, `what` the entry's name.  gatt rides
// the kernel's second instantiation: asking for it alone runs the `_full` sweep.
int backward_device(vsmpc_rollout* r, const double* d_log_bar, const double* d_state_bar, double* d_grad_state0, double* d_grad_cfg,
                    double* d_gpar, double* d_gtraj, double* d_gatt, int* d_flags, void* stream, const char* what) {
    if (const int rc = backward_refusal(r, d_log_bar, d_state_bar); rc != VSMPC_OK) return rc;
    ON_DEVICE(r->h->device);
    hipStream_t s = static_cast<hipStream_t>(stream);   // the caller's, the null stream too: its tensors are ordered on it
    const size_t B = size_t(r->batch);
    vsmpc_rollout::Tape& tp = r->tape;
    const bool att = d_gatt != nullptr, full = d_gpar != nullptr || d_gtraj != nullptr || att;
    if (full)
        if (const hipError_t e = grow_full(r); e != hipSuccess) return alloc_fail(e, what);
    if (att)
        if (const hipError_t e = grow_att(r); e != hipSuccess) return alloc_fail(e, what);
    HIP_TRY(seed_sbar(r, d_state_bar, hipMemcpyDeviceToDevice, s));
    if (const int rc = enqueue_sweep(r, d_log_bar, s, full, att); rc != VSMPC_OK) return rc;
    auto out = [&](void* dst, const void* src, size_t bytes) {
        return dst != nullptr ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s) : hipSuccess;
    };
    HIP_TRY(out(d_grad_state0, tp.sbar, B * VSMPC_PLANT_STATE * sizeof(double)));
    HIP_TRY(out(d_grad_cfg, tp.gcfg, B * VSMPC_GRAD_SIZE * sizeof(double)));
    HIP_TRY(out(d_flags, tp.flags, B * sizeof(int)));
    HIP_TRY(out(d_gpar, tp.gpar, B * VSMPC_PLANT_PARAMS * sizeof(double)));
    HIP_TRY(out(d_gtraj, tp.gtraj, B * traj_grad_size(r) * sizeof(double)));
    HIP_TRY(out(d_gatt, tp.gatt, B * att_grad_size(r) * sizeof(double)));
    return VSMPC_OK;
}

int backward_host(vsmpc_rollout* r, const double* log_bar, const double* state_bar, double* grad_state0, double* grad_cfg,
                  double* gpar, double* gtraj, double* gatt, int* flags, void* stream, const char* what) {
    if (const int rc = backward_refusal(r, log_bar, state_bar); rc != VSMPC_OK) return rc;
    ON_DEVICE(r->h->device);
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : r->own_stream.h;
    const size_t B = size_t(r->batch);
    vsmpc_rollout::Tape& tp = r->tape;
    const bool att = gatt != nullptr, full = gpar != nullptr || gtraj != nullptr || att;
    if (full)
        if (const hipError_t e = grow_full(r); e != hipSuccess) return alloc_fail(e, what);
    if (att)
        if (const hipError_t e = grow_att(r); e != hipSuccess) return alloc_fail(e, what);
    HIP_TRY(upload_rows(tp.log_bar.get(), log_bar, 0, size_t(tp.ticks), B * VSMPC_ROLLOUT_LOG, s));
    HIP_TRY(seed_sbar(r, state_bar, hipMemcpyHostToDevice, s));
    int rc = enqueue_sweep(r, log_bar ? tp.log_bar.get() : nullptr, s, full, att);
    hipError_t e = hipSuccess;
    if (rc == VSMPC_OK) e = download_rows(grad_state0, tp.sbar.get(), 0, B, VSMPC_PLANT_STATE, s);
    if (rc == VSMPC_OK && e == hipSuccess) e = download_rows(grad_cfg, tp.gcfg.get(), 0, B, VSMPC_GRAD_SIZE, s);
    if (rc == VSMPC_OK && e == hipSuccess) e = download_rows(flags, tp.flags.get(), 0, B, 1, s);
    if (rc == VSMPC_OK && e == hipSuccess) e = download_rows(gpar, tp.gpar.get(), 0, B, VSMPC_PLANT_PARAMS, s);
    if (rc == VSMPC_OK && e == hipSuccess) e = download_rows(gtraj, tp.gtraj.get(), 0, B, traj_grad_size(r), s);
    if (rc == VSMPC_OK && e == hipSuccess) e = download_rows(gatt, tp.gatt.get(), 0, B, att_grad_size(r), s);
    const hipError_t e2 = hipStreamSynchronize(s);   // nothing returns while copies from the caller's buffers are queued
    if (rc != VSMPC_OK) return rc;
    if (e != hipSuccess || e2 != hipSuccess) return hip_fail(e != hipSuccess ? e : e2, what);
    return VSMPC_OK;
}

}  // namespace

extern "C" {

int vsmpc_rollout_run(vsmpc_rollout* r, int ticks, double* log, void* stream) { return run(r, ticks, log, stream, false); }

int vsmpc_rollout_run_taped(vsmpc_rollout* r, int ticks, double* log, void* stream) { return run(r, ticks, log, stream, true); }

int vsmpc_rollout_backward_device(vsmpc_rollout* r, const double* d_log_bar, const double* d_state_bar, double* d_grad_state0,
                                  double* d_grad_cfg, int* d_flags, void* stream) {
    return backward_device(r, d_log_bar, d_state_bar, d_grad_state0, d_grad_cfg, nullptr, nullptr, nullptr, d_flags, stream,
                           "vsmpc_rollout_backward_device");
}

int vsmpc_rollout_backward(vsmpc_rollout* r, const double* log_bar, const double* state_bar, double* grad_state0,
                           double* grad_cfg, int* flags, void* stream) {
    return backward_host(r, log_bar, state_bar, grad_state0, grad_cfg, nullptr, nullptr, nullptr, flags, stream, "vsmpc_rollout_backward");
}

int vsmpc_rollout_backward_full_device(vsmpc_rollout* r, const double* d_log_bar, const double* d_state_bar, double* d_grad_state0,
                                       double* d_grad_cfg, double* d_grad_params, double* d_grad_traj, int* d_flags, void* stream) {
    if (const int rc = full_refusal(r); rc != VSMPC_OK) return rc;
    return backward_device(r, d_log_bar, d_state_bar, d_grad_state0, d_grad_cfg, d_grad_params, d_grad_traj, nullptr, d_flags, stream,
                           "vsmpc_rollout_backward_full_device");
}

int vsmpc_rollout_backward_full(vsmpc_rollout* r, const double* log_bar, const double* state_bar, double* grad_state0,
                                double* grad_cfg, double* grad_params, double* grad_traj, int* flags, void* stream) {
    if (const int rc = full_refusal(r); rc != VSMPC_OK) return rc;
    return backward_host(r, log_bar, state_bar, grad_state0, grad_cfg, grad_params, grad_traj, nullptr, flags, stream,
                         "vsmpc_rollout_backward_full");
}

int vsmpc_rollout_backward_attitude_device(vsmpc_rollout* r, const double* d_log_bar, const double* d_state_bar,
                                           double* d_grad_state0, double* d_grad_cfg, double* d_grad_params, double* d_grad_traj,
                                           double* d_grad_att, int* d_flags, void* stream) {
    if (const int rc = attitude_refusal(r, "vsmpc_rollout_backward_attitude_device needs attitude tracks set with "
                                           "VSMPC_ATTITUDE_ADJOINT (vsmpc_rollout_set_attitude_tracks_ex)"); rc != VSMPC_OK)
        return rc;
    return backward_device(r, d_log_bar, d_state_bar, d_grad_state0, d_grad_cfg, d_grad_params, d_grad_traj, d_grad_att, d_flags,
                           stream, "vsmpc_rollout_backward_attitude_device");
}

int vsmpc_rollout_backward_attitude(vsmpc_rollout* r, const double* log_bar, const double* state_bar, double* grad_state0,
                                    double* grad_cfg, double* grad_params, double* grad_traj, double* grad_att, int* flags,
                                    void* stream) {
    if (const int rc = attitude_refusal(r, "vsmpc_rollout_backward_attitude needs attitude tracks set with VSMPC_ATTITUDE_ADJOINT "
                                           "(vsmpc_rollout_set_attitude_tracks_ex)"); rc != VSMPC_OK)
        return rc;
    return backward_host(r, log_bar, state_bar, grad_state0, grad_cfg, grad_params, grad_traj, grad_att, flags, stream,
                         "vsmpc_rollout_backward_attitude");
}

int vsmpc_rollout_att_grad_size(const vsmpc_rollout* r) { return r == nullptr ? invalid_arg() : int(att_grad_size(r)); }

int vsmpc_rollout_traj_grad_size(const vsmpc_rollout* r) { return r == nullptr ? invalid_arg() : int(traj_grad_size(r)); }

int vsmpc_rollout_set_trajectories(vsmpc_rollout* r, const double* traj_pos, const double* traj_vel, const double* traj_alpha) {
    if (r == nullptr) return invalid_arg();
    ON_DEVICE(r->h->device);
    // the record of the next tick and the tape were built from the old tracks; the captured ticks read the same buffers
    r->valid = 0;
    r->tape.ticks = 0;
    HIP_TRY(hipDeviceSynchronize());   // a sweep a `_device` entry enqueued may still read them
    const size_t nt = size_t(r->rd.n_traj) * 3 * sizeof(double);
    if (traj_pos != nullptr) HIP_TRY(hipMemcpy(r->d_tpos, traj_pos, nt, hipMemcpyHostToDevice));
    if (traj_vel != nullptr) HIP_TRY(hipMemcpy(r->d_tvel, traj_vel, nt, hipMemcpyHostToDevice));
    if (traj_alpha != nullptr) HIP_TRY(hipMemcpy(r->d_talpha, traj_alpha, size_t(r->rd.n_alpha) * sizeof(double), hipMemcpyHostToDevice));
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
