// C-ABI of include/vsmpc.h, the hot entries: solve (device and host pointers, per-instance tunables), sensitivities,
// certificates and the one-submission tick, with their host<->device staging.
#include "vsmpc_host.hpp"

using namespace vsmpc;

hipError_t vsmpc::solve_launch(const vsmpc_handle* h, const double* d_in, int batch, double* d_x, double* d_fm, int* d_status,
                               int* d_iters, size_t first, hipStream_t s, const double* d_tun) {
    if (d_tun != nullptr) {
        if (h->runtime)
            return launch_solve_runtime_tuned(h->rt, h->dev, d_in, d_tun, batch, h->d_ws + first * size_t(h->rt.ws_doubles), d_x,
                                              d_fm, d_status, d_iters, s);
        return launch_solve_tuned(h->variant, h->form, h->dev, d_in, d_tun, batch, d_x, d_fm, d_status, d_iters, s);
    }
    if (h->runtime)
        return launch_solve_runtime(h->rt, h->dev, d_in, batch, h->d_ws + first * size_t(h->rt.ws_doubles), d_x, d_fm,
                                    d_status, d_iters, s);
    if (small_batch_kernel(h, batch))
        return launch_solve_small(h->variant, h->dev, d_in, batch, d_x, d_fm, d_status, d_iters, nullptr, s);
    return launch_solve(h->variant, h->form, h->dev, d_in, batch, d_x, d_fm, d_status, d_iters, nullptr, nullptr, nullptr, s);
}

namespace {

// carve-up of the mapped staging buffer (host or device view)
struct Stage {
    double* in; double* x; double* fm; int* st; int* it; double* kin; double* tun;
};
Stage stage_view(const vsmpc_handle* h, double* base) {
    Stage v;
    v.in = base;
    v.x = v.in + size_t(ZC_MAX) * h->n_in;
    v.fm = v.x + size_t(ZC_MAX) * h->n_var;
    v.st = reinterpret_cast<int*>(v.fm + size_t(ZC_MAX) * VSMPC_FM_SIZE);
    v.it = v.st + ZC_MAX;
    v.kin = v.fm + size_t(ZC_MAX) * (VSMPC_FM_SIZE + 1);
    v.tun = v.kin + size_t(ZC_MAX) * VSMPC_KIN_SIZE;   // (every block before it is a multiple of ZC_MAX doubles: 64-byte aligned)
    return v;
}

// the results of the first B instances out of the host view of the mapped staging buffer (x, first_move, iters: when wanted)
void stage_results(const vsmpc_handle* h, const Stage& hv, size_t B, double* x, double* first_move, int* status, int* iters) {
    if (x) memcpy(x, hv.x, B * h->n_var * sizeof(double));
    if (first_move) memcpy(first_move, hv.fm, B * VSMPC_FM_SIZE * sizeof(double));
    memcpy(status, hv.st, B * sizeof(int));
    if (iters) memcpy(iters, hv.it, B * sizeof(int));
}

// the results of instances first .. first + n - 1 from the handle's staging, on `s`; stops enqueuing at the first failure
hipError_t download_results(const vsmpc_handle* h, size_t first, size_t n, double* x, double* first_move, int* status,
                            int* iters, hipStream_t s) {
    hipError_t e = download_rows(x, h->d_x, first, n, h->n_var, s);
    if (e == hipSuccess) e = download_rows(first_move, h->d_fm, first, n, VSMPC_FM_SIZE, s);
    if (e == hipSuccess) e = download_rows(status, h->d_status, first, n, 1, s);
    if (e == hipSuccess) e = download_rows(iters, h->d_iters, first, n, 1, s);
    return e;
}

// vsmpc_solve_batch (tun == nullptr) and vsmpc_solve_batch_tuned (tun: host rows, one per instance, staged like the records)
int solve_batch_host(vsmpc_handle* h, const double* in, const double* tun, int batch, double* x, double* first_move,
                     int* status, int* iters, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    ON_DEVICE(h->device);
    const size_t B = size_t(batch);
    if (batch <= ZC_MAX) {
        // zero-copy path: the kernel reads the records from and writes the results to pinned host memory
        const Stage hv = stage_view(h, h->h_stage), dv = stage_view(h, h->d_stage);   // the same carve-up on both views
        memcpy(hv.in, in, B * h->n_in * sizeof(double));
        if (tun) memcpy(hv.tun, tun, B * VSMPC_TUNE_SIZE * sizeof(double));
        HIP_TRY(solve_launch(h, dv.in, batch, dv.x, dv.fm, dv.st, dv.it, 0, s, tun ? dv.tun : nullptr));
        HIP_TRY(hipStreamSynchronize(s));
        stage_results(h, hv, B, x, first_move, status, iters);
        return VSMPC_OK;
    }
    // Pinned output buffers (hipHostMalloc / vsmpc_alloc_host) are written by the kernel itself over PCIe (16 B per lane
    // posted writes): no device-to-host copies, no copy launches (batch 4096, all outputs: 1.01 ms against 1.11 ms with
    // one copy of the trajectories behind the last chunk; profiles/r02_v11_hostpath.json).
    auto device_view = [](const void* host) -> void* {
        if (host == nullptr) return nullptr;
        hipPointerAttribute_t at;
        if (hipPointerGetAttributes(&at, host) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        return at.type == hipMemoryTypeHost ? at.devicePointer : nullptr;
    };
    double* zx = static_cast<double*>(device_view(x));
    double* zfm = static_cast<double*>(device_view(first_move));
    int* zst = static_cast<int*>(device_view(status));
    int* zit = static_cast<int*>(device_view(iters));
    const bool direct = (x == nullptr || zx) && (first_move == nullptr || zfm) && zst && (iters == nullptr || zit);
    // chunks of PIPE_CHUNK instances rotate over the handle's streams: upload(k+1) | solve(k) | download(k-1)
    // overlap when the caller's buffers are pinned (hipHostMalloc / vsmpc_alloc_host); with pageable buffers the
    // runtime stages the copies itself and the chunks still overlap with the kernels
    HIP_TRY(hipEventRecord(h->pipe_start, s));                 // work queued on the caller's stream comes first
    const int nstreams = std::min(PIPE_STREAMS, (batch + PIPE_CHUNK - 1) / PIPE_CHUNK);
    for (int i = 0; i < nstreams; ++i) HIP_TRY(hipStreamWaitEvent(h->pipe[i], h->pipe_start, 0));
    // A failure in the middle leaves earlier chunks queued: kernels that write straight into the caller's pinned buffers,
    // copies into h->d_in.  Nothing returns before every pipe stream that was used has drained.
    hipError_t err = hipSuccess;
    auto ok = [&](hipError_t e) { if (e != hipSuccess && err == hipSuccess) err = e; return err == hipSuccess; };
    int k = 0;
    for (int first = 0; first < batch && err == hipSuccess; first += PIPE_CHUNK, ++k) {
        const int n = std::min(PIPE_CHUNK, batch - first);
        const size_t o = size_t(first), N = size_t(n);
        hipStream_t ps = h->pipe[k % nstreams];
        if (!ok(upload_rows(h->d_in, in, o, N, h->n_in, ps))) break;
        const double* dt = tun ? h->d_tun + o * VSMPC_TUNE_SIZE : nullptr;
        if (!ok(upload_rows(h->d_tun, tun, o, N, VSMPC_TUNE_SIZE, ps))) break;
        if (direct) {
            ok(solve_launch(h, h->d_in + o * h->n_in, n, x ? zx + o * h->n_var : nullptr,
                            first_move ? zfm + o * VSMPC_FM_SIZE : nullptr, zst + o, iters ? zit + o : nullptr, o, ps, dt));
            continue;
        }
        if (!ok(solve_launch(h, h->d_in + o * h->n_in, n, h->d_x + o * h->n_var, h->d_fm + o * VSMPC_FM_SIZE, h->d_status + o,
                             h->d_iters + o, o, ps, dt))) break;
        ok(download_results(h, o, N, x, first_move, status, iters, ps));
    }
    for (int i = 0; i < nstreams; ++i) {
        if (err == hipSuccess && ok(hipEventRecord(h->pipe_done[i], h->pipe[i])))
            ok(hipStreamWaitEvent(s, h->pipe_done[i], 0));   // the caller's stream continues after all of them
    }
    for (int i = 0; i < nstreams; ++i) {
        const hipError_t e = hipStreamSynchronize(h->pipe[i]);
        if (err == hipSuccess) err = e;
    }
    HIP_TRY(err);
    return VSMPC_OK;
}

}  // namespace

extern "C" {

int vsmpc_solve_batch_device(vsmpc_handle* h, const double* d_in, int batch, double* d_x, double* d_first_move,
                             int* d_status, int* d_iters, void* stream) {
    if (h == nullptr || d_in == nullptr || d_status == nullptr || batch < 0) return invalid_arg();
    if (batch > h->max_batch) return VSMPC_ERR_BATCH_TOO_LARGE;
    if (batch == 0) return VSMPC_OK;
    ON_DEVICE(h->device);   // an enqueue-only entry must not change the caller's current device either
    HIP_TRY(solve_launch(h, d_in, batch, d_x, d_first_move, d_status, d_iters, 0, static_cast<hipStream_t>(stream)));
    return VSMPC_OK;
}

int vsmpc_solve_batch(vsmpc_handle* h, const double* in, int batch, double* x, double* first_move, int* status,
                      int* iters, void* stream) {
    if (h == nullptr || in == nullptr || status == nullptr || batch < 0) return invalid_arg();
    if (batch > h->max_batch) return VSMPC_ERR_BATCH_TOO_LARGE;
    if (batch == 0) return VSMPC_OK;
    return solve_batch_host(h, in, nullptr, batch, x, first_move, status, iters, stream);
}

int vsmpc_solve_batch_tuned_device(vsmpc_handle* h, const double* d_in, const double* d_tunables, int batch, double* d_x,
                                   double* d_first_move, int* d_status, int* d_iters, void* stream) {
    if (h == nullptr || d_in == nullptr || d_tunables == nullptr || d_status == nullptr || batch < 0) return invalid_arg();
    if ((reinterpret_cast<size_t>(d_tunables) & 15) != 0) return invalid_arg();   // the kernels load 16 bytes per lane
    if (batch > h->max_batch) return VSMPC_ERR_BATCH_TOO_LARGE;
    if (batch == 0) return VSMPC_OK;
    ON_DEVICE(h->device);
    HIP_TRY(solve_launch(h, d_in, batch, d_x, d_first_move, d_status, d_iters, 0, static_cast<hipStream_t>(stream), d_tunables));
    return VSMPC_OK;
}

int vsmpc_solve_batch_tuned(vsmpc_handle* h, const double* in, const double* tunables, int batch, double* x,
                            double* first_move, int* status, int* iters, void* stream) {
    if (h == nullptr || in == nullptr || tunables == nullptr || status == nullptr || batch < 0) return invalid_arg();
    if (!h->tunables) return unsupported();
    if (batch > h->max_batch) return VSMPC_ERR_BATCH_TOO_LARGE;
    if (batch == 0) return VSMPC_OK;
    return solve_batch_host(h, in, tunables, batch, x, first_move, status, iters, stream);
}

int vsmpc_sensitivity_batch_device(vsmpc_handle* h, const double* d_in, int batch, double* d_x, double* d_first_move,
                                   int* d_status, int* d_iters, double* d_dx_dx0, double* d_dfm_dx0, int* d_active,
                                   int* d_sens_flags, void* stream) {
    if (h == nullptr || d_in == nullptr || d_status == nullptr || batch < 0) return invalid_arg();
    if (!h->sens) return unsupported();
    if (batch > h->max_batch) return VSMPC_ERR_BATCH_TOO_LARGE;
    if (batch == 0) return VSMPC_OK;
    ON_DEVICE(h->device);
    HIP_TRY(launch_sensitivity_runtime(h->rts, h->dev, d_in, batch, h->d_sws, d_x, d_first_move, d_status, d_iters, d_dx_dx0,
                                       d_dfm_dx0, d_active, d_sens_flags, static_cast<hipStream_t>(stream)));
    return VSMPC_OK;
}

int vsmpc_sensitivity_batch(vsmpc_handle* h, const double* in, int batch, double* x, double* first_move, int* status,
                            int* iters, double* dx_dx0, double* dfm_dx0, int* active, int* sens_flags, void* stream) {
    if (h == nullptr || in == nullptr || status == nullptr || batch < 0) return invalid_arg();
    if (!h->sens) return unsupported();
    if (batch > h->max_batch) return VSMPC_ERR_BATCH_TOO_LARGE;
    if (batch == 0) return VSMPC_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    ON_DEVICE(h->device);
    const size_t NV = size_t(h->rts.nv), J = SENS_NPAR, FM = VSMPC_FM_SIZE;
    // chunks of SENS_CHUNK instances in stream order: the staging of one chunk is read back before the next overwrites it
    hipError_t err = hipSuccess;
    auto ok = [&](hipError_t e) { if (e != hipSuccess && err == hipSuccess) err = e; return err == hipSuccess; };
    for (int first = 0; first < batch && err == hipSuccess; first += SENS_CHUNK) {
        const int n = std::min(SENS_CHUNK, batch - first);
        const size_t o = size_t(first), N = size_t(n);
        if (!ok(upload_rows(h->d_in, in, o, N, h->n_in, s))) break;
        if (!ok(launch_sensitivity_runtime(h->rts, h->dev, h->d_in + o * h->n_in, n, h->d_sws + o * size_t(h->rts.ws_doubles),
                                           x ? h->d_x + o * h->n_var : nullptr, first_move ? h->d_fm + o * FM : nullptr,
                                           h->d_status + o, iters ? h->d_iters + o : nullptr, dx_dx0 ? h->d_sdx : nullptr,
                                           dfm_dx0 ? h->d_sdfm : nullptr, active ? h->d_sact : nullptr,
                                           sens_flags ? h->d_sflags : nullptr, s)))
            break;
        ok(download_results(h, o, N, x, first_move, status, iters, s));
        if (dx_dx0)
            ok(hipMemcpyAsync(dx_dx0 + o * h->n_var * J, h->d_sdx, N * h->n_var * J * sizeof(double), hipMemcpyDeviceToHost, s));
        if (dfm_dx0) ok(hipMemcpyAsync(dfm_dx0 + o * FM * J, h->d_sdfm, N * FM * J * sizeof(double), hipMemcpyDeviceToHost, s));
        if (active) ok(hipMemcpyAsync(active + o * NV, h->d_sact, N * NV * sizeof(int), hipMemcpyDeviceToHost, s));
        if (sens_flags) ok(hipMemcpyAsync(sens_flags + o, h->d_sflags, N * sizeof(int), hipMemcpyDeviceToHost, s));
    }
    const hipError_t e = hipStreamSynchronize(s);   // nothing returns while copies into the caller's buffers are queued
    if (err == hipSuccess) err = e;
    if (err != hipSuccess) return hip_fail(err, "vsmpc_sensitivity_batch");
    return VSMPC_OK;
}

// Adjoint of the solve (include/vsmpc.h): adjoint_kernel_rt, or adjoint_kernel_rt_tuned with rows of tunables, on the
// workspace of the runtime handle or the one VSMPC_CREATE_ADJOINT allocated
static double* adjoint_workspace(const vsmpc_handle* h) { return h->runtime ? h->d_ws.get() : h->d_aws.get(); }
static const char* const ADJOINT_NEEDS_FLAG =
    "vsmpc_adjoint_batch needs a handle created with VSMPC_CREATE_ADJOINT (vsmpc_create_ex)";

int vsmpc_adjoint_batch_device(vsmpc_handle* h, const double* d_in, const double* d_tunables, const double* d_xbar,
                               const double* d_fmbar, int batch, double* d_x, double* d_first_move, int* d_status,
                               int* d_iters, double* d_grad_x0, double* d_grad_cfg, int* d_active, int* d_adj_flags,
                               void* stream) {
    if (h == nullptr || d_in == nullptr || d_xbar == nullptr || d_status == nullptr || batch < 0) return invalid_arg();
    if ((reinterpret_cast<size_t>(d_tunables) & 15) != 0) return invalid_arg();   // the kernel loads 16 bytes per lane
    if (!h->adjoint) return unsupported(ADJOINT_NEEDS_FLAG);
    if (batch > h->max_batch) return VSMPC_ERR_BATCH_TOO_LARGE;
    if (batch == 0) return VSMPC_OK;
    ON_DEVICE(h->device);
    HIP_TRY(launch_adjoint_runtime(h->rta, h->dev, d_in, d_tunables, batch, adjoint_workspace(h), d_x, d_first_move, d_status,
                                   d_iters, d_xbar, d_fmbar, d_grad_x0, d_grad_cfg, d_active, d_adj_flags,
                                   static_cast<hipStream_t>(stream)));
    return VSMPC_OK;
}

// the host-pointer entries of the adjoint and of the record adjoint (`record`: adjoint_record_kernel_rt, which also writes
// grad_in and grad_model): chunks of ADJ_CHUNK instances in stream order, the staging of one chunk is read back before the
// next overwrites it
static int adjoint_batch_host(vsmpc_handle* h, bool record, const double* in, const double* tunables, const double* xbar,
                              const double* fmbar, int batch, double* x, double* first_move, int* status, int* iters,
                              double* grad_x0, double* grad_cfg, int* active, int* adj_flags, double* grad_in,
                              double* grad_model, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    ON_DEVICE(h->device);
    const RtDims& d = record ? h->rtr : h->rta;
    const size_t NV = size_t(d.nv), FM = VSMPC_FM_SIZE, T = VSMPC_TUNE_SIZE, G = VSMPC_GRAD_SIZE, GM = VSMPC_GRAD_MODEL_SIZE;
    hipError_t err = hipSuccess;
    auto ok = [&](hipError_t e) { if (e != hipSuccess && err == hipSuccess) err = e; return err == hipSuccess; };
    for (int first = 0; first < batch && err == hipSuccess; first += ADJ_CHUNK) {
        const int n = std::min(ADJ_CHUNK, batch - first);
        const size_t o = size_t(first), N = size_t(n);
        if (!ok(upload_rows(h->d_in, in, o, N, h->n_in, s))) break;
        if (!ok(hipMemcpyAsync(h->d_axbar, xbar + o * h->n_var, N * h->n_var * sizeof(double), hipMemcpyHostToDevice, s))) break;
        if (fmbar && !ok(hipMemcpyAsync(h->d_afmbar, fmbar + o * FM, N * FM * sizeof(double), hipMemcpyHostToDevice, s))) break;
        if (tunables && !ok(hipMemcpyAsync(h->d_atun, tunables + o * T, N * T * sizeof(double), hipMemcpyHostToDevice, s))) break;
        const double* d_in = h->d_in + o * h->n_in;
        const double* d_tun = tunables ? h->d_atun.get() : nullptr;
        double* d_ws = adjoint_workspace(h) + o * size_t(d.ws_doubles);
        double* d_x = x ? h->d_x + o * h->n_var : nullptr;
        double* d_fm = first_move ? h->d_fm + o * FM : nullptr;
        int* d_it = iters ? h->d_iters + o : nullptr;
        const double* d_fmbar = fmbar ? h->d_afmbar.get() : nullptr;
        double* d_gx0 = grad_x0 ? h->d_agx0.get() : nullptr;
        double* d_gcfg = grad_cfg ? h->d_agcfg.get() : nullptr;
        int* d_act = active ? h->d_aact.get() : nullptr;
        int* d_fl = adj_flags ? h->d_aflags.get() : nullptr;
        if (!ok(record ? launch_adjoint_record_runtime(d, h->dev, d_in, d_tun, n, d_ws, d_x, d_fm, h->d_status + o, d_it, h->d_axbar,
                                                       d_fmbar, d_gx0, d_gcfg, d_act, d_fl, grad_in ? h->d_agin.get() : nullptr,
                                                       grad_model ? h->d_agmodel.get() : nullptr, s)
                       : launch_adjoint_runtime(d, h->dev, d_in, d_tun, n, d_ws, d_x, d_fm, h->d_status + o, d_it, h->d_axbar,
                                                d_fmbar, d_gx0, d_gcfg, d_act, d_fl, s)))
            break;
        ok(download_results(h, o, N, x, first_move, status, iters, s));
        if (grad_x0) ok(hipMemcpyAsync(grad_x0 + o * NX, h->d_agx0, N * NX * sizeof(double), hipMemcpyDeviceToHost, s));
        if (grad_cfg) ok(hipMemcpyAsync(grad_cfg + o * G, h->d_agcfg, N * G * sizeof(double), hipMemcpyDeviceToHost, s));
        if (active) ok(hipMemcpyAsync(active + o * NV, h->d_aact, N * NV * sizeof(int), hipMemcpyDeviceToHost, s));
        if (adj_flags) ok(hipMemcpyAsync(adj_flags + o, h->d_aflags, N * sizeof(int), hipMemcpyDeviceToHost, s));
        if (record && grad_in)
            ok(hipMemcpyAsync(grad_in + o * h->n_in, h->d_agin, N * h->n_in * sizeof(double), hipMemcpyDeviceToHost, s));
        if (record && grad_model)
            ok(hipMemcpyAsync(grad_model + o * GM, h->d_agmodel, N * GM * sizeof(double), hipMemcpyDeviceToHost, s));
    }
    const hipError_t e = hipStreamSynchronize(s);   // nothing returns while copies into the caller's buffers are queued
    if (err == hipSuccess) err = e;
    if (err != hipSuccess) return hip_fail(err, record ? "vsmpc_adjoint_record_batch" : "vsmpc_adjoint_batch");
    return VSMPC_OK;
}

int vsmpc_adjoint_batch(vsmpc_handle* h, const double* in, const double* tunables, const double* xbar, const double* fmbar,
                        int batch, double* x, double* first_move, int* status, int* iters, double* grad_x0, double* grad_cfg,
                        int* active, int* adj_flags, void* stream) {
    if (h == nullptr || in == nullptr || xbar == nullptr || status == nullptr || batch < 0) return invalid_arg();
    if (!h->adjoint) return unsupported(ADJOINT_NEEDS_FLAG);
    if (batch > h->max_batch) return VSMPC_ERR_BATCH_TOO_LARGE;
    if (batch == 0) return VSMPC_OK;
    return adjoint_batch_host(h, false, in, tunables, xbar, fmbar, batch, x, first_move, status, iters, grad_x0, grad_cfg, active,
                              adj_flags, nullptr, nullptr, stream);
}

// Adjoint of the record (include/vsmpc.h): adjoint_record_kernel_rt[_tuned] on the adjoint entry's workspace and staging,
// with the staging VSMPC_CREATE_ADJOINT_RECORD allocated for the two further outputs
static const char* const ADJOINT_RECORD_NEEDS_FLAG =
    "vsmpc_adjoint_record_batch needs a handle created with VSMPC_CREATE_ADJOINT_RECORD (vsmpc_create_ex)";

int vsmpc_adjoint_record_batch_device(vsmpc_handle* h, const double* d_in, const double* d_tunables, const double* d_xbar,
                                      const double* d_fmbar, int batch, double* d_x, double* d_first_move, int* d_status,
                                      int* d_iters, double* d_grad_x0, double* d_grad_cfg, int* d_active, int* d_adj_flags,
                                      double* d_grad_in, double* d_grad_model, void* stream) {
    if (h == nullptr || d_in == nullptr || d_xbar == nullptr || d_status == nullptr || batch < 0) return invalid_arg();
    if ((reinterpret_cast<size_t>(d_tunables) & 15) != 0) return invalid_arg();   // the kernel loads 16 bytes per lane
    if (!h->adjoint_record) return unsupported(ADJOINT_RECORD_NEEDS_FLAG);
    if (batch > h->max_batch) return VSMPC_ERR_BATCH_TOO_LARGE;
    if (batch == 0) return VSMPC_OK;
    ON_DEVICE(h->device);
    HIP_TRY(launch_adjoint_record_runtime(h->rtr, h->dev, d_in, d_tunables, batch, adjoint_workspace(h), d_x, d_first_move,
                                          d_status, d_iters, d_xbar, d_fmbar, d_grad_x0, d_grad_cfg, d_active, d_adj_flags,
                                          d_grad_in, d_grad_model, static_cast<hipStream_t>(stream)));
    return VSMPC_OK;
}

int vsmpc_adjoint_record_batch(vsmpc_handle* h, const double* in, const double* tunables, const double* xbar,
                               const double* fmbar, int batch, double* x, double* first_move, int* status, int* iters,
                               double* grad_x0, double* grad_cfg, int* active, int* adj_flags, double* grad_in,
                               double* grad_model, void* stream) {
    if (h == nullptr || in == nullptr || xbar == nullptr || status == nullptr || batch < 0) return invalid_arg();
    if (!h->adjoint_record) return unsupported(ADJOINT_RECORD_NEEDS_FLAG);
    if (batch > h->max_batch) return VSMPC_ERR_BATCH_TOO_LARGE;
    if (batch == 0) return VSMPC_OK;
    return adjoint_batch_host(h, true, in, tunables, xbar, fmbar, batch, x, first_move, status, iters, grad_x0, grad_cfg, active,
                              adj_flags, grad_in, grad_model, stream);
}

// Duals and KKT certificate of given primals: certify_kernel restates the oracle's solve_exact (the duals, OSQP's sign:
// y > 0 upper-active, y < 0 lower-active) and its kkt_certificate on the QP of assemble_dense (module cited in include/vsmpc.h)
int vsmpc_certify_batch_device(vsmpc_handle* h, const double* d_in, const double* d_x, const double* d_tunables, int batch,
                               double* d_y, double* d_cert, void* stream) {
    if (h == nullptr || d_in == nullptr || d_x == nullptr || d_cert == nullptr || batch < 0) return invalid_arg();
    // the kernel loads and stores 16 bytes per lane
    if (((reinterpret_cast<size_t>(d_in) | reinterpret_cast<size_t>(d_x) | reinterpret_cast<size_t>(d_tunables) |
          reinterpret_cast<size_t>(d_y)) & 15) != 0 || (reinterpret_cast<size_t>(d_cert) & 7) != 0)
        return invalid_arg();
    if (batch > h->max_batch) return VSMPC_ERR_BATCH_TOO_LARGE;
    if (batch == 0) return VSMPC_OK;
    ON_DEVICE(h->device);
    HIP_TRY(launch_certify(h->rt, h->dev, d_in, d_x, d_tunables, batch, d_y, d_cert, static_cast<hipStream_t>(stream)));
    return VSMPC_OK;
}

int vsmpc_certify_batch(vsmpc_handle* h, const double* in, const double* x, const double* tunables, int batch, double* y,
                        double* cert) {
    if (h == nullptr || in == nullptr || x == nullptr || cert == nullptr || batch < 0) return invalid_arg();
    if (!h->certify)
        return unsupported("vsmpc_certify_batch needs a handle created with VSMPC_CREATE_CERTIFY (vsmpc_create_ex)");
    if (batch > h->max_batch) return VSMPC_ERR_BATCH_TOO_LARGE;
    if (batch == 0) return VSMPC_OK;
    ON_DEVICE(h->device);
    const size_t B = size_t(batch);
    HIP_TRY(hipMemcpy(h->d_in, in, B * h->n_in * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->d_cx, x, B * h->n_var * sizeof(double), hipMemcpyHostToDevice));
    if (tunables) HIP_TRY(hipMemcpy(h->d_ctun, tunables, B * VSMPC_TUNE_SIZE * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(launch_certify(h->rt, h->dev, h->d_in, h->d_cx, tunables ? h->d_ctun : nullptr, batch,
                           y ? h->d_cy : nullptr, h->d_ccert, nullptr));
    // (copies on the null stream: ordered behind the launch, and complete on return)
    if (y) HIP_TRY(hipMemcpy(y, h->d_cy, B * h->n_con * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(cert, h->d_ccert, B * VSMPC_CERT_SIZE * sizeof(double), hipMemcpyDeviceToHost));
    return VSMPC_OK;
}

// One tick of the reference's drop-in surface in ONE submission: kinematics terms -> record -> solve, one synchronisation.
int vsmpc_tick(vsmpc_handle* h, const double* kin, double* in, int batch, double* x, double* first_move, int* status,
               int* iters, void* stream) {
    if (h == nullptr || kin == nullptr || in == nullptr || status == nullptr || batch < 0) return invalid_arg();
    if (batch > h->max_batch) return VSMPC_ERR_BATCH_TOO_LARGE;
    if (batch == 0) return VSMPC_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    ON_DEVICE(h->device);
    const size_t B = size_t(batch);
    if (batch <= ZC_MAX) {
        // the kinematics kernel reads the raw Robot quantities from, and writes LLIN | LANG | INERTIA into, the mapped
        // staging buffer; the solve kernel (next in stream order) reads the completed record from there
        const Stage hv = stage_view(h, h->h_stage), dv = stage_view(h, h->d_stage);
        memcpy(hv.kin, kin, B * VSMPC_KIN_SIZE * sizeof(double));
        memcpy(hv.in, in, B * h->n_in * sizeof(double));
        HIP_TRY(launch_kinematics_patch(dv.kin, batch, dv.in, h->n_in, h->kin, s));
        HIP_TRY(solve_launch(h, dv.in, batch, dv.x, dv.fm, dv.st, dv.it, 0, s));
        HIP_TRY(hipStreamSynchronize(s));
        for (size_t b = 0; b < B; ++b)   // hand the completed fields back (the caller's record is the record of the tick)
            memcpy(in + b * h->n_in + VSMPC_IN_LLIN, hv.in + b * h->n_in + VSMPC_IN_LLIN, (24 + 24 + 9) * sizeof(double));
        stage_results(h, hv, B, x, first_move, status, iters);
        return VSMPC_OK;
    }
    // as in solve_batch_host: the first error is kept, nothing more is enqueued, nothing returns with a copy still queued
    hipError_t err = upload_rows(h->d_kin, kin, 0, B, VSMPC_KIN_SIZE, s);
    if (err == hipSuccess) err = upload_rows(h->d_in, in, 0, B, h->n_in, s);
    if (err == hipSuccess) err = launch_kinematics_patch(h->d_kin, batch, h->d_in, h->n_in, h->kin, s);
    if (err == hipSuccess) err = solve_launch(h, h->d_in, batch, h->d_x, h->d_fm, h->d_status, h->d_iters, 0, s);
    if (err == hipSuccess) err = download_rows(in, h->d_in, 0, B, h->n_in, s);
    if (err == hipSuccess) err = download_results(h, 0, B, x, first_move, status, iters, s);
    const hipError_t e = hipStreamSynchronize(s);
    if (err == hipSuccess) err = e;
    if (err != hipSuccess) return hip_fail(err, "vsmpc_tick");
    return VSMPC_OK;
}

}  // extern "C"
