// C-ABI of include/vsmpc.h, the hot entries: solve (device and host pointers, per-instance tunables), sensitivities,
// adjoints, certificates and the one-submission tick, with their host<->device staging.  The runtime-sized kernels are
// launched through launch_runtime over an RtLaunch (vsmpc_launch.hpp); their chunked host-pointer entries are chunked_host
// and a table of staged rows each.
#include "vsmpc_host.hpp"

using namespace vsmpc;

// the fields of an RtLaunch that every entry of the runtime family has (the workspace and the kind's own are the caller's)
static RtLaunch solve_args(const double* d_in, const double* d_tun, double* d_x, double* d_fm, int* d_status, int* d_iters) {
    RtLaunch a;
    a.in = d_in; a.tun = d_tun;
    a.x = d_x; a.fm = d_fm; a.status = d_status; a.iters = d_iters;
    return a;
}

hipError_t vsmpc::solve_launch(const vsmpc_handle* h, const double* d_in, int batch, double* d_x, double* d_fm, int* d_status,
                               int* d_iters, size_t first, hipStream_t s, const double* d_tun) {
    if (h->runtime) {
        RtLaunch a = solve_args(d_in, d_tun, d_x, d_fm, d_status, d_iters);
        a.ws = h->d_ws + first * size_t(h->rt.ws_doubles);
        return launch_runtime(RT_SOLVE, h->rt, h->dev, batch, a, s);
    }
    if (d_tun != nullptr)
        return launch_solve_tuned(h->variant, h->form, h->dev, d_in, d_tun, batch, d_x, d_fm, d_status, d_iters, s);
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

// What the batch entries check behind their own null and alignment checks, in the precedence of the return codes: the create
// flag the entry needs (`why`: the text that names it, nullptr the plain one), the batch against the handle's, the empty
// batch.  GO: the entry goes on; any other value is what it returns.
constexpr int GO = 1;
int batch_entry(const vsmpc_handle* h, int batch, bool has_flag = true, const char* why = nullptr) {
    if (!has_flag) return unsupported(why);
    if (batch > h->max_batch) return VSMPC_ERR_BATCH_TOO_LARGE;
    return batch == 0 ? VSMPC_OK : GO;
}

// The chunked host-pointer driver of the runtime family (vsmpc_sensitivity_batch, vsmpc_adjoint_batch,
// vsmpc_adjoint_record_batch).  An entry is its kind and a table of staged rows, one per argument beyond the solve's own.
struct RtFamily {
    RtMode kind;
    const RtDims& d;
    double* ws;          // workspace of instance 0, max_batch x d.ws_doubles
    int chunk;           // instances per launch: what the staging holds
    const char* entry;   // the name a HIP failure is reported under
};
struct HostSolve { const double* in; double *x, *first_move; int *status, *iters; };   // what every host-pointer solve has
// the caller's rows (nullptr: not given / not wanted, nothing is enqueued), the device staging of one chunk, the bytes of one
// instance, the direction
struct StagedRow { void* host; void* dev; size_t bytes; bool upload; };
// a row of the table; `arg`, the field of the RtLaunch it serves, gets the staging where the caller gave a pointer
template <typename T>
StagedRow upload(const T* host, const StageBuf<T>& buf, const T*& arg) {
    arg = host ? buf.get() : nullptr;
    return {const_cast<T*>(host), buf.get(), buf.width * sizeof(T), true};
}
template <typename T>
StagedRow download(T* host, const StageBuf<T>& buf, T*& arg) {
    arg = host ? buf.get() : nullptr;
    return {host, buf.get(), buf.width * sizeof(T), false};
}
// instances first .. first + n - 1 of every row of one direction, in table order; stops enqueuing at the first failure
hipError_t copy_staged(const StagedRow* rows, size_t n_rows, bool up, size_t first, size_t n, hipStream_t s) {
    for (const StagedRow* r = rows; r != rows + n_rows; ++r) {
        if (r->upload != up || r->host == nullptr) continue;
        char* const host = static_cast<char*>(r->host) + first * r->bytes;
        const hipError_t e = up ? hipMemcpyAsync(r->dev, host, n * r->bytes, hipMemcpyHostToDevice, s)
                                : hipMemcpyAsync(host, r->dev, n * r->bytes, hipMemcpyDeviceToHost, s);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
// Chunks of f.chunk instances in stream order: upload, launch, download; the staging of one chunk is read back before the
// next overwrites it.  `a` holds the staged rows' fields (and nothing else yet).  The first error is kept, nothing is
// enqueued behind it, and nothing returns while copies into the caller's buffers are queued.
int chunked_host(vsmpc_handle* h, const RtFamily& f, const HostSolve& io, int batch, RtLaunch a, const StagedRow* rows,
                 size_t n_rows, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    ON_DEVICE(h->device);
    hipError_t err = hipSuccess;
    for (int first = 0; first < batch && err == hipSuccess; first += f.chunk) {
        const int n = std::min(f.chunk, batch - first);
        const size_t o = size_t(first), N = size_t(n);
        a.in = h->d_in + o * h->n_in;
        a.ws = f.ws + o * size_t(f.d.ws_doubles);
        a.x = io.x ? h->d_x + o * h->n_var : nullptr;
        a.fm = io.first_move ? h->d_fm + o * VSMPC_FM_SIZE : nullptr;
        a.status = h->d_status + o;
        a.iters = io.iters ? h->d_iters + o : nullptr;
        err = upload_rows(h->d_in, io.in, o, N, h->n_in, s);
        if (err == hipSuccess) err = copy_staged(rows, n_rows, true, o, N, s);
        if (err == hipSuccess) err = launch_runtime(f.kind, f.d, h->dev, n, a, s);
        if (err == hipSuccess) err = download_results(h, o, N, io.x, io.first_move, io.status, io.iters, s);
        if (err == hipSuccess) err = copy_staged(rows, n_rows, false, o, N, s);
    }
    const hipError_t e = hipStreamSynchronize(s);
    if (err == hipSuccess) err = e;
    if (err != hipSuccess) return hip_fail(err, f.entry);
    return VSMPC_OK;
}

// adjoint_kernel_rt and adjoint_record_kernel_rt run on the workspace of the runtime handle, or the one
// VSMPC_CREATE_ADJOINT allocated
double* adjoint_workspace(const vsmpc_handle* h) { return h->runtime ? h->d_ws.get() : h->adjoint.ws.get(); }
const char* const ADJOINT_NEEDS_FLAG = "vsmpc_adjoint_batch needs a handle created with VSMPC_CREATE_ADJOINT (vsmpc_create_ex)";
const char* const ADJOINT_RECORD_NEEDS_FLAG =
    "vsmpc_adjoint_record_batch needs a handle created with VSMPC_CREATE_ADJOINT_RECORD (vsmpc_create_ex)";
// (the kernels load a row of tunables 16 bytes per lane)
bool misaligned16(const void* p) { return (reinterpret_cast<size_t>(p) & 15) != 0; }

}  // namespace

extern "C" {

int vsmpc_solve_batch_device(vsmpc_handle* h, const double* d_in, int batch, double* d_x, double* d_first_move,
                             int* d_status, int* d_iters, void* stream) {
    if (h == nullptr || d_in == nullptr || d_status == nullptr || batch < 0) return invalid_arg();
    if (const int rc = batch_entry(h, batch); rc != GO) return rc;
    ON_DEVICE(h->device);   // an enqueue-only entry must not change the caller's current device either
    HIP_TRY(solve_launch(h, d_in, batch, d_x, d_first_move, d_status, d_iters, 0, static_cast<hipStream_t>(stream)));
    return VSMPC_OK;
}

int vsmpc_solve_batch(vsmpc_handle* h, const double* in, int batch, double* x, double* first_move, int* status,
                      int* iters, void* stream) {
    if (h == nullptr || in == nullptr || status == nullptr || batch < 0) return invalid_arg();
    if (const int rc = batch_entry(h, batch); rc != GO) return rc;
    return solve_batch_host(h, in, nullptr, batch, x, first_move, status, iters, stream);
}

int vsmpc_solve_batch_tuned_device(vsmpc_handle* h, const double* d_in, const double* d_tunables, int batch, double* d_x,
                                   double* d_first_move, int* d_status, int* d_iters, void* stream) {
    if (h == nullptr || d_in == nullptr || d_tunables == nullptr || d_status == nullptr || batch < 0) return invalid_arg();
    if (misaligned16(d_tunables)) return invalid_arg();
    if (const int rc = batch_entry(h, batch); rc != GO) return rc;
    ON_DEVICE(h->device);
    HIP_TRY(solve_launch(h, d_in, batch, d_x, d_first_move, d_status, d_iters, 0, static_cast<hipStream_t>(stream), d_tunables));
    return VSMPC_OK;
}

int vsmpc_solve_batch_tuned(vsmpc_handle* h, const double* in, const double* tunables, int batch, double* x,
                            double* first_move, int* status, int* iters, void* stream) {
    if (h == nullptr || in == nullptr || tunables == nullptr || status == nullptr || batch < 0) return invalid_arg();
    if (const int rc = batch_entry(h, batch, h->tunables); rc != GO) return rc;
    return solve_batch_host(h, in, tunables, batch, x, first_move, status, iters, stream);
}

// Sensitivities of the solution to X0 (include/vsmpc.h): sens_kernel_rt on the workspace VSMPC_CREATE_SENSITIVITY allocated
int vsmpc_sensitivity_batch_device(vsmpc_handle* h, const double* d_in, int batch, double* d_x, double* d_first_move,
                                   int* d_status, int* d_iters, double* d_dx_dx0, double* d_dfm_dx0, int* d_active,
                                   int* d_sens_flags, void* stream) {
    if (h == nullptr || d_in == nullptr || d_status == nullptr || batch < 0) return invalid_arg();
    if (const int rc = batch_entry(h, batch, h->sens.on); rc != GO) return rc;
    ON_DEVICE(h->device);
    RtLaunch a = solve_args(d_in, nullptr, d_x, d_first_move, d_status, d_iters);
    a.ws = h->sens.ws;
    a.dx = d_dx_dx0; a.dfm = d_dfm_dx0; a.active = d_active; a.flags = d_sens_flags;
    HIP_TRY(launch_runtime(RT_SENS, h->sens.dims, h->dev, batch, a, static_cast<hipStream_t>(stream)));
    return VSMPC_OK;
}

int vsmpc_sensitivity_batch(vsmpc_handle* h, const double* in, int batch, double* x, double* first_move, int* status,
                            int* iters, double* dx_dx0, double* dfm_dx0, int* active, int* sens_flags, void* stream) {
    if (h == nullptr || in == nullptr || status == nullptr || batch < 0) return invalid_arg();
    if (const int rc = batch_entry(h, batch, h->sens.on); rc != GO) return rc;
    const vsmpc_handle::Sens& k = h->sens;
    RtLaunch a;
    const StagedRow rows[] = {download(dx_dx0, k.dx, a.dx), download(dfm_dx0, k.dfm, a.dfm), download(active, k.active, a.active),
                              download(sens_flags, k.flags, a.flags)};
    return chunked_host(h, {RT_SENS, k.dims, k.ws, SENS_CHUNK, "vsmpc_sensitivity_batch"}, {in, x, first_move, status, iters},
                        batch, a, rows, std::size(rows), stream);
}

// Adjoint of the solve (include/vsmpc.h): adjoint_kernel_rt, or adjoint_kernel_rt_tuned with rows of tunables
int vsmpc_adjoint_batch_device(vsmpc_handle* h, const double* d_in, const double* d_tunables, const double* d_xbar,
                               const double* d_fmbar, int batch, double* d_x, double* d_first_move, int* d_status,
                               int* d_iters, double* d_grad_x0, double* d_grad_cfg, int* d_active, int* d_adj_flags,
                               void* stream) {
    if (h == nullptr || d_in == nullptr || d_xbar == nullptr || d_status == nullptr || batch < 0) return invalid_arg();
    if (misaligned16(d_tunables)) return invalid_arg();
    if (const int rc = batch_entry(h, batch, h->adjoint.on, ADJOINT_NEEDS_FLAG); rc != GO) return rc;
    ON_DEVICE(h->device);
    RtLaunch a = solve_args(d_in, d_tunables, d_x, d_first_move, d_status, d_iters);
    a.ws = adjoint_workspace(h);
    a.xbar = d_xbar; a.fmbar = d_fmbar;
    a.gx0 = d_grad_x0; a.gcfg = d_grad_cfg; a.active = d_active; a.flags = d_adj_flags;
    HIP_TRY(launch_runtime(RT_ADJOINT, h->adjoint.dims, h->dev, batch, a, static_cast<hipStream_t>(stream)));
    return VSMPC_OK;
}

int vsmpc_adjoint_batch(vsmpc_handle* h, const double* in, const double* tunables, const double* xbar, const double* fmbar,
                        int batch, double* x, double* first_move, int* status, int* iters, double* grad_x0, double* grad_cfg,
                        int* active, int* adj_flags, void* stream) {
    if (h == nullptr || in == nullptr || xbar == nullptr || status == nullptr || batch < 0) return invalid_arg();
    if (const int rc = batch_entry(h, batch, h->adjoint.on, ADJOINT_NEEDS_FLAG); rc != GO) return rc;
    const vsmpc_handle::Adjoint& k = h->adjoint;
    RtLaunch a;
    const StagedRow rows[] = {upload(xbar, k.xbar, a.xbar), upload(fmbar, k.fmbar, a.fmbar), upload(tunables, k.tun, a.tun),
                              download(grad_x0, k.gx0, a.gx0), download(grad_cfg, k.gcfg, a.gcfg),
                              download(active, k.active, a.active), download(adj_flags, k.flags, a.flags)};
    return chunked_host(h, {RT_ADJOINT, k.dims, adjoint_workspace(h), ADJ_CHUNK, "vsmpc_adjoint_batch"},
                        {in, x, first_move, status, iters}, batch, a, rows, std::size(rows), stream);
}

// Adjoint of the record (include/vsmpc.h): adjoint_record_kernel_rt[_tuned] on the adjoint entry's workspace and staging,
// with the staging VSMPC_CREATE_ADJOINT_RECORD allocated for the two further outputs
int vsmpc_adjoint_record_batch_device(vsmpc_handle* h, const double* d_in, const double* d_tunables, const double* d_xbar,
                                      const double* d_fmbar, int batch, double* d_x, double* d_first_move, int* d_status,
                                      int* d_iters, double* d_grad_x0, double* d_grad_cfg, int* d_active, int* d_adj_flags,
                                      double* d_grad_in, double* d_grad_model, void* stream) {
    if (h == nullptr || d_in == nullptr || d_xbar == nullptr || d_status == nullptr || batch < 0) return invalid_arg();
    if (misaligned16(d_tunables)) return invalid_arg();
    if (const int rc = batch_entry(h, batch, h->adjoint_record.on, ADJOINT_RECORD_NEEDS_FLAG); rc != GO) return rc;
    ON_DEVICE(h->device);
    RtLaunch a = solve_args(d_in, d_tunables, d_x, d_first_move, d_status, d_iters);
    a.ws = adjoint_workspace(h);
    a.xbar = d_xbar; a.fmbar = d_fmbar;
    a.gx0 = d_grad_x0; a.gcfg = d_grad_cfg; a.active = d_active; a.flags = d_adj_flags;
    a.gin = d_grad_in; a.gmodel = d_grad_model;
    HIP_TRY(launch_runtime(RT_ADJOINT_REC, h->adjoint_record.dims, h->dev, batch, a, static_cast<hipStream_t>(stream)));
    return VSMPC_OK;
}

int vsmpc_adjoint_record_batch(vsmpc_handle* h, const double* in, const double* tunables, const double* xbar,
                               const double* fmbar, int batch, double* x, double* first_move, int* status, int* iters,
                               double* grad_x0, double* grad_cfg, int* active, int* adj_flags, double* grad_in,
                               double* grad_model, void* stream) {
    if (h == nullptr || in == nullptr || xbar == nullptr || status == nullptr || batch < 0) return invalid_arg();
    if (const int rc = batch_entry(h, batch, h->adjoint_record.on, ADJOINT_RECORD_NEEDS_FLAG); rc != GO) return rc;
    const vsmpc_handle::Adjoint& k = h->adjoint;
    const vsmpc_handle::AdjointRecord& r = h->adjoint_record;
    RtLaunch a;
    const StagedRow rows[] = {upload(xbar, k.xbar, a.xbar), upload(fmbar, k.fmbar, a.fmbar), upload(tunables, k.tun, a.tun),
                              download(grad_x0, k.gx0, a.gx0), download(grad_cfg, k.gcfg, a.gcfg),
                              download(active, k.active, a.active), download(adj_flags, k.flags, a.flags),
                              download(grad_in, r.gin, a.gin), download(grad_model, r.gmodel, a.gmodel)};
    return chunked_host(h, {RT_ADJOINT_REC, r.dims, adjoint_workspace(h), ADJ_CHUNK, "vsmpc_adjoint_record_batch"},
                        {in, x, first_move, status, iters}, batch, a, rows, std::size(rows), stream);
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
    if (const int rc = batch_entry(h, batch); rc != GO) return rc;
    ON_DEVICE(h->device);
    HIP_TRY(launch_certify(h->rt, h->dev, d_in, d_x, d_tunables, batch, d_y, d_cert, static_cast<hipStream_t>(stream)));
    return VSMPC_OK;
}

int vsmpc_certify_batch(vsmpc_handle* h, const double* in, const double* x, const double* tunables, int batch, double* y,
                        double* cert) {
    if (h == nullptr || in == nullptr || x == nullptr || cert == nullptr || batch < 0) return invalid_arg();
    if (const int rc = batch_entry(h, batch, h->certify,
                                   "vsmpc_certify_batch needs a handle created with VSMPC_CREATE_CERTIFY (vsmpc_create_ex)");
        rc != GO)
        return rc;
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
    if (const int rc = batch_entry(h, batch); rc != GO) return rc;
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
