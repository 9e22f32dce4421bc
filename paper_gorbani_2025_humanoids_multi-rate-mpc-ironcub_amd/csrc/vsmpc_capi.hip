// C-ABI of include/vsmpc.h: configuration checks, handle lifecycle, getters, error texts (the entries that stage and launch:
// vsmpc_capi_solve / _debug / _rollout.hip).  No compute fallback lives here: every numeric result comes from the HIP kernels.
#include "vsmpc_host.hpp"

using namespace vsmpc;

// dt schedule: constraintsVSMPC.cpp:45-51 (beta1, beta2), :78-84, :156-159
void vsmpc::fill_dt(const vsmpc_config& c, double* dt) {
    const double nS = double(c.n_iter_small);
    const double beta2 = (c.period_large - nS * c.period_small) / (nS * (nS - 1.0));
    const double beta1 = c.period_small - beta2;
    auto warp = [&](double t) { return beta1 * t + beta2 * t * t; };
    for (int i = 0; i < c.n_iter; ++i)
        dt[i] = i < c.n_iter_small ? warp(double(i + 1)) - warp(double(i)) : c.period_large;
}

namespace {

// The tunables of a configuration in the form the kernels keep them in (sCfg order, CFG_*): the row of
// vsmpc_pack_tunables, and what fill_devcfg puts into the kernel argument.
void fill_tunables(const vsmpc_config& c, double* row) {
    static_assert(CFG_SIZE == VSMPC_TUNE_SIZE, "a row of tunables is the LDS configuration block");
    // diagonal of Q on the weighted rows (costsVSMPC.cpp:78-93): p, h_lin, rpy, h_ang | e_pos, e_rpy
    const double q[NWROWS] = {c.w_com_pos[0], c.w_com_pos[1], c.w_com_pos[2], c.w_lin_mom[0], c.w_lin_mom[1],
                              c.w_lin_mom[2], c.w_rpy[0], c.w_rpy[1], c.w_rpy[2], c.w_ang_mom[0],
                              c.w_ang_mom[1], c.w_ang_mom[2], c.w_com_pos_err[0], c.w_com_pos_err[1],
                              c.w_com_pos_err[2], c.w_rpy_err[0], c.w_rpy_err[1], c.w_rpy_err[2]};
    for (int i = 0; i < NWROWS; ++i) row[CFG_SQ + i] = std::sqrt(q[i]);
    for (int i = 0; i < NJ; ++i) row[CFG_WJ + i] = c.w_delta_joint[i] + c.w_reg_joint_pos;
    row[CFG_WREG] = c.w_reg_joint_pos;
    row[CFG_WTHR] = c.w_throttle;
    row[CFG_WINIT] = c.w_initial_throttle;
    row[CFG_VMIN] = Jet::v_of_throttle_div(c.throttle_min);  // constraintsVSMPC.cpp:329-332
    row[CFG_VMAX] = Jet::v_of_throttle_div(c.throttle_max);
    for (int i = CFG_VMAX + 1; i < CFG_SIZE; ++i) row[i] = 0.0;
}

void fill_devcfg(const vsmpc_config& c, DevCfg& d) {
    memset(&d, 0, sizeof(d));
    fill_dt(c, d.dt);
    double row[CFG_SIZE];
    fill_tunables(c, row);
    for (int i = 0; i < NWROWS; ++i) d.sq[i] = row[CFG_SQ + i];
    for (int i = 0; i < NJ; ++i) d.wj[i] = row[CFG_WJ + i];
    d.w_reg = row[CFG_WREG];
    d.w_thr = row[CFG_WTHR];
    d.w_init = row[CFG_WINIT];
    d.vmin = row[CFG_VMIN];
    d.vmax = row[CFG_VMAX];
    d.use_jet = c.use_jet_dynamic ? 1 : 0;
    d.max_as_iter = 64;
}

// the value checks on the tunables: the name of the first field that fails, or nullptr
const char* tunables_invalid(const vsmpc_config& c) {
    const struct { const double* v; int n; const char* name; } w[] = {
        {c.w_com_pos, 3, "w_com_pos"}, {c.w_lin_mom, 3, "w_lin_mom"}, {c.w_rpy, 3, "w_rpy"}, {c.w_ang_mom, 3, "w_ang_mom"},
        {c.w_com_pos_err, 3, "w_com_pos_err"}, {c.w_rpy_err, 3, "w_rpy_err"}, {&c.w_throttle, 1, "w_throttle"},
        {&c.w_initial_throttle, 1, "w_initial_throttle"}, {&c.w_reg_joint_pos, 1, "w_reg_joint_pos"}};
    for (const auto& f : w)
        for (int i = 0; i < f.n; ++i)
            if (!(f.v[i] >= 0.0)) return f.name;
    for (int i = 0; i < NJ; ++i)
        if (!(c.w_delta_joint[i] + c.w_reg_joint_pos > 0.0)) return "w_delta_joint";  // condensed Hessian must stay PD
    if (!(c.w_initial_throttle > 0.0)) return "w_initial_throttle";
    if (!(c.throttle_max > c.throttle_min)) return "throttle_max";
    return nullptr;
}

bool config_valid(const vsmpc_config& c) {
    if (c.n_iter < 2 || c.n_iter > MAX_STAGES) return false;
    if (c.n_iter_small < 2 || c.n_iter_small > c.control_horizon) return false;
    if (c.control_horizon > c.n_iter) return false;
    if (!(c.period_small > 0.0) || !(c.period_large > 0.0)) return false;
    return tunables_invalid(c) == nullptr;
}

// the thread-local texts of vsmpc_strerror: the last HIP failure, the last refusal of vsmpc_pack_tunables, and the reason
// of the last VSMPC_ERR_UNSUPPORTED_CONFIG (nullptr: the plain text)
thread_local char g_hip_msg[256] = "";
thread_local char g_arg_msg[160] = "";
thread_local const char* g_unsupported_msg = nullptr;

// the name of the first structural field in which `c` differs from the handle's configuration, or nullptr
const char* structural_mismatch(const vsmpc_config& c, const vsmpc_config& h) {
    if (c.n_iter != h.n_iter) return "n_iter";
    if (c.n_iter_small != h.n_iter_small) return "n_iter_small";
    if (c.control_horizon != h.control_horizon) return "control_horizon";
    if ((c.use_jet_dynamic != 0) != (h.use_jet_dynamic != 0)) return "use_jet_dynamic";
    if (c.period_mpc != h.period_mpc) return "period_mpc";
    if (c.period_small != h.period_small) return "period_small";
    if (c.period_large != h.period_large) return "period_large";
    return nullptr;
}

}  // namespace

int vsmpc::invalid_arg() {
    g_arg_msg[0] = '\0';
    return VSMPC_ERR_INVALID_ARG;
}

int vsmpc::invalid_field(const char* entry, const char* field) {
    snprintf(g_arg_msg, sizeof(g_arg_msg), "invalid argument (%s: invalid %s)", entry, field);
    return VSMPC_ERR_INVALID_ARG;
}

int vsmpc::unsupported(const char* why) {
    g_unsupported_msg = why;
    return VSMPC_ERR_UNSUPPORTED_CONFIG;
}

int vsmpc::hip_fail(hipError_t e, const char* what) { return hip_fail_into(g_hip_msg, e, what); }

extern "C" {

int vsmpc_create(const vsmpc_config* cfg, int device, int max_batch, vsmpc_handle** out) {
    // VSMPC_RUNTIME_HORIZON=1: unmodified programs get the runtime kernel for horizons outside the table
    const char* env = getenv("VSMPC_RUNTIME_HORIZON");
    const unsigned flags = (env != nullptr && env[0] == '1' && env[1] == '\0') ? VSMPC_CREATE_RUNTIME_FALLBACK : 0u;
    return vsmpc_create_ex(cfg, device, max_batch, flags, out);
}

int vsmpc_create_ex(const vsmpc_config* cfg, int device, int max_batch, unsigned flags, vsmpc_handle** out) {
    if (cfg == nullptr || out == nullptr || max_batch <= 0) return invalid_arg();
    *out = nullptr;
    const unsigned kernel_flags = VSMPC_CREATE_RUNTIME_FALLBACK | VSMPC_CREATE_RUNTIME_ONLY;
    if ((flags & ~(kernel_flags | VSMPC_CREATE_SENSITIVITY | VSMPC_CREATE_TUNABLES | VSMPC_CREATE_CERTIFY |
                   VSMPC_CREATE_ADJOINT | VSMPC_CREATE_ADJOINT_RECORD)) != 0u)
        return invalid_arg();
    if (!config_valid(*cfg)) return invalid_arg();
    const int variant = (flags & VSMPC_CREATE_RUNTIME_ONLY)
                            ? int(VARIANT_NONE)
                            : select_variant(cfg->n_iter, cfg->n_iter_small, cfg->control_horizon);
    if (variant == VARIANT_NONE && (flags & kernel_flags) == 0u) return unsupported();
    const bool runtime = variant == VARIANT_NONE;
    const RtDims rt = runtime_dims(cfg->n_iter, cfg->n_iter_small, cfg->control_horizon);
    if (runtime && runtime_lds_bytes(rt) > RT_MAX_LDS) return unsupported();   // (not for a valid config)
    const bool sens = (flags & VSMPC_CREATE_SENSITIVITY) != 0u;
    const RtDims rts = runtime_dims(cfg->n_iter, cfg->n_iter_small, cfg->control_horizon, true);
    if (sens && runtime_lds_bytes(rts) > RT_MAX_LDS) return unsupported();     // (not for a valid config)
    const bool adjoint_record = (flags & VSMPC_CREATE_ADJOINT_RECORD) != 0u;
    const bool adjoint = (flags & VSMPC_CREATE_ADJOINT) != 0u || adjoint_record;
    const RtDims rta = runtime_dims(cfg->n_iter, cfg->n_iter_small, cfg->control_horizon, false, true);
    if (adjoint && runtime_tuned_lds_bytes(rta) > RT_MAX_LDS) return unsupported();   // (not for a valid config)
    const RtDims rtr = runtime_dims(cfg->n_iter, cfg->n_iter_small, cfg->control_horizon, false, true, true);
    if (adjoint_record && runtime_tuned_lds_bytes(rtr) > RT_MAX_LDS) return unsupported();   // (not for a valid config)
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return invalid_arg();
    ON_DEVICE(device);

    vsmpc_handle* h = new (std::nothrow) vsmpc_handle();
    if (h == nullptr) return VSMPC_ERR_ALLOC;
    h->cfg = *cfg;
    fill_devcfg(*cfg, h->dev);
    h->variant = variant;
    h->runtime = runtime ? 1 : 0;
    h->rt = rt;
    h->sens.on = sens ? 1 : 0;
    h->sens.dims = rts;
    h->tunables = (flags & VSMPC_CREATE_TUNABLES) != 0u ? 1 : 0;
    h->certify = (flags & VSMPC_CREATE_CERTIFY) != 0u ? 1 : 0;
    h->adjoint.on = adjoint ? 1 : 0;
    h->adjoint.dims = rta;
    h->adjoint_record.on = adjoint_record ? 1 : 0;
    h->adjoint_record.dims = rtr;
    h->form = runtime ? 0 : initial_kernel_form();
    for (int i = 0; i < VSMPC_N_JOINTS; ++i) h->kin.sel[i] = 3 + i;   // the shipped robot: joints 3..10
    h->kin.constant_lambda = 0;
    if (h->form == 1 && !variant_has_structured(variant)) h->form = 0;
    h->device = device;
    h->max_batch = max_batch;
    h->small_mode = initial_small_batch_mode();
    h->cu_count = 0;
    {
        const hipError_t ea = hipDeviceGetAttribute(&h->cu_count, hipDeviceAttributeMultiprocessorCount, device);
        if (ea != hipSuccess) { delete h; return hip_fail(ea, "vsmpc_create"); }
    }
    const int N = cfg->n_iter, nS = cfg->n_iter_small, H = cfg->control_horizon;
    h->n_var = NX * (N + 1) + NJ * H + NTH * (H - nS + 1);
    h->n_con = NX * (N + 1) + NTH * (N - nS + 1);
    h->n_in = VSMPC_IN_XREF + 12 * (N - nS + 1);
    h->n_p = runtime ? rt.np : variant_condensed_dim(variant);

    const size_t B = size_t(max_batch);
    hipError_t e = hipSuccess;   // the first failure wins: nothing is allocated after it
    auto need = [&e](auto& buf, size_t n, bool wanted = true) { if (wanted && e == hipSuccess) e = buf.alloc(n); };
    // staging of a chunked entry: `width` elements for each of `chunk` instances (the copies read the width from the buffer)
    auto stage = [&e](auto& buf, size_t chunk, size_t width, bool wanted) { if (wanted && e == hipSuccess) e = buf.alloc(chunk, width); };
    need(h->d_in, B * h->n_in);
    need(h->d_x, B * h->n_var);
    need(h->d_fm, B * VSMPC_FM_SIZE);
    need(h->d_status, B);
    need(h->d_iters, B);
    need(h->d_lin, B * (NX * NX + NX * NJ + NX * NTH + NX));
    need(h->d_dbg, size_t(2) * h->n_p * h->n_p);
    need(h->d_kin, B * VSMPC_KIN_SIZE);
    need(h->d_kout, B * VSMPC_KIN_OUT);
    need(h->d_stamps, B * 16);
    need(h->d_ws, B * size_t(rt.ws_doubles), runtime);
    const size_t C = std::min(B, size_t(SENS_CHUNK));
    need(h->sens.ws, B * size_t(rts.ws_doubles), sens);
    stage(h->sens.dx, C, size_t(h->n_var) * SENS_NPAR, sens);
    stage(h->sens.dfm, C, size_t(VSMPC_FM_SIZE) * SENS_NPAR, sens);
    stage(h->sens.active, C, rts.nv, sens);
    stage(h->sens.flags, C, 1, sens);
    need(h->d_tun, B * VSMPC_TUNE_SIZE, h->tunables);
    need(h->d_cx, B * h->n_var, h->certify);
    need(h->d_cy, B * h->n_con, h->certify);
    need(h->d_ccert, B * VSMPC_CERT_SIZE, h->certify);
    need(h->d_ctun, B * VSMPC_TUNE_SIZE, h->certify);
    const size_t CA = std::min(B, size_t(ADJ_CHUNK));
    need(h->adjoint.ws, B * size_t(rta.ws_doubles), adjoint && !runtime);
    stage(h->adjoint.xbar, CA, h->n_var, adjoint);
    stage(h->adjoint.fmbar, CA, VSMPC_FM_SIZE, adjoint);
    stage(h->adjoint.tun, CA, VSMPC_TUNE_SIZE, adjoint);
    stage(h->adjoint.gx0, CA, NX, adjoint);
    stage(h->adjoint.gcfg, CA, VSMPC_GRAD_SIZE, adjoint);
    stage(h->adjoint.active, CA, rta.nv, adjoint);
    stage(h->adjoint.flags, CA, 1, adjoint);
    stage(h->adjoint_record.gin, CA, h->n_in, adjoint_record);
    stage(h->adjoint_record.gmodel, CA, VSMPC_GRAD_MODEL_SIZE, adjoint_record);
    for (int i = 0; i < PIPE_STREAMS && e == hipSuccess; ++i) {
        e = hipStreamCreateWithFlags(h->pipe[i].put(), hipStreamNonBlocking);
        if (e == hipSuccess) e = hipEventCreateWithFlags(h->pipe_done[i].put(), hipEventDisableTiming);
    }
    if (e == hipSuccess) e = hipEventCreateWithFlags(h->pipe_start.put(), hipEventDisableTiming);
    if (e == hipSuccess) {
        const size_t zc = size_t(ZC_MAX) * (h->n_in + h->n_var + VSMPC_FM_SIZE + 1 + VSMPC_KIN_SIZE + VSMPC_TUNE_SIZE) *
                          sizeof(double);  // ints share one double
        e = hipHostMalloc(h->stage.put(), zc, hipHostMallocMapped);
        h->h_stage = static_cast<double*>(h->stage.h);
        if (e == hipSuccess) e = hipHostGetDevicePointer(reinterpret_cast<void**>(&h->d_stage), h->h_stage, 0);
    }
    if (e == hipSuccess) e = hipEventCreate(h->ev0.put());
    if (e == hipSuccess) e = hipEventCreate(h->ev1.put());
    if (e != hipSuccess) {
        vsmpc_destroy(h);
        return e == hipErrorOutOfMemory ? VSMPC_ERR_ALLOC : hip_fail(e, "vsmpc_create");
    }
    *out = h;
    return VSMPC_OK;
}

void vsmpc_destroy(vsmpc_handle* h) {
    if (h == nullptr) return;
    DeviceScope scope(h->device);
    delete h;   // the owners free on the current device
}

int vsmpc_num_variables(const vsmpc_handle* h) { return h ? h->n_var : invalid_arg(); }
int vsmpc_num_constraints(const vsmpc_handle* h) { return h ? h->n_con : invalid_arg(); }
int vsmpc_input_doubles(const vsmpc_handle* h) { return h ? h->n_in : invalid_arg(); }
int vsmpc_max_batch(const vsmpc_handle* h) { return h ? h->max_batch : invalid_arg(); }
int vsmpc_condensed_dim(const vsmpc_handle* h) { return h ? h->n_p : invalid_arg(); }
const char* vsmpc_kernel_name(const vsmpc_handle* h) {
    return h ? (h->runtime ? runtime_kernel_name() : variant_kernel_name(h->variant)) : "none";
}
int vsmpc_num_throttle_unknowns(const vsmpc_handle* h) { return h ? h->rt.nv : invalid_arg(); }

int vsmpc_pack_tunables(const vsmpc_handle* h, const vsmpc_config* cfgs, int n, double* out) {
    if (h == nullptr || n < 0 || (n > 0 && (cfgs == nullptr || out == nullptr))) {
        snprintf(g_arg_msg, sizeof(g_arg_msg), "invalid argument (vsmpc_pack_tunables: null pointer or negative count)");
        return VSMPC_ERR_INVALID_ARG;
    }
    for (int i = 0; i < n; ++i) {
        const char* field = structural_mismatch(cfgs[i], h->cfg);
        if (field != nullptr) {
            snprintf(g_arg_msg, sizeof(g_arg_msg),
                     "invalid argument (vsmpc_pack_tunables: configuration %d differs from the handle in the structural field %s)",
                     i, field);
            return VSMPC_ERR_INVALID_ARG;
        }
        field = tunables_invalid(cfgs[i]);
        if (field != nullptr) {
            snprintf(g_arg_msg, sizeof(g_arg_msg), "invalid argument (vsmpc_pack_tunables: configuration %d has an invalid %s)", i,
                     field);
            return VSMPC_ERR_INVALID_ARG;
        }
    }
    for (int i = 0; i < n; ++i) fill_tunables(cfgs[i], out + size_t(i) * VSMPC_TUNE_SIZE);
    g_arg_msg[0] = '\0';
    return VSMPC_OK;
}

int vsmpc_set_kernel_form(vsmpc_handle* h, int form) {
    if (h == nullptr || form < 0 || form > 2) return invalid_arg();
    if (h->runtime && form != 0) return unsupported();   // the runtime kernel has one form
    if (form == 1 && !variant_has_structured(h->variant)) return unsupported();
    const int prev = h->form;
    h->form = form;
    return prev;
}

int vsmpc_set_small_batch_kernel(vsmpc_handle* h, int mode) {
    if (h == nullptr || mode < 0 || mode > 2) return invalid_arg();
    if (mode == 2 && (h->runtime || !variant_has_small(h->variant))) return unsupported("this horizon has no small-batch kind of the solve kernel");
    const int prev = h->small_mode;
    h->small_mode = mode;
    return prev;
}

int vsmpc_small_batch_kernel_for(const vsmpc_handle* h, int batch) {
    if (h == nullptr || batch <= 0) return invalid_arg();
    return small_batch_kernel(h, batch) ? 1 : 0;
}

size_t vsmpc_small_batch_lds_bytes(int n_iter, int n_iter_small, int control_horizon) {
    return variant_small_lds_bytes(select_variant(n_iter, n_iter_small, control_horizon));
}

void* vsmpc_alloc_host(size_t bytes) {
    void* p = nullptr;
    if (bytes == 0 || hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return p;
}

void vsmpc_free_host(void* p) {
    if (p != nullptr) (void)hipHostFree(p);
}

const char* vsmpc_strerror(int code) {
    switch (code) {
        case VSMPC_OK: return "ok";
        case VSMPC_ERR_INVALID_ARG: return g_arg_msg[0] ? g_arg_msg : "invalid argument";
        case VSMPC_ERR_UNSUPPORTED_CONFIG:
            return g_unsupported_msg ? g_unsupported_msg : "unsupported MPC configuration (no kernel instantiation)";
        case VSMPC_ERR_BATCH_TOO_LARGE: return "batch exceeds max_batch of the handle";
        case VSMPC_ERR_HIP: return g_hip_msg[0] ? g_hip_msg : "HIP runtime error";
        case VSMPC_ERR_ALLOC: return "allocation failed";
        default: return "unknown error";
    }
}

}  // extern "C"
