// C-ABI of include/vsmpc.h, the entries beside the hot path: linearisation and dense-QP debug assembly, the condensed
// matrices and phase stamps of the solve kernel, kinematics terms, the kinematics provider and the Jacobian of the tree plant's
// terms, event timing.
#include "vsmpc_host.hpp"

using namespace vsmpc;

bool vsmpc::tree_valid(const vsmpc_tree& tree) {
    if (tree.parent[0] != -1) return false;
    for (int b = 1; b < VSMPC_TREE_NB; ++b)
        if (tree.parent[b] < 0 || tree.parent[b] >= b) return false;      // parents precede children
    for (int j = 0; j < VSMPC_TREE_NJ; ++j)
        if (tree.robot_joint[j] < 0 || tree.robot_joint[j] >= VSMPC_KIN_NJ) return false;
    for (int i = 0; i < VSMPC_N_THRUSTS; ++i)
        if (tree.jet_body[i] < 0 || tree.jet_body[i] >= VSMPC_TREE_NB) return false;
    return true;
}

extern "C" {

int vsmpc_linearize_batch(vsmpc_handle* h, const double* in, int batch, double* A, double* Bj, double* Bt,
                          double* c, double* dt) {
    if (h == nullptr || in == nullptr || batch < 0) return invalid_arg();
    if (batch > h->max_batch) return VSMPC_ERR_BATCH_TOO_LARGE;
    if (dt) fill_dt(h->cfg, dt);
    if (batch == 0) return VSMPC_OK;
    ON_DEVICE(h->device);
    const size_t B = size_t(batch);
    double* dA = h->d_lin;
    double* dBj = dA + size_t(h->max_batch) * NX * NX;
    double* dBt = dBj + size_t(h->max_batch) * NX * NJ;
    double* dC = dBt + size_t(h->max_batch) * NX * NTH;
    HIP_TRY(hipMemcpy(h->d_in, in, B * h->n_in * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(launch_linearize_runtime(h->rt, h->dev, h->d_in, batch, dA, dBj, dBt, dC, nullptr));   // on every handle
    HIP_TRY(hipDeviceSynchronize());
    if (A) HIP_TRY(hipMemcpy(A, dA, B * NX * NX * sizeof(double), hipMemcpyDeviceToHost));
    if (Bj) HIP_TRY(hipMemcpy(Bj, dBj, B * NX * NJ * sizeof(double), hipMemcpyDeviceToHost));
    if (Bt) HIP_TRY(hipMemcpy(Bt, dBt, B * NX * NTH * sizeof(double), hipMemcpyDeviceToHost));
    if (c) HIP_TRY(hipMemcpy(c, dC, B * NX * sizeof(double), hipMemcpyDeviceToHost));
    return VSMPC_OK;
}

// Stacks the reference-ordered dense QP from the DEVICE linearisation; layout bookkeeping only
// (IMPCProblem.cpp:150-194; cost order variableSamplingMPC.cpp:70-76, row order :77-84).
int vsmpc_assemble_dense(vsmpc_handle* h, const double* in_one, double* H, double* g, double* Ac, double* lo,
                         double* hi) {
    if (h == nullptr || in_one == nullptr || H == nullptr || g == nullptr || Ac == nullptr || lo == nullptr ||
        hi == nullptr)
        return invalid_arg();
    std::vector<double> A(NX * NX), Bj(NX * NJ), Bt(NX * NTH), c(NX), dt(MAX_STAGES);
    int rc = vsmpc_linearize_batch(h, in_one, 1, A.data(), Bj.data(), Bt.data(), c.data(), dt.data());
    if (rc != VSMPC_OK) return rc;
    const vsmpc_config& cf = h->cfg;
    const int N = cf.n_iter, nS = cf.n_iter_small, Hc = cf.control_horizon;
    const int nvar = h->n_var, ncon = h->n_con;
    const int offJ = NX * (N + 1), offV = offJ + NJ * Hc, nvb = Hc - nS + 1;
    memset(H, 0, sizeof(double) * size_t(nvar) * nvar);
    memset(g, 0, sizeof(double) * nvar);
    memset(Ac, 0, sizeof(double) * size_t(ncon) * nvar);
    memset(lo, 0, sizeof(double) * ncon);
    memset(hi, 0, sizeof(double) * ncon);
    auto Hat = [&](int r, int cc) -> double& { return H[size_t(r) * nvar + cc]; };
    auto Aat = [&](int r, int cc) -> double& { return Ac[size_t(r) * nvar + cc]; };
    double q[NX] = {0};
    for (int i = 0; i < 3; ++i) {
        q[i] = cf.w_com_pos[i]; q[3 + i] = cf.w_lin_mom[i]; q[6 + i] = cf.w_rpy[i];
        q[9 + i] = cf.w_ang_mom[i]; q[20 + i] = cf.w_com_pos_err[i]; q[23 + i] = cf.w_rpy_err[i];
    }
    // ReferenceTrackingCost (costsVSMPC.cpp:166-178)
    for (int i = 1; i <= N; ++i) {
        const int col = (i - 1) < nS ? 0 : (i - 1) - nS;
        for (int r = 0; r < NX; ++r) {
            Hat(i * NX + r, i * NX + r) += q[r];
            if (r < 12) g[i * NX + r] += -q[r] * in_one[VSMPC_IN_XREF + col * 12 + r];
        }
    }
    // RegualarizationCost (costsVSMPC.cpp:375-409)
    for (int i = 0; i < Hc; ++i)
        for (int r = 0; r < NJ; ++r) Hat(offJ + i * NJ + r, offJ + i * NJ + r) += cf.w_delta_joint[r];
    for (int i = 0; i < Hc - nS; ++i)
        for (int r = 0; r < NTH; ++r) {
            const int a = offV + i * NTH + r, b = offV + (i + 1) * NTH + r;
            Hat(a, a) += cf.w_throttle; Hat(b, a) -= cf.w_throttle;
            Hat(a, b) -= cf.w_throttle; Hat(b, b) += cf.w_throttle;
        }
    // ThrottleInitialValueCost (costsVSMPC.cpp:468-487)
    double vprev[NTH];
    for (int r = 0; r < NTH; ++r) {
        vprev[r] = Jet::v_of_throttle_div(in_one[VSMPC_IN_UPREV + r]);
        Hat(offV + r, offV + r) += cf.w_initial_throttle;
        g[offV + r] += -cf.w_initial_throttle * vprev[r];
    }
    // JointPositionRegularizationCost (costsVSMPC.cpp:558-592)
    for (int i = 0; i < Hc; ++i)
        for (int r = 0; r < NJ; ++r) {
            Hat(offJ + i * NJ + r, offJ + i * NJ + r) += cf.w_reg_joint_pos;
            g[offJ + i * NJ + r] += cf.w_reg_joint_pos * in_one[VSMPC_IN_QERR + r];
        }
    // ConstraintSystemDynamicVS (constraintsVSMPC.cpp:76-131)
    for (int i = 0; i < N; ++i) {
        const double d = dt[i];
        const int jb = i < Hc ? i : Hc - 1;
        const int tb = i < nS ? 0 : (i < Hc ? i - (nS - 1) : Hc - nS);
        for (int r = 0; r < NX; ++r) {
            for (int cc = 0; cc < NX; ++cc) Aat(i * NX + r, i * NX + cc) = (r == cc ? 1.0 : 0.0) + d * A[r * NX + cc];
            Aat(i * NX + r, (i + 1) * NX + r) = -1.0;
            for (int cc = 0; cc < NJ; ++cc) Aat(i * NX + r, offJ + jb * NJ + cc) = d * Bj[r * NJ + cc];
            for (int cc = 0; cc < NTH; ++cc) Aat(i * NX + r, offV + tb * NTH + cc) = d * Bt[r * NTH + cc];
            lo[i * NX + r] = -d * c[r];
            hi[i * NX + r] = -d * c[r];
        }
    }
    // ConstraintInitialState (IQPUtilsMPC.cpp:71-92)
    const int r0 = N * NX;
    for (int r = 0; r < NX; ++r) {
        Aat(r0 + r, r) = 1.0;
        lo[r0 + r] = hi[r0 + r] = in_one[VSMPC_IN_X0 + r];
    }
    // ThrottleConstraint (constraintsVSMPC.cpp:338-365); trailing rows stay 0 in [0,0]
    const int r1 = r0 + NX;
    const bool hold = in_one[VSMPC_IN_HOLD] != 0.0;
    for (int i = 0; i < nvb; ++i)
        for (int r = 0; r < NTH; ++r) {
            Aat(r1 + i * NTH + r, offV + i * NTH + r) = 1.0;
            if (hold && i == 0) {
                lo[r1 + r] = hi[r1 + r] = vprev[r];
            } else {
                lo[r1 + i * NTH + r] = h->dev.vmin;
                hi[r1 + i * NTH + r] = h->dev.vmax;
            }
        }
    return VSMPC_OK;
}

int vsmpc_debug_condensed(vsmpc_handle* h, const double* in_one, double* M, double* Lfac) {
    if (h == nullptr || in_one == nullptr) return invalid_arg();
    if (h->runtime) return unsupported();
    ON_DEVICE(h->device);
    const size_t np2 = size_t(h->n_p) * h->n_p;
    HIP_TRY(hipMemcpy(h->d_in, in_one, h->n_in * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(h->d_dbg, 0, 2 * np2 * sizeof(double)));   // the kernel writes the lower triangles only
    // (always the shipped kernel: the small-batch kind never has all tiles of the condensed Hessian at one point)
    HIP_TRY(launch_solve(h->variant, h->form, h->dev, h->d_in, 1, h->d_x, h->d_fm, h->d_status, h->d_iters, h->d_dbg,
                         h->d_dbg + np2, nullptr, nullptr));
    HIP_TRY(hipDeviceSynchronize());
    if (M) HIP_TRY(hipMemcpy(M, h->d_dbg, np2 * sizeof(double), hipMemcpyDeviceToHost));
    if (Lfac) HIP_TRY(hipMemcpy(Lfac, h->d_dbg + np2, np2 * sizeof(double), hipMemcpyDeviceToHost));
    return VSMPC_OK;
}

int vsmpc_kinematics_batch(vsmpc_handle* h, const double* kin, int batch, double* out, double* records) {
    if (h == nullptr || kin == nullptr || out == nullptr || batch < 0) return invalid_arg();
    if (batch > h->max_batch) return VSMPC_ERR_BATCH_TOO_LARGE;
    if (batch == 0) return VSMPC_OK;
    ON_DEVICE(h->device);
    HIP_TRY(hipMemcpy(h->d_kin, kin, size_t(batch) * VSMPC_KIN_SIZE * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(launch_kinematics(h->d_kin, batch, h->d_kout, h->kin, nullptr));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, h->d_kout, size_t(batch) * VSMPC_KIN_OUT * sizeof(double), hipMemcpyDeviceToHost));
    if (records != nullptr) {  // patch the three fields of the input records (host side, layout bookkeeping only)
        for (int b = 0; b < batch; ++b) {
            double* rec = records + size_t(b) * h->n_in;
            const double* o = out + size_t(b) * VSMPC_KIN_OUT;
            memcpy(rec + VSMPC_IN_LLIN, o, 24 * sizeof(double));
            memcpy(rec + VSMPC_IN_LANG, o + 24, 24 * sizeof(double));
            memcpy(rec + VSMPC_IN_INERTIA, o + 48, 9 * sizeof(double));
        }
    }
    return VSMPC_OK;
}

int vsmpc_provider_batch(vsmpc_handle* h, const vsmpc_tree* tree, const double* state, int batch, double* kin,
                         double* robot, double* records) {
    if (h == nullptr || tree == nullptr || state == nullptr || batch < 0) return invalid_arg();
    if (batch > h->max_batch) return VSMPC_ERR_BATCH_TOO_LARGE;
    if (batch == 0) return VSMPC_OK;
    // the provider delivers the CURRENT frame Jacobians; jointsLambdaOption "constant" re-reads those slots as the
    // configure-time relative Jacobians and thrusts (vsmpc_set_kinematics_options): the combination has no meaning
    if (records != nullptr && h->kin.constant_lambda) return unsupported();
    if (!tree_valid(*tree)) return invalid_arg();
    ON_DEVICE(h->device);
    // scratch: the state records go through d_lin (1014 doubles per instance), the Robot-level outputs through d_x
    // (n_var >= 67 doubles per instance), the kinematics record through d_kin
    double* d_state = h->d_lin;
    double* d_robot = h->d_x;   // n_var >= 67 doubles per instance
    HIP_TRY(hipMemcpy(d_state, state, size_t(batch) * VSMPC_RS_SIZE * sizeof(double), hipMemcpyHostToDevice));
    if (records != nullptr)
        HIP_TRY(hipMemcpy(h->d_in, records, size_t(batch) * h->n_in * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(launch_provider(*tree, d_state, batch, h->d_kin, d_robot, records != nullptr ? h->d_in : nullptr, h->n_in, nullptr));
    if (records != nullptr) HIP_TRY(launch_kinematics_patch(h->d_kin, batch, h->d_in, h->n_in, h->kin, nullptr));
    HIP_TRY(hipDeviceSynchronize());
    if (kin != nullptr)
        HIP_TRY(hipMemcpy(kin, h->d_kin, size_t(batch) * VSMPC_KIN_SIZE * sizeof(double), hipMemcpyDeviceToHost));
    if (robot != nullptr)
        HIP_TRY(hipMemcpy(robot, d_robot, size_t(batch) * VSMPC_RO_SIZE * sizeof(double), hipMemcpyDeviceToHost));
    if (records != nullptr)
        HIP_TRY(hipMemcpy(records, h->d_in, size_t(batch) * h->n_in * sizeof(double), hipMemcpyDeviceToHost));
    return VSMPC_OK;
}

int vsmpc_tree_jacobian_batch_device(vsmpc_handle* h, const vsmpc_tree* tree, const double* d_q, const double* d_thrust, int batch,
                                     double* d_terms, double* d_jac, void* stream) {
    if (h == nullptr || tree == nullptr || d_q == nullptr || d_thrust == nullptr || batch <= 0) return invalid_arg();
    if (h->kin.constant_lambda) return unsupported();   // the provider delivers the current Jacobians (vsmpc_provider_batch)
    if (!tree_valid(*tree)) return invalid_arg();
    if (d_terms == nullptr && d_jac == nullptr) return VSMPC_OK;
    ON_DEVICE(h->device);
    HIP_TRY(launch_tree_jacobian(*tree, h->kin, d_q, VSMPC_TREE_NJ, d_thrust, VSMPC_N_THRUSTS, batch, d_terms, d_jac,
                                 static_cast<hipStream_t>(stream)));
    return VSMPC_OK;
}

int vsmpc_tree_jacobian_batch(vsmpc_handle* h, const vsmpc_tree* tree, const double* q, const double* thrust, int batch,
                              double* terms, double* jac) {
    if (h == nullptr || tree == nullptr || q == nullptr || thrust == nullptr || batch <= 0) return invalid_arg();
    if (h->kin.constant_lambda) return unsupported();
    if (!tree_valid(*tree)) return invalid_arg();
    if (terms == nullptr && jac == nullptr) return VSMPC_OK;
    ON_DEVICE(h->device);
    const size_t B = size_t(batch), nj = size_t(VSMPC_TT_SIZE) * VSMPC_TT_NDIR;
    DevBuf<double> d_q, d_t, d_terms, d_jac;   // a stand-alone entry of any batch: its own staging, freed on return
    hipError_t e = d_q.alloc(B * VSMPC_TREE_NJ);
    if (e == hipSuccess) e = d_t.alloc(B * VSMPC_N_THRUSTS);
    if (e == hipSuccess && terms != nullptr) e = d_terms.alloc(B * VSMPC_TT_SIZE);
    if (e == hipSuccess && jac != nullptr) e = d_jac.alloc(B * nj);
    if (e != hipSuccess) return e == hipErrorOutOfMemory ? VSMPC_ERR_ALLOC : hip_fail(e, "vsmpc_tree_jacobian_batch");
    HIP_TRY(hipMemcpy(d_q, q, B * VSMPC_TREE_NJ * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_t, thrust, B * VSMPC_N_THRUSTS * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(launch_tree_jacobian(*tree, h->kin, d_q, VSMPC_TREE_NJ, d_t, VSMPC_N_THRUSTS, batch, d_terms, d_jac, nullptr));
    HIP_TRY(hipDeviceSynchronize());
    if (terms != nullptr) HIP_TRY(hipMemcpy(terms, d_terms, B * VSMPC_TT_SIZE * sizeof(double), hipMemcpyDeviceToHost));
    if (jac != nullptr) HIP_TRY(hipMemcpy(jac, d_jac, B * nj * sizeof(double), hipMemcpyDeviceToHost));
    return VSMPC_OK;
}

int vsmpc_set_kinematics_options(vsmpc_handle* h, const int* joint_selector, int constant_lambda) {
    if (h == nullptr) return invalid_arg();
    if (joint_selector != nullptr) {
        for (int i = 0; i < VSMPC_N_JOINTS; ++i)
            if (joint_selector[i] < 0 || joint_selector[i] >= VSMPC_KIN_NJ) return invalid_arg();
        for (int i = 0; i < VSMPC_N_JOINTS; ++i) h->kin.sel[i] = joint_selector[i];
    }
    h->kin.constant_lambda = constant_lambda ? 1 : 0;
    return VSMPC_OK;
}

int vsmpc_debug_phase_cycles(vsmpc_handle* h, const double* in, int batch, unsigned long long* stamps16) {
    if (h == nullptr || in == nullptr || stamps16 == nullptr || batch <= 0) return invalid_arg();
    if (h->runtime) return unsupported();
    if (batch > h->max_batch) return VSMPC_ERR_BATCH_TOO_LARGE;
    ON_DEVICE(h->device);
    unsigned long long* d_st = h->d_stamps;
    HIP_TRY(hipMemset(d_st, 0, size_t(batch) * 16 * sizeof(unsigned long long)));
    HIP_TRY(hipMemcpy(h->d_in, in, size_t(batch) * h->n_in * sizeof(double), hipMemcpyHostToDevice));
    const bool small = small_batch_kernel(h, batch);   // the stamps of the kernel a solve of this batch runs on
    for (int rep = 0; rep < 3; ++rep)  // warm instruction caches, keep the last run
        HIP_TRY(small ? launch_solve_small(h->variant, h->dev, h->d_in, batch, h->d_x, h->d_fm, h->d_status, h->d_iters, d_st, nullptr)
                      : launch_solve(h->variant, h->form, h->dev, h->d_in, batch, h->d_x, h->d_fm, h->d_status, h->d_iters, nullptr,
                                     nullptr, d_st, nullptr));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(stamps16, d_st, size_t(batch) * 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return VSMPC_OK;
}

int vsmpc_timing_begin(vsmpc_handle* h, void* stream) {
    if (h == nullptr) return invalid_arg();
    HIP_TRY(hipEventRecord(h->ev0, static_cast<hipStream_t>(stream)));
    return VSMPC_OK;
}

int vsmpc_timing_end(vsmpc_handle* h, void* stream, int launches, float* ms_per_launch) {
    if (h == nullptr || ms_per_launch == nullptr || launches <= 0) return invalid_arg();
    HIP_TRY(hipEventRecord(h->ev1, static_cast<hipStream_t>(stream)));
    HIP_TRY(hipEventSynchronize(h->ev1));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, h->ev0, h->ev1));
    *ms_per_launch = ms / float(launches);
    return VSMPC_OK;
}

}  // extern "C"
