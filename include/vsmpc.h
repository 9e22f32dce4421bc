/*
 * vsmpc.h — C-ABI of the MI355X-native batched multi-rate ("variable sampling") MPC solve path.
 *
 * Drop-in boundary for ONE hot path of ami-iit/paper_gorbani_2025_humanoids_multi-rate-mpc-ironcub:
 * the per-tick  IMPCProblem::update() + VariableSamplingMPC::solveMPC()  pair
 *   (momentum-based-linear-mpc-lib/src/IMPCProblem/IMPCProblem.cpp:150-298,
 *    momentum-based-linear-mpc-lib/src/variableSamplingMPC/variableSamplingMPC.cpp:88-112),
 * i.e. linearise -> variable-sampling QP assembly -> QP solve -> first-move extraction, with a batch
 * axis over independent MPC instances added.  Plain C: pointers and sizes only, no C++/torch types.
 *
 * Each entry point cites the reference interface it replaces (paths relative to
 * /root/reference/src/flight-controller/).  INTEGRATION.md shows the reference-side binding.
 *
 * Threading: one handle per host thread / HIP stream; a handle is not thread-safe, distinct handles
 * are independent (the reference object is single-threaded and stateful too).
 * Errors: int return, 0 = VSMPC_OK, negative = API/HIP error (never throws, never aborts), plus a
 * per-instance status array mirroring the OsqpEigen::Status values the reference distinguishes
 * (IMPCProblem.cpp:285-294): the caller applies "consume only if Solved" (variableSamplingMPC.cpp:91).
 */
#ifndef VSMPC_H
#define VSMPC_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- sizes fixed by the reference (variableSamplingMPC/VSconstant.h:6-16) ---- */
#define VSMPC_N_STATES 26
#define VSMPC_N_JOINTS 8
#define VSMPC_N_THRUSTS 4

/* ---- return codes ---- */
#define VSMPC_OK 0
#define VSMPC_ERR_INVALID_ARG (-1)
#define VSMPC_ERR_UNSUPPORTED_CONFIG (-2)
#define VSMPC_ERR_BATCH_TOO_LARGE (-3)
#define VSMPC_ERR_HIP (-4)
#define VSMPC_ERR_ALLOC (-5)

/* ---- per-instance status (IMPCProblem.cpp:285-294) ---- */
#define VSMPC_STATUS_SOLVED 1        /* exact optimum found: OsqpEigen::Status::Solved          */
#define VSMPC_STATUS_MAX_ITER 2      /* active-set iteration cap hit: ...::MaxIterReached        */
#define VSMPC_STATUS_NUMERICAL 3     /* non-positive pivot / non-finite data: ...::NonCvx/error  */

/*
 * Configuration = the keys of group VS_MPC_CONFIG (src/config/vs_mcp_config.xml:7-43) that the path
 * reads (variableSamplingMPC.cpp:24-38, constraintsVSMPC.cpp:25-51,295-322, costsVSMPC.cpp:29-69,
 * 326-361,445-459,516-535).  XML/TOML parsing stays on the caller's side.
 */
typedef struct vsmpc_config {
    int n_iter;            /* nIter                */
    int n_iter_small;      /* nIterSmall           */
    int control_horizon;   /* controlHorizon       */
    int use_jet_dynamic;   /* useJetDynamic        */
    double period_mpc;     /* periodMPC            */
    double period_small;   /* periodMPCSmallSteps  */
    double period_large;   /* periodMPCLargeSteps  */
    double w_com_pos[3];       /* weightCoMPos      */
    double w_com_pos_err[3];   /* weightCoMPosError */
    double w_lin_mom[3];       /* weightLinMom      */
    double w_rpy[3];           /* weightRPY         */
    double w_rpy_err[3];       /* weightRPYError    */
    double w_ang_mom[3];       /* weightAngMom      */
    double w_delta_joint[8];   /* weightDeltaJoint  */
    double w_throttle;         /* weightThrottle; below 10 the QP is nearly singular: still solved, but the minimiser is no longer determined to 1e-8 */
    double w_initial_throttle; /* weightInitialThrottle */
    double w_reg_joint_pos;    /* weightRegularizationJointPos */
    double throttle_min;       /* throttleMin (percent) */
    double throttle_max;       /* throttleMax (percent) */
} vsmpc_config;

/*
 * Per-instance input record: `vsmpc_input_doubles()` doubles, array-of-records, C-contiguous
 * ([batch][n_in]).  It is the data the reference's update() pulls out of QPInput/Robot each tick
 * (utils/include/QPInput.h:12-124; consumers cited per field).  Offsets in doubles:
 */
#define VSMPC_IN_X0 0         /* 26 measured state X0: CoM, h_lin(body), unwrapped RPY, h_ang(body), T, Tdot,
                                    CoM - posCoMReference, rpy - RPYReference (constraintsVSMPC.cpp:206-230) */
#define VSMPC_IN_MASS 26      /*  1 Robot::getTotalMass (a float in the reference, utils/include/Robot.h:338) */
#define VSMPC_IN_WRB 27       /*  9 base rotation wR_b, row-major (systemDynamicsVSMPC.cpp:107,324)            */
#define VSMPC_IN_OMEGA 36     /*  3 omega_B = wR_b^T * base angular velocity (systemDynamicsVSMPC.cpp:108,325) */
#define VSMPC_IN_ALPHA 39     /*  1 alpha_gravity of this tick (systemDynamicsVSMPC.cpp:308)                   */
#define VSMPC_IN_GRAV 40      /*  3 Robot::getGravity (systemDynamicsVSMPC.cpp:309)                            */
#define VSMPC_IN_AMOM 43      /* 24 Robot::getMatrixAmomJets(true), 6x4 row-major (:93,:304)                   */
#define VSMPC_IN_LLIN 67      /* 24 Lambda_lin,B 3x8 row-major (systemDynamicsVSMPC.cpp:321-350)               */
#define VSMPC_IN_LANG 91      /* 24 Lambda_ang,B 3x8 row-major (systemDynamicsVSMPC.cpp:159-206)               */
#define VSMPC_IN_INERTIA 115  /*  9 I_G 3x3 row-major (systemDynamicsVSMPC.cpp:128-130)                        */
#define VSMPC_IN_RPY 124      /*  3 base RPY used for W^-1 (systemDynamicsVSMPC.cpp:132-147); W^-1 has no yaw
                                    term, so entry 2 is never read (tests/test_gpu_record_parity.py pins it)   */
#define VSMPC_IN_PREF 127     /*  3 QPInput::getPosCoMReference (systemDynamicsVSMPC.cpp:316)                  */
#define VSMPC_IN_RPYINIT 130  /*  3 configure-time RPY m_rpyInit (systemDynamicsVSMPC.cpp:67,100)              */
#define VSMPC_IN_T0 133       /*  4 linearisation thrust (systemDynamicsVSMPC.cpp:401-409)                     */
#define VSMPC_IN_TD0 137      /*  4 linearisation thrust rate                                                  */
#define VSMPC_IN_UPREV 141    /*  4 QPInput::getThrottleMPC, percent (systemDynamicsVSMPC.cpp:411)             */
#define VSMPC_IN_TDES 145     /*  4 QPInput::getThrustDesMPC (systemDynamicsVSMPC.cpp:415)                     */
#define VSMPC_IN_TDDES 149    /*  4 QPInput::getThrustDotDesMPC                                                */
#define VSMPC_IN_QERR 153     /*  8 q_cmd,sel - q_ref0 (costsVSMPC.cpp:574-589)                                */
#define VSMPC_IN_HOLD 161     /*  1 != 0 when the 20-tick hold pins v0 this tick (constraintsVSMPC.cpp:351)    */
#define VSMPC_IN_XREF 162     /* 12*(nIter-nIterSmall+1): reference window, column-major xref[col*12+row],
                                    rows = CoM, h_lin, RPY, h_ang (costsVSMPC.cpp:96-99,183-264).  Node k reads
                                    column 0 (k - 1 < nIterSmall) or k - 1 - nIterSmall (costsVSMPC.cpp:191-200),
                                    so the last column is never read (pinned by the same test)                 */

/* First-move block written per instance (variableSamplingMPC.cpp:99-102,138-151), 24 doubles. */
#define VSMPC_FM_DQ 0          /* 8 joint-position increments  x[off_joints .. +8]             */
#define VSMPC_FM_V0 8          /* 4 warped throttle v0         x[off_throttle .. +4]           */
#define VSMPC_FM_THROTTLE 12   /* 4 throttle percent, JetModel::destandardizeThrottle_u2T(v0)  */
#define VSMPC_FM_THRUST 16     /* 4 thrust reference    = node 1 thrust  X1[12:16]             */
#define VSMPC_FM_THRUSTDOT 20  /* 4 thrust-rate reference = node 1      X1[16:20]              */
#define VSMPC_FM_SIZE 24

typedef struct vsmpc_handle vsmpc_handle;

/* Replaces IMPCProblem::configure (IMPCProblem.cpp:3-148) + VariableSamplingMPC::setCostAndConstraints
 * (variableSamplingMPC.cpp:7-86): validates the configuration, selects the kernel instantiation and
 * allocates every device and staging buffer for `max_batch` instances on HIP device `device` (solve, linearise,
 * kinematics, diagnostics).  No allocation happens in any later call on the handle; a rollout object allocates at its
 * own create, grows its log buffer only when a longer logged run is requested, and allocates the buffers of a tree plant
 * or of per-instance tunables in the first vsmpc_rollout_set_tree / vsmpc_rollout_set_tunables that asks for them.
 * Horizons: any (nIter, nIterSmall, controlHorizon) listed in csrc/vsmpc_horizons.def has a kernel instantiation
 * (the kernels are straight-line code generated per horizon); others return VSMPC_ERR_UNSUPPORTED_CONFIG -- add the
 * horizon to VSMPC_HORIZONS and rebuild, or use the runtime-sized kernel (vsmpc_create_ex below, or
 * VSMPC_RUNTIME_HORIZON=1 in the environment). */
int vsmpc_create(const vsmpc_config* cfg, int device, int max_batch, vsmpc_handle** out);

/* vsmpc_create with a choice of solve kernel.  `flags`:
 *   0                              exactly vsmpc_create without the environment switch below (tabled horizons only);
 *   VSMPC_CREATE_RUNTIME_FALLBACK  the tabled instantiation where one exists, the RUNTIME-SIZED kernel otherwise;
 *   VSMPC_CREATE_RUNTIME_ONLY      always the runtime-sized kernel (A/B runs, cross-checks at tabled horizons; it takes
 *                                  precedence when both bits are set).
 * Unknown bits return VSMPC_ERR_INVALID_ARG.  The runtime-sized kernel (csrc/vsmpc_runtime.hip) solves every configuration
 * the validation accepts (2 <= nIter <= 40, 2 <= nIterSmall <= controlHorizon <= nIter) with the same record, outputs,
 * statuses and active-set rule as the tuned kernels, at a fraction of their speed (profiles/runtime_horizon_bench.txt).
 * It keeps the condensed matrix in device memory: (NP (NP + 1) / 2) doubles per instance of max_batch, NP = 8 HC +
 * 4 (HC - nS + 1) + 1 (paper horizon 59 KB, (40, 2, 40) 0.9 MB), allocated here.  Launches of one runtime handle share
 * that workspace: they must be ordered (one stream at a time, as for every handle).
 * On a runtime handle every solve entry point works (vsmpc_solve_batch, _device, vsmpc_tick, the rollout API and its graph
 * replay, vsmpc_timing_*), as do vsmpc_linearize_batch, vsmpc_assemble_dense, vsmpc_kinematics_batch and
 * vsmpc_provider_batch; vsmpc_kernel_name returns "solve_kernel_rt" and vsmpc_condensed_dim NP.  vsmpc_set_kernel_form
 * accepts form 0 only; vsmpc_debug_condensed and vsmpc_debug_phase_cycles return VSMPC_ERR_UNSUPPORTED_CONFIG.
 * Environment: VSMPC_RUNTIME_HORIZON=1 makes vsmpc_create behave as vsmpc_create_ex(.., VSMPC_CREATE_RUNTIME_FALLBACK, ..),
 * so that unmodified programs (the C++ wrapper, the pybind11 shim) run any horizon.
 * VSMPC_CREATE_SENSITIVITY (with any of the above, on tuned and runtime handles) also allocates the workspace of
 * vsmpc_sensitivity_batch below; handles created without it allocate nothing for it. */
#define VSMPC_CREATE_RUNTIME_FALLBACK 0x1u
#define VSMPC_CREATE_RUNTIME_ONLY 0x2u
#define VSMPC_CREATE_SENSITIVITY 0x4u
#define VSMPC_CREATE_TUNABLES 0x8u      /* device staging of vsmpc_solve_batch_tuned: max_batch x VSMPC_TUNE_SIZE doubles */
#define VSMPC_CREATE_CERTIFY 0x20u      /* device staging of vsmpc_certify_batch: max_batch x (nCon + VSMPC_CERT_SIZE) doubles
                                           for y and the certificate, max_batch x nVar for x, max_batch x VSMPC_TUNE_SIZE
                                           for the rows.  Bit 0x10 is reserved (refused like every unknown bit) */
#define VSMPC_CREATE_ADJOINT 0x40u      /* what vsmpc_adjoint_batch needs (below): the runtime-sized kernel's workspace where the
                                           handle has none, and the staging of the host-pointer entry */
#define VSMPC_CREATE_ADJOINT_RECORD 0x80u   /* what vsmpc_adjoint_record_batch needs (below): everything VSMPC_CREATE_ADJOINT
                                           allocates (the flag implies it) and the staging of grad_in and grad_model for the
                                           chunks of the host-pointer entry, min(max_batch, 256) x (n_in +
                                           VSMPC_GRAD_MODEL_SIZE) doubles.  No later call allocates */
int vsmpc_create_ex(const vsmpc_config* cfg, int device, int max_batch, unsigned flags, vsmpc_handle** out);
void vsmpc_destroy(vsmpc_handle* h);

/* IMPCProblem::getNOptimizationVariables / getNConstraints (IMPCProblem.h:71-78) and record sizes. */
int vsmpc_num_variables(const vsmpc_handle* h);    /* nVar  = 26(N+1)+8H+4(H-nS+1)  (588) */
int vsmpc_num_constraints(const vsmpc_handle* h);  /* nCon  = 26(N+1)+4(N-nS+1)     (512) */
int vsmpc_input_doubles(const vsmpc_handle* h);    /* n_in  = 162+12(N-nS+1)        (294) */
int vsmpc_max_batch(const vsmpc_handle* h);

/* Replaces update()+solveMPC() for `batch` independent instances (variable_sampling_mpc.py:111-112).
 * The caller's current HIP device is left as it was found (every entry point of this header does so).
 * Host buffers: in[batch*n_in]; x[batch*nVar] primal in the REFERENCE variable order
 * [X0..XN | U0..U_{H-1} | v0..v_{H-nS}]; first_move[batch*24]; status[batch]; iters[batch] (active-set
 * iterations).  x, first_move, iters may be NULL.  `stream` is a hipStream_t (NULL = default stream);
 * the call returns after the results are in the host buffers. */
int vsmpc_solve_batch(vsmpc_handle* h, const double* in, int batch, double* x, double* first_move,
                      int* status, int* iters, void* stream);

/* Same, all pointers are DEVICE pointers and the call only enqueues work on `stream` (no copies,
 * no synchronisation): the form a resident batch driver uses.  batch <= vsmpc_max_batch(h). */
int vsmpc_solve_batch_device(vsmpc_handle* h, const double* d_in, int batch, double* d_x,
                             double* d_first_move, int* d_status, int* d_iters, void* stream);

/*
 * Per-instance tunables: one launch whose instances each carry their own weights and throttle box (gain studies over the
 * batch axis).  The TUNABLES of an instance are the vsmpc_config fields that change neither a size nor the time grid: the
 * six 3-vectors of state weights, w_delta_joint[8], w_throttle, w_initial_throttle, w_reg_joint_pos, throttle_min and
 * throttle_max.  The STRUCTURAL fields (n_iter, n_iter_small, control_horizon, use_jet_dynamic and the three periods) stay
 * the handle's.
 *
 * vsmpc_pack_tunables converts `n` configurations into rows of VSMPC_TUNE_SIZE doubles, out[n][VSMPC_TUNE_SIZE] (host).
 * A row is OPAQUE: it is "produced by vsmpc_pack_tunables", in the form the kernels keep the configuration in, by the
 * same code that converts the handle's own configuration at create (a row packed from the handle's configuration is bit
 * for bit what the plain entries solve with).  Returns VSMPC_ERR_INVALID_ARG when a cfgs[i] differs from the handle in a
 * structural field or fails the value checks of vsmpc_create; vsmpc_strerror(VSMPC_ERR_INVALID_ARG) then names the
 * configuration and the field, until the next call on that thread that packs successfully or returns
 * VSMPC_ERR_INVALID_ARG for a reason of its own (which gets the plain text).  No device work.
 */
#define VSMPC_TUNE_SIZE 32
int vsmpc_pack_tunables(const vsmpc_handle* h, const vsmpc_config* cfgs, int n, double* out /* [n][VSMPC_TUNE_SIZE] */);
/* vsmpc_solve_batch with instance i solved under row i of `tunables` (host, [batch][VSMPC_TUNE_SIZE]): the same chunking
 * and the same treatment of pinned and pageable buffers.  Needs a handle created with VSMPC_CREATE_TUNABLES, which
 * allocates the device staging of the rows at create (otherwise VSMPC_ERR_UNSUPPORTED_CONFIG).  Tuned and runtime
 * handles; vsmpc_set_kernel_form applies as to vsmpc_solve_batch.  A non-finite tunable ends like a non-finite record:
 * status VSMPC_STATUS_NUMERICAL for that instance.  Sensitivities with per-instance tunables are out of scope:
 * vsmpc_sensitivity_batch always uses the handle's configuration. */
int vsmpc_solve_batch_tuned(vsmpc_handle* h, const double* in, const double* tunables, int batch, double* x,
                            double* first_move, int* status, int* iters, void* stream);
/* Same, all pointers are DEVICE pointers (d_tunables 16-byte aligned) and the call only enqueues work on `stream`.
 * Needs no create flag. */
int vsmpc_solve_batch_tuned_device(vsmpc_handle* h, const double* d_in, const double* d_tunables, int batch, double* d_x,
                                   double* d_first_move, int* d_status, int* d_iters, void* stream);

/*
 * Sensitivities of the solution to the measured state X0 (in[VSMPC_IN_X0 .. +26]).  X0 enters the QP only through the
 * initial-state rows, and the QP is solved exactly, so near a non-degenerate solution x* is an affine function of X0;
 * its Jacobian is one more solve with the final active set ("Sensitivities").  Needs a handle created with
 * VSMPC_CREATE_SENSITIVITY (otherwise VSMPC_ERR_UNSUPPORTED_CONFIG): it solves with sens_kernel_rt, the runtime-sized
 * kernel with 26 more condensed columns, whose workspace is (NPS (NPS + 1) / 2) doubles per instance of max_batch,
 * NPS = NP + 26 (87 KB at the paper horizon, 1.0 MB at (40, 2, 40)).  vsmpc_set_kernel_form does not affect it.
 * Per instance:
 *   x, first_move, status, iters   what vsmpc_solve_batch returns (bit for bit on a runtime handle, to rounding on a
 *                                  tuned one, with the same iterations)
 *   dx_dx0[nVar * 26]   row-major: entry i * 26 + j = d x_i / d X0_j, x in the reference variable order
 *   dfm_dx0[24 * 26]    rows of the first-move block; the throttle-percent rows are 0 where the clamp to [0, 100] is active
 *   active[NV]          final throttle states: 0 free, -1 at throttleMin, +1 at throttleMax, 2 pinned by the hold
 *   sens_flags          VSMPC_SENS_DEGENERATE: a non-pinned throttle is weakly active (bound, |reduced gradient| <=
 *                       VSMPC_SENS_GRAD_TOL (1 + max |s|), s the throttles' reduced gradient at v = 0) or nearly active (free,
 *                       within VSMPC_SENS_BOUND_TOL (1 + |v|) of a bound): the Jacobian is still written, the derivative of
 *                       the final active set's affine piece, i.e. one-sided;
 *                       VSMPC_SENS_UNSOLVED: status is not Solved, the Jacobian rows are zero
 * NV = vsmpc_num_throttle_unknowns(h) = 4 (HC - nS + 1).  Every output except status may be NULL.
 */
#define VSMPC_SENS_DEGENERATE 0x1
#define VSMPC_SENS_UNSOLVED 0x2
#define VSMPC_SENS_GRAD_TOL 1e-8
#define VSMPC_SENS_BOUND_TOL 1e-9
int vsmpc_num_throttle_unknowns(const vsmpc_handle* h);
/* Host buffers; returns after the results are in them.  Errors as vsmpc_solve_batch. */
int vsmpc_sensitivity_batch(vsmpc_handle* h, const double* in, int batch, double* x, double* first_move, int* status,
                            int* iters, double* dx_dx0, double* dfm_dx0, int* active, int* sens_flags, void* stream);
/* Same, all pointers are DEVICE pointers and the call only enqueues work on `stream`.  Launches of one handle share its
 * workspace: they must be ordered (one stream at a time). */
int vsmpc_sensitivity_batch_device(vsmpc_handle* h, const double* d_in, int batch, double* d_x, double* d_first_move,
                                   int* d_status, int* d_iters, double* d_dx_dx0, double* d_dfm_dx0, int* d_active,
                                   int* d_sens_flags, void* stream);

/*
 * Adjoint of the solve: the gradient of a scalar loss L on the plan with respect to the measured state X0 and to the
 * tunables (the weights and the throttle box), from the cotangents xbar = dL/dx ([batch][nVar], reference variable order) and,
 * optionally, fmbar = dL/d first_move ([batch][24]; NULL = none).  The QP is solved exactly, so the gradient is one more
 * linear solve with the factor the solver holds: with K the KKT matrix of the final active set, K [a; b] = [xbar; 0] gives
 * dL/dX0 = b on the initial-state rows, dL/d throttle limit = the sum of b over the throttles on that limit, and
 * dL/dw = -a' (dH/dw x + dg/dw) for every weight ("Adjoint"; executable model: tests/adjoint_model.py).  O(N)
 * recursions on 26-vectors and one right-hand side through the factor: no Jacobian is formed.
 * Needs a handle created with VSMPC_CREATE_ADJOINT (both entries; otherwise VSMPC_ERR_UNSUPPORTED_CONFIG, and
 * vsmpc_strerror names the flag).  It solves with adjoint_kernel_rt / adjoint_kernel_rt_tuned, the runtime-sized kernel with
 * five more phases behind the solve, on tuned handles too: a tuned handle gets no fast path here, as for the sensitivities.
 * tunables: rows of vsmpc_pack_tunables, one per instance, or NULL = the handle's configuration for every instance (bit for
 * bit what rows packed from the handle's configuration give).  Per instance:
 *   x, first_move, status, iters   what vsmpc_solve_batch[_tuned] returns (bit for bit on a runtime handle, to rounding on a
 *                                  tuned one, with the same iterations)
 *   grad_x0[26]                    dL/dX0 (X0 = in[VSMPC_IN_X0 .. +26]; for the other record fields: vsmpc_adjoint_record_batch)
 *   grad_cfg[VSMPC_GRAD_SIZE]      dL/d(field) in the order of the vsmpc_config fields (VSMPC_GRAD_* below): with respect to
 *                                  the values a caller writes -- weights, not their square roots; throttle limits in percent,
 *                                  not warped.  Entry 31 is 0.
 *   active[NV]                     final throttle states, as vsmpc_sensitivity_batch returns them
 *   adj_flags                      VSMPC_ADJ_DEGENERATE: a non-pinned throttle is weakly or nearly active, by the rule and the
 *                                  tolerances of VSMPC_SENS_DEGENERATE: the gradient is still written, that of the final active
 *                                  set's affine piece, i.e. one-sided;
 *                                  VSMPC_ADJ_UNSOLVED: status is not Solved, both gradients are zero
 * A non-finite entry of xbar or fmbar makes that instance's gradients NaN (and no other instance's).  Every sum has an order
 * fixed by the sizes alone: repeated and permuted batches are bit-identical.  in, xbar and status are required; every other
 * output, tunables and fmbar may be NULL.  batch 0: VSMPC_OK, nothing touched; batch > vsmpc_max_batch(h):
 * VSMPC_ERR_BATCH_TOO_LARGE.
 */
#define VSMPC_GRAD_W_COM_POS 0
#define VSMPC_GRAD_W_COM_POS_ERR 3
#define VSMPC_GRAD_W_LIN_MOM 6
#define VSMPC_GRAD_W_RPY 9
#define VSMPC_GRAD_W_RPY_ERR 12
#define VSMPC_GRAD_W_ANG_MOM 15
#define VSMPC_GRAD_W_DELTA_JOINT 18
#define VSMPC_GRAD_W_THROTTLE 26
#define VSMPC_GRAD_W_INITIAL_THROTTLE 27
#define VSMPC_GRAD_W_REG_JOINT_POS 28
#define VSMPC_GRAD_THROTTLE_MIN 29
#define VSMPC_GRAD_THROTTLE_MAX 30
#define VSMPC_GRAD_SIZE 32
#define VSMPC_ADJ_DEGENERATE 0x1
#define VSMPC_ADJ_UNSOLVED 0x2
/* Host buffers; returns after the results are in them.  Batches beyond 256 instances run in chunks in stream order. */
int vsmpc_adjoint_batch(vsmpc_handle* h, const double* in, const double* tunables, const double* xbar, const double* fmbar,
                        int batch, double* x, double* first_move, int* status, int* iters, double* grad_x0, double* grad_cfg,
                        int* active, int* adj_flags, void* stream);
/* Same, all pointers are DEVICE pointers (d_tunables 16-byte aligned) and the call only enqueues work on `stream`.  Launches
 * of one handle share its workspace: they must be ordered (one stream at a time), also against the handle's solves on a
 * runtime handle. */
int vsmpc_adjoint_batch_device(vsmpc_handle* h, const double* d_in, const double* d_tunables, const double* d_xbar,
                               const double* d_fmbar, int batch, double* d_x, double* d_first_move, int* d_status,
                               int* d_iters, double* d_grad_x0, double* d_grad_cfg, int* d_active, int* d_adj_flags,
                               void* stream);

/*
 * Adjoint of the record: vsmpc_adjoint_batch, and beside its outputs the gradient of L with respect to EVERY entry of the
 * input record -- the reference window, the previous throttle, the linearisation point, the posture error and the model
 * data of the kinematics provider -- and with respect to the linearisation itself.  With nu the multipliers of the solve
 * and K [a; b] = [xbar; 0] as above, dL/dp = -a' (dH/dp x + dg/dp + dE'/dp nu) + b' (de/dp - dE/dp x) for any parameter p of
 * the QP min 1/2 x'Hx + g'x, E x = e of the final active set ("Adjoint of the record"; executable model:
 * tests/adjoint_record_model.py).  nu is one more costate recursion, dL/d(A, Bj, Bt, c) a sum of rank-one terms over the
 * stages, and the record entries follow through the transposed linearisation: no Jacobian, no second factorisation, no
 * finite differences.
 * Needs a handle created with VSMPC_CREATE_ADJOINT_RECORD (both entries; otherwise VSMPC_ERR_UNSUPPORTED_CONFIG, and
 * vsmpc_strerror names the flag).  It solves with adjoint_record_kernel_rt / adjoint_record_kernel_rt_tuned: the adjoint
 * kernel with two more phases, on tuned handles too.  Arguments and outputs of vsmpc_adjoint_batch, bit for bit, plus, per
 * instance (each may be NULL):
 *   grad_in[n_in]                        dL/d in[.], entry by entry in the layout of the record (VSMPC_IN_*), all other
 *                                        entries held fixed.  grad_in[VSMPC_IN_X0 .. +26] is grad_x0.  The hold flag is a
 *                                        switch: 0.  The entries nothing reads (in[VSMPC_IN_RPY + 2] and, where nIter > nIterSmall,
 *                                        the last column of the window) get +0.0.  With use_jet_dynamic = 0 the entries of T0, TD0, TDES and
 *                                        TDDES are 0 and UPREV keeps its direct part (initial-throttle cost, hold pin).
 *   grad_model[VSMPC_GRAD_MODEL_SIZE]    dL/d(A | Bj | Bt | c), row-major blocks in the layout of vsmpc_linearize_batch at the
 *                                        offsets VSMPC_GRAD_MODEL_*: every entry of the four, also those the linearisation
 *                                        leaves at zero
 * The time grid (dt, the periods) is structural: no gradient.  Not Solved: VSMPC_ADJ_UNSOLVED and every entry of both is 0;
 * a non-finite entry of xbar or fmbar: every entry of both is NaN for that instance alone; VSMPC_ADJ_DEGENERATE as above (the
 * gradients are those of the final active set's affine piece).  Every sum has an order fixed by the sizes alone.
 */
#define VSMPC_GRAD_MODEL_A 0
#define VSMPC_GRAD_MODEL_BJ 676
#define VSMPC_GRAD_MODEL_BT 884
#define VSMPC_GRAD_MODEL_C 988
#define VSMPC_GRAD_MODEL_SIZE 1014
/* Host buffers; returns after the results are in them.  Batches beyond 256 instances run in chunks in stream order. */
int vsmpc_adjoint_record_batch(vsmpc_handle* h, const double* in, const double* tunables, const double* xbar,
                               const double* fmbar, int batch, double* x, double* first_move, int* status, int* iters,
                               double* grad_x0, double* grad_cfg, int* active, int* adj_flags, double* grad_in,
                               double* grad_model, void* stream);
/* Same, all pointers are DEVICE pointers (d_tunables 16-byte aligned) and the call only enqueues work on `stream`; ordering
 * as for vsmpc_adjoint_batch_device. */
int vsmpc_adjoint_record_batch_device(vsmpc_handle* h, const double* d_in, const double* d_tunables, const double* d_xbar,
                                      const double* d_fmbar, int batch, double* d_x, double* d_first_move, int* d_status,
                                      int* d_iters, double* d_grad_x0, double* d_grad_cfg, int* d_active, int* d_adj_flags,
                                      double* d_grad_in, double* d_grad_model, void* stream);

/*
 * Duals and a KKT certificate of a GIVEN primal, for every instance of a batch.  The QP is the reference-ordered dense one
 * (oracle/vsmpc_ref.py assemble_dense; IMPCProblem.cpp:150-194): min 1/2 x'Hx + g'x subject to lo <= Ac x <= hi.  `x` is an
 * input ([batch][nVar], reference variable order): usually what vsmpc_solve_batch returned, but the check never runs the
 * solver's code and judges any x.  With x given, stationarity of the state columns defines the equality duals (one
 * backward costate recursion through A), stationarity of the throttle columns defines the box multipliers, and the joint
 * columns' gradient is what is left ("Duals and certificate"): O(N) work on 26-vectors per instance.
 *
 * y[batch][nCon], nCon = vsmpc_num_constraints(h), in the reference's row order (dynamics blocks 0..N-1 | initial state |
 * throttle blocks) and with the sign of oracle/vsmpc_ref.py solve_exact, which is OSQP's: y > 0 where the upper bound of a
 * row is active, y < 0 where the lower one is.  The throttle rows behind block controlHorizon - nIterSmall are exactly 0
 * (constraintsVSMPC.cpp:338-365 leaves them [0, 0] with an empty row).  y may be NULL when only the certificate is wanted.
 *
 * cert[batch][VSMPC_CERT_SIZE] restates oracle/vsmpc_ref.py kkt_certificate on (x, y):
 *   STATIONARITY     max over the joint blocks j of |(W_dq + w_reg I) U_j + w_reg q_err + sum_{i: jb(i) = j} dt_i Bj' y_i|_inf.
 *                    Every other entry of Hx + g + Ac'y is zero by the construction of y (to the rounding of the recursion),
 *                    so this is |Hx + g + Ac'y|_inf
 *   STAT_SCALE       max(1, |g|_inf, |Hx|_inf), the oracle's scale of `stationarity_rel`
 *   PRIMAL           max over all rows of max(0, lo - Ac x, Ac x - hi): dynamics rows, X_0 = x0, the throttle box, and
 *                    the hold pin when in[VSMPC_IN_HOLD] != 0
 *   COMPLEMENTARITY  max over the throttle rows with lo < hi of max(y+ (hi - v), y- (v - lo)); pinned rows are excluded,
 *                    as in the oracle
 *   OBJECTIVE        1/2 x'Hx + g'x, the oracle's value (no constant term), summed in a fixed order
 *   DUAL_MAX         |y|_inf
 * and two reserved entries that are 0.  A non-finite record, tunable or x makes STATIONARITY and PRIMAL NaN.  Results do not
 * depend on an instance's position in the batch: repeated and permuted batches are bit-identical.
 * The certificate is a statement about this restated QP, not about the reference's solver output (parity unpinned).
 * tunables: rows of vsmpc_pack_tunables, one per instance, or NULL = the handle's configuration for every instance.
 */
#define VSMPC_CERT_STATIONARITY 0
#define VSMPC_CERT_STAT_SCALE 1
#define VSMPC_CERT_PRIMAL 2
#define VSMPC_CERT_COMPLEMENTARITY 3
#define VSMPC_CERT_OBJECTIVE 4
#define VSMPC_CERT_DUAL_MAX 5
#define VSMPC_CERT_SIZE 8
/* Host buffers; returns after the results are in them.  Needs a handle created with VSMPC_CREATE_CERTIFY (otherwise
 * VSMPC_ERR_UNSUPPORTED_CONFIG, and vsmpc_strerror names the flag).  NULL handle, in, x or cert: VSMPC_ERR_INVALID_ARG;
 * batch 0: VSMPC_OK, nothing touched; batch > vsmpc_max_batch(h): VSMPC_ERR_BATCH_TOO_LARGE.  Tuned and runtime handles. */
int vsmpc_certify_batch(vsmpc_handle* h, const double* in, const double* x, const double* tunables, int batch, double* y,
                        double* cert);
/* Same, all pointers are DEVICE pointers (d_in, d_x, d_tunables, d_y 16-byte aligned) and the call only enqueues one
 * launch on `stream`.  Needs no create flag: it uses no staging. */
int vsmpc_certify_batch_device(vsmpc_handle* h, const double* d_in, const double* d_x, const double* d_tunables, int batch,
                               double* d_y, double* d_cert, void* stream);

/* Parity split of the path: only the per-tick linearisation + discretisation, i.e.
 * SystemDynamicVS::updateDynamicMatrices/getAMatrix/getBJointsMatrix/getBThrottleMatrix/getCVector
 * (systemDynamicsVSMPC.cpp:495-585) and the dt schedule of constraintsVSMPC.cpp:45-51,78-84.
 * Host buffers, row-major per instance: A[batch*676], Bj[batch*208], Bt[batch*104], c[batch*26],
 * dt[nIter] (same for every instance). */
int vsmpc_linearize_batch(vsmpc_handle* h, const double* in, int batch, double* A, double* Bj,
                          double* Bt, double* c, double* dt);

/* Kinematics-derived inputs on the device (rows a3/a4 of the path): LinearMomentumDynamicVS::computeLambdaLin
 * (systemDynamicsVSMPC.cpp:321-350), AngularMomentumDynamicVS::computeLambdaAng + getRelativeJacobianCoM
 * (:159-226, "unfiltered" option) and the locked inertia of updateRPY (:128-130), from the raw Robot quantities.
 * kin[batch][VSMPC_KIN_SIZE] host buffer; out[batch][57] = Lambda_lin,B (24) | Lambda_ang,B (24) | I_G (9), all
 * row-major.  If `records` is not NULL (host, [batch][n_in]) the three fields are also written into the input
 * records at VSMPC_IN_LLIN / VSMPC_IN_LANG / VSMPC_IN_INERTIA. */
#define VSMPC_KIN_NJ 23        /* robot joints (MPCPyBindings.cpp:43) */
#define VSMPC_KIN_WRB 0        /*   9 wR_b row-major                                                   */
#define VSMPC_KIN_THRUST 9     /*   4 Robot::getJetThrusts                                             */
#define VSMPC_KIN_AXES 13      /*  12 Robot::getMatrixOfJetAxes 4x3                                    */
#define VSMPC_KIN_ARMS 25      /*  12 Robot::getMatrixOfJetArms 4x3                                    */
#define VSMPC_KIN_JREL 37      /* 276 getRelativeJacobianJetsBodyFrame()[i].bottomRows(3), 4 x (3x23)   */
#define VSMPC_KIN_JFRAME 313   /* 276 getJacobian(jet).topRightCorner(3,23), 4 x (3x23)                 */
#define VSMPC_KIN_JCOM 589     /*  69 getJacobianCoM().topRightCorner(3,23)                            */
#define VSMPC_KIN_MB 658       /*  36 getMassMatrix().block(0,0,6,6) row-major                         */
#define VSMPC_KIN_R 694        /*   3 p_CoM - p_base                                                   */
#define VSMPC_KIN_SIZE 697
#define VSMPC_KIN_OUT 57
int vsmpc_kinematics_batch(vsmpc_handle* h, const double* kin, int batch, double* out, double* records);

/* One tick of the reference's surface in ONE submission: update() [the kinematics-derived terms, systemDynamicsVSMPC.cpp:
 * 128-130,159-226,321-350] + solveMPC() [IMPCProblem.cpp:196-298, variableSamplingMPC.cpp:88-112] as the harness issues
 * them back to back (src/variable_sampling_mpc.py:111-112).  kin[batch][VSMPC_KIN_SIZE] and in[batch][n_in] are host
 * buffers; the device writes Lambda_lin,B | Lambda_ang,B | I_G into the records, solves them, and the call returns after
 * ONE synchronisation with the completed fields copied back into `in` (so `in` is the record that was solved) and the
 * results in x / first_move / status / iters (x, first_move, iters may be NULL).  batch <= 8 runs through the handle's
 * pinned, device-mapped staging buffer without any copy engine work: the form a 200 Hz single-robot caller uses
 * (include/VariableSamplingMPC.hpp, TickMachineT).  No allocation. */
int vsmpc_tick(vsmpc_handle* h, const double* kin, double* in, int batch, double* x, double* first_move, int* status,
               int* iters, void* stream);

/* Options of vsmpc_kinematics_batch, per handle.
 *   joint_selector[8] (or NULL = keep): robot joint index of every controlled joint, for the columns of Lambda_ang -- the
 *       reference selects them by NAME (`controlledJoints` against Robot::getJointName, systemDynamicsVSMPC.cpp:57-66,
 *       202-205).  Default 3..10, the shipped robot.  Lambda_lin keeps the reference's hard-coded offset 3 (:348).
 *   constant_lambda: jointsLambdaOption "constant" (systemDynamicsVSMPC.cpp:186-200,329-337).  The caller then delivers
 *       the CONFIGURE-TIME axes, arms and relative Jacobians; the JFRAME slot holds the relative Jacobians' TOP rows
 *       (4 x (3x23)) and JCOM[0..3] the thrusts of getRobot() that scale the angular term (the linear term keeps
 *       THRUST = getRobotReference()'s, as in the reference). */
int vsmpc_set_kinematics_options(vsmpc_handle* h, const int* joint_selector, int constant_lambda);

/* Batched kinematics provider: what the reference's Robot::setState caches for the path
 * (utils/src/Robot.cpp:198-335, getJacobian :505-514) on a SIMPLIFIED tree handed over as plain arrays: a floating base,
 * 8 revolute joints (joint j moves body j + 1; parents precede children), 4 jet frames.  iDynTree's conventions: MIXED
 * velocity representation, free-floating Jacobians [linear; angular] x [base 6 | joints].  The reference uses iDynTree
 * on the iRonCub URDF, neither of which is in this image: parity of this row is unpinned (oracle/robot_tree_ref.py). */
#define VSMPC_TREE_NB 9
#define VSMPC_TREE_NJ 8
typedef struct {
    int parent[VSMPC_TREE_NB];                 /* parent body (parent[0] = -1: the floating base) */
    int robot_joint[VSMPC_TREE_NJ];            /* index of tree joint j among the robot's 23 joints (Jacobian column) */
    double joint_axis[3 * VSMPC_TREE_NJ];      /* in the parent body's frame */
    double joint_origin[3 * VSMPC_TREE_NJ];    /* in the parent body's frame; the child frame sits there */
    double mass[VSMPC_TREE_NB];
    double com[3 * VSMPC_TREE_NB];             /* body frame */
    double inertia[6 * VSMPC_TREE_NB];         /* about the body CoM, body axes: xx xy xz yy yz zz */
    int jet_body[VSMPC_N_THRUSTS];
    double jet_origin[3 * VSMPC_N_THRUSTS];    /* body frame */
    double jet_axis[3 * VSMPC_N_THRUSTS];      /* thrust force direction, body frame (m_jetsAxesLocalFrames, Robot.cpp:256) */
    double gravity[3];
} vsmpc_tree;
/* state record per instance */
#define VSMPC_RS_P 0      /*  3 base position (world)                         */
#define VSMPC_RS_R 3      /*  9 wR_b row-major                                 */
#define VSMPC_RS_V 12     /*  3 base linear velocity (world, MIXED)           */
#define VSMPC_RS_W 15     /*  3 base angular velocity (world)                 */
#define VSMPC_RS_Q 18     /*  8 joint positions                               */
#define VSMPC_RS_QD 26    /*  8 joint velocities                              */
#define VSMPC_RS_T 34     /*  4 jet thrusts                                   */
#define VSMPC_RS_SIZE 38
/* Robot-level outputs per instance */
#define VSMPC_RO_COM 0    /*  3 getPositionCoM                                 */
#define VSMPC_RO_MOM 3    /*  6 getMomentum(false): centroidal, world axes     */
#define VSMPC_RO_MOMB 9   /*  6 getMomentum(true)                              */
#define VSMPC_RO_MASS 15  /*  1 getTotalMass                                   */
#define VSMPC_RO_AMOM 16  /* 24 getMatrixAmomJets(false) 6x4 row-major         */
#define VSMPC_RO_AMOMB 40 /* 24 getMatrixAmomJets(true)                        */
#define VSMPC_RO_RPY 64   /*  3 getBasePose().getRotation().asRPY()            */
#define VSMPC_RO_SIZE 67
/* state[batch][VSMPC_RS_SIZE] -> kin[batch][VSMPC_KIN_SIZE] (the record vsmpc_kinematics_batch reads; NULL = not wanted),
 * robot[batch][VSMPC_RO_SIZE] (NULL = not wanted) and, when `records` (batch input records of this handle's size) is
 * given, the fields update() pulls out of the Robot patched in place: X0 position / momentum / RPY / thrusts, MASS, WRB,
 * OMEGA, GRAV, AMOM, RPY, T0, and -- through the kinematics kernel on the device, no host round trip -- LLIN, LANG,
 * INERTIA.  Everything else of the record (references, throttle feedback, hold flag) stays the caller's. */
/* With jointsLambdaOption "constant" set on the handle, patching `records` is refused (VSMPC_ERR_UNSUPPORTED_CONFIG): that
 * option re-reads the Jacobian slots as configure-time quantities the provider does not deliver. */
int vsmpc_provider_batch(vsmpc_handle* h, const vsmpc_tree* tree, const double* state, int batch, double* kin,
                         double* robot, double* records);

/* What the kinematic-tree plant of a rollout (vsmpc_rollout_set_tree) hands a tick, as one smooth map of the plant's joints
 * and thrusts, and its Jacobian:
 *     (q[8], T[4]) -> terms = A_mom,body | Lambda_lin,B | Lambda_ang,B | I_B,   jac = d terms / d(q | T),
 * with the base at the origin, identity attitude and zero velocities -- the pose the rollout evaluates the provider and the
 * kinematics kernel at, so that `terms` is what vsmpc_provider_batch (AMOMB) followed by vsmpc_kinematics_batch returns
 * there (I_G = I_B at that pose).  One kernel (tree_jacobian_kernel) carries the twelve directions in forward mode; Lambda
 * is linear in T, so its thrust columns are Lambda at unit thrusts and every other row of those columns is zero.  Lambda_ang
 * takes its columns through the handle's joint selector (vsmpc_set_kinematics_options); with jointsLambdaOption "constant"
 * set the call is refused (VSMPC_ERR_UNSUPPORTED_CONFIG), as the provider's record patch is.  The tree's own geometry
 * (masses, origins, axes) is held fixed: there are no derivatives to it. */
#define VSMPC_TT_AMOM 0    /* 24 A_mom,body 6x4 row-major */
#define VSMPC_TT_LLIN 24   /* 24 Lambda_lin,B 3x8 */
#define VSMPC_TT_LANG 48   /* 24 Lambda_ang,B 3x8 */
#define VSMPC_TT_IB 72     /*  9 I_B */
#define VSMPC_TT_SIZE 81
#define VSMPC_TT_NDIR 12   /* 8 joints | 4 thrusts */
/* q[batch][8], thrust[batch][4] -> terms[batch][VSMPC_TT_SIZE] and jac[batch][VSMPC_TT_SIZE][VSMPC_TT_NDIR] (either may be
 * NULL: not wanted).  Any batch (the call stages it in device memory of its own, freed before it returns).  NULL handle, tree,
 * q or thrust, a batch <= 0 or an invalid tree (parents must precede children, indices in range): VSMPC_ERR_INVALID_ARG, the
 * NULL and batch checks before any device call. */
int vsmpc_tree_jacobian_batch(vsmpc_handle* h, const vsmpc_tree* tree, const double* q, const double* thrust, int batch,
                              double* terms, double* jac);
/* The same on device pointers: only enqueues on `stream` (the null stream too), allocates nothing, does not synchronise. */
int vsmpc_tree_jacobian_batch_device(vsmpc_handle* h, const vsmpc_tree* tree, const double* d_q, const double* d_thrust, int batch,
                                     double* d_terms, double* d_jac, void* stream);

/* Debug/parity: the reference-ordered dense QP of ONE instance, assembled on the host from the
 * DEVICE linearisation exactly as IMPCProblem::update stacks it (IMPCProblem.cpp:150-194):
 * H[nVar*nVar], g[nVar], Ac[nCon*nVar] (row-major), lo[nCon], hi[nCon]. */
int vsmpc_assemble_dense(vsmpc_handle* h, const double* in_one, double* H, double* g, double* Ac,
                         double* lo, double* hi);

/* Debug/parity: condensed problem of ONE instance after the device condensing + factorisation
 * phases.  M[np*np] row-major lower triangle of the augmented condensed Hessian (np =
 * vsmpc_condensed_dim(h); row NZ holds the condensed gradient), L likewise after the Cholesky. */
int vsmpc_condensed_dim(const vsmpc_handle* h);
int vsmpc_debug_condensed(vsmpc_handle* h, const double* in_one, double* M, double* Lfac);

/* Diagnostic build of the solve kernel (separate instantiation, never the timed one): s_memtime stamps of
 * workgroup thread 0 at the 10 phase boundaries P0..P6 of every instance, stamps16[batch*16]. */
int vsmpc_debug_phase_cycles(vsmpc_handle* h, const double* in, int batch, unsigned long long* stamps16);

/* Average device time per launch of the solve kernel over the launches enqueued between
 * vsmpc_timing_begin and vsmpc_timing_end on the handle's stream, measured with HIP events on the
 * stream the kernel is launched on.  Returns milliseconds through *ms_per_launch. */
int vsmpc_timing_begin(vsmpc_handle* h, void* stream);
int vsmpc_timing_end(vsmpc_handle* h, void* stream, int launches, float* ms_per_launch);

/*
 * ---- Closed-loop batched rollout --------------------------------------------------------------
 * The per-tick "advance" the reference hides inside its plugins and harness, for `batch` instances resident in HBM:
 *   build record (tick state machine: 20-tick hold constraintsVSMPC.cpp:351-372, reference window costsVSMPC.cpp:
 *   124-165, alpha cursor systemDynamicsVSMPC.cpp:308-311)  ->  solve  ->  apply the first move only if Solved
 *   (variableSamplingMPC.cpp:91-108)  ->  integrate a centroidal + jet plant over periodMPC in 1 ms sub-steps
 *   (the harness steps its simulator 5 x 1 ms per tick, ironcub_mujoco_simulator.py:122-139).
 * The plant is a synthetic stand-in for MuJoCo (out of scope): the centroidal-momentum model the MPC linearises with
 * the non-linear rotation kinematics and the non-linear jet polynomial (utils/src/JetModel.cpp:29-64).
 *
 * Plant state per instance, VSMPC_PLANT_STATE doubles: */
#define VSMPC_PS_P 0        /* 3 CoM position                                   */
#define VSMPC_PS_HLIN 3     /* 3 linear momentum, body frame                    */
#define VSMPC_PS_RPY 6      /* 3 base roll/pitch/yaw                            */
#define VSMPC_PS_HANG 9     /* 3 angular momentum, body frame                   */
#define VSMPC_PS_T 12       /* 4 jet thrusts                                    */
#define VSMPC_PS_TD 16      /* 4 jet thrust rates                               */
#define VSMPC_PS_Q 20       /* 8 controlled joint positions                     */
#define VSMPC_PS_U 28       /* 4 throttle command in percent (held between MPC moves) */
#define VSMPC_PS_TDES 32    /* 4 last MPC thrust reference   (QPInput::getThrustDesMPC)    */
#define VSMPC_PS_TDDES 36   /* 4 last MPC thrust-rate reference                            */
/* jet plant option (vsmpc_rollout_set_jet_plant, include/vsmpc_jet.h): NN thrust dynamics + EKF estimates; unused and
 * untouched with the polynomial jet plant */
#define VSMPC_PS_TNN 40     /* 4 thrust of the LSTM jet plant (float32 values), fed back to it     */
#define VSMPC_PS_EST 44     /* 8 EKF estimate (T, Tdot) per jet: what the MPC sees as measurement  */
#define VSMPC_PS_EKFP 52    /* 16 EKF covariance per jet, 2x2 row-major                           */
#define VSMPC_PLANT_STATE 68
/* Plant parameters per instance (constant over a rollout), VSMPC_PLANT_PARAMS doubles: */
#define VSMPC_PP_MASS 0
#define VSMPC_PP_INERTIA_B 1   /*   9 body-frame locked inertia, row-major                                          */
#define VSMPC_PP_AMOM0 10      /*  24 A_mom(q_ref0) 6x4 row-major, body frame                                      */
#define VSMPC_PP_DJ 34         /* 192 dA_mom/dq_j, [8][6][4]: A_mom(q) = A_mom0 + sum_j DJ[j] (q_j - q_ref0_j);
                                      Lambda_lin/ang column j = DJ[j] T (systemDynamicsVSMPC.cpp:159-206,321-350)   */
#define VSMPC_PP_QREF0 226     /*   8 posture reference q_ref0 (costsVSMPC.cpp:574-589)                             */
#define VSMPC_PP_PINIT 234     /*   3 configure-time CoM position (costsVSMPC.cpp:105)                              */
#define VSMPC_PP_RPYINIT 237   /*   3 configure-time RPY                                                            */
#define VSMPC_PP_DIST_F 240    /*   3 disturbance force, world frame [N]                                            */
#define VSMPC_PP_DIST_TAU 243  /*   3 disturbance torque, body frame [Nm]                                           */
#define VSMPC_PP_DIST_T0 246   /*   disturbance active for DIST_T0 <= t < DIST_T1 [s]                               */
#define VSMPC_PP_DIST_T1 247
#define VSMPC_PP_TICK0 248     /*   tick index of this instance at rollout start (phase of the hold / trajectory)   */
#define VSMPC_PLANT_PARAMS 249
/* Log row per tick and instance: p(3) rpy(3) T(4) throttle%(4) status iters */
#define VSMPC_ROLLOUT_LOG 16

typedef struct vsmpc_rollout vsmpc_rollout;

/* Allocates the resident rollout state for `batch` <= vsmpc_max_batch(h) instances.  The trajectories are shared by
 * all instances, as in the reference's TrajectoryManager (TrajectoryManager.cpp:23-39): CoM position OFFSETS and
 * velocities sampled every periodMPCLargeSteps (`n_traj` samples, [n_traj][3]), alpha_gravity sampled every
 * `alpha_dt` seconds (`n_alpha` samples, linearly up-sampled to the tick rate); both are clamped at their ends. */
int vsmpc_rollout_create(vsmpc_handle* h, int batch, const double* traj_pos, const double* traj_vel, int n_traj,
                         const double* traj_alpha, int n_alpha, double alpha_dt, vsmpc_rollout** out);
void vsmpc_rollout_destroy(vsmpc_rollout* r);
/* Host -> device: state[batch][VSMPC_PLANT_STATE], params[batch][VSMPC_PLANT_PARAMS]; resets the tick counters and
 * builds the record of tick 0 on the device. */
int vsmpc_rollout_reset(vsmpc_rollout* r, const double* state, const double* params);
/* Runs `ticks` closed-loop ticks on `stream`; log (host, may be NULL) receives [ticks][batch][VSMPC_ROLLOUT_LOG].
 * Returns after the last tick has completed. */
int vsmpc_rollout_run(vsmpc_rollout* r, int ticks, double* log, void* stream);
/* Device -> host copies of the current plant state / of the records the NEXT tick will solve ([batch][n_in], parity
 * hook: after reset the records of tick 0, after run(k) those of tick k). */
/* RPY / RPYDot tracks of the position trajectory (costsVSMPC.cpp:110-112,141-146: RPY reference = configure-time RPY +
 * track, angular-momentum reference = I_G W RPYDot at the attitude of the push), [n_traj][3] each, at the position
 * trajectory's rate; NULL = all zero (the shipped files).  Call before vsmpc_rollout_reset. */
int vsmpc_rollout_set_attitude_tracks(vsmpc_rollout* r, const double* traj_rpy, const double* traj_rpy_dot);
/* The same with flags; vsmpc_rollout_set_attitude_tracks is this call with flags 0.  Unknown bits: VSMPC_ERR_INVALID_ARG, and
 * the rollout stays as it was.
 *   VSMPC_ATTITUDE_ADJOINT   the rollout then accepts vsmpc_rollout_run_taped, vsmpc_rollout_backward[_device] and
 *                            vsmpc_rollout_backward_full[_device] with an RPYDot track too (without one as before), and
 *                            vsmpc_rollout_backward_attitude[_device] returns the gradient to both attitude tracks (below,
 *                            "Adjoint of the rollout: attitude tracks").  The sweep then runs the attitude instantiations
 *                            of its kernel.  The forward loop is the same with and without the flag, bit for bit.
 * Without the flag a rollout with an RPYDot track keeps refusing the taped run and the sweep. */
#define VSMPC_ATTITUDE_ADJOINT 1u
int vsmpc_rollout_set_attitude_tracks_ex(vsmpc_rollout* r, const double* traj_rpy, const double* traj_rpy_dot, unsigned flags);
/* Kinematic-tree plant: with a tree set, the plant's joint vectoring IS the kinematics the MPC linearises -- every tick the
 * batched kinematics provider (vsmpc_provider_batch's device code) is evaluated on the plant's own joint state, in the body
 * frame, and A_mom,body(q), the locked inertia I_B(q) and Lambda_lin,B / Lambda_ang,B (through vsmpc_kinematics_batch's
 * device code, from the tree's Jacobians) replace the plant parameters AMOM0 / DJ / INERTIA_B: what the harness does when it
 * refreshes the Robot from the simulator state every tick (src/mujoco_lib/ironcub_mujoco_simulator.py:318-346 ->
 * utils/src/Robot.cpp:198-335).  PP_MASS must be the tree's total mass; the controlled joints are the tree's eight
 * (tree->robot_joint[j] = 3 + j for the default selector).  NULL switches back to the parametric plant.  Call before
 * vsmpc_rollout_reset; a tick is then six launches instead of two (still replayed from a captured graph). */
int vsmpc_rollout_set_tree(vsmpc_rollout* r, const vsmpc_tree* tree);
/* The same with flags; vsmpc_rollout_set_tree is this call with flags 0.  Unknown bits: VSMPC_ERR_INVALID_ARG.
 *   VSMPC_TREE_ADJOINT   the rollout then accepts vsmpc_rollout_run_taped, vsmpc_rollout_backward[_device] and
 *                        vsmpc_rollout_backward_full[_device] on the tree plant (below, "Adjoint of the rollout").  The call
 *                        allocates the rows the sweep reads per launch -- the terms of vsmpc_tree_jacobian_batch and their
 *                        Jacobian, batch x VSMPC_TT_SIZE x (1 + VSMPC_TT_NDIR) doubles, kept until vsmpc_rollout_destroy; a
 *                        failure returns VSMPC_ERR_ALLOC and leaves the rollout as it was.  Refused when the handle has
 *                        jointsLambdaOption "constant" set at the time of this call (VSMPC_ERR_UNSUPPORTED_CONFIG), as the
 *                        provider's record patch is; the check is made here only: the rollout's tree plant, forward and
 *                        backward, never reads that option (it always forms the current Lambda terms).
 * Without the flag a rollout with a tree keeps refusing the taped run and the sweep. */
#define VSMPC_TREE_ADJOINT 1u
int vsmpc_rollout_set_tree_ex(vsmpc_rollout* r, const vsmpc_tree* tree, unsigned flags);
/* Per-instance tunables of the rollout's solves: tunables[batch][VSMPC_TUNE_SIZE] (host, rows of vsmpc_pack_tunables)
 * are copied to a device buffer the rollout owns, and every tick's solve launch -- those inside the captured graph too --
 * is then of the per-instance-tunables kind.  NULL restores the handle's shared configuration.  Call before
 * vsmpc_rollout_reset, like vsmpc_rollout_set_tree; the captured ticks are rebuilt.  The record and advance kernels read
 * no tunable: the solve is the only launch of a tick that changes.  The first call with rows allocates the device buffer
 * (batch x VSMPC_TUNE_SIZE doubles, kept until vsmpc_rollout_destroy), as vsmpc_rollout_set_tree allocates on first use;
 * a call that fails leaves the rollout as it was, runnable without a reset. */
int vsmpc_rollout_set_tunables(vsmpc_rollout* r, const double* tunables);
/*
 * Noise in the closed loop: seeded sensor noise on what the controller is handed, and gusts on the plant, drawn on the device
 * by a counter-based generator ("Noise in the closed loop"; executable model: tests/rollout_noise_model.py).  The
 * reference's own loop has the first: MujocoSim.simulate_noise adds np.random.normal(0, 0.015, 3) to the base linear and to the
 * base angular velocity the controller receives (src/mujoco_lib/ironcub_mujoco_simulator.py:271-288), which is
 * sigma_lin_vel = sigma_ang_vel = 0.015 here.
 *
 * Generator: Philox4x32-10, multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85.  Block j of loop b
 * at tick k is the output (w0, w1, w2, w3) of
 *     counter = (j, k, loop_lo, loop_hi)     key = (seed_lo, seed_hi)     loop = first_index + b  (64 bit)
 * with k the ticks since vsmpc_rollout_reset (PP_TICK0 is not added) and `loop` the loop's GLOBAL index, so that any slice of a
 * sharded batch draws what the whole batch would.  A block gives two standard normals, Box-Muller on 53-bit uniforms:
 *     u1 = (((uint64)w0 << 21 | w1 >> 11) + 0.5) 2^-53,  u2 likewise from (w2, w3)
 *     z[2j] = sqrt(-2 ln u1) cos(2 pi u2)     z[2j+1] = sqrt(-2 ln u1) sin(2 pi u2)
 * (the device evaluates the pair as sincospi(2 u2): the same angle, without the rounding of the product 2 pi u2).
 * A tick uses nine blocks: z[0:12] is the measurement of tick k, z[12:18] the gust held over tick k.  Nothing is stored: graph
 * replay, split runs and sharded batches reproduce each other bit for bit.
 *
 * Measurement: the record of tick k is built from a measured state in place of the plant state (the plant state itself, the
 * log rows and the integration stay the true ones), with R = R(rpy) of the true attitude and I_B the plant's (the parameter,
 * or I_B(q) of the kinematic tree):
 *     p     += sigma_pos z[0:3]          h_lin += m   R^T (sigma_lin_vel z[3:6])     (a world-frame velocity error)
 *     rpy   += sigma_rpy z[6:9]          h_ang += I_B R^T (sigma_ang_vel z[9:12])
 * and everything the record derives from these follows: X0, the position and attitude errors, omega, R, I_G, the window
 * column pushed on a release tick, the RPY unwrap.  The thrusts are not touched.
 * Gust: over the sub-steps of tick k the constant world force sigma_force z[12:15] and body torque sigma_torque z[15:18] act
 * beside the push of PP_DIST_F / PP_DIST_TAU, whatever the push's window.
 *
 * vsmpc_rollout_set_noise validates before it touches the device: a negative or non-finite sigma, or a negative first_index, is
 * VSMPC_ERR_INVALID_ARG with the field named in vsmpc_strerror's text, and the rollout stays as it was.  NULL switches the noise
 * off, as if it had never been set: the rollout then launches the kernels it launched before.  Either way the captured ticks
 * are dropped and vsmpc_rollout_reset is required before the next run, as after vsmpc_rollout_set_tree.  Noise combines with the
 * tree plant, the jet plant option, attitude tracks and per-instance tunables.  With noise set vsmpc_rollout_run_taped and every
 * vsmpc_rollout_backward* entry return VSMPC_ERR_UNSUPPORTED_CONFIG with a text that names the noise: the pathwise derivative
 * would need the noise's own dependence on the attitude, the mass and I_B.
 *
 * vsmpc_rollout_noise_draws returns what ticks tick0 .. tick0 + ticks - 1 of this rollout's loops draw, computed by the device
 * function the kernels call: z [ticks][batch][18] and, unless NULL, the generator's words [ticks][batch][9][4] (host buffers).
 * Needs noise set; runs nothing of the loop.
 */
typedef struct vsmpc_noise {
    unsigned long long seed;
    long long first_index;                                        /* global index of loop 0 of this rollout */
    double sigma_pos, sigma_lin_vel, sigma_rpy, sigma_ang_vel;    /* m, m/s, rad, rad/s */
    double sigma_force, sigma_torque;                             /* N, Nm */
} vsmpc_noise;
int vsmpc_rollout_set_noise(vsmpc_rollout* r, const vsmpc_noise* n);
int vsmpc_rollout_noise_draws(vsmpc_rollout* r, int tick0, int ticks, double* z, unsigned* words);
int vsmpc_rollout_get_state(vsmpc_rollout* r, double* state);
int vsmpc_rollout_get_records(vsmpc_rollout* r, double* records);

/*
 * Adjoint of the rollout: the gradient of a scalar loss L on the FLOWN trajectory -- on the log rows and on the final plant
 * state -- with respect to the plant state at the start of the run and to the gains, through every tick: record -> solve ->
 * first move -> plant -> next record ("Adjoint of the rollout"; executable model: tests/rollout_adjoint_model.py).
 *
 * vsmpc_rollout_run_taped does what vsmpc_rollout_run does -- same results, same log, bit for bit -- and keeps, for every tick
 * t of this run, in device memory the rollout owns: the plant state in front of the tick, the record the tick solved, the
 * solve's first move and its status, taken by device-to-device copies between the tick's launches (the ticks are launched
 * directly; the captured graph of vsmpc_rollout_run is not used and not touched).  The tape is allocated, or grown, by this
 * call: per instance and tick VSMPC_PLANT_STATE + n_in + VSMPC_FM_SIZE doubles plus one int (and VSMPC_ROLLOUT_LOG doubles
 * of staging for vsmpc_rollout_backward's log_bar), beside a few rows per instance for the sweep.  An allocation failure
 * returns VSMPC_ERR_ALLOC and leaves the rollout runnable, without a tape.  A later vsmpc_rollout_reset, _set_tree,
 * _set_tunables, _set_attitude_tracks, _set_jet_plant or untaped vsmpc_rollout_run invalidates the tape.
 * Supported: the parametric plant, and the kinematic-tree plant when the tree was set with VSMPC_TREE_ADJOINT
 * (vsmpc_rollout_set_tree_ex), both with the polynomial jet model, with or without an RPY track; with an RPYDot track when
 * the attitude tracks were set with VSMPC_ATTITUDE_ADJOINT (vsmpc_rollout_set_attitude_tracks_ex).  A rollout with a tree set
 * without VSMPC_TREE_ADJOINT (vsmpc_rollout_set_tree), with the jet plant option, or with an RPYDot track set without
 * VSMPC_ATTITUDE_ADJOINT (vsmpc_rollout_set_attitude_tracks) -- alone or beside each other -- is refused:
 * VSMPC_ERR_UNSUPPORTED_CONFIG, and vsmpc_strerror names the option.
 * On the tree plant the sweep sees the tree through tau = terms(q, T) of vsmpc_tree_jacobian_batch at the state between two
 * ticks: one launch of tree_jacobian_kernel per launch of advance_adjoint_kernel gives tau and d tau / d(q | T), and the tree
 * instantiations of the latter contract the cotangents of A_mom, Lambda and I_B with it ("Adjoint of the rollout:
 * kinematic-tree plant"; executable model: tests/rollout_tree_adjoint_model.py).  The joint selector of
 * vsmpc_set_kinematics_options is kept by value with the tape: changing it between the taped run and the sweep changes
 * nothing.  In vsmpc_rollout_backward_full's grad_params the blocks the tree plant does not read -- INERTIA_B, AMOM0, DJ --
 * are +0.0; everything else is as on the parametric plant.  The tree's own geometry (masses, origins, axes) is held fixed:
 * gradients to it are not computed.
 *
 * vsmpc_rollout_backward sweeps the tape from the last tick to the first, in stream order.  Per tick: the transpose of the plant
 * advance (advance_adjoint_kernel: the sub-steps are recomputed from the tape and run backwards) turns dL/d(state after the
 * tick), with the tick's log_bar row added, into the direct part of dL/d(state in front of it) and the cotangent of the first
 * move; the `_device` body of vsmpc_adjoint_record_batch on the taped record, with xbar = 0 and that fmbar and the rollout's
 * rows of tunables if it has any, gives dL/d(record) and the tick's dL/d(gains); the transpose of the record assembly (the
 * same kernel, in front of the previous tick's plant half) maps dL/d(record) back to the plant state and to the reference
 * window, whose cotangent (12 n_ref doubles per instance) the sweep carries: it shifts back one column at every release tick,
 * where the pushed column's h_lin entry R^T m v_ref hands its share to rpy, and ends at the first tick after a reset, where
 * every column was built with that tick's attitude.
 *   log_bar[ticks][batch][VSMPC_ROLLOUT_LOG]   dL/d(log rows of the taped run): p, rpy, T, throttle %; entries 14 and 15
 *                                              (status, iterations) are ignored.  May be NULL.
 *   state_bar[batch][VSMPC_PLANT_STATE]        dL/d(plant state after the last tick); entries 40.. are ignored.  May be NULL.
 *                                              Both NULL: VSMPC_ERR_INVALID_ARG, as is a rollout without a tape.
 *   grad_state0[batch][VSMPC_PLANT_STATE]      dL/d(plant state at the start of the taped run), entries 0..39; the jet-plant
 *                                              slots get +0.0
 *   grad_cfg[batch][VSMPC_GRAD_SIZE]           dL/d(every weight and throttle limit), summed over the ticks, in the order
 *                                              and units of VSMPC_GRAD_* (vsmpc_adjoint_batch); with rows of
 *                                              vsmpc_rollout_set_tunables every instance under its own row
 *   flags[batch]                               OR over the ticks of VSMPC_ADJ_DEGENERATE and VSMPC_ADJ_UNSOLVED
 * Every output may be NULL.  A tick whose taped status is not Solved did not consume its move: the cotangent of the move is
 * zero, the latched entries (joints, throttle, thrust references) pass straight through, VSMPC_ADJ_UNSOLVED is set.  The
 * sum over the ticks has an order fixed by the tick count alone: repeated and permuted batches are bit-identical.  Gradients
 * with respect to the plant parameters and the trajectories (the alpha track among them) are returned by
 * vsmpc_rollout_backward_full, below; the tick grid, the hold pattern and the disturbance window are structural.  Needs a
 * handle created with VSMPC_CREATE_ADJOINT_RECORD
 * (otherwise VSMPC_ERR_UNSUPPORTED_CONFIG, and vsmpc_strerror names the flag); it uses that entry's workspace, so it must
 * be ordered against the handle's other adjoint calls.
 */
int vsmpc_rollout_run_taped(vsmpc_rollout* r, int ticks, double* log, void* stream);
/* Host buffers; returns after the results are in them. */
int vsmpc_rollout_backward(vsmpc_rollout* r, const double* log_bar, const double* state_bar, double* grad_state0,
                           double* grad_cfg, int* flags, void* stream);
/* Same, all pointers are DEVICE pointers and the call only enqueues work on `stream`. */
int vsmpc_rollout_backward_device(vsmpc_rollout* r, const double* d_log_bar, const double* d_state_bar, double* d_grad_state0,
                                  double* d_grad_cfg, int* d_flags, void* stream);

/*
 * The same sweep, with the gradients to the plant parameters and to the reference trajectories beside it ("Adjoint
 * of the rollout: parameters and tracks"; executable model: tests/rollout_param_adjoint_model.py):
 *   grad_params[batch][VSMPC_PLANT_PARAMS]     dL/d(every plant parameter) of the loop, in the order of VSMPC_PP_*: mass, I_B,
 *                                              A_mom0, DJ, q_ref0, PINIT, RPYINIT, the push force and torque.  DIST_T0, DIST_T1
 *                                              and TICK0 are structural: +0.0
 *   grad_traj[batch][6 n_traj + n_alpha]       dL/d(traj_pos [n_traj][3] | traj_vel [n_traj][3] | traj_alpha [n_alpha]), in that
 *                                              order (vsmpc_rollout_traj_grad_size doubles).  The tracks are shared by all
 *                                              loops: one row per loop, the caller sums.  A sample that no window column of
 *                                              the run holds, or that no tick and no sub-step reads, is +0.0
 * Every output may be NULL; with grad_params == grad_traj == NULL the call runs exactly what vsmpc_rollout_backward runs, and
 * grad_state0, grad_cfg and flags are those of vsmpc_rollout_backward bit for bit either way.  The sums have fixed orders (no
 * atomics): repeated and permuted batches are bit-identical here too.  The derivative is taken with the tick state at the
 * start of the taped run -- the reference window and the unwrap counters -- held fixed: when the taped run begins at a reset,
 * that window is built from the tracks, PINIT, RPYINIT and the mass, and is differentiated; when it begins later, the window
 * cotangent left at its first tick is dropped, as vsmpc_rollout_backward drops it.  A tick that was not Solved contributes
 * nothing through its solve, and still through its plant half and the window.  The first call that asks for either output
 * allocates batch x (VSMPC_PLANT_PARAMS + 6 n_traj + n_alpha) doubles, kept until vsmpc_rollout_destroy; a failure returns
 * VSMPC_ERR_ALLOC and leaves the rollout and its tape usable.  Refusals as vsmpc_rollout_backward's; a rollout with a tree set
 * without VSMPC_TREE_ADJOINT, with the jet plant option, or with an RPYDot track set without VSMPC_ATTITUDE_ADJOINT is refused
 * by name (VSMPC_ERR_UNSUPPORTED_CONFIG).  With VSMPC_ATTITUDE_ADJOINT the rollout is accepted with or without an RPYDot
 * track; grad_params[INERTIA_B] and grad_state0 then hold the shares of the window columns' angular-momentum reference too.
 */
int vsmpc_rollout_backward_full(vsmpc_rollout* r, const double* log_bar, const double* state_bar, double* grad_state0,
                                double* grad_cfg, double* grad_params, double* grad_traj, int* flags, void* stream);
int vsmpc_rollout_backward_full_device(vsmpc_rollout* r, const double* d_log_bar, const double* d_state_bar, double* d_grad_state0,
                                       double* d_grad_cfg, double* d_grad_params, double* d_grad_traj, int* d_flags, void* stream);
/* 6 n_traj + n_alpha: doubles in one row of grad_traj */
int vsmpc_rollout_traj_grad_size(const vsmpc_rollout* r);

/*
 * Adjoint of the rollout: attitude tracks (the section of that name; executable model:
 * tests/rollout_attitude_adjoint_model.py).  On a rollout whose attitude tracks were set with VSMPC_ATTITUDE_ADJOINT the sweep
 * also pulls back rows 9..11 of every window column, the angular-momentum reference R I_B R^T W(roll, pitch) RPYDot[idx]
 * frozen with the attitude and the locked inertia of the tick that pushed it (I_B: the parameter block, or the tree's I_B(q)):
 * to rpy through R and W, to I_B -- grad_params[INERTIA_B] on the parametric plant, through d tau / dq to the joints on the
 * tree plant -- and to the RPYDot sample; rows 6..8, RPYINIT + RPY[idx], go to the RPY sample.  A release tick does this for
 * the column it pushed, the first tick after a reset for every column of the fill.
 *   grad_att[batch][6 n_traj]   dL/d(traj_rpy [n_traj][3] | traj_rpy_dot [n_traj][3]), in that order
 *                               (vsmpc_rollout_att_grad_size doubles), one row per loop, the caller sums.  A sample that no
 *                               window column of the run holds is +0.0.  A track that is NULL reads as zeros: its gradient is
 *                               still returned (at a zero RPYDot track it is W^T R I_B^T R^T w, not zero).
 * The other arguments and outputs are vsmpc_rollout_backward_full's; with grad_att == NULL the call runs what
 * vsmpc_rollout_backward_full runs, and the outputs the three entries share are bit-identical among them on such a rollout.
 * One lane sums a sample's columns in column order: repeated and permuted batches are bit-identical.  The first call that asks
 * for grad_att allocates batch x 6 n_traj doubles, kept until vsmpc_rollout_destroy; a failure returns VSMPC_ERR_ALLOC and
 * leaves the rollout and its tape usable.  Without VSMPC_ATTITUDE_ADJOINT: VSMPC_ERR_UNSUPPORTED_CONFIG, and vsmpc_strerror
 * names the flag.  Still refused under the flag: the jet plant option, and a tree set without VSMPC_TREE_ADJOINT.
 */
int vsmpc_rollout_backward_attitude(vsmpc_rollout* r, const double* log_bar, const double* state_bar, double* grad_state0,
                                    double* grad_cfg, double* grad_params, double* grad_traj, double* grad_att, int* flags,
                                    void* stream);
int vsmpc_rollout_backward_attitude_device(vsmpc_rollout* r, const double* d_log_bar, const double* d_state_bar,
                                           double* d_grad_state0, double* d_grad_cfg, double* d_grad_params, double* d_grad_traj,
                                           double* d_grad_att, int* d_flags, void* stream);
/* 6 n_traj: doubles in one row of grad_att */
int vsmpc_rollout_att_grad_size(const vsmpc_rollout* r);
/* New values for the rollout's tracks, of the lengths given at vsmpc_rollout_create (host; NULL keeps a track): a loop that
 * optimises the trajectory need not re-create the rollout.  Written into the device buffers the rollout already holds, which
 * the captured tick graph reads too: it is not rebuilt.  Invalidates the tape and requires vsmpc_rollout_reset before the next
 * run, like vsmpc_rollout_set_attitude_tracks. */
int vsmpc_rollout_set_trajectories(vsmpc_rollout* r, const double* traj_pos, const double* traj_vel, const double* traj_alpha);

/* Pinned host memory for the caller's in/x/first_move/status buffers (thin wrappers of hipHostMalloc / hipHostFree,
 * so that a C caller need not link the HIP runtime).  With pinned OUTPUT buffers vsmpc_solve_batch lets the kernel write
 * the results straight into them (no device-to-host copies) while the uploads of the next chunk overlap the solves of
 * the current one; with pageable buffers the runtime stages the copies itself.  Returns NULL on failure. */
void* vsmpc_alloc_host(size_t bytes);
void vsmpc_free_host(void* p);

/* How the solve kernel condenses the QP (what constraintsVSMPC.cpp:76-131 / costsVSMPC.cpp:166-200 imply once the states
 * are eliminated).  STRUCTURED (form 1; the default where the horizon has it: nIter <= 18, even controlHorizon): forward /
 * adjoint recursions on 3 generator columns per joint block + the throttle columns, O(N^2) small 3x3 work.  SYRK (form 2;
 * every horizon): the sensitivity recursion of all condensed columns + C = sum_k Y_k^T Y_k on the matrix cores.  Form 0
 * restores the horizon's default.  The two forms agree to rounding (different summation order), not bit for bit.
 * Per handle; a new handle starts with the default (or with VSMPC_FORM=structured|syrk from the environment).
 * Returns the previous setting, VSMPC_ERR_INVALID_ARG, or VSMPC_ERR_UNSUPPORTED_CONFIG (form 1 without the instantiation). */
int vsmpc_set_kernel_form(vsmpc_handle* h, int form);

/* Which kernel serves small batches.  A horizon whose shipped kernel runs two workgroups per CU (the paper horizon 17/7/12)
 * also has a SMALL-BATCH KIND of it, solve_kernel_small: when the batch does not exceed the compute units of the device a CU
 * runs one workgroup anyway, so that kind takes the LDS of a whole CU, keeps the arrays of the condensing apart from the
 * Cholesky's ring and forms most Hessian tiles beside the first two panel streams instead of in front of them.  Same
 * arithmetic per tile, same outputs bit for bit.  `mode`: 0 auto -- the small-batch kind when batch <= CU count (read from the
 * device at create) and the handle's form is structured; 1 never; 2 always where the horizon has the kind (measurements).  It
 * applies to vsmpc_solve_batch, vsmpc_solve_batch_device, vsmpc_tick, the rollout (whose captured tick graph is rebuilt when
 * the answer changes) and vsmpc_debug_phase_cycles; the per-instance-tunables entries (vsmpc_solve_batch_tuned*, a rollout
 * with tunables), the SYRK form and vsmpc_debug_condensed keep the shipped kernel.  Per handle; a new handle starts with auto
 * (or with VSMPC_SMALL_BATCH=auto|never|always from the environment).  Returns the previous setting, VSMPC_ERR_INVALID_ARG,
 * or VSMPC_ERR_UNSUPPORTED_CONFIG (mode 2 on a horizon without the kind, or on a runtime handle). */
int vsmpc_set_small_batch_kernel(vsmpc_handle* h, int mode);
/* 1 when a solve of `batch` instances on this handle runs on the small-batch kind, 0 when on the shipped kernel;
 * VSMPC_ERR_INVALID_ARG for a NULL handle or batch <= 0.  No device work. */
int vsmpc_small_batch_kernel_for(const vsmpc_handle* h, int batch);
/* Dynamic LDS (bytes) a workgroup of the small-batch kind is launched with at this horizon (at most the 160 KB of a CU), or
 * 0 when the horizon is not in the build's table or has no such kind.  No handle, no device work. */
size_t vsmpc_small_batch_lds_bytes(int n_iter, int n_iter_small, int control_horizon);

const char* vsmpc_strerror(int code);
const char* vsmpc_kernel_name(const vsmpc_handle* h);

#ifdef __cplusplus
}
#endif
#endif /* VSMPC_H */
