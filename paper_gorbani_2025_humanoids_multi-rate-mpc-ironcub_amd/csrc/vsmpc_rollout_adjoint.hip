// Adjoint of the closed-loop rollout (include/vsmpc.h: vsmpc_rollout_backward): the transposes of the two rollout kernels of
// vsmpc_rollout.hip, in one kernel that the backward sweep launches between the record adjoints of consecutive ticks.
//
//   advance_adjoint_kernel   second half of tick t, then first half of tick t - 1 (either may be absent):
//     record half   transpose of assemble_record at the taped state s_t: the solve adjoint's grad_in of tick t is pulled
//                   back to the plant state (X0, the errors against window column 0, R and I_G = R I_B R^T through rpy,
//                   omega through I_B^-1, A_mom and the posture error through q, Lambda = DJ T and the linearisation point
//                   through T, the previous commands) and to the reference window; then the transpose of the window FIFO:
//                   on a release tick the pushed column's h_lin entry R^T m v_ref goes to rpy and the cotangent shifts back
//                   one column; at a tick that built the window (`first`) every column's h_lin entry does.  The tick's
//                   grad_cfg and flags are accumulated here, in tick order.
//     plant half    transpose of advance_kernel at the taped (s_{t-1}, first move, status): the sub-steps are recomputed and
//                   kept in LDS, then run backwards, one state component per lane as the forward kernel runs them.  Out come
//                   the direct part of dL/ds_{t-1} and the cotangent of the first move; on a tick that was not Solved the
//                   move was not consumed: its cotangent is zero and the latched entries pass straight through.
//
//   parameters and tracks (the PT instantiation, vsmpc_rollout_backward_full): the last step of the chain rule at both halves.
//                   Record half: the record's entries that are plant parameters or are built from them (mass, I_G and omega
//                   through I_B, A_mom and Lambda through A_mom0 / DJ / q_ref0, the posture error, RPYINIT), alpha of the tick
//                   to its two track samples, and every window column at the moment its cotangent is complete -- the pushed
//                   column in front of the shift, every column at the `first` fill -- to PINIT, RPYINIT, the mass and the
//                   column's trajectory sample (position directly, velocity m R w).  Plant half, every sub-step: the mass
//                   (p' = R h_lin / m, alpha m R^T g), I_B^-1 through omega, the push where push_active holds, alpha of the
//                   sub-step to its two samples; behind the sub-steps A_mom0, DJ and q_ref0 from the cotangent of A_mom(q).
//
//   attitude tracks (the ATT instantiations, vsmpc_rollout_set_attitude_tracks_ex with VSMPC_ATTITUDE_ADJOINT): rows 6..11 of
//                   the window columns too, at the same two moments -- the h_ang entry R I_B R^T W(roll, pitch) RPYDot to rpy,
//                   to I_B and to the RPYDot sample, the RPY entry to its sample (vsmpc_rollout_attitude_adjoint.hip,
//                   vsmpc_rollout_attitude_tree_adjoint.hip: launch_advance_adjoint hands a launch with a.attitude to them).
//
// Layout: the device code is csrc/vsmpc_rollout_adjoint_device.hpp -- advance_adjoint_body<PT, TREE, ATT>, a driver over one function
// per phase (stage-in; record half: set-up, pull-back to the state, to the parameters, FIFO shift, `first` fill; plant half:
// set-up, forward sub-steps, backward sub-steps, what follows them; write-out), each with its contract above it.  This unit
// holds the parametric plant's kernel template and the launcher; vsmpc_rollout_tree_adjoint.hip holds the tree plant's.
//
// Mirror of tests/rollout_adjoint_model.py (plant_adjoint, record_adjoint) and tests/rollout_param_adjoint_model.py, which are
// checked against central differences of the forward loop model; the tree instantiations mirror
// tests/rollout_tree_adjoint_model.py.  Polynomial jet model only (the entry refuses the jet plant option).
#include "vsmpc_rollout_adjoint_device.hpp"

namespace vsmpc {

template <bool PT>
__global__ __launch_bounds__(RO_BLOCK) void advance_adjoint_kernel(RolloutDev rd, RolloutAdj a) {
    advance_adjoint_body<PT, false>(rd, a);
}

hipError_t launch_advance_adjoint(const RolloutDev& rd, const RolloutAdj& a, hipStream_t stream) {
    if (a.attitude) return launch_advance_attitude_adjoint(rd, a, stream);
    if (a.tree_terms != nullptr && a.tree_jac != nullptr) return launch_advance_tree_adjoint(rd, a, stream);
    if (a.gpar != nullptr && a.gtraj != nullptr)
        hipLaunchKernelGGL(advance_adjoint_kernel<true>, dim3(a.batch), dim3(RO_BLOCK), 0, stream, rd, a);
    else
        hipLaunchKernelGGL(advance_adjoint_kernel<false>, dim3(a.batch), dim3(RO_BLOCK), 0, stream, rd, a);
    return hipGetLastError();
}

}  // namespace vsmpc
