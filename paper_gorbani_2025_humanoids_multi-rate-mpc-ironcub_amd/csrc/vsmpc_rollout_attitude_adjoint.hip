// The attitude-track instantiations of the rollout's backward sweep on the parametric plant
// (vsmpc_rollout_set_attitude_tracks_ex with VSMPC_ATTITUDE_ADJOINT): advance_adjoint_body
// (vsmpc_rollout_adjoint_device.hpp, where the phases and the differences are described) with ATT on -- the window columns'
// h_ang entry R I_B R^T W(roll, pitch) RPYDot is pulled back to rpy, to I_B and, with PT, to the RPYDot sample, rows 6..8 to the
// RPY sample -- its kernel template and launcher in a unit of their own so that the other kernels stay what they were.
// Mirror of tests/rollout_attitude_adjoint_model.py.
#include "vsmpc_rollout_adjoint_device.hpp"

namespace vsmpc {

template <bool PT>
__global__ __launch_bounds__(RO_BLOCK) void advance_attitude_adjoint_kernel(RolloutDev rd, RolloutAdj a) {
    advance_adjoint_body<PT, false, true>(rd, a);
}

hipError_t launch_advance_attitude_adjoint(const RolloutDev& rd, const RolloutAdj& a, hipStream_t stream) {
    if (a.tree_terms != nullptr && a.tree_jac != nullptr) return launch_advance_attitude_tree_adjoint(rd, a, stream);
    if (a.gpar != nullptr && a.gtraj != nullptr)
        hipLaunchKernelGGL(advance_attitude_adjoint_kernel<true>, dim3(a.batch), dim3(RO_BLOCK), 0, stream, rd, a);
    else
        hipLaunchKernelGGL(advance_attitude_adjoint_kernel<false>, dim3(a.batch), dim3(RO_BLOCK), 0, stream, rd, a);
    return hipGetLastError();
}

}  // namespace vsmpc
