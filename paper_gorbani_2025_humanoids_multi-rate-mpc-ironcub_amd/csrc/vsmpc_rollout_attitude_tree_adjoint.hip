// The attitude-track instantiations of the rollout's backward sweep on the kinematic-tree plant (VSMPC_ATTITUDE_ADJOINT on a
// rollout whose tree was set with VSMPC_TREE_ADJOINT): advance_adjoint_body (vsmpc_rollout_adjoint_device.hpp) with TREE and
// ATT on -- the h_ang entries' cotangent of I_B joins tau_bar's I_B rows and goes through J to the joints -- in a unit of their
// own, as the other three families.
// Mirror of tests/rollout_attitude_adjoint_model.py (backward with a tree).
#include "vsmpc_rollout_adjoint_device.hpp"

namespace vsmpc {

template <bool PT>
__global__ __launch_bounds__(RO_BLOCK) void advance_attitude_tree_adjoint_kernel(RolloutDev rd, RolloutAdj a) {
    advance_adjoint_body<PT, true, true>(rd, a);
}

hipError_t launch_advance_attitude_tree_adjoint(const RolloutDev& rd, const RolloutAdj& a, hipStream_t stream) {
    if (a.gpar != nullptr && a.gtraj != nullptr)
        hipLaunchKernelGGL(advance_attitude_tree_adjoint_kernel<true>, dim3(a.batch), dim3(RO_BLOCK), 0, stream, rd, a);
    else
        hipLaunchKernelGGL(advance_attitude_tree_adjoint_kernel<false>, dim3(a.batch), dim3(RO_BLOCK), 0, stream, rd, a);
    return hipGetLastError();
}

}  // namespace vsmpc
