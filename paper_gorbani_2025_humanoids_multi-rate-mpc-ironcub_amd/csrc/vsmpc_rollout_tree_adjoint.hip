// The kinematic-tree plant's instantiations of the rollout's backward sweep (vsmpc_rollout_set_tree_ex with
// VSMPC_TREE_ADJOINT): advance_adjoint_body (vsmpc_rollout_adjoint_device.hpp, where the phases and the differences are
// described) with TREE on, its kernel template and launcher in a unit of their own so that the parametric plant's kernels
// stay what they were.
// Mirror of tests/rollout_tree_adjoint_model.py.
#include "vsmpc_rollout_adjoint_device.hpp"

namespace vsmpc {

template <bool PT>
__global__ __launch_bounds__(RO_BLOCK) void advance_tree_adjoint_kernel(RolloutDev rd, RolloutAdj a) {
    advance_adjoint_body<PT, true>(rd, a);
}

hipError_t launch_advance_tree_adjoint(const RolloutDev& rd, const RolloutAdj& a, hipStream_t stream) {
    if (a.gpar != nullptr && a.gtraj != nullptr)
        hipLaunchKernelGGL(advance_tree_adjoint_kernel<true>, dim3(a.batch), dim3(RO_BLOCK), 0, stream, rd, a);
    else
        hipLaunchKernelGGL(advance_tree_adjoint_kernel<false>, dim3(a.batch), dim3(RO_BLOCK), 0, stream, rd, a);
    return hipGetLastError();
}

}  // namespace vsmpc
