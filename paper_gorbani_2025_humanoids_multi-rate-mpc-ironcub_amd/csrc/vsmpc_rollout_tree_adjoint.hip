// The kinematic-tree plant's instantiations of the rollout's backward sweep (vsmpc_rollout_set_tree_ex with
// VSMPC_TREE_ADJOINT): the body of advance_adjoint_kernel (vsmpc_rollout_adjoint_body.inc, where the differences are
// described) compiled with TREE on, in a unit of its own so that the parametric plant's kernels stay what they were.
// Mirror of tests/rollout_tree_adjoint_model.py.
#include "vsmpc_device.hpp"
#include "vsmpc_launch.hpp"
#include "vsmpc_rollout_device.hpp"

namespace vsmpc {

#define VS_ADJ_KERNEL advance_tree_adjoint_kernel
#define VS_ADJ_TREE true
#include "vsmpc_rollout_adjoint_body.inc"

hipError_t launch_advance_tree_adjoint(const RolloutDev& rd, const RolloutAdj& a, hipStream_t stream) {
    if (a.gpar != nullptr && a.gtraj != nullptr)
        hipLaunchKernelGGL(advance_tree_adjoint_kernel<true>, dim3(a.batch), dim3(RO_BLOCK), 0, stream, rd, a);
    else
        hipLaunchKernelGGL(advance_tree_adjoint_kernel<false>, dim3(a.batch), dim3(RO_BLOCK), 0, stream, rd, a);
    return hipGetLastError();
}

}  // namespace vsmpc
