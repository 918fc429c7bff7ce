// robogym_disturb_rollout_ipm.hip -- the pose-disturbance kernels (step_group.h, disturb.h) of the interior-point mode for
// rg_rollout.
#include "step_group.h"

namespace rg {

hipError_t launch_disturb_rollout_ipm(const KernelArgs &a, const GroupSide &side, hipStream_t stream) {
    return launch_group<DisturbFamily, false, true, RG_QP_CVXOPT>(a, side, stream);
}

}  // namespace rg
