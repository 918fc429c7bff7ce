// robogym_disturb_rollout.hip -- the pose-disturbance kernels (step_group.h, disturb.h) of the exact mode for rg_rollout.
#include "step_group.h"

namespace rg {

hipError_t launch_disturb_rollout(const KernelArgs &a, const GroupSide &side, hipStream_t stream) {
    return launch_group<DisturbFamily, false, true, RG_QP_EXACT>(a, side, stream);
}

}  // namespace rg
