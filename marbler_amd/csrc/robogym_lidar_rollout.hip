// robogym_lidar_rollout.hip -- the lidar kernels (step_group.h) of the exact mode for rg_rollout.
#include "step_group.h"

namespace rg {

hipError_t launch_lidar_rollout(const KernelArgs &a, const GroupSide &side, hipStream_t stream) {
    return launch_group<LidarFamily, false, true, RG_QP_EXACT>(a, side, stream);
}

}  // namespace rg
