// robogym_lidar.hip -- the lidar kernels (step_group.h) of the exact mode for one env step per launch (rg_step, plain and with
// the gymma block) and for rg_get_obs.
#include "step_group.h"

namespace rg {

hipError_t launch_lidar_step(const KernelArgs &a, const GroupSide &side, hipStream_t stream) {
    return launch_group<LidarFamily, false, false, RG_QP_EXACT>(a, side, stream);
}

hipError_t launch_lidar_obs(const KernelArgs &a, const GroupSide &side, hipStream_t stream) {
    return launch_group<LidarFamily, true, false, RG_QP_EXACT>(a, side, stream);
}

}  // namespace rg
