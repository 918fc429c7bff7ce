// robogym_lidar_ipm.hip -- the lidar kernels (step_group.h) of the interior-point mode for one env step per launch, with that
// mode's scheduling flags (build.py FILE_FLAGS, as robogym_kernels_ipm.hip).  (rg_get_obs runs no controller: it uses the
// exact mode's observation-only kernel in either mode.)
#include "step_group.h"

namespace rg {

hipError_t launch_lidar_step_ipm(const KernelArgs &a, const GroupSide &side, hipStream_t stream) {
    return launch_group<LidarFamily, false, false, RG_QP_CVXOPT>(a, side, stream);
}

}  // namespace rg
