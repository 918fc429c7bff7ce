// robogym_lidar_ipm.hip -- the lidar kernels (lidar_kernels.h) of the interior-point mode for one env step per launch, with that
// mode's scheduling flags (build.py FILE_FLAGS, as robogym_kernels_ipm.hip).  (rg_get_obs runs no controller: it uses the
// exact mode's observation-only kernel in either mode.)
#include "lidar_kernels.h"

namespace rg {

hipError_t launch_lidar_step_ipm(const KernelArgs &a, const rg_lidar_params &lp, hipStream_t stream) {
    return launch_lidar_group<false, false, RG_QP_CVXOPT>(a, lp, stream);
}

}  // namespace rg
