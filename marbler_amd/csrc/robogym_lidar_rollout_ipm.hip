// robogym_lidar_rollout_ipm.hip -- the lidar kernels (lidar_kernels.h) of the interior-point mode for rg_rollout.
#include "lidar_kernels.h"

namespace rg {

hipError_t launch_lidar_rollout_ipm(const KernelArgs &a, const rg_lidar_params &lp, hipStream_t stream) {
    return launch_lidar_group<false, true, RG_QP_CVXOPT>(a, lp, stream);
}

}  // namespace rg
