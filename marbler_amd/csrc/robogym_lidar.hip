// robogym_lidar.hip -- the lidar kernels (lidar_kernels.h) of the exact mode for one env step per launch (rg_step, plain and with
// the gymma block) and for rg_get_obs.
#include "lidar_kernels.h"

namespace rg {

hipError_t launch_lidar_step(const KernelArgs &a, const rg_lidar_params &lp, hipStream_t stream) {
    return launch_lidar_group<false, false, RG_QP_EXACT>(a, lp, stream);
}

hipError_t launch_lidar_obs(const KernelArgs &a, const rg_lidar_params &lp, hipStream_t stream) {
    return launch_lidar_group<true, false, RG_QP_EXACT>(a, lp, stream);
}

}  // namespace rg
