// robogym_team_rollout.hip -- the team kernels (team_kernels.h) of the exact mode for rg_rollout.
#include "team_kernels.h"

namespace rg {

hipError_t launch_team_rollout(const KernelArgs &a, const rg_team_params &tp, hipStream_t stream) {
    return launch_team_group<false, true, RG_QP_EXACT>(a, tp, stream);
}

}  // namespace rg
