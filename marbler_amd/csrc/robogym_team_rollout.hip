// robogym_team_rollout.hip -- the team kernels (step_group.h) of the exact mode for rg_rollout.
#include "step_group.h"

namespace rg {

hipError_t launch_team_rollout(const KernelArgs &a, const GroupSide &side, hipStream_t stream) {
    return launch_group<TeamFamily, false, true, RG_QP_EXACT>(a, side, stream);
}

}  // namespace rg
