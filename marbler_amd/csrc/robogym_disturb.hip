// robogym_disturb.hip -- the pose-disturbance kernels (step_group.h, disturb.h) of the exact mode for one env step per launch
// (rg_step, plain and with the gymma block).
#include "step_group.h"

namespace rg {

hipError_t launch_disturb_step(const KernelArgs &a, const GroupSide &side, hipStream_t stream) {
    return launch_group<DisturbFamily, false, false, RG_QP_EXACT>(a, side, stream);
}

}  // namespace rg
