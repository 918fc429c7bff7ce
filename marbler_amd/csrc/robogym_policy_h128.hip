// robogym_policy_h128.hip -- instantiates rg_policy_rollout's kernels (policy_rollout.h) for hidden size 128: five scenarios x
// GW = 4, 8, 16 (ArcticTransport: 4).  Its own translation unit so that the builds run in parallel.
#include "policy_rollout.h"

namespace rg {

hipError_t launch_policy_rollout_h128(const KernelArgs &k, const rg_actor_weights &w, const rg_policy_io &io, int32_t T, hipStream_t stream) {
    return launch_policy_h<128>(k, w, io, T, stream);
}

}  // namespace rg
