// robogym_policy_sample_h128.hip -- instantiates rg_policy_rollout_sample's kernels (policy_rollout.h, policy_rollout_sample_kernel)
// for hidden size 128: five scenarios x GW = 4, 8, 16 (ArcticTransport: 4).  Its own translation unit so that the builds run in parallel.
#include "policy_rollout.h"

namespace rg {

hipError_t launch_policy_rollout_sample_h128(const KernelArgs &k, const rg_actor_weights &w, const rg_policy_io &io,
                                             const rg_policy_sample &sample, int32_t T, hipStream_t stream) {
    return launch_policy_h<128, true>(k, w, io, T, stream, &sample);
}

}  // namespace rg
