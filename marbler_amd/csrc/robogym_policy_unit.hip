// robogym_policy_unit.hip -- instantiates the kernels of rg_policy_rollout (policy_rollout.h; with -DRG_UNIT_SAMPLE=1 those of
// rg_policy_rollout_sample, policy_rollout_sample_kernel) for hidden size -DRG_UNIT_H: five scenarios x GW = 4, 8, 16
// (ArcticTransport: 4).  Compiled once per (hidden size, sampling) (build.py policy_units), so that the four compile side by side.
#include "policy_rollout.h"

#define RG_CAT_(a, b) a##b
#define RG_CAT(a, b) RG_CAT_(a, b)

namespace rg {

#if RG_UNIT_SAMPLE
hipError_t RG_CAT(launch_policy_rollout_sample_h, RG_UNIT_H)(const KernelArgs &k, const rg_actor_weights &w, const rg_policy_io &io,
                                                             const rg_policy_sample &sample, int32_t T, hipStream_t stream) {
    return launch_policy_h<RG_UNIT_H, true>(k, w, io, T, stream, &sample);
}
#else
hipError_t RG_CAT(launch_policy_rollout_h, RG_UNIT_H)(const KernelArgs &k, const rg_actor_weights &w, const rg_policy_io &io, int32_t T,
                                                      hipStream_t stream) {
    return launch_policy_h<RG_UNIT_H>(k, w, io, T, stream);
}
#endif

}  // namespace rg
