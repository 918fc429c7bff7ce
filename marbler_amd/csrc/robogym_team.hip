// robogym_team.hip -- the team kernels (step_group.h) of the exact mode for one env step per launch (rg_step, plain and with
// the gymma block) and for rg_get_obs, and the index writer of rg_reset / rg_set_teams.
#include "step_group.h"

namespace rg {

hipError_t launch_team_step(const KernelArgs &a, const GroupSide &side, hipStream_t stream) {
    return launch_group<TeamFamily, false, false, RG_QP_EXACT>(a, side, stream);
}

hipError_t launch_team_obs(const KernelArgs &a, const GroupSide &side, hipStream_t stream) {
    return launch_group<TeamFamily, true, false, RG_QP_EXACT>(a, side, stream);
}

// One lane per env: the team index of the episode each (masked) env has just started -- rg_reset advanced reset_count, so that
// episode is reset_count - 1 -- or, in the fixed mode, env_offset + e mod C (rg_set_teams, mask NULL: every env).
__global__ __launch_bounds__(256) void team_index_kernel(const rg_team_params tp, const int32_t *reset_count, const uint8_t *mask,
                                                         int32_t E, int64_t env_offset, uint64_t seed) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    if (mask && !mask[e]) return;
    const int32_t episode = tp.mode == RG_TEAM_FIXED ? 0 : reset_count[e] - 1;
    tp.team_index[e] = team_draw(tp, static_cast<uint64_t>(env_offset + e), episode, seed);
}

hipError_t launch_team_index(const KernelArgs &a, const rg_team_params &tp, hipStream_t stream) {
    hipLaunchKernelGGL(team_index_kernel, dim3((a.E + 255) / 256), dim3(256), 0, stream, tp, a.st.reset_count, a.reset_mask, a.E,
                       a.env_offset, a.seed);
    return hipGetLastError();
}

}  // namespace rg
