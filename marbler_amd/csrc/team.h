// team.h -- the team pool (rg_set_teams, include/robogym.h rg_team_params): C capability sets, one per env and episode.
// Out of parity scope by construction (the reference has no pool); every value is held to the float32 oracle loaded with the
// env's set.
//
// Spec (DESIGN.md "Team pool"): env e carries t = team_index[e] in [0, C); the step reads set t's agent_step / sensing_radius /
// capture_radius / torque ([C][N] tables, row t) wherever the plain kernels read rg_scenario_params'.  The index is drawn when
// an episode starts, from the reset sampler's stream family at a block no sampler draw reaches (team_draw below).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_common.h"

namespace rg {

// the team kernels' argument block: the step's own and the pool's, side by side (the existing kernels never see the latter)
struct TeamArgs {
    KernelArgs k;
    rg_team_params tp;
};

// LDS the team kernels add to the step's block (Lds<GW> is left as it is): MaterialTransport's partner torques for the reward
// replay, staged next to lds.aload.  Instantiated by the team kernels only (team_lds below).
struct TeamLds {
    int torque[WAVE];
};
template <int SCN, int GW>
__device__ __forceinline__ TeamLds &team_lds() {
    __shared__ TeamLds tl;
    return tl;
}

// Philox block of the team draw: far above every block the reset sampler uses (at most MAX_DRAWS / 4 = 32)
constexpr uint32_t TEAM_BLOCK = 0x80000000u;

// The team index of the episode that env ge starts with `episode` (= the reset_count value the reset sampler draws it with).
// RG_TEAM_EPISODE: (uint64(w0) * C) >> 32, w0 = word 0 of philox4x32_10((ge_lo, ge_hi, episode, 0x80000000), (seed_lo, seed_hi));
// RG_TEAM_FIXED: ge mod C.
__device__ __forceinline__ int team_draw(const rg_team_params &tp, uint64_t ge, int32_t episode, uint64_t seed) {
    const uint32_t C = static_cast<uint32_t>(tp.n_sets);
    if (tp.mode == RG_TEAM_FIXED) return static_cast<int>(ge % C);
    uint32_t blk[4];
    philox4x32_10(static_cast<uint32_t>(ge), static_cast<uint32_t>(ge >> 32), static_cast<uint32_t>(episode), TEAM_BLOCK,
                  static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32), blk);
    return static_cast<int>((static_cast<uint64_t>(blk[0]) * C) >> 32);
}

// an index as stored, clamped into the table (a caller's write outside [0, C) reads set C - 1, never past the tables)
__device__ __forceinline__ int team_clamp(int t, int C) {
    const uint32_t u = static_cast<uint32_t>(t), hi = static_cast<uint32_t>(C - 1);
    return static_cast<int>(u < hi ? u : hi);
}

}  // namespace rg
