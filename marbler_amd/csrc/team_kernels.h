// team_kernels.h -- the step kernels of a handle with a team pool (rg_set_teams): the lane-group step (step_group.h) reading
// every agent's capabilities from set team_index[e] of the pool (team.h), and drawing the index of every episode it starts.
// Every form the handle launches: single step (plain, and with the gymma block), multi-step rollout, observation only; exact
// mode for GW 4, 8, 16 and the interior-point mode for GW 4, 8.  The agent-count-specialised bodies of the plain kernels
// (GW 8, NT = 5..8: plain step and rollout) are kept.  Not ArcticTransport (its agent types are fixed).  Instantiated by
// robogym_team*.hip, one translation unit per (mode, launch kind), each with its mode's flags (build.py FILE_FLAGS).
// No thread-per-env form: with a pool the handle always uses these.
#pragma once
#include "lidar_kernels.h"   // kernarg_block
#include "step_group.h"

namespace rg {

template <int SCN, int GW, bool OBS_ONLY, int NT, bool ROLLOUT, bool GYM, int QPM>
__global__ __launch_bounds__(WAVE) void team_step_kernel(const TeamArgs ta) {
    __shared__ Lds<GW> lds;
    const KernelArgs &a = ta.k;
    const int N = NT > 0 ? NT : a.p.n_agents;
    if constexpr (QPM == RG_QP_CVXOPT) {
        static_assert(GW == 4 || GW == 8, "the interior-point mode admits n_agents <= 8");
        static_assert(!OBS_ONLY, "an observation-only launch runs no controller");
        using Q = ipm::GroupLds<GW>;
        __shared__ Q qp_lds;
        if constexpr (!ROLLOUT) {
            step_once<SCN, GW, false, NT, true, GYM, QPM, Q, WgSync, false, true>(a, lds, step_view(a, 0, N, a.p.obs_dim), &qp_lds,
                                                                                  nullptr, &ta.tp);
        } else {
            for (int t = 0; t < a.num_steps; ++t) {
                if (t) __syncthreads();
                const TeamArgs &ts = *(const TeamArgs *)kernarg_block<TeamArgs>();   // (see the exact mode's loop below)
                step_once<SCN, GW, false, NT, false, false, QPM, Q, WgSync, false, true>(ts.k, lds, step_view(ts.k, t, N, ts.k.p.obs_dim),
                                                                                         &qp_lds, nullptr, &ts.tp);
            }
        }
    } else if constexpr (!ROLLOUT) {
        step_once<SCN, GW, OBS_ONLY, NT, true, GYM, 0, void, WgSync, false, true>(a, lds, step_view(a, 0, N, a.p.obs_dim),
                                                                                  static_cast<void *>(nullptr), nullptr, &ta.tp);
    } else {
        for (int t = 0; t < a.num_steps; ++t) {
            if (t) __syncthreads();
            // the argument block re-addressed every step, as in lidar_kernels.h: left loop-invariant, the compiler hoists its
            // loads out of the step loop and holds them across the whole step
            const TeamArgs &ts = *(const TeamArgs *)kernarg_block<TeamArgs>();
            step_once<SCN, GW, false, NT, false, false, 0, void, WgSync, false, true>(ts.k, lds, step_view(ts.k, t, N, ts.k.p.obs_dim),
                                                                                     static_cast<void *>(nullptr), nullptr, &ts.tp);
        }
    }
}

template <int SCN, int GW, int NT, bool OBS_ONLY, bool ROLLOUT, bool GYM, int QPM>
static void launch_team_k(const TeamArgs &ta, int grid, hipStream_t stream) {
    hipLaunchKernelGGL((team_step_kernel<SCN, GW, OBS_ONLY, NT, ROLLOUT, GYM, QPM>), dim3(grid), dim3(WAVE), 0, stream, ta);
}

// the kernel choice of launch_step_scn / launch_ipm_scn (step_group.h), wave filling included
template <int SCN, bool OBS_ONLY, bool ROLLOUT, int QPM>
static hipError_t launch_team_scn(const TeamArgs &ta_in, hipStream_t stream) {
    TeamArgs ta = ta_in;
    const int n = ta.k.p.n_agents;
    const int gw = group_width(n);
    int epw = WAVE / gw;
    while (epw >= 2 && (ta.k.E + epw / 2 - 1) / (epw / 2) <= RG_MAX_WAVES) epw /= 2;
    ta.k.envs_per_wave = epw;
    const int grid = (ta.k.E + epw - 1) / epw;
    if constexpr (!OBS_ONLY && !ROLLOUT) {
        if (ta.k.io.elapsed) {   // gymma block: generic agent count, as the plain kernels
            if (gw == 4) launch_team_k<SCN, 4, 0, false, false, true, QPM>(ta, grid, stream);
            else if (gw == 8) launch_team_k<SCN, 8, 0, false, false, true, QPM>(ta, grid, stream);
            else if constexpr (QPM == 0) launch_team_k<SCN, 16, 0, false, false, true, QPM>(ta, grid, stream);
            else return hipErrorInvalidValue;
            return hipGetLastError();
        }
    }
    if constexpr (QPM == RG_QP_CVXOPT) {
        if (gw == 4) launch_team_k<SCN, 4, 0, false, ROLLOUT, false, QPM>(ta, grid, stream);
        else if (gw == 8) launch_team_k<SCN, 8, 0, false, ROLLOUT, false, QPM>(ta, grid, stream);
        else return hipErrorInvalidValue;   // (rg_create admits n_agents <= 8 in the interior-point mode)
    } else if constexpr (OBS_ONLY) {
        if (gw == 4) launch_team_k<SCN, 4, 0, true, false, false, 0>(ta, grid, stream);
        else if (gw == 8) launch_team_k<SCN, 8, 0, true, false, false, 0>(ta, grid, stream);
        else launch_team_k<SCN, 16, 0, true, false, false, 0>(ta, grid, stream);
    } else {
        if (gw == 4) launch_team_k<SCN, 4, 0, false, ROLLOUT, false, 0>(ta, grid, stream);
        else if (gw == 16) launch_team_k<SCN, 16, 0, false, ROLLOUT, false, 0>(ta, grid, stream);
        else if (n == 5) launch_team_k<SCN, 8, 5, false, ROLLOUT, false, 0>(ta, grid, stream);
        else if (n == 6) launch_team_k<SCN, 8, 6, false, ROLLOUT, false, 0>(ta, grid, stream);
        else if (n == 7) launch_team_k<SCN, 8, 7, false, ROLLOUT, false, 0>(ta, grid, stream);
        else launch_team_k<SCN, 8, 8, false, ROLLOUT, false, 0>(ta, grid, stream);
    }
    return hipGetLastError();
}

template <bool OBS_ONLY, bool ROLLOUT, int QPM>
static hipError_t launch_team_group(const KernelArgs &a, const rg_team_params &tp, hipStream_t stream) {
    TeamArgs ta;
    ta.k = a;
    ta.tp = tp;
    switch (a.p.scenario) {
        case RG_SCN_PREDATOR_CAPTURE_PREY: return launch_team_scn<RG_SCN_PREDATOR_CAPTURE_PREY, OBS_ONLY, ROLLOUT, QPM>(ta, stream);
        case RG_SCN_WAREHOUSE: return launch_team_scn<RG_SCN_WAREHOUSE, OBS_ONLY, ROLLOUT, QPM>(ta, stream);
        case RG_SCN_MATERIAL_TRANSPORT: return launch_team_scn<RG_SCN_MATERIAL_TRANSPORT, OBS_ONLY, ROLLOUT, QPM>(ta, stream);
        case RG_SCN_SIMPLE: return launch_team_scn<RG_SCN_SIMPLE, OBS_ONLY, ROLLOUT, QPM>(ta, stream);
        default: return hipErrorInvalidValue;   // ArcticTransport: refused by rg_set_teams
    }
}

}  // namespace rg
