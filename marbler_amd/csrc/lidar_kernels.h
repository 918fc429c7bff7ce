// lidar_kernels.h -- the step kernels of a handle with the lidar on (rg_set_lidar): the lane-group step (step_group.h) with the
// range block of lidar.h written at the end of its observation phase.  Generic agent count (NT = 0), every form the handle
// launches: single step (plain, and with the gymma block), multi-step rollout, observation only; exact mode for GW 4, 8, 16 and
// the interior-point mode for GW 4, 8 (ArcticTransport: GW 4).  Instantiated by robogym_lidar*.hip, one translation unit per
// (mode, launch kind) so that they compile side by side and each gets its mode's flags (build.py FILE_FLAGS).
// No thread-per-env form: with the lidar on the handle always uses these.
#pragma once
#include "step_group.h"

namespace rg {

// the kernel's argument block (its only argument, at offset 0) through an address the compiler cannot see through
template <typename T>
__device__ __forceinline__ const __attribute__((address_space(4))) T *kernarg_block() {
    typedef const __attribute__((address_space(4))) T *ArgPtr;
    ArgPtr pp = (ArgPtr)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(pp));
    return pp;
}

template <int SCN, int GW, bool OBS_ONLY, bool ROLLOUT, bool GYM, int QPM>
__global__ __launch_bounds__(WAVE) void lidar_step_kernel(const LidarArgs la) {
    __shared__ Lds<GW> lds;
    const KernelArgs &a = la.k;
    const int N = a.p.n_agents;
    if constexpr (QPM == RG_QP_CVXOPT) {
        static_assert(GW == 4 || GW == 8, "the interior-point mode admits n_agents <= 8");
        static_assert(!OBS_ONLY, "an observation-only launch runs no controller");
        using Q = ipm::GroupLds<GW>;
        __shared__ Q qp_lds;
        if constexpr (!ROLLOUT) {
            step_once<SCN, GW, false, 0, true, GYM, QPM, Q, WgSync, true>(a, lds, step_view(a, 0, N, a.p.obs_dim), &qp_lds, &la.lid);
        } else {
            for (int t = 0; t < a.num_steps; ++t) {
                if (t) __syncthreads();
                const LidarArgs &ls = *(const LidarArgs *)kernarg_block<LidarArgs>();   // (see the exact mode's loop below)
                step_once<SCN, GW, false, 0, false, false, QPM, Q, WgSync, true>(ls.k, lds, step_view(ls.k, t, N, ls.k.p.obs_dim), &qp_lds,
                                                                                 &ls.lid);
            }
        }
    } else if constexpr (!ROLLOUT) {
        step_once<SCN, GW, OBS_ONLY, 0, true, GYM, 0, void, WgSync, true>(a, lds, step_view(a, 0, N, a.p.obs_dim),
                                                                          static_cast<void *>(nullptr), &la.lid);
    } else {
        for (int t = 0; t < a.num_steps; ++t) {
            if (t) __syncthreads();
            // the argument block re-addressed every step (an opaque copy of the kernel-argument segment's address, as in
            // policy_rollout.h): left loop-invariant, the compiler hoists its loads out of the step loop and holds them across
            // the whole step -- PredatorCapturePrey GW 4: 273 VGPRs + 17 AGPRs and 148 bytes of scratch, against 169 and none
            const LidarArgs &ls = *(const LidarArgs *)kernarg_block<LidarArgs>();
            step_once<SCN, GW, false, 0, false, false, 0, void, WgSync, true>(ls.k, lds, step_view(ls.k, t, N, ls.k.p.obs_dim),
                                                                             static_cast<void *>(nullptr), &ls.lid);
        }
    }
}

template <int SCN, int GW, bool OBS_ONLY, bool ROLLOUT, int QPM>
static void launch_lidar_gw(const LidarArgs &la, int grid, hipStream_t stream) {
    if constexpr (!OBS_ONLY && !ROLLOUT) {
        if (la.k.io.elapsed) {   // gymma block
            hipLaunchKernelGGL((lidar_step_kernel<SCN, GW, false, false, true, QPM>), dim3(grid), dim3(WAVE), 0, stream, la);
            return;
        }
    }
    hipLaunchKernelGGL((lidar_step_kernel<SCN, GW, OBS_ONLY, ROLLOUT, false, QPM>), dim3(grid), dim3(WAVE), 0, stream, la);
}

// the wave filling of launch_step_scn (partly filled waves for batches that leave SIMDs idle); ArcticTransport keeps full waves
template <int SCN, bool OBS_ONLY, bool ROLLOUT, int QPM>
static hipError_t launch_lidar_scn(const LidarArgs &la_in, hipStream_t stream) {
    LidarArgs la = la_in;
    if constexpr (SCN == RG_SCN_ARCTIC_TRANSPORT) {
        launch_lidar_gw<SCN, 4, OBS_ONLY, ROLLOUT, QPM>(la, (la.k.E + 15) / 16, stream);
    } else {
        const int gw = group_width(la.k.p.n_agents);
        int epw = WAVE / gw;
        while (epw >= 2 && (la.k.E + epw / 2 - 1) / (epw / 2) <= RG_MAX_WAVES) epw /= 2;
        la.k.envs_per_wave = epw;
        const int grid = (la.k.E + epw - 1) / epw;
        if (gw == 4) launch_lidar_gw<SCN, 4, OBS_ONLY, ROLLOUT, QPM>(la, grid, stream);
        else if (gw == 8) launch_lidar_gw<SCN, 8, OBS_ONLY, ROLLOUT, QPM>(la, grid, stream);
        else if constexpr (QPM == 0) launch_lidar_gw<SCN, 16, OBS_ONLY, ROLLOUT, QPM>(la, grid, stream);
        else return hipErrorInvalidValue;   // (rg_create admits n_agents <= 8 in the interior-point mode)
    }
    return hipGetLastError();
}

template <bool OBS_ONLY, bool ROLLOUT, int QPM>
static hipError_t launch_lidar_group(const KernelArgs &a, const rg_lidar_params &lp, hipStream_t stream) {
    LidarArgs la;
    la.k = a;
    la.lid = lp;
    switch (a.p.scenario) {
        case RG_SCN_PREDATOR_CAPTURE_PREY: return launch_lidar_scn<RG_SCN_PREDATOR_CAPTURE_PREY, OBS_ONLY, ROLLOUT, QPM>(la, stream);
        case RG_SCN_WAREHOUSE: return launch_lidar_scn<RG_SCN_WAREHOUSE, OBS_ONLY, ROLLOUT, QPM>(la, stream);
        case RG_SCN_MATERIAL_TRANSPORT: return launch_lidar_scn<RG_SCN_MATERIAL_TRANSPORT, OBS_ONLY, ROLLOUT, QPM>(la, stream);
        case RG_SCN_SIMPLE: return launch_lidar_scn<RG_SCN_SIMPLE, OBS_ONLY, ROLLOUT, QPM>(la, stream);
        case RG_SCN_ARCTIC_TRANSPORT: return launch_lidar_scn<RG_SCN_ARCTIC_TRANSPORT, OBS_ONLY, ROLLOUT, QPM>(la, stream);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace rg
