// robogym_resident.hip -- the resident form of the sixteen 16-lane-row step kernels (step_group.h, kernel_args.h ResidentCall).
// A translation unit of its own: its flags (build.py) make the leading kernel arguments preloaded ones, which would change every
// kernel they were applied to.
#include "step_group.h"

namespace rg {

void resident_image(KernelArgs &a, const LaunchPlan &plan) {
    a.io = rg_step_io{};
    a.actions = nullptr;
    a.reset_mask = nullptr;
    a.auto_reset = 0;
    a.reset_flags = 0;
    a.seed = 0;
    a.num_steps = 1;
    a.envs_per_wave = plan.envs_per_wave;
}

// `a`: the launch's block as rg_step filled it (its per-call members are the kernel's arguments); side.image: the image of the
// same handle.  The entry of a plan with `resident` and no shape (launch_plan.h).
hipError_t launch_step_resident(const KernelArgs &a, const GroupSide &side, hipStream_t stream) {
    if constexpr (kStampsBuild) {
        return hipErrorInvalidValue;   // (a stamps build has no row kernels)
    } else {
        return for_scenario(a.p.scenario, [&](auto scn) -> hipError_t {
            constexpr int SCN = decltype(scn)::value;
            if constexpr (SCN == RG_SCN_ARCTIC_TRANSPORT) {
                return hipErrorInvalidValue;
            } else {
                const int grid = side.plan.grid;
                const dim3 g(grid), b(WAVE);
                switch (side.plan.nt) {
                    case 5: hipLaunchKernelGGL((step_kernel<SCN, 8, false, 5, false, 16, true>), g, b, 0, stream, side.image, a.actions, a.seed, a.auto_reset, grid, a.io); break;
                    case 6: hipLaunchKernelGGL((step_kernel<SCN, 8, false, 6, false, 16, true>), g, b, 0, stream, side.image, a.actions, a.seed, a.auto_reset, grid, a.io); break;
                    case 7: hipLaunchKernelGGL((step_kernel<SCN, 8, false, 7, false, 16, true>), g, b, 0, stream, side.image, a.actions, a.seed, a.auto_reset, grid, a.io); break;
                    case 8: hipLaunchKernelGGL((step_kernel<SCN, 8, false, 8, false, 16, true>), g, b, 0, stream, side.image, a.actions, a.seed, a.auto_reset, grid, a.io); break;
                    default: return hipErrorInvalidValue;
                }
                return hipGetLastError();
            }
        });
    }
}

}  // namespace rg
