// robogym_kernels.hip -- instantiates the lane-group kernels (step_group.h) for one env step per launch
// (rg_step, rg_get_obs) and the explicit reset (rg_reset).
#include "step_group.h"

namespace rg {

hipError_t launch_step(const KernelArgs &a, const GroupSide &side, hipStream_t stream) {
    return launch_group<PlainFamily, false, false, RG_QP_EXACT>(a, side, stream);
}

hipError_t launch_obs(const KernelArgs &a, const GroupSide &side, hipStream_t stream) {
    return launch_group<PlainFamily, true, false, RG_QP_EXACT>(a, side, stream);
}

hipError_t launch_reset(const KernelArgs &a, hipStream_t stream) {
    return for_scenario(a.p.scenario, [&](auto scn) -> hipError_t {
        constexpr int SCN = decltype(scn)::value;
        const LaunchPlan pl = plan_launch(a.p, a.E, PlanHandle{}, PlanCall{GROUP_RESET, false, false, 0});   // (the same for every handle)
        const int gw = pl.gw, grid = pl.grid;
        if (gw == 4) hipLaunchKernelGGL((reset_kernel<SCN, 4>), dim3(grid), dim3(WAVE), 0, stream, a);
        else if constexpr (SCN != RG_SCN_ARCTIC_TRANSPORT) {
            if (gw == 8) hipLaunchKernelGGL((reset_kernel<SCN, 8>), dim3(grid), dim3(WAVE), 0, stream, a);
            else hipLaunchKernelGGL((reset_kernel<SCN, 16>), dim3(grid), dim3(WAVE), 0, stream, a);
        }
        return hipGetLastError();
    });
}

}  // namespace rg
