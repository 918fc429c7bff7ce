// robogym_resident_shapes.hip -- the resident row kernels of the reference shapes (kernel_args.h RG_REF_SHAPES): the kernels of
// robogym_resident.hip again, with the shape's members of the parameter block as compile-time constants (step_group.h step_once
// SH).  A translation unit of its own with that file's flags (build.py): the preloaded leading arguments, and the compile runs
// beside the others.
#include "step_group.h"

namespace rg {

// `a`, `side` as launch_step_resident takes them; side.plan.shape: the row of the table that the image's block matched (match_shape:
// the host has compared every field the kernel assumes).  A shape this build does not hold is an error, not a fall-back.
hipError_t launch_step_shape(const KernelArgs &a, const GroupSide &side, hipStream_t stream) {
    if constexpr (kStampsBuild) {
        return hipErrorInvalidValue;   // (a stamps build has no row kernels)
    } else {
        const int grid = side.plan.grid;
        const dim3 g(grid), b(WAVE);
#define RG_X(id, scn, n, P, D, M, CA, U, PERIOD, PENALIZE)                                                                            \
    if (side.plan.shape == (id)) {                                                                                                      \
        if (a.p.scenario != (scn) || a.p.n_agents != (n)) return hipErrorInvalidValue;                                               \
        hipLaunchKernelGGL((step_kernel<scn, 8, false, n, false, 16, true, Shape<P, D, M, CA, U, PERIOD, PENALIZE>>), g, b, 0, stream, \
                           side.image, a.actions, a.seed, a.auto_reset, grid, a.io);                                                 \
        return hipGetLastError();                                                                                                    \
    }
        RG_REF_SHAPES(RG_X)
#undef RG_X
        return hipErrorInvalidValue;
    }
}

}  // namespace rg
