// robogym_group_unit.hip -- one translation unit of the lane-group step kernels (step_group.h): the entries of the rows of
// kernel_args.h RG_GROUP_ENTRIES that the build hands it, -DRG_UNIT_ROWS="X(entry, family, mode, kind) ..." (build.py
// group_units: a family's single launches of one solver mode are a unit, its rollout is another, so that they compile side by
// side, each with its mode's flags).  An entry is launch_group of its row and nothing else.
#include <tuple>

#include "step_group.h"

namespace rg {

using Families = std::tuple<PlainFamily, LidarFamily, TeamFamily, DisturbFamily>;   // by GroupFamily (launch_plan.h)

#define X(entry, family, mode, kind)                                                                     \
    hipError_t entry(const KernelArgs &a, const GroupSide &side, hipStream_t stream) {                   \
        return launch_group<std::tuple_element_t<family, Families>, kind == GROUP_OBS, kind == GROUP_ROLLOUT, mode>(a, side, stream); \
    }
RG_UNIT_ROWS
#undef X

}  // namespace rg
