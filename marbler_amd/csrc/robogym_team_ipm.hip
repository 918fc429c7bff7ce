// robogym_team_ipm.hip -- the team kernels (team_kernels.h) of the interior-point mode for one env step per launch, with that
// mode's scheduling flags (build.py FILE_FLAGS, as robogym_kernels_ipm.hip).  (rg_get_obs runs no controller: it uses the
// exact mode's observation-only kernel in either mode.)
#include "team_kernels.h"

namespace rg {

hipError_t launch_team_step_ipm(const KernelArgs &a, const rg_team_params &tp, hipStream_t stream) {
    return launch_team_group<false, false, RG_QP_CVXOPT>(a, tp, stream);
}

}  // namespace rg
