// TEST BUILD ONLY (tests/test_launch_plan.py): marbler_amd/csrc/launch_plan.h compiled by the host compiler alone, under
// ASan + UBSan.  Reads one launch per line on stdin --
//   scenario n_agents qp_mode num_envs side force tpe_supported span resident shapes kind gym image image_shape
// -- and prints its plan on one line, in the order of the struct's members, followed by image_wanted.
#include <stdio.h>
#include <string.h>

#include "launch_plan.h"

int main() {
    rg_scenario_params p;
    memset(&p, 0, sizeof(p));
    rg::PlanHandle h;
    rg::PlanCall c;
    int num_envs, tpe_supported, span, resident, shapes, gym, image;
    while (scanf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d", &p.scenario, &p.n_agents, &p.qp_mode, &num_envs, &h.side, &h.force,
                 &tpe_supported, &span, &resident, &shapes, &c.kind, &gym, &image, &c.image_shape) == 14) {
        h.tpe_supported = tpe_supported != 0;
        h.span = span != 0;
        h.resident = resident != 0;
        h.shapes = shapes != 0;
        c.gym = gym != 0;
        c.image = image != 0;
        const rg::LaunchPlan pl = rg::plan_launch(p, num_envs, h, c);
        printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", pl.tpe, pl.family, pl.mode, pl.kind, pl.gw, pl.nt, pl.rollout, pl.gym,
               pl.rows, pl.resident, pl.shape, pl.envs_per_wave, pl.grid, pl.form, rg::image_wanted(p, num_envs, h));
    }
    return feof(stdin) ? 0 : 2;   // a malformed line is an error
}
