// launch_plan.h -- which kernel a launch of the env runs, at what grid, in which form: decided HERE and nowhere else.
//
// Plain host C++ (no HIP runtime call, no device code: a host compiler builds it alone, tests/sanitize/plan_host.cpp does).
// plan_launch() is a pure function of the parameter block, the batch size, the handle's switches and the call; robogym_capi.hip
// computes a plan per launch and everything behind it -- the entry it selects, the dispatcher of step_group.h, the resident
// launchers, rg_step_form -- reads that one struct and derives nothing.  Every form of every kernel gives word-for-word identical
// results, so no output test can see a wrong choice here: tests/test_launch_plan.py enumerates this function instead.
#pragma once
#include <stdint.h>

#include "../../include/robogym.h"
#include "probes/diag.h"

namespace rg {

constexpr int WAVE = 64;

// The lane-group step kernels (step_group.h) come in four families -- plain, with the lidar block (rg_set_lidar), with a team
// pool (rg_set_teams), with the pose disturbance (rg_set_disturbance); a handle has at most one side block on, and "which one"
// is said with the family's name (GROUP_PLAIN: none).  The launch kinds: GROUP_STEP, GROUP_ROLLOUT, GROUP_OBS and GROUP_RESET are
// what a call asks for; GROUP_STEP_RESIDENT and GROUP_STEP_SHAPE are the plan's own answer to GROUP_STEP (kernel_args.h).
enum GroupFamily { GROUP_PLAIN, GROUP_LIDAR, GROUP_TEAM, GROUP_DISTURB };
enum GroupKind { GROUP_STEP, GROUP_ROLLOUT, GROUP_OBS, GROUP_STEP_RESIDENT, GROUP_STEP_SHAPE, GROUP_RESET };

// lanes per env of the lane-group kernels (ArcticTransport has exactly 4 agents, which rg_create enforces: GW 4)
inline int group_width(int N) { return N <= 4 ? 4 : N <= 8 ? 8 : 16; }

// A batch that leaves SIMDs idle with full wavefronts runs with partly filled ones instead (more
// waves, each carrying fewer envs, as long as there is at most one wave per SIMD: 1024): a wave's
// time is the maximum over its envs (QP sweeps, replays, resets), and the idle SIMDs are free.
// (A stamps build keeps full waves: its eight slots are the wave's first eight envs.)
struct WaveFill {
    int epw, grid;   // env slots used per wave, waves
};
inline int waves_for(int E, int epw) { return (E - 1) / epw + 1; }   // E >= 1 (rg_create); no overflow near INT32_MAX
inline WaveFill wave_fill(int E, int gw) {
    int epw = WAVE / gw;
    if constexpr (!kStampsBuild) {
        while (epw >= 2 && waves_for(E, epw / 2) <= RG_MAX_WAVES) epw /= 2;
    }
    return {epw, waves_for(E, epw)};
}

// Which step kernel: both give identical results.  The lane-group kernel has the shorter chain for
// small batches and is linear in the batch; the thread-per-env kernel's time is a step function of how many
// generations of wavefronts the batch needs (65 536 envs per generation and wave slot per SIMD), so it takes
// over where one of its steps undercuts the line.  Measured cross-overs on MI355X, final kernels of round 3
// (tools/crossover_probe.py, profiles/r3_crossover_probe.txt): the sparse collision pre-test made
// the lane-group kernel 5-8 % faster at these batch sizes and moved every threshold up from round 2's 53 248 / 65 536;
// the one-division restart of the barrier QP then favoured the lane-group kernel at N = 6, where the thread-per-env kernel
// runs on spilled registers, and compiling the thread-per-env files without the SLP vectoriser (build.py FILE_FLAGS: 57 fewer
// spilled values at N = 6, -22 %) gave most of that back: the table below is the last measurement of round 3.
// For N >= 7 the per-lane register footprint (28 pairs) leaves one wave per SIMD and the lane-group kernel -- at
// 92 % VALU issue there -- stays ahead at every batch size.  RG_STEP_KERNEL=group|tpe forces one (tests, profiling).
inline int32_t tpe_min_envs(const rg_scenario_params &p) {
    const bool mt = p.scenario == RG_SCN_MATERIAL_TRANSPORT, pcp = p.scenario == RG_SCN_PREDATOR_CAPTURE_PREY;
    // RG_QP_CVXOPT: the launch is the interior-point iteration, one wave per SIMD in either kernel.  A lane group carries one env
    // through it in ~0.7 x the time a single lane needs, a wavefront of lanes carries eight times as many: the lane-group kernel
    // while its waves fit the chip at once (8 192 envs), the other one from the second generation on.  Measured ladder, round 5
    // (tools/ipm_probe.py --cross, profiles/r5_ipm_crossover.jsonl): N = 5  8 192 envs 166 vs 211 us, 16 384 290 vs 215;
    // N = 4  16 384 95 vs 95, 24 576 157 vs 99; at 65 536 x 5 981 vs 260 us.
    if (p.qp_mode == RG_QP_CVXOPT) return p.n_agents == 5 ? 12288 : 20480;
    switch (p.n_agents) {
        case 2: return 65536;
        case 3: return pcp ? 98304 : 65536;
        case 4: return p.scenario == RG_SCN_SIMPLE ? 393216 : p.scenario == RG_SCN_ARCTIC_TRANSPORT ? 131072 : 196608;
        case 5: return mt ? 49152 : 65536;
        case 6: return mt ? 65536 : p.scenario == RG_SCN_WAREHOUSE ? 262144 : pcp ? 98304 : 131072;
        default: return INT32_MAX;
    }
}

// What a handle contributes, fixed between two calls of rg_create / rg_set_*: the side block that is on, and the environment
// switches as rg_create read them (`resident` and `shapes` already folded with "this build has the entry").
enum KernelForce { KERNEL_DEFAULT, KERNEL_GROUP, KERNEL_TPE };   // RG_STEP_KERNEL unset | group | tpe
struct PlanHandle {
    int side;             // GroupFamily of the side block that is on (GROUP_PLAIN: none)
    int force;            // KernelForce
    bool tpe_supported;   // the thread-per-env kernel exists for this parameter block (step_tpe.h)
    bool span;            // RG_STEP_SPAN: an env may take a 16-lane row
    bool resident;        // RG_STEP_RESIDENT
    bool shapes;          // RG_STEP_SHAPE
};
// What a call contributes: what it asks for, and the handle's image at this moment.
struct PlanCall {
    int kind;          // GROUP_STEP, GROUP_ROLLOUT, GROUP_OBS or GROUP_RESET
    bool gym;          // a step whose io carries the gymma block
    bool image;        // the handle has a valid resident image
    int image_shape;   // the reference shape that image's block matched (kernel_args.h match_shape), or 0
};

// The launch, named completely.
struct LaunchPlan {
    bool tpe;             // the thread-per-env kernel (step and rollout of a handle without side block): nothing below applies
    int family, mode;     // the RG_GROUP_ENTRIES row ...
    int kind;             // ... with GROUP_STEP_RESIDENT / GROUP_STEP_SHAPE where the step takes the resident form
    int gw, nt;           // lanes per env; the agent count the body is specialised for (0: generic)
    bool rollout, gym;
    bool rows;            // one env per 16-lane row (step_group.h step_once SPAN)
    bool resident;        // ... reading the handle's image
    int shape;            // ... with this reference shape compiled in (0: none)
    int envs_per_wave;    // KernelArgs::envs_per_wave exactly as the kernel is to see it (0: every slot of the wave)
    int grid;
    int form;             // RG_FORM_* (rg_step_form)
};

inline LaunchPlan plan_launch(const rg_scenario_params &p, int num_envs, const PlanHandle &h, const PlanCall &c) {
    LaunchPlan pl = {};
    const bool step = c.kind == GROUP_STEP, rollout = c.kind == GROUP_ROLLOUT, controller = step || rollout;
    pl.kind = c.kind;
    pl.rollout = rollout;
    pl.gym = step && c.gym;
    pl.form = RG_FORM_BY_VALUE;
    // the side blocks are built into the lane-group kernels only; rg_get_obs and rg_reset have no thread-per-env form
    pl.tpe = controller && h.side == GROUP_PLAIN && h.tpe_supported &&
             (h.force == KERNEL_TPE || (h.force == KERNEL_DEFAULT && num_envs >= tpe_min_envs(p)));
    if (pl.tpe) return pl;
    // an observation-only launch runs no controller and uses the exact mode's kernel in either mode, and displaces nothing: a
    // disturbed handle's is the plain family's; the explicit reset is one kernel for every handle
    pl.family = c.kind == GROUP_RESET || (c.kind == GROUP_OBS && h.side == GROUP_DISTURB) ? GROUP_PLAIN : h.side;
    pl.mode = controller ? p.qp_mode : RG_QP_EXACT;
    pl.gw = group_width(p.n_agents);
    // ArcticTransport and the reset kernel: full waves
    const bool full = p.scenario == RG_SCN_ARCTIC_TRANSPORT || c.kind == GROUP_RESET;
    const WaveFill wf = full ? WaveFill{WAVE / pl.gw, waves_for(num_envs, WAVE / pl.gw)} : wave_fill(num_envs, pl.gw);
    pl.envs_per_wave = full || kStampsBuild ? 0 : wf.epw;
    pl.grid = wf.grid;
    // bodies specialised for the agent count: GW 8 of the exact mode's step and rollout in the plain and team families.  The gymma
    // block's, the observation-only, the interior-point and every lidar and disturbance kernel are generic.
    const bool by_n = pl.gw == 8 && pl.mode == RG_QP_EXACT && controller && !pl.gym && (pl.family == GROUP_PLAIN || pl.family == GROUP_TEAM);
    pl.nt = by_n ? p.n_agents : 0;
    // at most 4 envs per wave (batches up to 4096 envs): each env on a 16-lane row, the upper half a replica that takes over part
    // of the order-free work -- the plain family's single step among the kernels above (a stamps build has no row kernels)
    pl.rows = by_n && step && pl.family == GROUP_PLAIN && h.span && wf.epw <= 4 && !kStampsBuild;
    // ... in the resident form where the handle has an image, with the shape that image's block matched
    pl.resident = pl.rows && h.resident && c.image;
    pl.shape = pl.resident && h.shapes ? c.image_shape : 0;
    if (pl.resident) {
        pl.kind = pl.shape ? GROUP_STEP_SHAPE : GROUP_STEP_RESIDENT;
        pl.form = pl.shape ? RG_FORM_SHAPE + pl.shape : RG_FORM_RESIDENT;
    }
    return pl;
}

// does the handle want a resident image?  Exactly where its plain single step takes rows.
inline bool image_wanted(const rg_scenario_params &p, int num_envs, const PlanHandle &h) {
    return plan_launch(p, num_envs, h, PlanCall{GROUP_STEP, false, false, 0}).rows;
}

}  // namespace rg
