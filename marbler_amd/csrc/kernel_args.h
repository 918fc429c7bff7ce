// kernel_args.h -- the one argument block of every launch (host <-> device contract).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/robogym.h"
#include "launch_plan.h"

namespace rg {

// Scalars derived from the parameter block, computed ONCE on the host (rg_create) in binary32 with
// the same expressions the CPU oracle uses (IEEE +,-,*,/,sqrt: identical on x86 SSE and gfx950;
// this translation unit is compiled with -ffp-contract=off on both sides).
struct Consts {
    float dt, pd, inv_pd, r2, wlim, vmax, wmax, pvl, bml;
    float xmin, xmax, ymin, ymax, coll_off, coll_lim2;
    float thr_pre;         // collision pre-test: threshold on the squared distance of the binary16-rounded points
    float lin_pre;         // the same threshold as a distance (collision limit + rounding bound): the sparse pre-test widens it by travel
    float xc, xh, yc, yh;  // boundary pre-test: arena centre and half extents
};

// Conservative pre-tests of _validate (roboEnv.py:82-94).  The exact float tests run only when a
// pre-test fires; a pre-test may fire needlessly but never misses:
//  * collision: the collision points are rounded toward zero to binary16 pairs.  For |coordinate| <
//    2^(m+1) m the spacing is 2^(m-10) m, so each rounded coordinate is off by less than that, their
//    packed difference by less than twice that plus its own rounding (<= 2^-14 m below 0.25 m), and the
//    distance by sqrt(2) times the per-axis error; `pre_margin` is that bound with 5 % on top.
//  * boundary: a robot moves at most |dt v| (1 + 1e-6) per sub-step, so all pre-update positions of a
//    chunk of C sub-steps lie within (C-1) |dt v| of the first; the test is |x - xc| + margin > xh.
//  * sparse collision pre-test (lane-group kernel): inside a controller period a robot's collision point moves at
//    most m = (|dt v| + coll_off |dt w|)(1 + 1e-5) per sub-step (the body's Euler step, plus the chord of the heading
//    change times the offset), so |f_i(u) - f_j(u)| >= |f_i(u0) - f_j(u0)| - 2 (u - u0) max(m): one test of sub-step u0
//    against lin_pre + 2 span max(m) stands for sub-steps u0 .. u0 + span.  Valid while the widened threshold stays
//    below 0.24 m (the binary16 difference is then below 0.25 m per axis, where its own rounding is <= 2^-14 m).
// WHERE "never misses" holds.  The collision bound is computed for collision points within the arena's largest |coordinate|
// plus 0.25 m (make_consts below) and for the constants rg_create admits (include/robogym.h, rps constants): arena corners within
// 100 m of the origin, collision limits up to 1 m, |collision_offset| + |dt v| <= 0.25 m -- so a robot inside the arena, or one
// sub-step beyond a wall, has its collision point inside that range.  Over that domain tests/test_physical_regimes.py emulates
// the rounding and finds the figure below thr_pre with about half the margin to spare.  A robot FARTHER out can only have been
// put there (rg_bind_state, a restored snapshot: poses are state, not parameters): at |x| >= 4 m the default arena's bound is
// already too small, near 1000 m a robot shares a binary16 cell with a ghost point, beyond 65504 m every point rounds to the
// same one.  Such a robot is outside the arena when the step begins, so the boundary pre-test fires, the step's first chunk
// reaches the exact replay, and the boundary test ends the env in the step's FIRST sub-step.  That sub-step is the only one in
// which the binary16 figure can be wrong, and the lane-group kernel's replay runs its exact pair rounds there whenever a robot
// of the wave is outside the arena, whatever the figure says (step_group.h).  Every later sub-step keeps consulting the figure
// (which sub-steps need pair rounds), and that rests on the domain rule above: a robot that WALKS out is tested one sub-step
// past the wall, |collision_offset| + |dt v| <= 0.25 m from the arena, where the bound still holds, and its env ends there.
// The thread-per-env kernel's replay runs the whole exact test anyway.  A needless replay is all a far robot otherwise costs.
constexpr float PRE_SLACK = 2e-6f;  // roundings of the position updates and of xc / xh
inline float pre_margin(float max_abs_coordinate) {
    float spacing = 0.0009765625f;  // 2^-10: binary16 spacing in [1, 2)
    for (float lim = 2.0f; lim <= max_abs_coordinate && lim < 1024.0f; lim *= 2.0f) spacing *= 2.0f;
    return 1.05f * 1.41421356f * (2.0f * spacing + 6.103515625e-05f);
}

inline Consts make_consts(const rg_scenario_params &p) {
    Consts k;
    k.dt = p.time_step;
    k.pd = p.projection_distance;
    k.inv_pd = 1.0f / p.projection_distance;
    k.r2 = p.safety_radius * p.safety_radius;
    k.wlim = p.angular_velocity_limit;
    k.vmax = p.max_linear_velocity;
    k.wmax = 2.0f * (p.wheel_radius / p.robot_diameter) * (p.max_linear_velocity / p.wheel_radius);
    k.pvl = p.position_velocity_limit;
    k.bml = p.barrier_magnitude_limit;
    k.xmin = p.bound_x0;
    k.ymin = p.bound_y0;
    k.xmax = p.bound_x0 + p.bound_w;
    k.ymax = p.bound_y0 + p.bound_h;
    const bool off = p.collision_variant == RG_COLLISION_OFFSET;
    k.coll_off = off ? p.collision_offset : 0.0f;
    const float lim = off ? p.collision_diameter : p.robot_diameter;
    k.coll_lim2 = lim * lim;
    const float ax = fmaxf(fabsf(k.xmin), fabsf(k.xmax)), ay = fmaxf(fabsf(k.ymin), fabsf(k.ymax));
    const float lp = lim + pre_margin(fmaxf(ax, ay) + 0.25f);  // robots that left the arena fire the boundary test
    k.thr_pre = lp * lp * 1.00001f;
    k.lin_pre = lp;
    k.xc = 0.5f * (k.xmin + k.xmax);
    k.xh = 0.5f * (k.xmax - k.xmin);
    k.yc = 0.5f * (k.ymin + k.ymax);
    k.yh = 0.5f * (k.ymax - k.ymin);
    return k;
}

struct KernelArgs {
    rg_scenario_params p;
    Consts k;
    rg_state st;
    rg_step_io io;
    const int32_t *actions;
    const uint8_t *reset_mask;
    int32_t E;
    int32_t envs_per_wave; // lane-group kernel: env slots used per wavefront (0 = all 64/GW); set from LaunchPlan::envs_per_wave (launch_plan.h)
    int32_t num_steps;  // env steps per launch (rg_step: 1); io and actions carry a leading dimension of this size
    int32_t auto_reset;
    int32_t reset_flags;  // rg_reset: RG_RESET_*
    int32_t next_stride;  // floats per env of st.next_init (0 = the precomputed-reset blocks are not in use)
    int64_t env_offset;
    uint64_t seed;
};

// floats per env of rg_state.next_init: poses [3N] | prey [2P] / zone loads [2] / terrain [24] + goal column, rounded up to 4
inline int next_init_stride(const rg_scenario_params &p) {
    int w = 3 * p.n_agents;
    if (p.scenario == RG_SCN_PREDATOR_CAPTURE_PREY || p.scenario == RG_SCN_SIMPLE) w += 2 * p.num_prey;
    else if (p.scenario == RG_SCN_MATERIAL_TRANSPORT) w += 2;
    else if (p.scenario == RG_SCN_ARCTIC_TRANSPORT) w += 25;
    return (w + 3) & ~3;
}

// f(std::integral_constant<int, SCN>()) for the scenario id `scn`: where a launch turns the scenario into a template argument
template <typename F>
inline hipError_t for_scenario(int scn, F &&f) {
    switch (scn) {
        case RG_SCN_PREDATOR_CAPTURE_PREY: return f(std::integral_constant<int, RG_SCN_PREDATOR_CAPTURE_PREY>());
        case RG_SCN_WAREHOUSE: return f(std::integral_constant<int, RG_SCN_WAREHOUSE>());
        case RG_SCN_MATERIAL_TRANSPORT: return f(std::integral_constant<int, RG_SCN_MATERIAL_TRANSPORT>());
        case RG_SCN_SIMPLE: return f(std::integral_constant<int, RG_SCN_SIMPLE>());
        case RG_SCN_ARCTIC_TRANSPORT: return f(std::integral_constant<int, RG_SCN_ARCTIC_TRANSPORT>());
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_reset(const KernelArgs &a, hipStream_t stream);

// The lane-group step kernels (step_group.h) come in four families -- plain, with the lidar block (rg_set_lidar), with a team
// pool (rg_set_teams), with the pose disturbance (rg_set_disturbance) -- and every (family, solver mode, launch kind) has ONE entry.
// The list: X(entry, family, qp_mode, kind).  The build reads it too (build.py group_units): a family's single launches of a mode
// and its rollout are a translation unit each, compiled from robogym_group_unit.hip side by side, each with its mode's flags.
// An observation-only launch (rg_get_obs) runs no controller: it exists in the exact mode only and serves both.  The disturbance
// family has none: rg_get_obs displaces nothing, and a disturbed handle's goes to the plain entry.  (GroupFamily, GroupKind and
// the plan that selects a row: launch_plan.h.)
#define RG_GROUP_ENTRIES(X)                                              \
    X(launch_step, GROUP_PLAIN, RG_QP_EXACT, GROUP_STEP)                 \
    X(launch_step_resident, GROUP_PLAIN, RG_QP_EXACT, GROUP_STEP_RESIDENT) \
    X(launch_step_shape, GROUP_PLAIN, RG_QP_EXACT, GROUP_STEP_SHAPE)     \
    X(launch_obs, GROUP_PLAIN, RG_QP_EXACT, GROUP_OBS)                   \
    X(launch_rollout, GROUP_PLAIN, RG_QP_EXACT, GROUP_ROLLOUT)           \
    X(launch_step_ipm, GROUP_PLAIN, RG_QP_CVXOPT, GROUP_STEP)            \
    X(launch_rollout_ipm, GROUP_PLAIN, RG_QP_CVXOPT, GROUP_ROLLOUT)      \
    X(launch_lidar_step, GROUP_LIDAR, RG_QP_EXACT, GROUP_STEP)           \
    X(launch_lidar_obs, GROUP_LIDAR, RG_QP_EXACT, GROUP_OBS)             \
    X(launch_lidar_rollout, GROUP_LIDAR, RG_QP_EXACT, GROUP_ROLLOUT)     \
    X(launch_lidar_step_ipm, GROUP_LIDAR, RG_QP_CVXOPT, GROUP_STEP)      \
    X(launch_lidar_rollout_ipm, GROUP_LIDAR, RG_QP_CVXOPT, GROUP_ROLLOUT) \
    X(launch_team_step, GROUP_TEAM, RG_QP_EXACT, GROUP_STEP)             \
    X(launch_team_obs, GROUP_TEAM, RG_QP_EXACT, GROUP_OBS)               \
    X(launch_team_rollout, GROUP_TEAM, RG_QP_EXACT, GROUP_ROLLOUT)       \
    X(launch_team_step_ipm, GROUP_TEAM, RG_QP_CVXOPT, GROUP_STEP)        \
    X(launch_team_rollout_ipm, GROUP_TEAM, RG_QP_CVXOPT, GROUP_ROLLOUT)  \
    X(launch_disturb_step, GROUP_DISTURB, RG_QP_EXACT, GROUP_STEP)       \
    X(launch_disturb_rollout, GROUP_DISTURB, RG_QP_EXACT, GROUP_ROLLOUT) \
    X(launch_disturb_step_ipm, GROUP_DISTURB, RG_QP_CVXOPT, GROUP_STEP)  \
    X(launch_disturb_rollout_ipm, GROUP_DISTURB, RG_QP_CVXOPT, GROUP_ROLLOUT)
// what a family's kernels take next to the KernelArgs: the handle's lidar and pool blocks and its disturbance scales (the plain
// family reads none of them)
// the disturbance's two scales (disturb.h: k of sigma_xy and of sigma_theta), computed once by rg_set_disturbance in binary64:
// k = binary32(double(sigma) * sqrt(3.0 / 1048575.0)) -- the variates' own standard deviation is sqrt((2^20 - 1) / 3)
struct DisturbScale {
    float k_xy, k_theta;
};
inline float disturb_scale(float sigma) { return static_cast<float>(static_cast<double>(sigma) * sqrt(3.0 / 1048575.0)); }
struct GroupSide {
    const rg_lidar_params *lidar;
    const rg_team_params *teams;
    const DisturbScale *disturb;
    const struct KernelArgs *image;   // the handle's resident image on the device (below), or null; read where plan.resident
    const LaunchPlan &plan;           // the launch as plan_launch named it (launch_plan.h): every launcher reads it and derives nothing
};

// The resident form of the 16-lane-row step kernels (robogym_resident.hip).  What rg_create / rg_bind_state fix -- p, k, st, E,
// envs_per_wave as the plan names it, next_stride, env_offset -- lies in an IMAGE of the block in device memory that the
// handle owns, written where one of them changes and never again once a launch may read it (a change takes a fresh slot), and
// the kernel takes the image's address and the per-call arguments alone: 136 bytes of kernel arguments instead of 0.8 KB, the
// leading ones handed over in scalar registers (build.py RESIDENT_PRELOAD).  GROUP_STEP_RESIDENT is the plan's own kind
// (launch_plan.h: rows, and the handle has an image); no call asks for it.
struct ResidentCall {   // the kernel-argument segment of a resident kernel (its parameters in this order)
    const KernelArgs *image;
    const int32_t *actions;
    uint64_t seed;
    int32_t auto_reset;
    int32_t grid;   // the launch's grid (behind a by-value struct the hidden grid size is not among the preloaded arguments)
    rg_step_io io;
};
static_assert(sizeof(ResidentCall) <= 256, "the per-call arguments fit one register of dwords (device_common.h load_arg_regs_resident)");
// the image of a handle's block: the per-call members cleared, envs_per_wave as the handle's plain single step's plan names it
void resident_image(KernelArgs &a, const LaunchPlan &plan);

// SHAPES.  Seven members of the parameter block are fixed by rg_create for the handle's life, yet a kernel that reads them at run
// time pays for the question on every launch: loops with clamps over the prey and the neighbour rows, both observation formats,
// the staging paths of more than 8 prey, the sub-step loop's bookkeeping.  A Shape names them as compile-time constants, the way
// NT names the agent count; -1 = read at run time (NoShape: every kernel but the ones below).  P num_prey, D obs_dim,
// M num_neighbors, CA capability_aware != 0, U update_frequency, PERIOD controller_period, PENALIZE penalize_violations != 0.
template <int P_, int D_, int M_, int CA_, int U_, int PERIOD_, int PENALIZE_>
struct Shape {
    static constexpr int P = P_, D = D_, M = M_, CA = CA_, U = U_, PERIOD = PERIOD_, PENALIZE = PENALIZE_;
};
using NoShape = Shape<-1, -1, -1, -1, -1, -1, -1>;
// The reference shapes -- the configurations of bench.py's bench_overrides(), values from configs/*.yaml through params.py --
// in ONE table that the kernels (robogym_resident_shapes.hip), the dispatcher (match_shape below) and the tests (rg_shape_info)
// all read: X(id, scenario, n_agents, P, D, M, CA, U, PERIOD, PENALIZE).  A field the scenario's kernel never reads stays -1.
// Each row is a kernel to build and keep correct: no further ones.  Ids start at 1 (0 = no shape).
// RG_SHAPE_FIELDS (A/B builds, listed in probes/diag.h): bit i clear = the table's field i stays a run-time value.
#ifndef RG_SHAPE_FIELDS
#define RG_SHAPE_FIELDS 127
#endif
#define RG_SF(bit, v) ((RG_SHAPE_FIELDS >> (bit)) & 1 ? (v) : -1)
#define RG_REF_SHAPES(X)                                                                                                      \
    X(1, RG_SCN_PREDATOR_CAPTURE_PREY, 5, RG_SF(0, 6), RG_SF(1, 16), RG_SF(2, 3), RG_SF(3, 0), RG_SF(4, 29), RG_SF(5, 15), RG_SF(6, 1)) \
    X(2, RG_SCN_WAREHOUSE, 8, -1, RG_SF(1, 18), RG_SF(2, 5), -1, RG_SF(4, 29), RG_SF(5, 15), RG_SF(6, 1))                               \
    X(3, RG_SCN_MATERIAL_TRANSPORT, 6, -1, RG_SF(1, 9), -1, RG_SF(3, 0), RG_SF(4, 74), RG_SF(5, 15), RG_SF(6, 1))
// The shape of a parameter block, or 0: scenario and agent count, and EXACTLY every field the shape compiles in (the two flags
// as the kernel reads them: zero or not).  The one place that decides; plain host code (the tests call it without a GPU).
inline int match_shape(const rg_scenario_params &p) {
#define RG_X(id, scn, n, P, D, M, CA, U, PERIOD, PENALIZE)                                                                       \
    if (p.scenario == (scn) && p.n_agents == (n) && ((P) < 0 || p.num_prey == (P)) && ((D) < 0 || p.obs_dim == (D)) &&            \
        ((M) < 0 || p.num_neighbors == (M)) && ((CA) < 0 || (p.capability_aware != 0) == ((CA) != 0)) &&                          \
        ((U) < 0 || p.update_frequency == (U)) && ((PERIOD) < 0 || p.controller_period == (PERIOD)) &&                           \
        ((PENALIZE) < 0 || (p.penalize_violations != 0) == ((PENALIZE) != 0)))                                                   \
        return id;
    RG_REF_SHAPES(RG_X)
#undef RG_X
    return 0;
}
// row `id` of the table as ten ints (id, scenario, n_agents, then the seven fields); false: no such row
inline bool shape_row(int id, int32_t out[10]) {
#define RG_X(i, scn, n, P, D, M, CA, U, PERIOD, PENALIZE)                          \
    if (id == (i)) {                                                               \
        const int32_t r[10] = {i, scn, n, P, D, M, CA, U, PERIOD, PENALIZE};       \
        for (int c = 0; c < 10; ++c) out[c] = r[c];                                \
        return true;                                                               \
    }
    RG_REF_SHAPES(RG_X)
#undef RG_X
    return false;
}
// (the resident launch of shape plan.shape: launch_step_shape, robogym_resident_shapes.hip; GROUP_STEP_SHAPE is the plan's own
// kind, like GROUP_STEP_RESIDENT)
typedef hipError_t GroupLaunch(const KernelArgs &a, const GroupSide &side, hipStream_t stream);
#define RG_X(entry, family, mode, kind) GroupLaunch entry;
RG_GROUP_ENTRIES(RG_X)
#undef RG_X

// the k-th step's slice of the action and output arrays
struct StepView {
    const int32_t *actions;
    rg_step_io io;
    // the launch's other per-call arguments, where they lie (the block's own members, except in the resident form below)
    const int32_t *auto_reset;
    const uint64_t *seed;
    int32_t grid;   // resident form: the launch's grid (0: gridDim.x)
};
__host__ __device__ inline StepView step_view(const KernelArgs &a, int k, int n_agents, int obs_dim) {
    StepView v;
    const size_t e = static_cast<size_t>(a.E) * k, en = e * n_agents;
    v.actions = a.actions ? a.actions + en : nullptr;
    v.io.obs = a.io.obs ? a.io.obs + en * obs_dim : nullptr;
    v.io.reward = a.io.reward ? a.io.reward + en : nullptr;
    v.io.done = a.io.done ? a.io.done + e : nullptr;
    v.io.dist_travelled = a.io.dist_travelled ? a.io.dist_travelled + en : nullptr;
    v.io.violation = a.io.violation ? a.io.violation + e : nullptr;
    v.io.remaining = a.io.remaining ? a.io.remaining + e : nullptr;
    v.io.qp_sweeps = a.io.qp_sweeps ? a.io.qp_sweeps + e : nullptr;
    v.io.elapsed = a.io.elapsed;  // state: the same counter for every step of a multi-step launch
    v.io.truncated = a.io.truncated ? a.io.truncated + e : nullptr;
    v.io.ended = a.io.ended ? a.io.ended + e : nullptr;
    v.io.reward_sum = a.io.reward_sum ? a.io.reward_sum + e : nullptr;
    v.io.time_limit = a.io.time_limit;
    v.io.zero_obs_on_end = a.io.zero_obs_on_end;
    v.auto_reset = &a.auto_reset;
    v.seed = &a.seed;
    v.grid = 0;
    return v;
}
// thread-per-env step kernel (robogym_tpe.hip): same results, chosen by the host for large batches
bool tpe_supported(const rg_scenario_params &p);
hipError_t launch_step_tpe(const KernelArgs &a, hipStream_t stream);
// rg_rollout: num_steps env steps per launch (robogym_rollout_tpe.hip)
hipError_t launch_rollout_tpe(const KernelArgs &a, hipStream_t stream);

}  // namespace rg
