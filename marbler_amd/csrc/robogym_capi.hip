// robogym_capi.hip -- the C ABI declared in include/robogym.h (host side).
//
// Plain pointers and sizes in, status codes out; no torch types.  The handle owns nothing on
// the device: state and outputs live in caller-owned HBM (torch-ROCm tensors).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <new>

#include "../../include/robogym.h"
#include "actor_common.h"
#include "host_checks.h"
#include "kernel_args.h"

struct rg_handle {
    rg_scenario_params params;
    rg::Consts consts;
    rg_state state;
    int32_t num_envs;
    int64_t env_offset;
    int32_t device;
    hipStream_t stream;
    bool bound;
    // What the launch plan (launch_plan.h) takes from the handle: the side block that is on and the switches rg_create read from
    // the environment (RG_STEP_KERNEL, RG_STEP_SPAN, RG_STEP_RESIDENT, RG_STEP_SHAPE), and what refresh() caches of its answer.
    rg::PlanHandle sw;
    bool use_tpe;      // step with the thread-per-env kernel (robogym_tpe.hip) instead of the lane-group kernel
    bool want_image;   // the handle's plain single step takes 16-lane rows: it can use a resident image
    bool seed_seen;      // the precomputed-reset blocks (rg_state.next_init) were drawn with last_seed
    uint64_t last_seed;
    rg_lidar_params lidar;   // rays == 0: off (rg_set_lidar)
    rg_team_params teams;    // n_sets == 0: no pool (rg_set_teams)
    bool disturbed;          // the pose disturbance is on (rg_set_disturbance), with the scales below
    rg::DisturbScale disturb;
    // The resident image of the argument block (kernel_args.h ResidentCall): what rg_create / rg_bind_state fix, in device memory
    // of the handle's device, for the resident form of the row kernels.  An image is IMMUTABLE once written: a launch -- or a
    // captured graph that replays one -- may read it at any later time.  Whatever alters it (a re-bind; rg_set_*) makes the
    // current one stale, and the next one is written into a fresh slot; the slots live until rg_destroy.  No valid image (the
    // slots used up, no memory, a write due while the stream is being captured, RG_STEP_RESIDENT=0): the launch goes by value.
    rg::KernelArgs *image_slots; // device: RG_IMAGE_SLOTS slots of RG_IMAGE_STRIDE bytes (allocated with the first image)
    int32_t images_used;
    const rg::KernelArgs *image; // the image of the handle as it is now, or null
    // The reference shape that `image`'s block matched (kernel_args.h match_shape; 0: none, or RG_STEP_SHAPE=0): decided where the
    // image is written, so a change that makes the image stale is matched again with the next one.
    int32_t image_shape;
    mutable int32_t last_form;   // rg_step_form: RG_FORM_* of the last rg_step launch
    bool image_stale;            // the handle has changed since `image` was written (or none was written yet)
};
constexpr int RG_IMAGE_SLOTS = 8;
constexpr size_t RG_IMAGE_STRIDE = 1024;
static_assert(sizeof(rg::KernelArgs) <= RG_IMAGE_STRIDE, "an image slot holds the block");
static void write_image(rg_handle *h);
static void drop_image(rg_handle *h) {   // the handle changes: its image no longer describes it
    h->image = nullptr;
    h->image_shape = 0;
    h->image_stale = true;
}
// The plan of a launch of the handle as it is now.
static rg::LaunchPlan plan(const rg_handle *h, int kind, bool gym = false) {
    return rg::plan_launch(h->params, h->num_envs, h->sw, rg::PlanCall{kind, gym, h->image != nullptr, h->image_shape});
}
// The handle has changed (rg_create, rg_set_*, rg_bind_state): what it caches of the plan is computed again, and its image no
// longer describes it.
static void refresh(rg_handle *h) {
    h->sw.side = h->teams.n_sets ? rg::GROUP_TEAM : h->lidar.rays ? rg::GROUP_LIDAR : h->disturbed ? rg::GROUP_DISTURB : rg::GROUP_PLAIN;
    drop_image(h);
    h->use_tpe = plan(h, rg::GROUP_STEP).tpe;
    h->want_image = rg::image_wanted(h->params, h->num_envs, h->sw);
}

static thread_local char g_err[512] = "";

// The handle's device is current for the duration of a call; the caller's device is restored on return.
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    hipError_t err;
    explicit DeviceGuard(int device) {
        err = hipGetDevice(&prev);
        if (err == hipSuccess && prev != device) {
            err = hipSetDevice(device);
            switched = (err == hipSuccess);
        }
    }
    ~DeviceGuard() {
        if (switched) (void)hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
};

static int fail(int code, const char *fmt, const char *detail = "") { return rg::Fail{g_err, sizeof(g_err), nullptr}.text(code, fmt, detail); }

// The rps constants' admitted domain (include/robogym.h "rps constants"): every limit is stated there with its reason.
// !(v > lo) also refuses a NaN; the message names the field.
static int check_constants(const rg_scenario_params *p) {
    const char *const msg = "rps constant %s is outside its admitted domain (include/robogym.h, rps constants)";
    const struct {
        const char *name;
        float v, hi;
    } positive[] = {{"time_step", p->time_step, 1.0f},
                    {"bound_w", p->bound_w, 200.0f},
                    {"bound_h", p->bound_h, 200.0f},
                    {"robot_diameter", p->robot_diameter, 1.0f},
                    {"wheel_radius", p->wheel_radius, 1.0f},
                    {"max_linear_velocity", p->max_linear_velocity, 2.0f},
                    {"collision_diameter", p->collision_diameter, 1.0f},
                    {"projection_distance", p->projection_distance, 1.0f},
                    {"angular_velocity_limit", p->angular_velocity_limit, 100.0f},
                    {"position_velocity_limit", p->position_velocity_limit, 2.0f}};
    for (const auto &f : positive)
        if (!(f.v > 0.0f && f.v <= f.hi)) return fail(-15, msg, f.name);
    if (!(p->projection_distance >= 1e-4f)) return fail(-15, msg, "projection_distance");
    // the arena: every corner coordinate within 100 m of the origin (the binary16 pre-test, csrc/kernel_args.h)
    if (!(fabsf(p->bound_x0) <= 100.0f)) return fail(-15, msg, "bound_x0");
    if (!(fabsf(p->bound_y0) <= 100.0f)) return fail(-15, msg, "bound_y0");
    if (!(fabsf(p->bound_x0 + p->bound_w) <= 100.0f)) return fail(-15, msg, "bound_w");
    if (!(fabsf(p->bound_y0 + p->bound_h) <= 100.0f)) return fail(-15, msg, "bound_h");
    // a collision point stays within 0.25 m of the arena until the boundary test has fired: one sub-step's travel + the offset
    if (!(fabsf(p->collision_offset) + p->time_step * p->max_linear_velocity <= 0.25f)) return fail(-15, msg, "collision_offset");
    // the heading advances min(update_frequency, controller_period) sub-steps at once and is wrapped once: at most one turn
    const float wmax = 2.0f * (p->wheel_radius / p->robot_diameter) * (p->max_linear_velocity / p->wheel_radius);
    if (!(wmax > 0.0f && wmax <= 1e6f))
        return fail(-15, msg, "wheel_radius / robot_diameter / max_linear_velocity (wmax = 2 (wheel_radius / robot_diameter)(max_linear_velocity / wheel_radius) must lie in (0, 1e6])");
    const float w = fminf(p->angular_velocity_limit, wmax);
    const int n = p->update_frequency < p->controller_period ? p->update_frequency : p->controller_period;
    if (!(static_cast<float>(n) * p->time_step * w <= 6.2831853f))
        return fail(-15, "rps constant %s: a controller period turns a robot by more than 2 pi (include/robogym.h, rps constants)", "time_step");
    return 0;
}

static int check_params(const rg_scenario_params *p) {
    if (!p) return fail(-1, "params is NULL");
    if (p->scenario < RG_SCN_PREDATOR_CAPTURE_PREY || p->scenario > RG_SCN_ARCTIC_TRANSPORT)
        return fail(-2, "unknown scenario id");
    if (p->n_agents < 1 || p->n_agents > RG_MAX_AGENTS) return fail(-3, "n_agents must be in 1..16");
    if (p->update_frequency < 1 || p->controller_period < 1) return fail(-4, "update_frequency / controller_period < 1");
    if (p->obs_dim < 1) return fail(-5, "obs_dim < 1");
    if (p->qp_max_sweeps < 1 || !(p->qp_rtol >= 0.0f)) return fail(-5, "qp_max_sweeps < 1 or qp_rtol < 0");
    if (p->qp_mode != RG_QP_EXACT && p->qp_mode != RG_QP_CVXOPT) return fail(-5, "unknown qp_mode");
    if (p->qp_mode == RG_QP_CVXOPT) {
        if (p->n_agents > RG_QP_CVXOPT_MAX_AGENTS) return fail(-3, "qp_mode RG_QP_CVXOPT is built for n_agents <= 8");
        if (p->ipm_maxiters < 0 || !(p->ipm_reltol >= 0.0f) || !(p->ipm_feastol > 0.0f) || !(p->ipm_abstol >= 0.0f))
            return fail(-5, "ipm_maxiters < 0, or a negative / zero cvxopt tolerance");
    }
    if (p->collision_variant != RG_COLLISION_CENTER && p->collision_variant != RG_COLLISION_OFFSET)
        return fail(-6, "unknown collision_variant");
    const rg_grid &g = p->agent_grid;
    // rps generate_initial_conditions asserts cells > N (Appendix A.7)
    if (g.nx < 1 || g.ny < 1 || g.nx * g.ny <= p->n_agents || g.nx * g.ny > 64)
        return fail(-7, "agent reset grid must have n_agents < nx*ny <= 64");
    if (p->scenario == RG_SCN_PREDATOR_CAPTURE_PREY) {
        if (p->num_prey < 1 || p->num_prey > RG_MAX_PREY) return fail(-8, "num_prey must be in 1..64");
        const rg_grid &q = p->prey_grid;
        if (q.nx < 1 || q.ny < 1 || q.nx * q.ny <= p->num_prey || q.nx * q.ny > 64)
            return fail(-9, "prey reset grid must have num_prey < nx*ny <= 64");
        const int od = p->capability_aware ? 6 : 4;
        const int nb = p->num_neighbors >= p->n_agents - 1 ? p->n_agents - 1 : p->num_neighbors;
        if (p->obs_dim < od * (nb + 1)) return fail(-10, "obs_dim too small for PredatorCapturePrey");
        // the 4-float observation blocks are written with 16-byte stores
        if (od == 4 && (p->obs_dim & 3)) return fail(-10, "obs_dim must be a multiple of 4 for PredatorCapturePrey without capability_aware");
    } else if (p->scenario == RG_SCN_WAREHOUSE) {
        const int nb = p->num_neighbors >= p->n_agents - 1 ? p->n_agents - 1 : p->num_neighbors;
        if (p->obs_dim < 3 * (nb + 1)) return fail(-10, "obs_dim too small for Warehouse");
    } else if (p->scenario == RG_SCN_SIMPLE) {
        if (p->num_prey != 1) return fail(-8, "Simple has one goal (num_prey = 1)");
        const rg_grid &q = p->prey_grid;
        if (q.nx < 1 || q.ny < 1 || q.nx * q.ny <= 1 || q.nx * q.ny > 64) return fail(-9, "goal reset grid must have 1 < nx*ny <= 64");
        if (p->obs_dim < 2 * (p->n_agents + 1)) return fail(-10, "obs_dim too small for Simple");
    } else if (p->scenario == RG_SCN_ARCTIC_TRANSPORT) {
        if (p->n_agents != 4) return fail(-3, "ArcticTransport has exactly 4 agents");
        if (p->obs_dim < 30) return fail(-10, "obs_dim too small for ArcticTransport");
    } else {
        if (p->obs_dim < (p->capability_aware ? 11 : 9)) return fail(-10, "obs_dim too small for MaterialTransport");
    }
    return check_constants(p);
}

// rg_policy_rollout's kernels live in their own translation units (robogym_policy_unit.hip, one per hidden size and selector).  Declared
// weak: the host-only sanitizer build of this file links without them, and the entry point then refuses to run.
namespace rg {
hipError_t launch_policy_rollout_h64(const KernelArgs &, const rg_actor_weights &, const rg_policy_io &, int32_t, hipStream_t)
    __attribute__((weak));
hipError_t launch_policy_rollout_h128(const KernelArgs &, const rg_actor_weights &, const rg_policy_io &, int32_t, hipStream_t)
    __attribute__((weak));
hipError_t launch_policy_rollout_sample_h64(const KernelArgs &, const rg_actor_weights &, const rg_policy_io &, const rg_policy_sample &,
                                            int32_t, hipStream_t) __attribute__((weak));
hipError_t launch_policy_rollout_sample_h128(const KernelArgs &, const rg_actor_weights &, const rg_policy_io &, const rg_policy_sample &,
                                             int32_t, hipStream_t) __attribute__((weak));
// The lane-group step kernels' entries (kernel_args.h RG_GROUP_ENTRIES, in translation units of their own), and the team pool's index
// writer next to them: weak for the same reason.
#define RG_X(entry, family, mode, kind) GroupLaunch entry __attribute__((weak));
RG_GROUP_ENTRIES(RG_X)
#undef RG_X
hipError_t launch_team_index(const KernelArgs &, const rg_team_params &, hipStream_t) __attribute__((weak));
void resident_image(KernelArgs &, const LaunchPlan &) __attribute__((weak));
}  // namespace rg

// The scenario's own observation width: the columns its builder writes (the lidar block may start at or after it).
static int own_obs_width(const rg_scenario_params &p) {
    const int nb = p.num_neighbors >= p.n_agents - 1 ? p.n_agents - 1 : p.num_neighbors;
    switch (p.scenario) {
        case RG_SCN_PREDATOR_CAPTURE_PREY: return (p.capability_aware ? 6 : 4) * (nb + 1);
        case RG_SCN_WAREHOUSE: return 3 * (nb + 1);
        case RG_SCN_SIMPLE: return 2 * (p.n_agents + 1);
        case RG_SCN_ARCTIC_TRANSPORT: return 30;
        default: return p.capability_aware ? 11 : 9;
    }
}

// The entry of every (family, solver mode, launch kind) of the lane-group step kernels.
static const struct GroupEntry {
    rg::GroupLaunch *launch;
    int family, mode, kind;
} g_group[] = {
#define RG_X(entry, family, mode, kind) {rg::entry, rg::family, mode, rg::kind},
    RG_GROUP_ENTRIES(RG_X)
#undef RG_X
};

// does this build hold every kernel of the family?  (The host-only sanitizer build holds none.)
static bool group_family_built(int family) {
    for (const GroupEntry &g : g_group)
        if (g.family == family && !g.launch) return false;
    return true;
}

extern "C" {

int rg_abi_version(void) { return RG_ABI_VERSION; }

const char *rg_last_error(void) { return g_err; }

int rg_sizeof_params(void) { return static_cast<int>(sizeof(rg_scenario_params)); }
int rg_sizeof_state(void) { return static_cast<int>(sizeof(rg_state)); }
int rg_sizeof_step_io(void) { return static_cast<int>(sizeof(rg_step_io)); }
int rg_sizeof_policy_io(void) { return static_cast<int>(sizeof(rg_policy_io)); }
int rg_sizeof_policy_sample(void) { return static_cast<int>(sizeof(rg_policy_sample)); }
int rg_sizeof_lidar_params(void) { return static_cast<int>(sizeof(rg_lidar_params)); }
int rg_sizeof_team_params(void) { return static_cast<int>(sizeof(rg_team_params)); }
int rg_sizeof_disturbance_params(void) { return static_cast<int>(sizeof(rg_disturbance_params)); }
int rg_next_init_stride(const rg_scenario_params *params) {
    if (check_params(params) != 0) return -1;
    return rg::next_init_stride(*params);
}

rg_handle *rg_create(const rg_scenario_params *params, int32_t num_envs, int64_t env_offset, int32_t device,
                     void *hip_stream) {
    if (check_params(params) != 0) return nullptr;
    if (num_envs < 1) {
        fail(-11, "num_envs < 1");
        return nullptr;
    }
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count < 1) {
        fail(-12, "no HIP device visible: librobogym_hip has no CPU fallback");
        return nullptr;
    }
    if (device < 0 || device >= count) {
        fail(-13, "device index out of range");
        return nullptr;
    }
    if (!group_family_built(rg::GROUP_PLAIN)) {   // (a library that lacks one of its translation units)
        fail(-100, "rg_create: this build has no lane-group step kernels");
        return nullptr;
    }
    rg_handle *h = new (std::nothrow) rg_handle();
    if (!h) {
        fail(-14, "out of host memory");
        return nullptr;
    }
    h->params = *params;
    h->consts = rg::make_consts(*params);
    memset(&h->state, 0, sizeof(h->state));
    h->num_envs = num_envs;
    h->env_offset = env_offset;
    h->device = device;
    h->stream = static_cast<hipStream_t>(hip_stream);
    h->bound = false;
    h->seed_seen = false;
    h->last_seed = 0;
    const auto on = [](const char *name) {   // a switch that only "0" turns off
        const char *v = getenv(name);
        return !(v && !strcmp(v, "0"));
    };
    const char *force = getenv("RG_STEP_KERNEL");
    h->sw.force = !force ? rg::KERNEL_DEFAULT : !strcmp(force, "group") ? rg::KERNEL_GROUP : !strcmp(force, "tpe") ? rg::KERNEL_TPE : rg::KERNEL_DEFAULT;
    h->sw.tpe_supported = rg::tpe_supported(*params);
    h->sw.span = on("RG_STEP_SPAN");
    h->sw.resident = on("RG_STEP_RESIDENT") && rg::resident_image && rg::launch_step_resident;
    h->sw.shapes = on("RG_STEP_SHAPE") && rg::launch_step_shape;
    h->last_form = RG_FORM_NONE;
    h->image_slots = nullptr;
    h->images_used = 0;
    memset(&h->lidar, 0, sizeof(h->lidar));
    memset(&h->teams, 0, sizeof(h->teams));
    h->disturbed = false;
    h->disturb = rg::DisturbScale{0.0f, 0.0f};
    refresh(h);
    return h;
}

int rg_set_lidar(rg_handle *h, const rg_lidar_params *lp) {
    if (!h) return fail(-1, "handle is NULL");
    if (!lp || lp->rays == 0) {
        memset(&h->lidar, 0, sizeof(h->lidar));
        refresh(h);
        return 0;
    }
    if (h->disturbed) return fail(-57, "rg_set_lidar: the handle has the pose disturbance on (rg_set_disturbance); the disturbance and the lidar do not combine");
    if (h->teams.n_sets) return fail(-54, "rg_set_lidar: the handle has a team pool (rg_set_teams); a pool and the lidar do not combine");
    if (lp->rays < 4 || lp->rays > RG_LIDAR_MAX_RAYS || (lp->rays & 3))
        return fail(-50, "rg_set_lidar: rays must be 0 or a multiple of 4 in 4..32");
    if (lp->offset + lp->rays != h->params.obs_dim)
        return fail(-51, "rg_set_lidar: offset + rays must equal obs_dim (the lidar block ends the observation row)");
    if (lp->offset < own_obs_width(h->params))
        return fail(-52, "rg_set_lidar: offset lies inside the scenario's own observation columns");
    if (!(lp->range > 0.0f && lp->range <= 3.402823466e38f)) return fail(-53, "rg_set_lidar: range must be positive and finite");
    if (!group_family_built(rg::GROUP_LIDAR)) return fail(-100, "rg_set_lidar: this build has no lidar kernels");
    h->lidar = *lp;
    refresh(h);
    return 0;
}

int rg_set_disturbance(rg_handle *h, const rg_disturbance_params *dp) {
    if (!h) return fail(-1, "handle is NULL");
    if (!dp || (dp->sigma_xy == 0.0f && dp->sigma_theta == 0.0f)) {
        h->disturbed = false;
        h->disturb = rg::DisturbScale{0.0f, 0.0f};
        refresh(h);
        return 0;
    }
    // (a NaN fails both comparisons)
    if (!(dp->sigma_xy >= 0.0f && dp->sigma_xy <= RG_DISTURB_MAX_SIGMA_XY))
        return fail(-70, "rg_set_disturbance: sigma_xy must be a finite number of metres in [0, 0.1]");
    if (!(dp->sigma_theta >= 0.0f && dp->sigma_theta <= RG_DISTURB_MAX_SIGMA_THETA))
        return fail(-71, "rg_set_disturbance: sigma_theta must be a finite number of radians in [0, 0.5]");
    if (h->lidar.rays) return fail(-72, "rg_set_disturbance: the handle has the lidar on (rg_set_lidar); the disturbance and the lidar do not combine");
    if (h->teams.n_sets) return fail(-73, "rg_set_disturbance: the handle has a team pool (rg_set_teams); the disturbance and a pool do not combine");
    if (!group_family_built(rg::GROUP_DISTURB)) return fail(-100, "rg_set_disturbance: this build has no disturbance kernels");
    h->disturb = rg::DisturbScale{rg::disturb_scale(dp->sigma_xy), rg::disturb_scale(dp->sigma_theta)};
    h->disturbed = true;
    refresh(h);
    return 0;
}

int rg_destroy(rg_handle *h) {
    if (!h) return fail(-1, "handle is NULL");
    if (h->image_slots) {
        DeviceGuard guard(h->device);
        if (guard.err == hipSuccess) (void)hipFree(h->image_slots);
    }
    delete h;
    return 0;
}

int rg_set_stream(rg_handle *h, void *hip_stream) {
    if (!h) return fail(-1, "handle is NULL");
    h->stream = static_cast<hipStream_t>(hip_stream);
    return 0;
}

int rg_bind_state(rg_handle *h, const rg_state *st) {
    if (!h || !st) return fail(-1, "handle or state is NULL");
    if (!st->poses || !st->carry_dist || !st->episode_steps || !st->reset_count)
        return fail(-20, "poses, carry_dist, episode_steps and reset_count are required");
    switch (h->params.scenario) {
        case RG_SCN_PREDATOR_CAPTURE_PREY:
            if (!st->prey_loc || !st->prey_sensed || !st->prey_captured)
                return fail(-21, "PredatorCapturePrey needs prey_loc, prey_sensed, prey_captured");
            if (!rg::all_aligned(8, st->prey_loc)) return fail(-26, "prey_loc must be 8-byte aligned");
            break;
        case RG_SCN_WAREHOUSE:
            if (!st->loaded) return fail(-21, "Warehouse needs loaded");
            break;
        case RG_SCN_SIMPLE:
            if (!st->prey_loc) return fail(-21, "Simple needs prey_loc (its goal)");
            break;
        case RG_SCN_ARCTIC_TRANSPORT:
            if (!st->grid || !st->goal_col || !st->pixel_type || !st->reached_goal)
                return fail(-21, "ArcticTransport needs grid, goal_col, pixel_type, reached_goal");
            if (!rg::all_aligned(4, st->grid)) return fail(-26, "grid must be 4-byte aligned");
            break;
        default:
            if (!st->load || !st->zone_load || !st->messages)
                return fail(-21, "MaterialTransport needs load, zone_load, messages");
    }
    const int nstat = (st->ep_return != nullptr) + (st->done_return_sum != nullptr) + (st->done_count != nullptr) +
                      (st->done_steps_sum != nullptr);
    if (nstat != 0 && nstat != 4) return fail(-25, "rollout statistics arrays: set all four or none");
    if ((st->next_init != nullptr) != (st->next_episode != nullptr)) return fail(-25, "next_init / next_episode: set both or none");
    if (!rg::all_aligned(16, st->next_init)) return fail(-26, "next_init must be 16-byte aligned");
    h->state = *st;
    h->bound = true;
    refresh(h);
    write_image(h);   // (no image is no error: the steps go by value until one can be written)
    // whatever the rebound next_init / next_episode arrays hold was not drawn by this handle under a seed it knows:
    // the first rg_step / rg_rollout after a bind marks every block stale (sync_seed), whatever the caller put there
    h->seed_seen = false;
    return 0;
}

static int fill_args(rg_handle *h, rg::KernelArgs &a);
#define RG_ON_DEVICE(h)                                                                           \
    DeviceGuard guard_((h)->device);                                                              \
    if (guard_.err != hipSuccess) return fail(-31, "cannot select the handle's device: %s", hipGetErrorString(guard_.err))

// Writes the handle's image into a fresh slot, if it may use the resident form at all.  Called where the handle changes
// (rg_bind_state) and, while the image is stale, by rg_step: a write that could not be made then is made by the first step
// that can.  Synchronous (hipMemcpy from host memory: the image is on the device when this returns), so never while the handle's
// stream is being captured.  Leaves h->image null where there is none: never an error.
static void write_image(rg_handle *h) {
    h->image = nullptr;
    h->image_shape = 0;
    if (!h->sw.resident || !h->bound || !h->want_image) {
        h->image_stale = false;   // no row kernel serves this handle as it is (launch_plan.h image_wanted); a change marks it stale again
        return;
    }
    if (h->images_used >= RG_IMAGE_SLOTS) {
        h->image_stale = false;   // the slots are used up: by value from here on
        return;
    }
    rg::KernelArgs a;
    (void)fill_args(h, a);   // (bound: it cannot fail)
    rg::resident_image(a, plan(h, rg::GROUP_STEP));
    DeviceGuard guard(h->device);
    if (guard.err != hipSuccess) return;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(h->stream, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) {
        (void)hipGetLastError();
        return;   // stays stale: written by the first step outside the capture
    }
    if (!h->image_slots) {
        void *mem = nullptr;
        if (hipMalloc(&mem, RG_IMAGE_SLOTS * RG_IMAGE_STRIDE) != hipSuccess) {
            (void)hipGetLastError();
            h->images_used = RG_IMAGE_SLOTS;   // no memory: by value
            h->image_stale = false;
            return;
        }
        h->image_slots = static_cast<rg::KernelArgs *>(mem);
    }
    rg::KernelArgs *slot = reinterpret_cast<rg::KernelArgs *>(reinterpret_cast<char *>(h->image_slots) + RG_IMAGE_STRIDE * h->images_used);
    h->images_used += 1;   // (a slot whose write failed is not used again either)
    h->image_stale = false;
    if (hipMemcpy(slot, &a, sizeof(a), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError();
        return;
    }
    h->image = slot;
    h->image_shape = h->sw.shapes ? rg::match_shape(a.p) : 0;
}

static int fill_args(rg_handle *h, rg::KernelArgs &a) {
    if (!h) return fail(-1, "handle is NULL");
    if (!h->bound) return fail(-22, "rg_bind_state has not been called");
    memset(&a, 0, sizeof(a));
    a.p = h->params;
    a.k = h->consts;
    a.st = h->state;
    a.E = h->num_envs;
    a.num_steps = 1;
    a.env_offset = h->env_offset;
    // the precomputed-reset blocks serve the lane-group kernel (latency regime); the thread-per-env kernel ignores them
    a.next_stride = (!h->use_tpe && h->state.next_init) ? rg::next_init_stride(h->params) : 0;
    return 0;
}

// The blocks of rg_state.next_init are functions of (seed, global env, episode): a new seed makes them stale.
static int sync_seed(rg_handle *h, uint64_t seed) {
    if (h->state.next_episode && (!h->seed_seen || h->last_seed != seed)) {
        // first use after rg_bind_state, or a new seed: every tag <- -1 (one 4 E-byte memset on the stream; the caller's
        // initialisation of next_episode is not trusted)
        const hipError_t err = hipMemsetAsync(h->state.next_episode, 0xFF, sizeof(int32_t) * static_cast<size_t>(h->num_envs), h->stream);
        if (err != hipSuccess) return fail(-30, "hipMemsetAsync(next_episode) failed: %s", hipGetErrorString(err));
        h->seed_seen = true;
        h->last_seed = seed;
    }
    return 0;
}

static int check_io(const rg_step_io *io) {
    if (!io->obs || !io->reward || !io->done || !io->dist_travelled || !io->violation || !io->remaining)
        return fail(-24, "every rg_step_io array except qp_sweeps and the gymma block is required");
    if (!rg::all_aligned(16, io->obs)) return fail(-26, "obs must be 16-byte aligned");
    if (io->elapsed) {
        if (!io->truncated || !io->ended || !io->reward_sum) return fail(-24, "gymma block: elapsed needs truncated, ended and reward_sum");
        if (io->time_limit < 1) return fail(-29, "gymma block: time_limit must be > 0");
    }
    return 0;
}

static int launched(hipError_t err) {
    if (err != hipSuccess) return fail(-30, "kernel launch failed: %s", hipGetErrorString(err));
    return 0;
}

// The lane-group launch that `pl` names: its row of RG_GROUP_ENTRIES, the block with envs_per_wave as the kernel is to see it.
static int launch_group_entry(const rg_handle *h, rg::KernelArgs &a, const rg::LaunchPlan &pl) {
    a.envs_per_wave = pl.envs_per_wave;
    const rg::GroupSide side = {&h->lidar, &h->teams, &h->disturb, h->image, pl};
    for (const GroupEntry &g : g_group)
        if (g.family == pl.family && g.mode == pl.mode && g.kind == pl.kind && g.launch) return launched(g.launch(a, side, h->stream));
    return fail(-100, "this build has no lane-group step kernels");
}

int rg_reset(rg_handle *h, const uint8_t *mask, uint64_t seed, int32_t flags) {
    rg::KernelArgs a;
    if (int rc = fill_args(h, a)) return rc;
    if (flags & ~RG_RESET_BOOK_EPISODE) return fail(-28, "unknown rg_reset flags");
    a.reset_mask = mask;
    a.seed = seed;
    a.reset_flags = flags;
    RG_ON_DEVICE(h);
    if (int rc = launched(rg::launch_reset(a, h->stream))) return rc;
    // the team index of every episode just started (a second launch on the same stream: the reset kernels stay as they are)
    if (h->teams.n_sets) return launched(rg::launch_team_index(a, h->teams, h->stream));
    return 0;
}

int rg_step(rg_handle *h, const int32_t *actions, const rg_step_io *io, int32_t auto_reset, uint64_t seed) {
    rg::KernelArgs a;
    if (int rc = fill_args(h, a)) return rc;
    if (!actions || !io) return fail(-23, "actions or io is NULL");
    if (int rc = check_io(io)) return rc;
    a.actions = actions;
    a.io = *io;
    a.auto_reset = auto_reset;
    a.seed = seed;
    RG_ON_DEVICE(h);
    if (int rc = sync_seed(h, seed)) return rc;
    if (h->image_stale) write_image(h);
    const rg::LaunchPlan pl = plan(h, rg::GROUP_STEP, io->elapsed != nullptr);
    h->last_form = pl.form;   // (the struct that selects the kernel)
    if (pl.tpe) return launched(rg::launch_step_tpe(a, h->stream));
    return launch_group_entry(h, a, pl);
}

int rg_rollout(rg_handle *h, const int32_t *actions, int32_t num_steps, const rg_step_io *io, int32_t auto_reset,
               uint64_t seed) {
    rg::KernelArgs a;
    if (int rc = fill_args(h, a)) return rc;
    if (!actions || !io) return fail(-23, "actions or io is NULL");
    if (num_steps < 1) return fail(-27, "num_steps < 1");
    if (io->elapsed) return fail(-29, "the gymma block of rg_step_io belongs to rg_step (one launch per step)");
    if (int rc = check_io(io)) return rc;
    // (Until round 4 every step's [E][N][D] slice had to keep 16-byte alignment.  Not needed: the only 16-byte observation stores
    // are the 4-float blocks of PredatorCapturePrey without capabilities, whose D is a multiple of 4 -- every slice of that
    // format is aligned whatever E and N are; all other formats are written dword by dword, and the staged copies of the
    // thread-per-env kernel test their destination's alignment themselves (step_tpe.h copy_span / stage_obs_rows).)
    a.actions = actions;
    a.io = *io;
    a.num_steps = num_steps;
    a.auto_reset = auto_reset;
    a.seed = seed;
    RG_ON_DEVICE(h);
    if (int rc = sync_seed(h, seed)) return rc;
    const rg::LaunchPlan pl = plan(h, rg::GROUP_ROLLOUT);
    if (!pl.tpe) return launch_group_entry(h, a, pl);
    // thread-per-env: the multi-step kernel holds more values live (313 VGPRs at N = 5: one wave per
    // SIMD); it pays while the batch is at most one wave per SIMD (the latency regime), beyond that
    // num_steps single-step launches are faster (measured at 524288 envs: 166 vs 197 us per step)
    if (h->num_envs <= 65536) return launched(rg::launch_rollout_tpe(a, h->stream));
    a.num_steps = 1;
    for (int32_t k = 0; k < num_steps; ++k) {
        const rg::StepView v = rg::step_view(a, k, h->params.n_agents, h->params.obs_dim);
        rg::KernelArgs ak = a;
        ak.actions = v.actions;
        ak.io = v.io;
        if (int rc = launched(rg::launch_step_tpe(ak, h->stream))) return rc;
    }
    return 0;
}

// rg_policy_rollout (sample == NULL) and rg_policy_rollout_sample: the same checks, in the same order
static int policy_rollout(rg_handle *h, const rg_actor_weights *w, int32_t num_steps, const rg_policy_io *pio,
                          const rg_policy_sample *sample, bool sampling, const rg_step_io *io, int32_t auto_reset, uint64_t seed) {
    rg::KernelArgs a;
    if (int rc = fill_args(h, a)) return rc;
    if (!w || !pio || !io) return fail(-23, "weights, policy io or step io is NULL");
    if (num_steps < 1) return fail(-27, "num_steps < 1");
    if (h->params.qp_mode == RG_QP_CVXOPT) return fail(-40, "rg_policy_rollout: the interior-point mode (barrier_solver: cvxopt) is not supported");
    if (h->lidar.rays) return fail(-49, "rg_policy_rollout: a handle with the lidar observation on (rg_set_lidar) is not supported");
    if (h->teams.n_sets) return fail(-39, "rg_policy_rollout: a handle with a team pool (rg_set_teams) is not supported");
    if (h->disturbed) return fail(-38, "rg_policy_rollout: a handle with the pose disturbance on (rg_set_disturbance) is not supported");
    if (!w->use_rnn || w->gru_packed != 3)
        return fail(-41, "rg_policy_rollout: the actor must be a GRU with gru_packed == 3 (two binary16 planes, pack_gru='f16x2')");
    if (w->hidden_dim != 64 && w->hidden_dim != 128) return fail(-42, "rg_policy_rollout: hidden_dim must be 64 or 128");
    const int N = h->params.n_agents;
    if (w->n_sets != 1 && w->n_sets != N) return fail(-43, "rg_policy_rollout: n_sets must be 1 (shared) or n_agents");
    if (w->input_dim != h->params.obs_dim + (pio->append_agent_id ? N : 0))
        return fail(-44, "rg_policy_rollout: the actor's input_dim != obs_dim (+ n_agents with append_agent_id)");
    if (!rg::input_width_fits(w->input_dim)) return fail(-44, "rg_policy_rollout: input_dim above 64 is not supported");
    if (w->n_actions < 1 || w->n_actions > 32) return fail(-45, "rg_policy_rollout: n_actions must be in 1..32");
    if (!w->w1 || !w->b1 || !w->wih || !w->bih || !w->whh || !w->bhh || !w->w2 || !w->b2) return fail(-46, "rg_policy_rollout: a weight array is NULL");
    if (!pio->hidden || !pio->actions) return fail(-47, "rg_policy_rollout: hidden and actions are required");
    if (!rg::all_aligned(16, pio->hidden, pio->obs, w->w1, w->wih, w->whh, w->w2)) return fail(-26, "rg_policy_rollout: hidden, obs, w1, wih, whh and w2 must be 16-byte aligned");
    if (pio->explore_u && !(pio->epsilon >= 1e-6f && pio->epsilon <= 1.0f)) return fail(-48, "rg_policy_rollout: epsilon must be in [1e-6, 1] with explore_u");
    if (!io->elapsed) return fail(-29, "rg_policy_rollout: the step io must carry the gymma block (elapsed, truncated, ended, reward_sum)");
    if (int rc = check_io(io)) return rc;
    auto launch = w->hidden_dim == 64 ? rg::launch_policy_rollout_h64 : rg::launch_policy_rollout_h128;
    auto launch_sample = w->hidden_dim == 64 ? rg::launch_policy_rollout_sample_h64 : rg::launch_policy_rollout_sample_h128;
    if (sampling ? !launch_sample : !launch) return fail(-100, "rg_policy_rollout: this build has no device code");
    a.io = *io;
    a.auto_reset = auto_reset;
    a.seed = seed;
    a.next_stride = 0;   // AHEAD = false inside the launch, as in rg_rollout
    RG_ON_DEVICE(h);
    if (int rc = sync_seed(h, seed)) return rc;
    if (sampling) return launched(launch_sample(a, *w, *pio, *sample, num_steps, h->stream));
    return launched(launch(a, *w, *pio, num_steps, h->stream));
}

int rg_policy_rollout(rg_handle *h, const rg_actor_weights *w, int32_t num_steps, const rg_policy_io *pio, const rg_step_io *io,
                      int32_t auto_reset, uint64_t seed) {
    return policy_rollout(h, w, num_steps, pio, nullptr, false, io, auto_reset, seed);
}

int rg_policy_rollout_sample(rg_handle *h, const rg_actor_weights *w, int32_t num_steps, const rg_policy_io *pio,
                             const rg_policy_sample *sample, const rg_step_io *io, int32_t auto_reset, uint64_t seed) {
    // the selector's own arguments first (they need no handle), then every check of rg_policy_rollout
    if (!sample || !sample->sample_u) return fail(-55, "rg_policy_rollout_sample: sample or its sample_u is NULL");
    if (pio && pio->explore_u) return fail(-56, "rg_policy_rollout_sample: sample_u and explore_u do not combine (explore_u must be NULL)");
    return policy_rollout(h, w, num_steps, pio, sample, true, io, auto_reset, seed);
}

int rg_set_teams(rg_handle *h, const rg_team_params *tp) {
    if (!h) return fail(-1, "handle is NULL");
    if (!tp || tp->n_sets == 0) {
        memset(&h->teams, 0, sizeof(h->teams));
        refresh(h);
        return 0;
    }
    if (h->disturbed) return fail(-65, "rg_set_teams: the handle has the pose disturbance on (rg_set_disturbance); the disturbance and a pool do not combine");
    if (tp->n_sets < 1 || tp->n_sets > RG_TEAM_MAX_SETS) return fail(-60, "rg_set_teams: n_sets must be 0 or in 1..64");
    if (tp->mode != RG_TEAM_EPISODE && tp->mode != RG_TEAM_FIXED)
        return fail(-61, "rg_set_teams: unknown mode (RG_TEAM_EPISODE or RG_TEAM_FIXED)");
    if (h->params.scenario == RG_SCN_ARCTIC_TRANSPORT)
        return fail(-62, "rg_set_teams: ArcticTransport's agent types are fixed by the scenario; it takes no team pool");
    if (h->lidar.rays) return fail(-63, "rg_set_teams: the handle has the lidar on (rg_set_lidar); a pool and the lidar do not combine");
    const int sc = h->params.scenario;
    if (!tp->team_index || !tp->agent_step || (sc == RG_SCN_PREDATOR_CAPTURE_PREY && (!tp->sensing_radius || !tp->capture_radius)) ||
        (sc == RG_SCN_MATERIAL_TRANSPORT && !tp->torque))
        return fail(-64, "rg_set_teams: team_index, agent_step and the scenario's other tables (PredatorCapturePrey: sensing_radius, "
                         "capture_radius; MaterialTransport: torque) are required");
    if (!group_family_built(rg::GROUP_TEAM) || !rg::launch_team_index) return fail(-100, "rg_set_teams: this build has no team kernels");
    if (tp->mode == RG_TEAM_FIXED) {   // the index of every env for the handle's life: env_offset + e mod C
        rg::KernelArgs a;
        if (int rc = fill_args(h, a)) return rc;
        RG_ON_DEVICE(h);
        if (int rc = launched(rg::launch_team_index(a, *tp, h->stream))) return rc;
    }
    h->teams = *tp;
    refresh(h);
    return 0;
}

int rg_step_kernel(const rg_handle *h) {
    if (!h) return fail(-1, "handle is NULL");
    return h->use_tpe ? 1 : 0;
}

int rg_step_form(const rg_handle *h) {
    if (!h) return fail(-1, "handle is NULL");
    return h->last_form;
}

int rg_shape_match(const rg_scenario_params *params) {
    if (!params) return fail(-1, "params is NULL");
    return rg::match_shape(*params);
}

int rg_shape_info(int32_t shape, int32_t *row) {
    if (!row) return fail(-1, "row is NULL");
    return rg::shape_row(shape, row) ? 0 : fail(-80, "rg_shape_info: no such reference shape");
}

int rg_get_obs(rg_handle *h, float *obs) {
    rg::KernelArgs a;
    if (int rc = fill_args(h, a)) return rc;
    if (!obs) return fail(-23, "obs is NULL");
    if (!rg::all_aligned(16, obs)) return fail(-26, "obs must be 16-byte aligned");
    a.io.obs = obs;
    RG_ON_DEVICE(h);
    return launch_group_entry(h, a, plan(h, rg::GROUP_OBS));
}

}  // extern "C"
