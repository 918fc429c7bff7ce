/* robogym.h -- C ABI of librobogym_hip.so: the MI355X-native (gfx950) vectorised
 * Robotarium-gym step engine.
 *
 * Drop-in boundary.  Each entry point names the reference interface
 * it replaces; paths are relative to /root/reference/robotarium_gym/.  The reference is pure
 * Python and has no FFI of its own: the binding a maintainer would add is the ctypes layer in
 * marbler_amd/_lib.py (shown in INTEGRATION.md).
 *
 * Conventions
 *  - Every pointer in rg_state / rg_step_io / rg_step arguments is a DEVICE pointer into memory
 *    owned by the caller (torch-ROCm tensors: `tensor.data_ptr()`).  The library never allocates
 *    or frees caller-visible memory.
 *  - All calls are asynchronous on the HIP stream given to rg_create; no call synchronises.
 *  - Every call on a handle runs with the handle's device current (hipSetDevice(device of rg_create))
 *    and restores the caller's current device before returning: a handle created for GPU 1 launches
 *    on GPU 1 whatever device the calling thread has selected.  The stream must belong to that device.
 *  - Return value: 0 = OK, negative = error (text via rg_last_error()).  No exceptions cross
 *    the ABI.  A handle is re-entrant across handles, not thread-safe within one.
 *  - E envs, N agents per env, P prey, D per-agent observation length.
 */
#ifndef ROBOGYM_H
#define ROBOGYM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 7: + rg_policy_rollout() and rg_policy_io (T actor steps and env steps in one launch), rg_sizeof_policy_io(); later, purely
 * additive (no existing layout or entry point changed): + rg_set_lidar(), rg_lidar_params, rg_sizeof_lidar_params(); + rg_set_teams(),
 * rg_team_params, rg_sizeof_team_params(); + rg_actor_forward_sample(), rg_policy_rollout_sample(), rg_policy_sample,
 * rg_sizeof_policy_sample() (soft-policies action sampling); + rg_set_disturbance(), rg_disturbance_params,
 * rg_sizeof_disturbance_params() (per-step pose disturbance); + rg_render(), rg_render_params, rg_sizeof_render_params(),
 * rg_render_last_error() (batched RGB frames of the envs' state); + rg_episodes_append(), rg_episode_buffer, rg_episode_stream,
 * rg_sizeof_episode_buffer(), rg_sizeof_episode_stream(), rg_episodes_last_error() (a collector's stream as padded episodes);
 * + rg_actor_unroll(), rg_actor_unroll_io, rg_sizeof_actor_unroll_io(), rg_actor_unroll_last_error() (the actor over every time
 * step of an episode batch in one launch); + rg_td_targets(), rg_mixer_weights, rg_td_targets_io, rg_sizeof_mixer_weights(),
 * rg_sizeof_td_targets_io(), rg_td_targets_last_error() (the target mixer and the double-Q TD targets of an episode batch in one
 * launch).
 * 6 (round 5): rg_scenario_params ends in the barrier-QP solver selection (qp_mode + cvxopt's options): RG_QP_CVXOPT computes the
 * interior-point iterate the reference's stack computes (utilities/controller.py:13-16,23) instead of the exact projection;
 * rg_step_io.zero_obs_on_end; + rg_actor_forward_explore(), rg_actor_pack_gru_f16x2() and rg_actor_weights.gru_packed == 3.
 * 5 (round 4): + rg_actor_pack_gru_bf16x3() and rg_actor_weights.gru_packed == 2; rg_rollout takes every shape (no E*N*D % 4
 * rule); the one-lane-per-env step kernel covers N <= 6. */
#define RG_ABI_VERSION 7
#define RG_MAX_AGENTS 16
#define RG_MAX_PREY 64

/* scenarios/<S>/ : wrapper.py:12-16 env_dict */
enum {
    RG_SCN_PREDATOR_CAPTURE_PREY = 0,
    RG_SCN_WAREHOUSE = 1,
    RG_SCN_MATERIAL_TRANSPORT = 2,
    RG_SCN_SIMPLE = 3,
    RG_SCN_ARCTIC_TRANSPORT = 4
};
#define RG_ARCTIC_ROWS 8
#define RG_ARCTIC_COLS 12
/* rps _validate collision test */
enum { RG_COLLISION_CENTER = 0, RG_COLLISION_OFFSET = 1 };
/* info['message'] of the reference (utilities/roboEnv.py:82-94) as a code */
enum { RG_VIOL_NONE = 0, RG_VIOL_COLLISION = 1, RG_VIOL_BOUNDARY = 2, RG_VIOL_COLLISION_BOUNDARY = 3 };
/* How `si_barrier_cert` (utilities/controller.py:13-16,23: rps' certificate closure -> cvxopt `qp`) is evaluated:
 * RG_QP_EXACT  -- the exact solution of the QP (the Euclidean projection), by Hildreth sweeps (qp_rtol, qp_max_sweeps);
 * RG_QP_CVXOPT -- the iterate cvxopt's interior-point method stops at under rps' options (reltol = feastol = 1e-2, maxiters 50,
 *                 abstol 1e-7): an approximate, strictly interior solution -- what the reference's own stack returns.  Restated
 *                 coneqp in binary64 (csrc/ipm_qp.h); n_agents <= 8. */
enum { RG_QP_EXACT = 0, RG_QP_CVXOPT = 1 };
#define RG_QP_CVXOPT_MAX_AGENTS 8

/* Reset geometry of rps generate_initial_conditions (Appendix A.7) + the scenario's shift
 * (misc.py:49-63, warehouse.py:93-98): N distinct cells of an nx x ny grid;
 *   x = ((cx*spacing - w2) + ox1) + ox2,  y = ((cy*spacing - h2) + oy1) + oy2.
 * nx, ny are computed by the host in float64 exactly as the reference does
 * (floor(width/spacing), where width itself is a float64 difference of YAML values). */
typedef struct rg_grid {
    int32_t nx, ny;
    float spacing, w2, h2, ox1, ox2, oy1, oy2;
} rg_grid;

/* The scenario config.yaml (scenarios/<S>/config.yaml, read by wrapper.py:27-31) plus the rps
 * constants (Appendix A), flattened.  This is the block broadcast to every GPU at init. */
typedef struct rg_scenario_params {
    int32_t scenario;
    int32_t n_agents;
    int32_t obs_dim;                 /* D */
    int32_t update_frequency;        /* U, roboEnv.py:52 */
    int32_t controller_period;       /* 15, roboEnv.py:63 */
    int32_t max_episode_steps;
    int32_t penalize_violations;     /* roboEnv.py:82 */
    int32_t barrier_has_unsafe_gain; /* 1 = certificate2 ('safe'), 0 = certificate ('default'), controller.py:13-16 */
    int32_t collision_variant;       /* RG_COLLISION_* */
    int32_t capability_aware;
    int32_t num_prey;                /* P */
    int32_t num_neighbors;           /* K */
    int32_t torque[RG_MAX_AGENTS];   /* MaterialTransport.py:72-76 */
    /* rps constants (config keys of the same names, defaults in marbler_amd/params.py RPS_CONSTANTS).
     * The domain rg_create admits -- anything else is refused with error -15 and a message naming the field.  All 13 finite, and:
     *   time_step                (0, 1] s
     *   bound_w, bound_h         (0, 200] m
     *   bound_x0, bound_y0       every corner coordinate (bound_x0, bound_x0 + bound_w, bound_y0, bound_y0 + bound_h) within
     *                            100 m of the origin.  The collision pre-test rounds collision points to binary16
     *                            (csrc/kernel_args.h pre_margin): its rounding bound follows the arena's largest coordinate up to
     *                            1024 m, finished envs are parked on ghost points at x >= 1000 m, y = -1000 m, and the bound was
     *                            checked by emulation for arenas up to 200 m across -- hence a limit well below 1000 m.
     *   robot_diameter, collision_diameter   (0, 1] m: the collision limits the pre-test's bound was checked for
     *   wheel_radius             (0, 1] m, and wmax = 2 (wheel_radius / robot_diameter)(max_linear_velocity / wheel_radius) in
     *                            (0, 1e6] rad/s (a limit no robot needs; it keeps dt * wmax finite)
     *   max_linear_velocity      (0, 2] m/s
     *   position_velocity_limit  (0, 2] m/s
     *   projection_distance      [1e-4, 1] m (its reciprocal is a factor of every angular velocity)
     *   angular_velocity_limit   (0, 100] rad/s
     *   collision_offset         any sign, |collision_offset| + time_step * max_linear_velocity <= 0.25 m: the pre-test's rounding
     *                            bound is computed for collision points within 0.25 m of the arena, which is where one sub-step
     *                            beyond the wall -- the boundary test then fires -- may carry them
     *   and min(update_frequency, controller_period) * time_step * min(angular_velocity_limit, wmax) <= 2 pi: the heading advances
     *   a whole controller period at once and is wrapped once.
     * Poses are state, not parameters: rg_bind_state takes any finite pose.  A step that begins with a robot outside the arena
     * judges its first sub-step -- the one that ends the env -- with the exact pair test, not the pre-test (csrc/kernel_args.h). */
    float time_step, bound_x0, bound_y0, bound_w, bound_h;
    float robot_diameter, wheel_radius, max_linear_velocity;
    float collision_offset, collision_diameter;
    float projection_distance, angular_velocity_limit, position_velocity_limit;
    float barrier_gain, unsafe_barrier_gain, safety_radius, barrier_magnitude_limit;
    /* barrier QP solver (sim_spec_v0: Hildreth sweeps): stop when the largest change of a sweep is
     * <= qp_rtol * max(|u|_inf, barrier_magnitude_limit), or after qp_max_sweeps sweeps */
    float qp_rtol;
    int32_t qp_max_sweeps;
    /* scenario */
    float left, right, up, down;
    float agent_step[RG_MAX_AGENTS];     /* step_dist, or MaterialTransport per-agent speed */
    float sensing_radius[RG_MAX_AGENTS]; /* PredatorCapturePrey.py:40-44 */
    float capture_radius[RG_MAX_AGENTS];
    float time_penalty, sense_reward, capture_reward, violation_reward;
    float load_reward, unload_reward, goal_width;
    float unload_multiplier, load_multiplier, end_goal_width, zone1_radius;
    float reward_scaler;                          /* Simple (simple.py:219-222) */
    float arctic_normal_step, arctic_slow_step, arctic_fast_step; /* ArcticTransport agent.py:89-113 */
    float not_reached_penalty, dist_multiplier;   /* ArcticTransport.py:125-134 */
    /* reset (misc.py:49-63, scenario reset()) */
    rg_grid agent_grid, prey_grid;
    int32_t keep_theta;              /* Warehouse keeps the sampled heading, misc.py:58,62 zero it */
    int32_t shared_reward;           /* config key: episode return adds reward[0] (1) or sum(reward) (0), misc.py:178-181 */
    float zone1_mean, zone1_std, zone2_mean, zone2_std; /* MaterialTransport.py:99-100 */
    /* barrier QP solver (ABI 6): RG_QP_*; the ipm_* fields are cvxopt's `solvers.options` as rps sets them at import
     * (abstol 1e-7 = cvxopt's default, reltol = feastol = 1e-2, maxiters 50) and are read in RG_QP_CVXOPT mode only */
    int32_t qp_mode;
    float ipm_abstol, ipm_reltol, ipm_feastol;
    int32_t ipm_maxiters;
} rg_scenario_params;

/* Env state in HBM (replaces the Python objects: scenario.agent_poses 3xN = the live alias of
 * rps.Robotarium.poses, roboEnv.previous_pose, scenario.episode_steps, prey / loaded / load /
 * zone / message attributes).  Arrays a scenario does not use may be NULL. */
typedef struct rg_state {
    float *poses;           /* [E][3][N]: x row, y row, theta row, as the reference's 3xN */
    float *carry_dist;      /* [E][N]: length of the last sub-iteration of the previous step, not yet
                               added to dist_travelled (roboEnv.py:55-59 lags one iteration) */
    int32_t *episode_steps; /* [E] */
    int32_t *reset_count;   /* [E] episodes started so far (RNG stream position) */
    float *prey_loc;        /* [E][P][2]   PredatorCapturePrey; Simple keeps its goal here (P = 1) */
    uint8_t *prey_sensed;   /* [E][P] */
    uint8_t *prey_captured; /* [E][P] */
    uint8_t *loaded;        /* [E][N]      Warehouse */
    int32_t *load;          /* [E][N]      MaterialTransport */
    int32_t *zone_load;     /* [E][2] */
    int32_t *messages;      /* [E][4] */
    uint8_t *grid;          /* [E][8*12]   ArcticTransport terrain: 0 normal, 1 ice, 2 water, 3 goal */
    int32_t *goal_col;      /* [E]         ArcticTransport goal_loc[1] (goal_loc[0] is always 1) */
    uint8_t *pixel_type;    /* [E][N]      ArcticTransport Agent.pixel_type (read by the NEXT step's goals) */
    uint8_t *reached_goal;  /* [E][N]      ArcticTransport Agent.reached_goal */
    /* Optional rollout statistics (all four NULL, or all four set), the on-device form of the
     * accumulators in utilities/misc.py:151-206 (episodeReward, episodeSteps, totalReward): */
    float *ep_return;       /* [E] return of the running episode */
    float *done_return_sum; /* [E] sum of the returns of the episodes this env has finished */
    int32_t *done_count;    /* [E] number of episodes this env has finished */
    int32_t *done_steps_sum;/* [E] total length of those episodes */
    /* Optional scratch of the lane-group step kernel (both NULL, or both set; contents are derived data, never part of a
     * snapshot): an env's NEXT initial state, drawn ahead of time at the end of a launch in which the env did not finish,
     * so that the launch in which it does finish copies it instead of running the sampler on its critical path.
     * next_init: [E][rg_next_init_stride(params)] floats; next_episode: [E], the episode index (= reset_count) the block
     * was drawn for, -1 = none.  The library marks every block stale itself (next_episode <- -1, one memset on the
     * handle's stream) on the first rg_step / rg_rollout after rg_bind_state and whenever their `seed` argument changes;
     * a caller that rewrites state arrays behind the handle's back (restoring a snapshot) resets next_episode to -1. */
    float *next_init;
    int32_t *next_episode;
} rg_state;

/* Everything Wrapper.step returns (wrapper.py:41-44), batched. */
typedef struct rg_step_io {
    float *obs;            /* [E][N][D] */
    float *reward;         /* [E][N] */
    uint8_t *done;         /* [E]  (the reference repeats it N times) */
    float *dist_travelled; /* [E][N]  info['dist_travelled'] */
    uint8_t *violation;    /* [E]     info['message'] as RG_VIOL_* */
    int32_t *remaining;    /* [E]     info['remaining'], -1 when the reference omits the key */
    int32_t *qp_sweeps;    /* [E] or NULL: diagnostic, max barrier-QP sweeps in this step */
    /* Optional (elapsed NULL = off): what EPyMARL's gymma wrapper puts around the env -- gym's TimeLimit and the
     * reductions float(sum(reward_n)), all(done_n) (README.md:25-28 of the reference; the wrapper itself is external) --
     * computed by the same launch instead of a dozen elementwise launches around it. */
    int32_t *elapsed;      /* [E] in/out (state, not per step): steps since the env's last (re)start, TimeLimit's counter */
    uint8_t *truncated;    /* [E] out: 1 = the time limit, not the scenario, ended the episode in this step (info['TimeLimit.truncated']) */
    uint8_t *ended;        /* [E] out: done | truncated -- what gymma returns as `terminated`; with auto_reset such an env is
                              reset in the same launch, and a truncated episode is booked in the statistics like a finished one */
    float *reward_sum;     /* [E] out: the sum of the agents' rewards in agent order */
    int32_t time_limit;    /* TimeLimit's max_episode_steps (> 0) */
    int32_t zero_obs_on_end; /* (with the gymma block) nonzero: the observation rows of an env that ENDS in this step are written as
                              zeros -- gymma users see the reset observation (what the reference's reset() returns,
                              PredatorCapturePrey.py:136) as the next observation of an episode that just ended; `obs` may then
                              point straight into the trainer's [T + 1][E][N][D] batch, slot t + 1 */
} rg_step_io;

typedef struct rg_handle rg_handle;

int rg_abi_version(void);
const char *rg_last_error(void);
/* sizeof(rg_scenario_params / rg_state / rg_step_io) as compiled, for binding self-checks */
int rg_sizeof_params(void);
int rg_sizeof_state(void);
int rg_sizeof_step_io(void);
/* floats per env of rg_state.next_init for this parameter block */
int rg_next_init_stride(const rg_scenario_params *params);

/* Replaces Wrapper.__init__ -> scenario.__init__ -> roboEnv.__init__ -> Controller.__init__
 * (wrapper.py:20-34, PredatorCapturePrey.py:15-59, roboEnv.py:12-24, controller.py:5-18).
 * `env_offset` is the global index of this shard's env 0 (RNG streams are keyed by global env
 * index, so results do not depend on how envs are sharded over GPUs). */
rg_handle *rg_create(const rg_scenario_params *params, int32_t num_envs, int64_t env_offset, int32_t device,
                     void *hip_stream);
int rg_destroy(rg_handle *h);

/* Binds the caller-owned state arrays.  Must be called before reset/step. */
int rg_bind_state(rg_handle *h, const rg_state *state);

/* Replaces scenario.reset() + roboEnv.reset() (PredatorCapturePrey.py:114-136, warehouse.py:84-100,
 * MaterialTransport.py:94-111, roboEnv.py:27-36,98-118, misc.py:49-63).  mask: [E] uint8 device
 * pointer, nonzero = reset that env; NULL = all.
 * The running return of a reset env (rg_state.ep_return) restarts at zero.  flags:
 * RG_RESET_BOOK_EPISODE -- the abandoned episode (if it has taken at least one step) is first added to
 * done_return_sum / done_count / done_steps_sum, as an episode that a time limit outside the scenario
 * cut short (gym's TimeLimit in EPyMARL's gymma wrapper; `run_env` counts such episodes, misc.py:186-206). */
#define RG_RESET_BOOK_EPISODE 1
int rg_reset(rg_handle *h, const uint8_t *mask, uint64_t seed, int32_t flags);

/* Replaces Wrapper.step -> scenario.step -> roboEnv.step -> Controller.set_velocities ->
 * rps.Robotarium.{get_poses,set_velocities,step} and the scenario's tracking / observation /
 * reward / termination code (wrapper.py:41-44, PredatorCapturePrey.py:138-216, warehouse.py:102-178,
 * MaterialTransport.py:113-189, roboEnv.py:38-96, controller.py:20-24).
 * actions: [E][N] int32.  If auto_reset != 0, envs that finish are reset in the same launch
 * (their returned obs/reward/done are those of the terminal step). */
int rg_step(rg_handle *h, const int32_t *actions, const rg_step_io *io, int32_t auto_reset, uint64_t seed);

/* num_steps consecutive rg_step()s in ONE launch, for action sequences that are known up front
 * (random-policy rollouts -- misc.py:134-221 `run_env` with a random policy --, replayed logs,
 * open-loop plans).  actions: [K][E][N]; every array of io has a leading dimension K and receives
 * what the k-th rg_step would have returned; results are bit-identical to K calls of rg_step.
 * Envs advance independently inside the launch (no device-wide synchronisation between steps), so
 * the launch takes K mean steps, not K worst-case steps. */
int rg_rollout(rg_handle *h, const int32_t *actions, int32_t num_steps, const rg_step_io *io, int32_t auto_reset,
               uint64_t seed);

/* The HIP stream later launches of this handle go to (rg_create's stream until changed).  Lets the
 * caller record rg_step into a hipGraph: set the capturing stream, capture, replay -- the evaluation
 * loop of misc.py:155-185 (policy forward, arg-max, env step) becomes one graph launch per step. */
int rg_set_stream(rg_handle *h, void *hip_stream);

/* The observation the scenario would build from the current state without stepping (the
 * reference returns zeros from reset(), PredatorCapturePrey.py:136; EPyMARL's gymma layer is
 * where get_obs() lives).  obs: [E][N][D]. */
int rg_get_obs(rg_handle *h, float *obs);

/* Which step kernel this handle launches: 0 = lane group per env (small / medium batches, and N >= 7 at every batch size:
 * the one-lane-per-env kernel is instantiated for N <= 6 only since round 4), 1 = one lane per env (chip-filling batches).  Chosen in rg_create from (scenario, n_agents, num_envs) -- measured cross-overs, csrc/robogym_capi.hip
 * tpe_min_envs -- or forced by the environment variable RG_STEP_KERNEL=group|tpe.  Both give bit-identical results; the
 * query exists so that tests and profiles can say which one ran.  Negative: error. */
int rg_step_kernel(const rg_handle *h);

/* Which form the handle's last rg_step launch took (csrc/kernel_args.h ResidentCall, RG_REF_SHAPES).  All forms give bit-identical
 * results; the query exists so that tests and profiles can say which one ran.
 *   RG_FORM_NONE      no rg_step yet
 *   RG_FORM_BY_VALUE  the whole argument block by value (every kernel but the 16-lane-row ones; RG_STEP_RESIDENT=0; no image)
 *   RG_FORM_RESIDENT  a row kernel reading the handle's resident image, every parameter a run-time value
 *   RG_FORM_SHAPE + s the resident row kernel of reference shape s >= 1: the handle's parameter block matched row s of the table
 *                     field for field, and the kernel holds those fields as constants.  RG_STEP_SHAPE=0 at rg_create: never.
 * Negative: error. */
#define RG_FORM_NONE 0
#define RG_FORM_BY_VALUE 1
#define RG_FORM_RESIDENT 2
#define RG_FORM_SHAPE 16
int rg_step_form(const rg_handle *h);
/* The reference shape a parameter block matches (1 ..), or 0.  Host code only: needs no device. */
int rg_shape_match(const rg_scenario_params *params);
/* Row `shape` of the table as ten ints: id, scenario, n_agents, then num_prey, obs_dim, num_neighbors, capability_aware,
 * update_frequency, controller_period, penalize_violations as the shape's kernel holds them (-1: read at run time).
 * 0, or negative where there is no such row. */
int rg_shape_info(int32_t shape, int32_t *row);

/* ---- lidar range observation (opt-in; out of parity scope: the reference has no lidar) --------------------------------
 * With rays > 0, every observation row the handle writes (rg_step, rg_rollout, rg_get_obs) carries `rays` floats at columns
 * offset .. offset + rays - 1 = obs_dim - 1, after the scenario's own columns.  Ray k of an agent at pose (x, y, theta) points
 * along (cos theta, sin theta) rotated by (dir[k][0], dir[k][1]) = binary32(cos, sin of 2 pi k / rays): ray 0 straight ahead,
 * counter-clockwise.  Its range t is the smallest positive distance from the robot's centre to the disk (radius
 * robot_diameter / 2) of another robot of the same env, or to a wall of the arena [bound_x0, bound_x0 + bound_w] x
 * [bound_y0, bound_y0 + bound_h]; the value stored is min(t, range) / range: exactly 1 when nothing lies within range, 0 when the
 * centre lies inside another robot's disk, 0 on every ray of an agent whose centre lies outside the arena.  A row the
 * engine zeroes (zero_obs_on_end) is zero in the lidar columns too.
 * Layout: 16 + 256 bytes, no padding; checked against the binding with rg_sizeof_lidar_params(). */
#define RG_LIDAR_MAX_RAYS 32
typedef struct rg_lidar_params {
    int32_t rays;                        /* R: 0 (off) or a multiple of 4 in 4..32 */
    int32_t offset;                      /* first lidar column: >= the scenario's own width, offset + rays == obs_dim */
    float range;                         /* L in metres: > 0, finite */
    float inv_range;                     /* binary32(1 / L) */
    float dir[RG_LIDAR_MAX_RAYS][2];     /* rows 0 .. rays - 1: the direction table above */
} rg_lidar_params;
int rg_sizeof_lidar_params(void);
/* Turns the lidar on for every later launch of the handle (lp->rays > 0), or off (lp NULL or lp->rays == 0: the default kernel
 * choice comes back).  With the lidar on the handle steps with the lane-group kernel at every batch size (rg_step_kernel()
 * reports 0) and rg_policy_rollout refuses it.  Errors: -1 NULL handle, -50 rays not a multiple of 4 in 4..32, -51
 * offset + rays != obs_dim, -52 offset below the scenario's own width, -53 range not positive and finite, -54 a handle with a
 * team pool (rg_set_teams), -100 a build without the lidar kernels. */
int rg_set_lidar(rg_handle *h, const rg_lidar_params *lp);

/* ---- team pool: per-episode agent capabilities (opt-in; out of parity scope: the reference has no pool) ----------------
 * A handle with a pool carries C capability sets (1 <= C <= RG_TEAM_MAX_SETS); set t gives every agent a its own values in row t
 * of [C][N] tables: agent_step[t][a] (PredatorCapturePrey, Warehouse, Simple: step_dist; MaterialTransport: speed),
 * sensing_radius[t][a], capture_radius[t][a] (PredatorCapturePrey) and torque[t][a] (MaterialTransport).  Every env e carries a
 * team index team_index[e] in [0, C), and every launch of the handle (rg_step, rg_rollout, rg_get_obs) reads set
 * team_index[e]'s values wherever it reads rg_scenario_params' agent_step / sensing_radius / capture_radius / torque, the
 * partners' values included.  The index is part of the env's state; the engine writes it when an episode starts:
 *   RG_TEAM_EPISODE: t = (uint64(w0) * C) >> 32, w0 = word 0 of philox4x32_10(counter = (ge_lo, ge_hi, episode, 0x80000000),
 *                    key = (seed_lo, seed_hi)), ge = env_offset + e, episode = the reset_count value the reset sampler draws
 *                    the episode with -- rg_reset (masked or not) and the step's auto-reset (drawn-ahead blocks included).
 *                    (The block 0x80000000 lies far above the sampler's own blocks: no existing draw changes.)
 *   RG_TEAM_FIXED:   t = ge mod C, written by rg_set_teams and kept for the handle's life.
 * The tables and the index array are caller-owned device memory (the library never allocates) and must stay valid while the
 * pool is set; an index outside [0, C) (a caller's write) is read as C - 1.  Tables a scenario does not read may be NULL.
 * Layout: 8 + 5 pointers = 48 bytes, no padding; checked against the binding with rg_sizeof_team_params(). */
#define RG_TEAM_MAX_SETS 64
#define RG_TEAM_EPISODE 0
#define RG_TEAM_FIXED 1
typedef struct rg_team_params {
    int32_t n_sets;                 /* C: 0 (off) or 1..64 */
    int32_t mode;                   /* RG_TEAM_EPISODE | RG_TEAM_FIXED */
    const float *agent_step;        /* [C][N] every scenario */
    const float *sensing_radius;    /* [C][N] PredatorCapturePrey */
    const float *capture_radius;    /* [C][N] PredatorCapturePrey */
    const int32_t *torque;          /* [C][N] MaterialTransport */
    int32_t *team_index;            /* [E]    the envs' team indices (state) */
} rg_team_params;
int rg_sizeof_team_params(void);
/* Sets the handle's pool for every later launch (tp->n_sets > 0), or removes it (tp NULL or tp->n_sets == 0: the handle's own
 * kernel choice comes back).  With a pool the handle steps with the lane-group kernel at every batch size (rg_step_kernel()
 * reports 0) and rg_policy_rollout refuses it.  RG_TEAM_FIXED writes team_index on the handle's stream (needs rg_bind_state
 * first).  Errors: -1 NULL handle, -22 fixed mode before rg_bind_state, -60 n_sets outside 1..64, -61 unknown mode,
 * -62 ArcticTransport (its agent types are fixed), -63 a handle with the lidar on, -64 a table the scenario reads or
 * team_index is NULL, -30 the launch failed, -100 a build without the team kernels.  rg_set_lidar refuses a handle with a
 * pool (-54). */
int rg_set_teams(rg_handle *h, const rg_team_params *tp);

/* ---- pose disturbance: a random pose error every step (opt-in; out of parity scope: the reference has no such thing) ----
 * With it on, the first thing an env step (rg_step, rg_rollout) does is displace every agent's stored pose by a bounded,
 * zero-mean, near-Gaussian amount of standard deviation sigma_xy metres per axis and sigma_theta radians; the rest of the step
 * reads the displaced pose, so the error accumulates as a random walk through the integrated pose.  The draw is a function of
 * (seed, global env, episode, step of the episode, agent) alone -- no state is added -- and rg_get_obs applies nothing.  The
 * spec (Philox block, variates, scale, update) is csrc/disturb.h and DESIGN.md "Pose disturbance".
 * Layout: 16 bytes, no padding; checked against the binding with rg_sizeof_disturbance_params(). */
#define RG_DISTURB_MAX_SIGMA_XY 0.1f
#define RG_DISTURB_MAX_SIGMA_THETA 0.5f
typedef struct rg_disturbance_params {
    float sigma_xy;      /* metres, 0 <= sigma_xy <= 0.1 */
    float sigma_theta;   /* radians, 0 <= sigma_theta <= 0.5 */
    float reserved[2];   /* ignored */
} rg_disturbance_params;
int rg_sizeof_disturbance_params(void);
/* Turns the disturbance on for every later rg_step / rg_rollout of the handle (either sigma > 0), or off (dp NULL or both
 * zero: the default kernel choice comes back).  With it on the handle steps with the lane-group kernel at every batch size
 * (rg_step_kernel() reports 0), and rg_policy_rollout / rg_policy_rollout_sample refuse it (-38).  Errors: -1 NULL handle,
 * -70 sigma_xy not a finite number in [0, 0.1], -71 sigma_theta not a finite number in [0, 0.5], -72 a handle with the lidar
 * on, -73 a handle with a team pool, -100 a build without the disturbance kernels.  rg_set_lidar (-57) and rg_set_teams (-65)
 * refuse a disturbed handle. */
int rg_set_disturbance(rg_handle *h, const rg_disturbance_params *dp);

/* ---- rendering: RGB frames of the envs' state (opt-in; replaces scenarios/<S>/visualize.py as utilities/roboEnv.py:67-76 shows it) ----
 * K frames of K envs in ONE launch: frame k is the picture of env env_index[k] (NULL: env k), height x width pixels of three
 * bytes (R, G, B), row 0 at the top.  The picture -- what is drawn, in which order and colour, and the binary32 arithmetic that
 * decides whether a shape covers a pixel's centre -- is stated once in csrc/render.h (DESIGN.md section 4 "Render"): the arena,
 * the scenario's zones or terrain, prey / goal markers, PredatorCapturePrey's capability rings, the robots in their class colour and
 * their headings.  The call is handle-free: it reads the state arrays of `state` that the scenario's picture needs (poses; prey_loc,
 * prey_sensed, prey_captured for PredatorCapturePrey and Simple; grid for ArcticTransport), writes `rgb` and nothing else, never
 * allocates or synchronises, and launches on `hip_stream` of the caller's CURRENT device.  A non-finite pose draws nothing; what
 * lies outside the view is clipped; an env_index entry outside [0, E) gives a frame with the arena and the fixed zones only.
 * Layout: 4 ints, one pointer, 4 floats = 40 bytes, no padding; checked against the binding with rg_sizeof_render_params(). */
#define RG_RENDER_ARENA 1
#define RG_RENDER_ZONES 2
#define RG_RENDER_MARKERS 4
#define RG_RENDER_RINGS 8
#define RG_RENDER_ROBOTS 16
#define RG_RENDER_HEADING 32
typedef struct rg_render_params {
    int32_t width, height;        /* pixels; width a multiple of 4 in 8..1024, height in 8..1024 */
    int32_t n_frames;             /* K >= 1 */
    int32_t layers;               /* bit mask RG_RENDER_ARENA | _ZONES | _MARKERS | _RINGS | _ROBOTS | _HEADING; 0 = all */
    const int32_t *env_index;     /* [K] device pointer, each in [0, E); NULL = envs 0 .. K-1 (then K <= E) */
    float view_x0, view_y0, view_w, view_h;  /* world rectangle the image shows (corner within 1000 m of the origin, sizes at most 1000 m); view_w == 0: the arena (bound_x0, bound_y0, bound_w, bound_h) */
} rg_render_params;
int rg_sizeof_render_params(void);
/* Every argument is checked before the first HIP call.  Errors (text via rg_render_last_error(), which names the field): -1 params,
 * -2 state, -3 rp, -4 rgb NULL; -5 rgb not 4-byte aligned; -80 scenario, -81 n_agents, -82 num_prey, -83 the arena, -84 robot_diameter
 * of params outside their domain; -85 num_envs < 1; -86 width outside 8..1024, -87 width not a multiple of 4, -88 height outside
 * 8..1024, -89 n_frames < 1, -90 more work-groups than a launch takes, -91 unknown layer bits, -92 env_index NULL with
 * n_frames > num_envs, -93 view_x0 / view_y0 not finite or beyond 1000 m, -94 view_w, -95 view_h not finite, negative or above 1000 m, -96 view_w > 0 with
 * view_h == 0; -97 state.poses, -98 a prey array, -99 state.grid NULL where the scenario's picture needs it; -30 the launch failed. */
int rg_render(const rg_scenario_params *params, const rg_state *state, int32_t num_envs, const rg_render_params *rp,
              uint8_t *rgb /* [K][height][width][3] */, void *hip_stream);
const char *rg_render_last_error(void);

/* ---- episode buffer: a collector's time-major stream as episode-major slots padded to episode_limit + 1 (opt-in) ----
 * The layout EPyMARL's learners read (components/episode_buffer.py EpisodeBatch / ReplayBuffer, external to the reference), filled
 * on the device in ONE launch per collection.  The rule is stated once in csrc/episodes.h (DESIGN.md section 4 "Episode buffer"):
 *   buffer  E envs x R slots (slot s = e R + r), episode limit L, N agents, row width D:
 *           obs [E R][L+1][N][D] f32, actions [E R][L+1][N] i32, reward [E R][L+1] f32, terminated / filled [E R][L+1] u8,
 *           optional prob [E R][L+1][N] f32; per slot length i32, episode_return f32, complete u8, fresh u8, episode_index i32;
 *           per env cursor [E][4] i32 = the open slot or -1, the position in it, episodes opened, overflow counter.
 *   stream  obs [T+1][E][N][D], actions [T][E][N], reward [T][E], terminated [T][E] u8, episode_start [T][E] u8, optional
 *           prob [T][E][N]: what BatchedRunner.run(T) returns.
 *   per env, for t = 0 .. T-1 in order: (1) episode_start[t,e] abandons an episode that is still open (not complete; the new
 *   one takes its slot and index) and opens a new one in slot e R + (opened mod R) at position 0, zeroing the slot's filled,
 *   terminated and reward rows and its length, episode_return, complete and fresh; (2) without an open episode the transition
 *   is dropped; (3) otherwise row p takes obs, actions, reward, terminated and prob of (t, e), filled[p] = 1 and
 *   episode_return += reward[t,e] (binary32, step order); (4) terminated[t,e]: row p+1 takes obs[t+1,e], filled[p+1] = 1,
 *   length = p+1, complete = fresh = 1, the episode closes; (5) p+1 == L without termination: force-closed as in (4) and the
 *   overflow counter goes up.  Nothing is written outside a slot.  An env that opens more than R episodes in one call
 *   overwrites its own older slots exactly as the sequential rule does.
 * Handle-free; reads the stream, writes the buffer and nothing else; never allocates, copies or synchronises (safe under stream
 * capture); launches on `hip_stream` of the caller's CURRENT device.  Rows are copied with 16-byte accesses where N D and the
 * obs bases allow it, with 8- or 4-byte ones where not: no width is refused.
 * Layouts: 12 pointers + 6 ints = 120 bytes; 6 pointers + 2 ints = 56 bytes; checked with rg_sizeof_episode_buffer / _stream(). */
typedef struct rg_episode_buffer {
    float *obs;
    int32_t *actions;
    float *reward;
    uint8_t *terminated, *filled;
    float *prob;                  /* NULL: the buffer keeps no prob (then the stream's must be NULL too) */
    int32_t *length;
    float *episode_return;
    uint8_t *complete, *fresh;
    int32_t *episode_index;
    int32_t *cursor;              /* [E][4] */
    int32_t num_envs, slots_per_env, episode_limit, n_agents, obs_dim;   /* E, R, L, N, D: each >= 1 */
    int32_t reserved;             /* 0 */
} rg_episode_buffer;
typedef struct rg_episode_stream {
    const float *obs;
    const int32_t *actions;
    const float *reward;
    const uint8_t *terminated, *episode_start;
    const float *prob;            /* NULL exactly when the buffer's is */
    int32_t T;                    /* >= 1 */
    int32_t reserved;             /* 0 */
} rg_episode_stream;
int rg_sizeof_episode_buffer(void);
int rg_sizeof_episode_stream(void);
/* Every argument is checked before the first HIP call.  Errors (text via rg_episodes_last_error(), which names the field):
 * -1 buffer, -2 stream NULL; -110 num_envs, -111 slots_per_env, -112 episode_limit, -113 n_agents, -114 obs_dim, -115 T below 1;
 * -116 the buffer's, -117 the stream's largest array has more than 2^31 - 1 elements; -120 - i: pointer field i is NULL, and
 * -150 - i: it is not aligned to its element (4 bytes for f32 / i32), with i counting buffer.obs, actions, reward, terminated,
 * filled, length, episode_return, complete, fresh, episode_index, cursor (0..10), stream.obs, actions, reward, terminated,
 * episode_start (11..15), buffer.prob (16), stream.prob (17); -136 prob in the buffer but not in the stream, -137 in the stream
 * but not in the buffer; -30 the launch failed. */
int rg_episodes_append(const rg_episode_buffer *buffer, const rg_episode_stream *stream, void *hip_stream);
const char *rg_episodes_last_error(void);

/* ---- policy inference for evaluation rollouts ------------------------
 * The EPyMARL recurrent actor the reference evaluates with (utilities/rnn_agent.py:5-29 `RNNAgent`:
 * fc1 -> ReLU -> GRUCell -> fc2; utilities/rnn_ns_agent.py:5-36 `RNNNSAgent`: one per agent), for all
 * E x N agents in one launch on the matrix cores (f32-input MFMA: float32 products and sums).
 * Weight arrays are torch's parameter layouts ([out][in] row-major), stacked over n_sets = 1 (shared)
 * or N (one set per agent).  use_rnn = 0 (rnn_agent.py:13,27: Linear + ReLU instead of the GRU): that
 * layer's weight / bias go in wih / bih, whh / bhh are ignored. */
typedef struct {
    const float *w1, *b1;   /* [S][H][I], [S][H] */
    const float *wih, *bih; /* [S][3H][H], [S][3H]   (use_rnn = 0: [S][H][H], [S][H]) */
    const float *whh, *bhh; /* [S][3H][H], [S][3H] */
    const float *w2, *b2;   /* [S][A][H], [S][A] */
    int32_t n_sets, input_dim, hidden_dim, n_actions, use_rnn;
    int32_t gru_packed;     /* 0: wih / whh in torch's layout; 1: the float32 streaming order written by rg_actor_pack_gru;
                               2: three bfloat16 planes written by rg_actor_pack_gru_bf16x3 (6 bytes per weight);
                               3: two binary16 planes written by rg_actor_pack_gru_f16x2 (4 bytes per weight) */
} rg_actor_weights;

/* One actor step (misc.py:160-170: `actor(obs, hs)` then arg-max).  obs [E][N][D]; with
 * append_agent_id the one-hot agent id is appended to each row (misc.py:162-164), D (+N) must equal
 * input_dim.  hidden [E][N][H] is updated in place; restart [E] (or NULL) nonzero = a new episode in that
 * env: its hidden state and its observation are taken as zero (what the reference's reset() returns,
 * PredatorCapturePrey.py:136) -- pass the done flags of the previous rg_step.  q [E][N][A] (or NULL) receives the action values,
 * actions [E][N] (or NULL) the greedy action.  hidden_dim 64 or 128, n_actions <= 32, input_dim <= 64. */
int rg_actor_forward(const rg_actor_weights *w, int32_t num_envs, int32_t n_agents, const float *obs,
                     int32_t obs_dim, int32_t append_agent_id, const uint8_t *restart, float *hidden, float *q,
                     int32_t *actions, void *hip_stream);
/* The same launch with the epsilon-greedy selection of EPyMARL's action selector (components/action_selectors.py, external to
 * the reference: its runners explore this way during training) folded in: explore_u [E][N] holds one uniform draw in [0, 1) per
 * agent; with k = (int)(u * (n_actions / epsilon)) in binary32, the action is k when k < n_actions (that is u < epsilon, and k is
 * then uniform over the actions) and the greedy action otherwise.  epsilon in [1e-6, 1]; actions must not be NULL. */
int rg_actor_forward_explore(const rg_actor_weights *w, int32_t num_envs, int32_t n_agents, const float *obs,
                             int32_t obs_dim, int32_t append_agent_id, const uint8_t *restart, float *hidden, float *q,
                             int32_t *actions, const float *explore_u, float epsilon, void *hip_stream);
/* The same launch with the soft-policies selection of EPyMARL's action selectors (SoftPoliciesSelector, external to the reference:
 * what the zoo's MAPPO checkpoints collect data with: "action_selector": "soft_policies", "agent_output_type": "pi_logits") folded
 * in: the action is SAMPLED from softmax(q) and prob [E][N] (or NULL) receives the probability it had.  sample_u [E][N] holds one
 * uniform draw in [0, 1) per agent.  The rule, in binary32, per agent row: m = the row maximum of q as written; e_c =
 * soft_exp(q_c - m), an explicit sequence of IEEE operations (csrc/actor_common.h states it; no library or hardware exponential);
 * c_k = the partial sums of ((e_0 + e_1) + e_2) + ... in column order, Z the last; the action is the first k with u * Z < c_k, or
 * the last k with e_k > 0 if there is none; prob = e_action / Z.  A row whose maximum is not finite (a NaN, +inf, all -inf) takes
 * the greedy action and prob = NaN.  q and hidden are what rg_actor_forward writes.  sample_u and actions must not be NULL (-12). */
int rg_actor_forward_sample(const rg_actor_weights *w, int32_t num_envs, int32_t n_agents, const float *obs,
                            int32_t obs_dim, int32_t append_agent_id, const uint8_t *restart, float *hidden, float *q,
                            int32_t *actions, const float *sample_u, float *prob, void *hip_stream);
/* Optional, once per actor: reorder a GRU weight array ([S][3H][H], torch layout) into the order the
 * kernel streams it (1 KB per load instruction instead of 64 scattered 16-byte pieces).  dst: a device
 * buffer of the same size; use it as wih / whh with gru_packed = 1. */
int rg_actor_pack_gru(const float *src, int32_t n_sets, int32_t hidden_dim, float *dst, void *hip_stream);
/* The same matrix as three bfloat16 planes -- w = hi + mid + lo exactly up to 2^-24 |w|, each plane the top 16 bits of what
 * the planes before it leave -- in the order the kernel streams them.  dst: 6 bytes per weight = 3/2 of the size of src,
 * 16-byte aligned; use it as wih / whh with gru_packed = 2.  The GRU's products then run on the bfloat16 matrix cores (16 x
 * the float32 MFMA rate) as six plane products per float32 product, the hidden state and fc1's output being split the same
 * way on the fly; the three products of order 2^-24 are left out, which keeps the error below the rounding error of a
 * float32 dot product of the same length (rnn_agent.py:24 `self.rnn(x, h_in)` evaluated in float32 is the reference). */
int rg_actor_pack_gru_bf16x3(const float *src, int32_t n_sets, int32_t hidden_dim, void *dst, void *hip_stream);
/* The same matrix as TWO binary16 planes -- hi = binary16(w), lo' = binary16(2^11 (w - hi)): w = hi + 2^-11 lo' up to 2^-22 |w|
 * -- in the order the kernel streams them.  dst: 4 bytes per weight = the size of src, 16-byte aligned; use it as wih / whh with
 * gru_packed = 3.  A float32 product is then THREE plane products on the binary16 matrix cores (hi hi into one accumulator, the
 * two cross products into a second that joins it scaled by 2^-11), the hidden state and fc1's output being split the same way on
 * the fly: half the matrix-core time of the three-plane form, error at the level of a float32 GEMM's own roundings (measured
 * max 3.9e-7 against 9.5e-7 on 128-long dot products).  Range: binary16's -- activations above 65 504 saturate (the hidden state
 * is in [-1, 1], fc1's output a ReLU of the observation's affine image); below 2^-14 the first plane is a binary16 denormal, which
 * the matrix cores take as it is. */
int rg_actor_pack_gru_f16x2(const float *src, int32_t n_sets, int32_t hidden_dim, void *dst, void *hip_stream);
const char *rg_actor_last_error(void);

/* ---- actor unroll: the recurrent actor over every time step of an episode batch in ONE launch ----
 * What a learner does first with an episode-major batch (EPyMARL: mac.init_hidden(B), then mac.forward(batch, t) for every t; the
 * target network's pass and MAPPO's old-policy logits are the same computation).  The rule is stated once in csrc/actor_unroll.h
 * (DESIGN.md section 4 "Actor unroll").  For every episode b < B and agent n < N independently:
 *   h_{-1} = hidden_in[b][n], or zero when hidden_in is NULL; for t = 0 .. rows-1 in order,
 *   (q[b][t][n][:], h_t) = actor(obs[b][t][n][:] (+ one-hot n), h_{t-1}); actions[b][t][n] is the greedy action (the first
 *   maximum, a NaN counting as the largest value); hidden_out[b][n] = h_{rows-1}.
 * The observation at t = 0 is read as stored (this is not rg_actor_forward's restart flag, which also zeroes the observation), and
 * there are no `filled` masks: every one of the `rows` time steps is computed.  Bit-identical to `rows` calls of rg_actor_forward
 * (gru_packed == 3, restart = NULL) on the time slices with the hidden state carried through memory.
 * obs_pitch / out_pitch: the rows an episode takes in obs / in q and actions (>= rows): a slice [:, :rows] of a longer batch is read
 * and written in place.  Rows t >= rows of q and actions are not touched.
 * Handle-free; never allocates, copies or synchronises (safe under stream capture); launches on `hip_stream` of the caller's CURRENT
 * device.  Layout: 5 pointers + 8 ints = 72 bytes, checked with rg_sizeof_actor_unroll_io(). */
typedef struct rg_actor_unroll_io {
    const float *obs;        /* [B][obs_pitch][N][D] */
    float *q;                /* [B][out_pitch][N][A] or NULL */
    int32_t *actions;        /* [B][out_pitch][N]    or NULL */
    const float *hidden_in;  /* [B][N][H] or NULL: zeros */
    float *hidden_out;       /* [B][N][H] or NULL; may equal hidden_in */
    int32_t num_episodes, n_agents, obs_dim, rows, obs_pitch, out_pitch, append_agent_id, reserved;
} rg_actor_unroll_io;
int rg_sizeof_actor_unroll_io(void);
/* Every argument is checked before the first HIP call.  Errors (text via rg_actor_unroll_last_error(), which names the argument):
 * -1 w, -2 io, -3 io.obs NULL; -4 a weight array NULL; -5 use_rnn == 0 or gru_packed != 3 (the two-binary16-plane GRU only);
 * -6 hidden_dim not 64 / 128; -7 n_actions outside 1..32; -8 n_sets not 1 or n_agents; -9 num_episodes, -10 n_agents (also above
 * 65536), -11 obs_dim, -12 rows below 1; -13 obs_dim (+ n_agents) != input_dim; -14 padded input width above 64; -15 obs_pitch,
 * -16 out_pitch below rows; -17 reserved != 0; -18 q, actions and hidden_out all NULL; -19 hidden_in, hidden_out, w1, wih, whh or
 * w2 not 16-byte aligned; -20 num_episodes * max(pitch) * n_agents * max(obs_dim, n_actions) above 2^31 - 1; -30 the launch failed. */
int rg_actor_unroll(const rg_actor_weights *w, const rg_actor_unroll_io *io, void *hip_stream);
const char *rg_actor_unroll_last_error(void);

/* ---- TD targets: target mixer and double-Q targets of an episode batch in ONE launch ----
 * The gradient-free half of a Q-learner's training step (EPyMARL: what q_learner.train computes under detach() from the target
 * network's unroll; QMixer with mixing_embed_dim 32, hypernet_layers 2, hypernet_embed 64; `state` is the concatenated
 * observations).  The rule is stated once in csrc/td_targets.h (DESIGN.md section 4 "TD targets"):
 *
 * Inputs.
 *   - qt [B][q_pitch][N][A] f32: the target actor's unroll.
 *   - sel [B][q_pitch][N] i32 or NULL: the online actor's greedy actions, which is double-Q.
 *   - obs [B][obs_pitch][N][D] f32: the state of row (b, t) is the S = N D contiguous floats of obs[b][t], read in place.
 *   - reward f32, terminated u8 and filled u8, each [B][flag_pitch].
 *   - rows >= 2, with T = rows - 1.
 *   - gamma.
 *   - kind in {none, vdn, qmix} and the mixer's weights.
 * Outputs.
 *   - targets [B][out_pitch] f32.  For `none` it is [B][out_pitch][N].
 *   - Optional mask [B][out_pitch] f32.
 *   - Optional agent_q [B][out_pitch][N] f32: the per-agent value before mixing.
 * For every b < B and t < T independently:
 *   - Mask.  mask[b][t] = filled[b][t] && (t == 0 || !terminated[b][t-1]), as 0.0 / 1.0.  This is EPyMARL's
 *     mask[:, 1:] *= 1 - terminated[:, :-1].
 *   - Masked rows.  A row with mask == 0 gets targets = 0.0 and agent_q = 0.0.  None of its qt, sel or obs rows is read.
 *   - Terminal rows.  A row with mask == 1 and terminated[b][t] gets targets = reward[b][t] and agent_q = 0.0.  Row t+1 is not read.
 *   - Agent values.  Otherwise a_n = sel[b][t+1][n] and agent_q[n] = qt[b][t+1][n][a_n].
 *       - An a_n outside [0, A) makes agent_q[n] NaN, and with it that row's target (with `none`: that agent's), and reads nothing
 *         out of bounds.
 *       - With sel == NULL, agent_q[n] is the maximum of qt[b][t+1][n][:] by the actor epilogue's existing rule: the first maximum,
 *         with a NaN counting as the largest value.
 *       - avail_actions is all ones in this project and plays no part.
 *   - Mixing.
 *       - none: y_n = agent_q[n].
 *       - vdn: y is the binary32 sum over n = 0 .. N-1 in that order: ((agent_q[0] + agent_q[1]) + agent_q[2]) + ...
 *       - qmix: EPyMARL's QMixer.forward on (agent_q, state[b][t+1]):
 *           w1 = |W1b relu(W1a s + b1a) + b1b|, viewed [N][32].
 *           b1 = Wb s + bb.
 *           hidden = elu(agent_q w1 + b1).
 *           wf = |Wfb relu(Wfa s + bfa) + bfb|, [32].
 *           v = Vb relu(Va s + ba) + bv.
 *           y = hidden wf + v.
 *   - Target.  targets = fl(reward[b][t] + fl(gamma y)).  The product is rounded before the sum, with no contraction.
 * Rows t >= T of the outputs are not touched.
 * With none and vdn this fixes every bit.  The qmix arithmetic is float32 with a summation order of the kernel's choosing.
 *
 * The mixer's weights, packed once on the host into the K-major layout the kernel streams (marbler_amd/targets.py TargetMixer; torch's
 * Linear.weight is [out][in], every matrix here is its transpose [in][out]); qmix only, NULL otherwise; each 16-byte aligned:
 *   w_in [SP][192]: the four first layers side by side -- columns 0..63 hyper_w_1.0, 64..127 hyper_w_final.0, 128..159 V.0,
 *        160..191 hyper_b_1 -- with SP = state_dim rounded up to a multiple of 4 and the rows behind state_dim zero; b_in [192];
 *   w_w1 [64][N 32] hyper_w_1.2, b_w1 [N 32]; w_wf [64][32] hyper_w_final.2, b_wf [32]; w_v [32] V.2, b_v [1].
 * Layout: 8 pointers + 6 ints = 88 bytes, checked with rg_sizeof_mixer_weights(). */
enum { RG_MIXER_NONE = 0, RG_MIXER_VDN = 1, RG_MIXER_QMIX = 2 };
typedef struct rg_mixer_weights {
    const float *w_in, *b_in, *w_w1, *b_w1, *w_wf, *b_wf, *w_v, *b_v;
    int32_t kind;             /* RG_MIXER_* */
    int32_t n_agents;         /* must equal io.n_agents */
    int32_t state_dim;        /* qmix: must equal io.n_agents * io.obs_dim */
    int32_t embed_dim;        /* qmix: mixing_embed_dim, must be 32 */
    int32_t hypernet_embed;   /* qmix: must be 64 (with hypernet_layers 2) */
    int32_t reserved;
} rg_mixer_weights;
int rg_sizeof_mixer_weights(void);
/* Layout: 9 pointers + 9 ints + 1 float + 1 int = 116 bytes, 120 with the tail padding, checked with rg_sizeof_td_targets_io(). */
typedef struct rg_td_targets_io {
    const float *qt;            /* [B][q_pitch][N][A] */
    const int32_t *sel;         /* [B][q_pitch][N] or NULL: the maximum over the actions */
    const float *obs;           /* [B][obs_pitch][N][D]; read with qmix only (may be NULL otherwise) */
    const float *reward;        /* [B][flag_pitch] */
    const uint8_t *terminated;  /* [B][flag_pitch] */
    const uint8_t *filled;      /* [B][flag_pitch] */
    float *targets;             /* [B][out_pitch], with RG_MIXER_NONE [B][out_pitch][N] */
    float *mask;                /* [B][out_pitch] or NULL */
    float *agent_q;             /* [B][out_pitch][N] or NULL */
    int32_t num_episodes, n_agents, obs_dim, n_actions, rows;
    int32_t q_pitch, obs_pitch, flag_pitch, out_pitch;   /* rows an episode takes in qt and sel; obs; the flags; the outputs */
    float gamma;
    int32_t reserved;
} rg_td_targets_io;
int rg_sizeof_td_targets_io(void);
/* Handle-free; never allocates, copies or synchronises (safe under stream capture); launches on `hip_stream` of the caller's CURRENT
 * device.  Every argument is checked before the first HIP call.  Errors (text via rg_td_targets_last_error(), which names the
 * argument): -1 m, -2 io NULL; -3 qt, reward, terminated, filled or targets NULL (obs with qmix); -4 an unknown kind; -5 qmix with
 * a weight array NULL; -6 or not 16-byte aligned; -7 embed_dim not 32 / hypernet_embed not 64; -8 m.n_agents != io.n_agents;
 * -9 qmix: m.state_dim != io.n_agents * io.obs_dim; -10 num_episodes below 1; -11 rows below 2; -12 n_agents outside
 * 1..RG_MAX_AGENTS; -13 n_actions outside 1..32; -14 obs_dim below 1, or with qmix the padded state wider than 256; -15 obs_pitch,
 * -16 q_pitch, -17 flag_pitch below rows; -18 out_pitch below rows - 1; -19 gamma not finite or outside [0, 1]; -20 m.reserved or
 * io.reserved != 0; -21 an array of more than 2^31 - 1 elements; -30 the launch failed. */
int rg_td_targets(const rg_mixer_weights *m, const rg_td_targets_io *io, void *hip_stream);
const char *rg_td_targets_last_error(void);

/* ---- policy-in-the-loop rollouts ---------------------------------------------------------------
 * The evaluation / data-collection loop of misc.py:155-185 (`actor(obs, hs)`, arg-max, env.step; the actor of
 * utilities/rnn_agent.py:5-29) -- what the actor launch followed by the env step launch computes, T times -- in ONE launch.
 * Every array is a device pointer; E, N, D, H as above, T = num_steps. */
typedef struct rg_policy_io {
    float *hidden;             /* [E][N][H] in/out: the actor's hidden state before the first and after the last time step */
    const uint8_t *restart;    /* [E] or NULL: nonzero = the env starts a new episode at the first time step (zero observation
                                  and zero hidden state, as the actor launch's restart flag) */
    int32_t append_agent_id;   /* the one-hot agent id goes after each observation row */
    int32_t restart_on_done;   /* later time steps restart an env after the previous step's `done` (nonzero) or its `ended` =
                                  done | truncated (zero: what a gymma runner does) */
    const float *explore_u;    /* [T][E][N] or NULL: epsilon-greedy uniforms, the rule of the actor's explore entry point */
    float epsilon;             /* in [1e-6, 1] when explore_u is given */
    int32_t *actions;          /* [T][E][N] out (required: the env step reads the actions from here) */
    float *obs;                /* [T + 1][E][N][D] or NULL: obs[0] is read as the first input, obs[t + 1] receives step t's
                                  observation (the trainer's batch layout); NULL: the step io's obs, read and rewritten in place */
    float *reward_sum;         /* [T][E] or NULL (then the step io's reward_sum, rewritten every step) */
    uint8_t *ended;            /* [T][E] or NULL (then the step io's ended, rewritten every step) */
    float *dist_sum;           /* [E][N] or NULL: += dist_travelled of every step, float32 additions in step order */
} rg_policy_io;
int rg_sizeof_policy_io(void);
/* num_steps time steps of: the actor for every agent row (the two-binary16-plane GRU, gru_packed == 3, hidden_dim 64 or 128),
 * its greedy or epsilon-greedy action, one env step with the gymma block (io must carry it: elapsed, truncated, ended,
 * reward_sum, time_limit; zero_obs_on_end as the caller sets it), the new observation and end flags feeding the next time step.
 * Replaces the loop body of misc.py:155-185 with utilities/rnn_agent.py:5-29 as the policy.  Results are bit-identical to
 * alternating the actor launch (restart flags: `restart` first, then the previous step's ended or done flags) and the env step
 * launch num_steps times; the arrays of io without a leading T hold the last step's values, as they would then.
 * Envs advance independently (no device-wide synchronisation), auto-reset runs inside the launch.  Refused with a reason in
 * the last-error text: the interior-point mode (RG_QP_CVXOPT), gru_packed other than 3 or use_rnn = 0, hidden_dim other than
 * 64 / 128, an input width other than obs_dim (+ n_agents with append_agent_id), num_steps < 1, a missing gymma block, a handle
 * with the lidar on (-49), a handle with a team pool (-39). */
int rg_policy_rollout(rg_handle *h, const rg_actor_weights *w, int32_t num_steps, const rg_policy_io *pio, const rg_step_io *io,
                      int32_t auto_reset, uint64_t seed);

/* rg_policy_rollout with the soft-policies selection of rg_actor_forward_sample at every time step (the sampled action feeds the
 * env step of the same time step inside the launch).  Bit-identical to alternating rg_actor_forward_sample and the env step launch.
 * pio->explore_u must be NULL (-56); sample and sample->sample_u must not be (-55); every refusal of rg_policy_rollout applies. */
typedef struct rg_policy_sample {
    const float *sample_u;     /* [T][E][N]: one uniform draw in [0, 1) per agent and time step */
    float *prob;               /* [T][E][N] or NULL: the probability the stored action had */
} rg_policy_sample;
int rg_sizeof_policy_sample(void);
int rg_policy_rollout_sample(rg_handle *h, const rg_actor_weights *w, int32_t num_steps, const rg_policy_io *pio,
                             const rg_policy_sample *sample, const rg_step_io *io, int32_t auto_reset, uint64_t seed);

#ifdef __cplusplus
}
#endif
#endif /* ROBOGYM_H */
