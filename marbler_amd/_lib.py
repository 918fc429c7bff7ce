"""ctypes binding of include/robogym.h (librobogym_hip.so).

This is the "FFI stub" a maintainer of the reference would add: the
reference is pure Python, so the boundary is Python -> C ABI.  There is NO CPU fallback:
if the library is missing, or no HIP device is visible, construction fails loudly.
"""
import ctypes as C
import os

MAX_AGENTS, MAX_PREY = 16, 64
ABI_VERSION = 7
RESET_BOOK_EPISODE = 1

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ROBOGYM_LIB") or os.path.join(_HERE, "librobogym_hip.so")  # override: diagnostic builds


class RgGrid(C.Structure):
    _fields_ = [("nx", C.c_int32), ("ny", C.c_int32), ("spacing", C.c_float), ("w2", C.c_float),
                ("h2", C.c_float), ("ox1", C.c_float), ("ox2", C.c_float), ("oy1", C.c_float),
                ("oy2", C.c_float)]


class RgScenarioParams(C.Structure):
    _fields_ = [
        ("scenario", C.c_int32), ("n_agents", C.c_int32), ("obs_dim", C.c_int32),
        ("update_frequency", C.c_int32), ("controller_period", C.c_int32),
        ("max_episode_steps", C.c_int32), ("penalize_violations", C.c_int32),
        ("barrier_has_unsafe_gain", C.c_int32), ("collision_variant", C.c_int32),
        ("capability_aware", C.c_int32), ("num_prey", C.c_int32), ("num_neighbors", C.c_int32),
        ("torque", C.c_int32 * MAX_AGENTS),
        ("time_step", C.c_float), ("bound_x0", C.c_float), ("bound_y0", C.c_float),
        ("bound_w", C.c_float), ("bound_h", C.c_float),
        ("robot_diameter", C.c_float), ("wheel_radius", C.c_float), ("max_linear_velocity", C.c_float),
        ("collision_offset", C.c_float), ("collision_diameter", C.c_float),
        ("projection_distance", C.c_float), ("angular_velocity_limit", C.c_float),
        ("position_velocity_limit", C.c_float),
        ("barrier_gain", C.c_float), ("unsafe_barrier_gain", C.c_float), ("safety_radius", C.c_float),
        ("barrier_magnitude_limit", C.c_float), ("qp_rtol", C.c_float), ("qp_max_sweeps", C.c_int32),
        ("left", C.c_float), ("right", C.c_float), ("up", C.c_float), ("down", C.c_float),
        ("agent_step", C.c_float * MAX_AGENTS), ("sensing_radius", C.c_float * MAX_AGENTS),
        ("capture_radius", C.c_float * MAX_AGENTS),
        ("time_penalty", C.c_float), ("sense_reward", C.c_float), ("capture_reward", C.c_float),
        ("violation_reward", C.c_float),
        ("load_reward", C.c_float), ("unload_reward", C.c_float), ("goal_width", C.c_float),
        ("unload_multiplier", C.c_float), ("load_multiplier", C.c_float), ("end_goal_width", C.c_float),
        ("zone1_radius", C.c_float), ("reward_scaler", C.c_float),
        ("arctic_normal_step", C.c_float), ("arctic_slow_step", C.c_float), ("arctic_fast_step", C.c_float),
        ("not_reached_penalty", C.c_float), ("dist_multiplier", C.c_float),
        ("agent_grid", RgGrid), ("prey_grid", RgGrid), ("keep_theta", C.c_int32), ("shared_reward", C.c_int32),
        ("zone1_mean", C.c_float), ("zone1_std", C.c_float), ("zone2_mean", C.c_float),
        ("zone2_std", C.c_float),
        ("qp_mode", C.c_int32), ("ipm_abstol", C.c_float), ("ipm_reltol", C.c_float), ("ipm_feastol", C.c_float), ("ipm_maxiters", C.c_int32),
    ]


class RgState(C.Structure):
    _fields_ = [("poses", C.c_void_p), ("carry_dist", C.c_void_p), ("episode_steps", C.c_void_p),
                ("reset_count", C.c_void_p), ("prey_loc", C.c_void_p), ("prey_sensed", C.c_void_p),
                ("prey_captured", C.c_void_p), ("loaded", C.c_void_p), ("load", C.c_void_p),
                ("zone_load", C.c_void_p), ("messages", C.c_void_p), ("grid", C.c_void_p),
                ("goal_col", C.c_void_p), ("pixel_type", C.c_void_p), ("reached_goal", C.c_void_p),
                ("ep_return", C.c_void_p),
                ("done_return_sum", C.c_void_p), ("done_count", C.c_void_p), ("done_steps_sum", C.c_void_p),
                ("next_init", C.c_void_p), ("next_episode", C.c_void_p)]


class RgStepIO(C.Structure):
    _fields_ = [("obs", C.c_void_p), ("reward", C.c_void_p), ("done", C.c_void_p),
                ("dist_travelled", C.c_void_p), ("violation", C.c_void_p), ("remaining", C.c_void_p),
                ("qp_sweeps", C.c_void_p),
                ("elapsed", C.c_void_p), ("truncated", C.c_void_p), ("ended", C.c_void_p), ("reward_sum", C.c_void_p),
                ("time_limit", C.c_int32), ("zero_obs_on_end", C.c_int32)]


class RgActorWeights(C.Structure):
    _fields_ = [("w1", C.c_void_p), ("b1", C.c_void_p), ("wih", C.c_void_p), ("bih", C.c_void_p),
                ("whh", C.c_void_p), ("bhh", C.c_void_p), ("w2", C.c_void_p), ("b2", C.c_void_p),
                ("n_sets", C.c_int32), ("input_dim", C.c_int32), ("hidden_dim", C.c_int32),
                ("n_actions", C.c_int32), ("use_rnn", C.c_int32), ("gru_packed", C.c_int32)]


class RgPolicyIO(C.Structure):
    _fields_ = [("hidden", C.c_void_p), ("restart", C.c_void_p), ("append_agent_id", C.c_int32), ("restart_on_done", C.c_int32),
                ("explore_u", C.c_void_p), ("epsilon", C.c_float), ("actions", C.c_void_p), ("obs", C.c_void_p),
                ("reward_sum", C.c_void_p), ("ended", C.c_void_p), ("dist_sum", C.c_void_p)]


class RgPolicySample(C.Structure):
    _fields_ = [("sample_u", C.c_void_p), ("prob", C.c_void_p)]


LIDAR_MAX_RAYS = 32


class RgLidarParams(C.Structure):
    _fields_ = [("rays", C.c_int32), ("offset", C.c_int32), ("range", C.c_float), ("inv_range", C.c_float),
                ("dir", (C.c_float * 2) * LIDAR_MAX_RAYS)]


TEAM_MAX_SETS = 64
TEAM_EPISODE, TEAM_FIXED = 0, 1


class RgTeamParams(C.Structure):
    _fields_ = [("n_sets", C.c_int32), ("mode", C.c_int32), ("agent_step", C.c_void_p), ("sensing_radius", C.c_void_p),
                ("capture_radius", C.c_void_p), ("torque", C.c_void_p), ("team_index", C.c_void_p)]


DISTURB_MAX_SIGMA_XY, DISTURB_MAX_SIGMA_THETA = 0.1, 0.5


class RgDisturbanceParams(C.Structure):
    _fields_ = [("sigma_xy", C.c_float), ("sigma_theta", C.c_float), ("reserved", C.c_float * 2)]


# rg_render: the layer bits of rg_render_params.layers (include/robogym.h RG_RENDER_*), in draw order
RENDER_ARENA, RENDER_ZONES, RENDER_MARKERS, RENDER_RINGS, RENDER_ROBOTS, RENDER_HEADING = 1, 2, 4, 8, 16, 32


class RgRenderParams(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("n_frames", C.c_int32), ("layers", C.c_int32),
                ("env_index", C.c_void_p), ("view_x0", C.c_float), ("view_y0", C.c_float), ("view_w", C.c_float),
                ("view_h", C.c_float)]


# rg_episodes_append: the buffer's arrays and the collector's stream (include/robogym.h; the rule: csrc/episodes.h)
class RgEpisodeBuffer(C.Structure):
    _fields_ = [("obs", C.c_void_p), ("actions", C.c_void_p), ("reward", C.c_void_p), ("terminated", C.c_void_p),
                ("filled", C.c_void_p), ("prob", C.c_void_p), ("length", C.c_void_p), ("episode_return", C.c_void_p),
                ("complete", C.c_void_p), ("fresh", C.c_void_p), ("episode_index", C.c_void_p), ("cursor", C.c_void_p),
                ("num_envs", C.c_int32), ("slots_per_env", C.c_int32), ("episode_limit", C.c_int32), ("n_agents", C.c_int32),
                ("obs_dim", C.c_int32), ("reserved", C.c_int32)]


class RgEpisodeStream(C.Structure):
    _fields_ = [("obs", C.c_void_p), ("actions", C.c_void_p), ("reward", C.c_void_p), ("terminated", C.c_void_p),
                ("episode_start", C.c_void_p), ("prob", C.c_void_p), ("T", C.c_int32), ("reserved", C.c_int32)]


# rg_actor_unroll: the actor over every time step of an episode batch (include/robogym.h; the rule: csrc/actor_unroll.h)
class RgActorUnrollIO(C.Structure):
    _fields_ = [("obs", C.c_void_p), ("q", C.c_void_p), ("actions", C.c_void_p), ("hidden_in", C.c_void_p),
                ("hidden_out", C.c_void_p), ("num_episodes", C.c_int32), ("n_agents", C.c_int32), ("obs_dim", C.c_int32),
                ("rows", C.c_int32), ("obs_pitch", C.c_int32), ("out_pitch", C.c_int32), ("append_agent_id", C.c_int32),
                ("reserved", C.c_int32)]


# rg_td_targets: the target mixer and the TD targets of an episode batch (include/robogym.h; the rule: csrc/td_targets.h)
MIXER_NONE, MIXER_VDN, MIXER_QMIX = 0, 1, 2


class RgMixerWeights(C.Structure):
    _fields_ = [("w_in", C.c_void_p), ("b_in", C.c_void_p), ("w_w1", C.c_void_p), ("b_w1", C.c_void_p), ("w_wf", C.c_void_p),
                ("b_wf", C.c_void_p), ("w_v", C.c_void_p), ("b_v", C.c_void_p), ("kind", C.c_int32), ("n_agents", C.c_int32),
                ("state_dim", C.c_int32), ("embed_dim", C.c_int32), ("hypernet_embed", C.c_int32), ("reserved", C.c_int32)]


class RgTdTargetsIO(C.Structure):
    _fields_ = [("qt", C.c_void_p), ("sel", C.c_void_p), ("obs", C.c_void_p), ("reward", C.c_void_p), ("terminated", C.c_void_p),
                ("filled", C.c_void_p), ("targets", C.c_void_p), ("mask", C.c_void_p), ("agent_q", C.c_void_p),
                ("num_episodes", C.c_int32), ("n_agents", C.c_int32), ("obs_dim", C.c_int32), ("n_actions", C.c_int32),
                ("rows", C.c_int32), ("q_pitch", C.c_int32), ("obs_pitch", C.c_int32), ("flag_pitch", C.c_int32),
                ("out_pitch", C.c_int32), ("gamma", C.c_float), ("reserved", C.c_int32)]


# rg_nstep_returns: the target critic and MAPPO's n-step returns of an episode batch (include/robogym_returns.h; the rule:
# csrc/nstep_returns.h)
CRITIC_CV, CRITIC_CV_NS = 0, 1
NSTEP_MAX, RETURNS_MAX_ROWS = 32, 4096


class RgCriticWeights(C.Structure):
    _fields_ = [("w1", C.c_void_p), ("w1_id", C.c_void_p), ("b1", C.c_void_p), ("w2", C.c_void_p), ("b2", C.c_void_p),
                ("w3", C.c_void_p), ("b3", C.c_void_p), ("kind", C.c_int32), ("n_agents", C.c_int32), ("state_dim", C.c_int32),
                ("hidden_dim", C.c_int32), ("net_stride", C.c_int32), ("reserved", C.c_int32)]


class RgNstepReturnsIO(C.Structure):
    _fields_ = [("obs", C.c_void_p), ("reward", C.c_void_p), ("terminated", C.c_void_p), ("filled", C.c_void_p),
                ("returns", C.c_void_p), ("values", C.c_void_p), ("mask", C.c_void_p),
                ("num_episodes", C.c_int32), ("n_agents", C.c_int32), ("obs_dim", C.c_int32), ("rows", C.c_int32),
                ("nstep", C.c_int32), ("add_value_last_step", C.c_int32), ("obs_pitch", C.c_int32), ("flag_pitch", C.c_int32),
                ("out_pitch", C.c_int32), ("value_pitch", C.c_int32), ("gamma", C.c_float), ("value_scale", C.c_float),
                ("value_shift", C.c_float), ("reserved", C.c_int32)]


# rg_gru_scan_forward / rg_gru_scan_backward: the GRU recurrence of an episode batch with gradients (include/robogym_learn.h; the
# rule: csrc/gru_scan.h)
GRU_SCAN_MAX_ROWS = 4096


class RgGruScanWeights(C.Structure):
    _fields_ = [("w_hh", C.c_void_p), ("b_hh", C.c_void_p), ("w_hh_t", C.c_void_p), ("n_sets", C.c_int32), ("hidden_dim", C.c_int32),
                ("reserved", C.c_int32 * 2)]


class RgGruScanIO(C.Structure):
    _fields_ = [("gi", C.c_void_p), ("hidden_in", C.c_void_p), ("h", C.c_void_p), ("gates", C.c_void_p), ("hidden_out", C.c_void_p),
                ("dh_ext", C.c_void_p), ("d_hidden_out", C.c_void_p), ("dgi", C.c_void_p), ("dghn", C.c_void_p),
                ("d_hidden_in", C.c_void_p), ("num_episodes", C.c_int32), ("n_agents", C.c_int32), ("rows", C.c_int32),
                ("gi_pitch", C.c_int32), ("save_pitch", C.c_int32), ("grad_pitch", C.c_int32), ("reserved", C.c_int32 * 2)]


# rg_mixer_forward / rg_mixer_backward: the online mixer's pass of an episode batch with gradients (include/robogym_learn.h; the
# rule: csrc/mixer_grad.h)
class RgMixerGradWeights(C.Structure):
    _fields_ = [("m", RgMixerWeights), ("w1b", C.c_void_p), ("wfb", C.c_void_p)]


class RgMixerGradIO(C.Structure):
    _fields_ = [("q", C.c_void_p), ("actions", C.c_void_p), ("obs", C.c_void_p), ("mask", C.c_void_p), ("mixed", C.c_void_p),
                ("d_mixed", C.c_void_p), ("d_q", C.c_void_p), ("d_pre", C.c_void_p), ("d_p2", C.c_void_p), ("g", C.c_void_p),
                ("num_episodes", C.c_int32), ("n_agents", C.c_int32), ("obs_dim", C.c_int32), ("n_actions", C.c_int32),
                ("rows", C.c_int32), ("q_pitch", C.c_int32), ("obs_pitch", C.c_int32), ("out_pitch", C.c_int32),
                ("aux_pitch", C.c_int32), ("reserved", C.c_int32)]


# rg_step_form: which form the last rg_step launch took (include/robogym.h RG_FORM_*)
FORM_NONE, FORM_BY_VALUE, FORM_RESIDENT, FORM_SHAPE = 0, 1, 2, 16


def reference_shapes():
    """The library's table of reference shapes (csrc/kernel_args.h RG_REF_SHAPES): [{id, scenario, n_agents, num_prey, ...}],
    a field the shape's kernel reads at run time is -1.  Host code: needs no GPU."""
    lib = load()
    names = ("id", "scenario", "n_agents", "num_prey", "obs_dim", "num_neighbors", "capability_aware", "update_frequency",
             "controller_period", "penalize_violations")
    out, row = [], (C.c_int32 * 10)()
    while lib.rg_shape_info(len(out) + 1, C.byref(row)) == 0:
        out.append(dict(zip(names, list(row))))
    return out


_P, _INT, _STR, _VP, _I32, _U64 = C.POINTER, C.c_int, C.c_char_p, C.c_void_p, C.c_int32, C.c_uint64
_ACTOR_STEP = [_P(RgActorWeights), _I32, _I32, _VP, _I32, _I32, _VP, _VP, _VP, _VP]      # what the three rg_actor_forward* share
_PACK = [_VP, _I32, _I32, _VP, _VP]
LATE = True
# every entry of include/robogym.h: (name, restype, argtypes or None for "takes nothing", late).  A late entry is one a library
# of an earlier build lacks: tolerated in one loaded through ROBOGYM_LIB (an A/B run against it), never in the package's own
ENTRIES = (
    ("rg_abi_version", _INT, None, False), ("rg_last_error", _STR, None, False),
    ("rg_sizeof_params", _INT, None, False), ("rg_sizeof_state", _INT, None, False), ("rg_sizeof_step_io", _INT, None, False),
    ("rg_next_init_stride", _INT, [_P(RgScenarioParams)], False),
    ("rg_create", _VP, [_P(RgScenarioParams), _I32, C.c_int64, _I32, _VP], False), ("rg_destroy", _INT, [_VP], False),
    ("rg_bind_state", _INT, [_VP, _P(RgState)], False), ("rg_set_stream", _INT, [_VP, _VP], False),
    ("rg_reset", _INT, [_VP, _VP, _U64, _I32], False), ("rg_step", _INT, [_VP, _VP, _P(RgStepIO), _I32, _U64], False),
    ("rg_rollout", _INT, [_VP, _VP, _I32, _P(RgStepIO), _I32, _U64], False), ("rg_get_obs", _INT, [_VP, _VP], False),
    ("rg_step_kernel", _INT, [_VP], False),
    ("rg_actor_forward", _INT, _ACTOR_STEP + [_VP], False),
    ("rg_actor_forward_explore", _INT, _ACTOR_STEP + [_VP, C.c_float, _VP], False),
    ("rg_actor_pack_gru", _INT, _PACK, False), ("rg_actor_pack_gru_bf16x3", _INT, _PACK, False),
    ("rg_actor_pack_gru_f16x2", _INT, _PACK, False), ("rg_actor_last_error", _STR, None, False),
    ("rg_sizeof_policy_io", _INT, None, False),
    ("rg_policy_rollout", _INT, [_VP, _P(RgActorWeights), _I32, _P(RgPolicyIO), _P(RgStepIO), _I32, _U64], False),
    ("rg_sizeof_lidar_params", _INT, None, False), ("rg_set_lidar", _INT, [_VP, _P(RgLidarParams)], False),
    ("rg_sizeof_team_params", _INT, None, False), ("rg_set_teams", _INT, [_VP, _P(RgTeamParams)], False),
    ("rg_actor_forward_sample", _INT, _ACTOR_STEP + [_VP, _VP, _VP], False), ("rg_sizeof_policy_sample", _INT, None, False),
    ("rg_policy_rollout_sample", _INT, [_VP, _P(RgActorWeights), _I32, _P(RgPolicyIO), _P(RgPolicySample), _P(RgStepIO), _I32, _U64], False),
    ("rg_sizeof_disturbance_params", _INT, None, False), ("rg_set_disturbance", _INT, [_VP, _P(RgDisturbanceParams)], False),
    ("rg_step_form", _INT, [_VP], LATE), ("rg_shape_match", _INT, [_P(RgScenarioParams)], LATE),
    ("rg_shape_info", _INT, [_I32, _P(_I32 * 10)], LATE),
    ("rg_sizeof_render_params", _INT, None, LATE),
    ("rg_render", _INT, [_P(RgScenarioParams), _P(RgState), _I32, _P(RgRenderParams), _VP, _VP], LATE),
    ("rg_render_last_error", _STR, None, LATE),
    ("rg_sizeof_episode_buffer", _INT, None, LATE), ("rg_sizeof_episode_stream", _INT, None, LATE),
    ("rg_episodes_append", _INT, [_P(RgEpisodeBuffer), _P(RgEpisodeStream), _VP], LATE), ("rg_episodes_last_error", _STR, None, LATE),
    ("rg_sizeof_actor_unroll_io", _INT, None, LATE),
    ("rg_actor_unroll", _INT, [_P(RgActorWeights), _P(RgActorUnrollIO), _VP], LATE), ("rg_actor_unroll_last_error", _STR, None, LATE),
    ("rg_sizeof_mixer_weights", _INT, None, LATE), ("rg_sizeof_td_targets_io", _INT, None, LATE),
    ("rg_td_targets", _INT, [_P(RgMixerWeights), _P(RgTdTargetsIO), _VP], LATE), ("rg_td_targets_last_error", _STR, None, LATE))
EXPORTS = tuple(e[0] for e in ENTRIES)
LATE_QUERIES = tuple(e[0] for e in ENTRIES if e[3])
# the layout check: (sizeof query, the ctypes struct it must agree with)
LAYOUTS = (("rg_sizeof_params", RgScenarioParams), ("rg_sizeof_state", RgState), ("rg_sizeof_step_io", RgStepIO),
           ("rg_sizeof_policy_io", RgPolicyIO), ("rg_sizeof_policy_sample", RgPolicySample), ("rg_sizeof_lidar_params", RgLidarParams),
           ("rg_sizeof_team_params", RgTeamParams), ("rg_sizeof_disturbance_params", RgDisturbanceParams),
           ("rg_sizeof_render_params", RgRenderParams), ("rg_sizeof_episode_buffer", RgEpisodeBuffer),
           ("rg_sizeof_episode_stream", RgEpisodeStream), ("rg_sizeof_actor_unroll_io", RgActorUnrollIO),
           ("rg_sizeof_mixer_weights", RgMixerWeights), ("rg_sizeof_td_targets_io", RgTdTargetsIO))

# The entries of include/robogym_returns.h, beside the table above (robogym.h's function list and ENTRIES stay as they are): typed
# and layout-checked on first use by load_returns().  (name, restype, argtypes or None)
RETURNS_ENTRIES = (
    ("rg_sizeof_critic_weights", _INT, None), ("rg_sizeof_nstep_returns_io", _INT, None),
    ("rg_nstep_returns", _INT, [_P(RgCriticWeights), _P(RgNstepReturnsIO), _VP]), ("rg_nstep_returns_last_error", _STR, None))
RETURNS_LAYOUTS = (("rg_sizeof_critic_weights", RgCriticWeights), ("rg_sizeof_nstep_returns_io", RgNstepReturnsIO))

# The entries of include/robogym_learn.h, likewise: typed and layout-checked on first use by load_learn().
LEARN_ENTRIES = (
    ("rg_sizeof_gru_scan_weights", _INT, None), ("rg_sizeof_gru_scan_io", _INT, None),
    ("rg_gru_scan_forward", _INT, [_P(RgGruScanWeights), _P(RgGruScanIO), _VP]),
    ("rg_gru_scan_backward", _INT, [_P(RgGruScanWeights), _P(RgGruScanIO), _VP]), ("rg_gru_scan_last_error", _STR, None))
LEARN_LAYOUTS = (("rg_sizeof_gru_scan_weights", RgGruScanWeights), ("rg_sizeof_gru_scan_io", RgGruScanIO))

# The mixer entries of include/robogym_learn.h, in a table of their own (LEARN_ENTRIES stays as it is): typed and layout-checked on
# first use by load_mixer_grad().
MIXER_GRAD_ENTRIES = (
    ("rg_sizeof_mixer_grad_weights", _INT, None), ("rg_sizeof_mixer_grad_io", _INT, None),
    ("rg_mixer_forward", _INT, [_P(RgMixerGradWeights), _P(RgMixerGradIO), _VP]),
    ("rg_mixer_backward", _INT, [_P(RgMixerGradWeights), _P(RgMixerGradIO), _VP]), ("rg_mixer_grad_last_error", _STR, None))
MIXER_GRAD_LAYOUTS = (("rg_sizeof_mixer_grad_weights", RgMixerGradWeights), ("rg_sizeof_mixer_grad_io", RgMixerGradIO))

_lib = None
_returns_ready = False
_learn_ready = False
_mixer_grad_ready = False


class RobogymError(RuntimeError):
    pass


def load():
    """Load librobogym_hip.so and type its entry points.  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RobogymError(
            f"{LIB_PATH} not found: build it with `python -m marbler_amd.build` (hipcc, gfx950). "
            "marbler_amd has no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, restype, argtypes, late in ENTRIES:
        if not hasattr(lib, name):
            if late and os.environ.get("ROBOGYM_LIB"):
                continue
            raise RobogymError(f"{LIB_PATH} does not export {name}")
        f = getattr(lib, name)
        f.restype = restype
        if argtypes is not None:
            f.argtypes = argtypes
    if lib.rg_abi_version() != ABI_VERSION:
        raise RobogymError(f"ABI version {lib.rg_abi_version()} != {ABI_VERSION}; rebuild the library")
    for query, struct in LAYOUTS:
        if hasattr(lib, query) and getattr(lib, query)() != C.sizeof(struct):
            raise RobogymError(f"struct layout of the binding differs from the compiled library; rebuild ({struct.__name__} is "
                               f"{C.sizeof(struct)} bytes here, {query}() says {getattr(lib, query)()})")
    _lib = lib
    return lib


def _load_table(entries, layouts, header, feature):
    """load(), with a side header's entries typed and its struct layouts checked."""
    lib = load()
    for name, restype, argtypes in entries:
        if not hasattr(lib, name):
            raise RobogymError(f"{LIB_PATH} does not export {name} (include/{header}): it was built before {feature}")
        f = getattr(lib, name)
        f.restype = restype
        if argtypes is not None:
            f.argtypes = argtypes
    for query, struct in layouts:
        if getattr(lib, query)() != C.sizeof(struct):
            raise RobogymError(f"struct layout of the binding differs from the compiled library; rebuild ({struct.__name__} is "
                               f"{C.sizeof(struct)} bytes here, {query}() says {getattr(lib, query)()})")
    return lib


def load_returns():
    """load(), with the entries of include/robogym_returns.h typed and their struct layouts checked (once).  A library that lacks
    them -- one of an earlier build, loaded through ROBOGYM_LIB -- raises RobogymError here, when the feature is called, not at
    load()."""
    global _returns_ready
    if _returns_ready:
        return load()
    lib = _load_table(RETURNS_ENTRIES, RETURNS_LAYOUTS, "robogym_returns.h", "n-step returns")
    _returns_ready = True
    return lib


def load_learn():
    """load(), with the entries of include/robogym_learn.h typed and their struct layouts checked (once), exactly as
    load_returns() does it for its header."""
    global _learn_ready
    if _learn_ready:
        return load()
    lib = _load_table(LEARN_ENTRIES, LEARN_LAYOUTS, "robogym_learn.h", "the GRU scan")
    _learn_ready = True
    return lib


def load_mixer_grad():
    """load(), with the mixer entries of include/robogym_learn.h typed and their struct layouts checked (once), as load_learn()
    does it for the GRU scan's."""
    global _mixer_grad_ready
    if _mixer_grad_ready:
        return load()
    lib = _load_table(MIXER_GRAD_ENTRIES, MIXER_GRAD_LAYOUTS, "robogym_learn.h", "the trainable mixer")
    _mixer_grad_ready = True
    return lib


def check(rc, what):
    if rc != 0:
        raise RobogymError(f"{what} failed ({rc}): {load().rg_last_error().decode()}")
