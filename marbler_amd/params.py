"""Scenario config (the reference's YAML keys, verbatim) -> rg_scenario_params.

Mirrors what the reference does with `objectview(yaml)` in wrapper.py:27-31 and the scenario
constructors (PredatorCapturePrey.py:15-59, warehouse.py:48-82, MaterialTransport.py:49-92),
plus the rps constants of SURVEY.md Appendix A and the reset geometry of misc.py:49-63.
All derived integers (grid sizes) are computed in float64 exactly as the reference does.
"""
import collections
import ctypes
import math
import os

import numpy as np
import yaml

from ._lib import DISTURB_MAX_SIGMA_THETA, DISTURB_MAX_SIGMA_XY, LIDAR_MAX_RAYS, MAX_AGENTS, MAX_PREY, TEAM_EPISODE, TEAM_FIXED, TEAM_MAX_SETS, RgDisturbanceParams, RgGrid, RgLidarParams, RgScenarioParams

SCENARIO_IDS = {"PredatorCapturePrey": 0, "Warehouse": 1, "MaterialTransport": 2, "Simple": 3, "ArcticTransport": 4}
COLLISION_VARIANTS = {"center": 0, "offset": 1}
BARRIER_SOLVERS = {"exact": 0, "cvxopt": 1}      # RG_QP_EXACT, RG_QP_CVXOPT
CVXOPT_MAX_AGENTS = 8
CONFIG_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "configs")

# sim_spec_v0: which of the two upstream collision tests rps' _validate uses (SURVEY.md
# Appendix A.4).  'offset' = centres shifted 0.025 m along the heading, distance <= 0.135 m:
# the variant that ships with the per-robot dict counters the reference reads
# (roboEnv.py:84-86).  Override with config key `collision_variant: center`.
DEFAULT_COLLISION_VARIANT = "offset"

# sim_spec_v0 barrier-QP solver constants (float32): relative tolerance and sweep cap of the
# Hildreth iteration that stands in for cvxopt's interior-point qp (which the reference runs at
# reltol 1e-2).  Config keys `qp_rtol`, `qp_max_sweeps` override.
QP_RTOL = 1.25e-6
QP_MAX_SWEEPS = 40


# the rps constants of rg_scenario_params (the simulated GRITSBot and its arena) and their values
RPS_CONSTANTS = {"time_step": 0.033, "bound_x0": -1.6, "bound_y0": -1.0, "bound_w": 3.2, "bound_h": 2.0,
                 "robot_diameter": 0.11, "wheel_radius": 0.016, "max_linear_velocity": 0.2,
                 "collision_offset": 0.025, "collision_diameter": 0.135,
                 "projection_distance": 0.05, "angular_velocity_limit": math.pi, "position_velocity_limit": 0.15}


def default_config_path(scenario):
    return os.path.join(CONFIG_DIR, scenario + ".yaml")


def load_config(scenario, config_path=None, overrides=None):
    with open(config_path or default_config_path(scenario), "r") as f:
        cfg = yaml.safe_load(f)
    if overrides:
        cfg.update(overrides)
    return cfg


def _grid(count, width, height, spacing, what):
    """rps generate_initial_conditions (Appendix A.7) geometry."""
    nx = int(np.floor(width / spacing))
    ny = int(np.floor(height / spacing))
    if nx == 0 or ny == 0:
        raise ValueError(f"{what}: spacing {spacing} too large for a {width} x {height} area")
    if not nx * ny > count:
        raise ValueError(f"{what}: {count} items need more than {nx}x{ny} = {nx * ny} grid cells "
                         f"(rps asserts cells > N; lower the spacing)")
    if nx * ny > 64:
        raise ValueError(f"{what}: {nx}x{ny} grid exceeds the 64 cells the device sampler supports")
    g = RgGrid()
    g.nx, g.ny, g.spacing, g.w2, g.h2 = nx, ny, spacing, width / 2, height / 2
    return g


def _dummy_grid():
    g = RgGrid()
    g.nx = g.ny = 1
    return g


def _check_agents(N):
    if not 1 <= N <= MAX_AGENTS:
        raise ValueError(f"n_agents must be in 1..{MAX_AGENTS}")


def make_params(scenario, cfg):
    if scenario not in SCENARIO_IDS:
        raise KeyError(f"scenario {scenario!r} is not built (have {sorted(SCENARIO_IDS)})")
    p = RgScenarioParams()
    p.scenario = SCENARIO_IDS[scenario]
    p.update_frequency = int(cfg["update_frequency"])
    # roboEnv.py:63 `if iterations % 15 == 0 or self.args.robotarium`: with `robotarium: True` (the setting of a
    # Robotarium submission) the controller runs on every sub-iteration; in simulation that is all the flag changes
    p.controller_period = 1 if cfg.get("robotarium", False) else 15
    p.max_episode_steps = int(cfg["max_episode_steps"])
    p.penalize_violations = int(bool(cfg["penalize_violations"]))
    p.shared_reward = int(bool(cfg.get("shared_reward", scenario != "Warehouse")))
    if cfg.get("real_time", False):
        raise ValueError("real_time: True paces the simulator to wall-clock time (rps sim_in_real_time): not a batched mode "
                         "(the single-env `Wrapper` honours it: marbler_amd/wrapper.py)")
    bc = cfg.get("barrier_certificate", "safe")                # roboEnv.py:15-18
    if bc == "custom" or callable(bc):
        raise ValueError("barrier_certificate: custom -- Controller(type='custom', custom=<closure>) (utilities/controller.py:17-18) hands "
                         "the QP to a Python callable, which a batched device engine cannot run.  The PARAMETRIC family rps offers is "
                         "reachable from the config instead: barrier_certificate: safe|default (certificate2 | certificate) with the "
                         "keys safety_radius, barrier_gain, unsafe_barrier_gain, magnitude_limit overriding their defaults")
    if bc not in ("safe", "default"):
        raise ValueError("barrier_certificate must be 'safe' or 'default'")
    p.barrier_has_unsafe_gain = 1 if bc == "safe" else 0       # controller.py:13-16
    # the arguments of rps' create_single_integrator_barrier_certificate{2,}: the reference passes safety_radius=.2 for 'safe'
    # and leaves the rest at rps' defaults; a config may set any of them -- what the reference would
    # write as Controller('custom', create_single_integrator_barrier_certificate2(barrier_gain=..., safety_radius=...))
    p.safety_radius = float(cfg.get("safety_radius", 0.2 if bc == "safe" else 0.17))
    p.barrier_gain = float(cfg.get("barrier_gain", 100.0))
    p.unsafe_barrier_gain = float(cfg.get("unsafe_barrier_gain", 1e6))
    p.barrier_magnitude_limit = float(cfg.get("magnitude_limit", 0.2))
    for key, val in (("safety_radius", p.safety_radius), ("barrier_gain", p.barrier_gain), ("unsafe_barrier_gain", p.unsafe_barrier_gain),
                     ("magnitude_limit", p.barrier_magnitude_limit)):
        if not (val > 0.0 and math.isfinite(val)):
            raise ValueError(f"{key} must be a positive finite number (got {val!r})")
    # How the certificate's QP is evaluated (include/robogym.h RG_QP_*).  `exact`: the projection (sim_spec_v0's default, Hildreth
    # sweeps).  `cvxopt`: the interior-point iterate the reference's stack computes -- rps hands the QP to cvxopt at reltol =
    # feastol = 1e-2, maxiters 50 (utilities/controller.py:13-16,23) -- restated, unpinned against the real
    # package; cvxopt_* keys = `cvxopt.solvers.options`.
    solver = cfg.get("barrier_solver", "exact")
    if solver not in BARRIER_SOLVERS:
        raise ValueError(f"barrier_solver must be one of {sorted(BARRIER_SOLVERS)} (got {solver!r})")
    p.qp_mode = BARRIER_SOLVERS[solver]
    p.ipm_abstol, p.ipm_reltol = float(cfg.get("cvxopt_abstol", 1e-7)), float(cfg.get("cvxopt_reltol", 1e-2))
    p.ipm_feastol, p.ipm_maxiters = float(cfg.get("cvxopt_feastol", 1e-2)), int(cfg.get("cvxopt_maxiters", 50))
    p.qp_rtol = float(cfg.get("qp_rtol", QP_RTOL))
    p.qp_max_sweeps = int(cfg.get("qp_max_sweeps", QP_MAX_SWEEPS))
    p.collision_variant = COLLISION_VARIANTS[cfg.get("collision_variant", DEFAULT_COLLISION_VARIANT)]
    # the rps constants: config keys of the block's own field names override them; the library states and
    # checks the domain each admits (include/robogym.h "rps constants", rg_create)
    for key, val in RPS_CONSTANTS.items():
        v = cfg.get(key, val)
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise ValueError(f"{key} must be a number (got {v!r})")
        setattr(p, key, float(v))
    L, R, U, D = cfg["LEFT"], cfg["RIGHT"], cfg["UP"], cfg["DOWN"]
    p.left, p.right, p.up, p.down = L, R, U, D
    height = D - U
    if scenario == "PredatorCapturePrey":
        npred, ncap = int(cfg["predator"]), int(cfg["capture"])
        N = npred + ncap
        p.n_agents = N
        _check_agents(N)
        p.capability_aware = int(bool(cfg["capability_aware"]))
        p.num_prey = int(cfg["num_prey"])
        if not 1 <= p.num_prey <= MAX_PREY:
            raise ValueError(f"num_prey must be in 1..{MAX_PREY}")
        p.num_neighbors = int(cfg["num_neighbors"])
        p.obs_dim = (6 if p.capability_aware else 4) * (p.num_neighbors + 1)
        for a in range(N):
            p.agent_step[a] = cfg["step_dist"]
            p.sensing_radius[a] = cfg["predator_radius"] if a < npred else 0.0
            p.capture_radius[a] = 0.0 if a < npred else cfg["capture_radius"]
        p.time_penalty, p.sense_reward, p.capture_reward = \
            cfg["time_penalty"], cfg["sense_reward"], cfg["capture_reward"]
        p.violation_reward = -5.0                               # PredatorCapturePrey.py:159
        thresh = cfg["ROBOT_INIT_RIGHT_THRESH"]
        width = thresh - L                                     # PredatorCapturePrey.py:123-125
        g = _grid(N, width, height, cfg["start_dist"], "agents")
        g.ox1 = -(width / 2 - thresh)                           # misc.py:57
        p.agent_grid = g
        width = R - cfg["PREY_INIT_LEFT_THRESH"]               # :128-129 (shift uses ROBOT_INIT_RIGHT_THRESH)
        q = _grid(p.num_prey, width, height, cfg["step_dist"], "prey")
        q.ox1 = (width / 2 - thresh)                            # misc.py:61
        p.prey_grid = q
        p.keep_theta = 0
    elif scenario == "Warehouse":
        N = int(cfg["n_agents"])
        p.n_agents = N
        _check_agents(N)
        p.num_neighbors = int(cfg["num_neighbors"])
        p.obs_dim = 3 * (p.num_neighbors + 1)
        for a in range(N):
            p.agent_step[a] = cfg["step_dist"]
        p.load_reward, p.unload_reward, p.goal_width = cfg["load_reward"], cfg["unload_reward"], cfg["goal_width"]
        p.violation_reward = -5.0                               # warehouse.py:116
        g = _grid(N, R - L, height, cfg["start_dist"], "agents")   # warehouse.py:90-98
        g.ox1, g.ox2 = (1.5 + L) / 2, -((1.5 - R) / 2)
        g.oy1, g.oy2 = -((1 + U) / 2), (1 - D) / 2
        p.agent_grid = g
        p.prey_grid = _dummy_grid()
        p.keep_theta = 1
    elif scenario == "Simple":
        N = int(cfg["n_agents"])
        p.n_agents = N
        _check_agents(N)
        p.num_prey = 1                                          # the single goal (simple.py:74)
        p.obs_dim = 2 * (N + 1)                                 # simple.py:98
        for a in range(N):
            p.agent_step[a] = cfg["step_dist"]
        p.reward_scaler = cfg["reward_scaler"]
        p.violation_reward = -5.0                               # simple.py:174
        thresh = cfg["ROBOT_INIT_RIGHT_THRESH"]
        width = thresh - L                                     # simple.py:136-140
        g = _grid(N, width, height, cfg["start_dist"], "agents")
        g.ox1 = -(width / 2 - thresh)
        p.agent_grid = g
        width = R - cfg["PREY_INIT_LEFT_THRESH"]               # simple.py:143-146
        q = _grid(1, width, height, cfg["step_dist"], "goal")
        q.ox1 = (width / 2 - thresh)
        p.prey_grid = q
        p.keep_theta = 0
    elif scenario == "ArcticTransport":
        N = int(cfg["n_agents"])
        if N != 4:
            raise ValueError("ArcticTransport is hard-wired to 4 agents (ArcticTransport.py:26-31)")
        p.n_agents = 4
        p.obs_dim = 30                                          # ArcticTransport.py:19
        p.arctic_normal_step, p.arctic_slow_step, p.arctic_fast_step = \
            cfg["normal_step"], cfg["slow_step"], cfg["fast_step"]
        p.not_reached_penalty, p.dist_multiplier = cfg["not_reached_penalty"], cfg["dist_multiplier"]
        p.violation_reward = -30.0                              # ArcticTransport.py:103
        g = _dummy_grid()                                       # fixed start poses (ArcticTransport.py:30-33)
        g.nx, g.ny = 8, 1
        p.agent_grid = g
        p.prey_grid = _dummy_grid()
        p.keep_theta = 0
    else:
        nf, ns = int(cfg["n_fast_agents"]), int(cfg["n_slow_agents"])
        N = int(cfg["n_agents"])
        if nf + ns != N:
            raise ValueError("n_fast_agents + n_slow_agents must equal n_agents")
        if N < 4:
            raise ValueError("MaterialTransport broadcasts the messages of agents 0-3: n_agents >= 4")
        p.n_agents = N
        _check_agents(N)
        p.capability_aware = int(bool(cfg["capability_aware"]))
        p.obs_dim = 11 if p.capability_aware else 9
        for a in range(N):
            p.agent_step[a] = cfg["fast_step"] if a < nf else cfg["slow_step"]
            p.torque[a] = int(cfg["small_torque"] if a < nf else cfg["large_torque"])
        p.time_penalty = cfg["time_penalty"]
        p.unload_multiplier, p.load_multiplier = cfg["unload_multiplier"], cfg["load_multiplier"]
        p.end_goal_width, p.zone1_radius = cfg["end_goal_width"], cfg["zone1_radius"]
        p.violation_reward = -6.0                               # MaterialTransport.py:137
        for z in ("zone1", "zone2"):
            if cfg[z].get("distribution", "normal") != "normal":
                raise ValueError("only the 'normal' zone distribution of the reference config is built")
        p.zone1_mean, p.zone1_std = cfg["zone1"]["loc"], cfg["zone1"]["scale"]
        p.zone2_mean, p.zone2_std = cfg["zone2"]["loc"], cfg["zone2"]["scale"]
        width = cfg["end_goal_width"]                           # MaterialTransport.py:106-109
        thresh = L + cfg["end_goal_width"]
        g = _grid(N, width, height, cfg["start_dist"], "agents")
        g.ox1 = -(width / 2 - thresh)
        p.agent_grid = g
        p.prey_grid = _dummy_grid()
        p.keep_theta = 0
    p.obs_dim += lidar_config(cfg)[0]   # the lidar block follows the scenario's own columns
    if p.qp_mode == BARRIER_SOLVERS["cvxopt"] and p.n_agents > CVXOPT_MAX_AGENTS:
        raise ValueError(f"barrier_solver: cvxopt is built for n_agents <= {CVXOPT_MAX_AGENTS} (its QP is solved in one lane: 2N unknowns, "
                         f"N(N-1)/2 rows in registers); got {p.n_agents}")
    return p


def lidar_config(cfg):
    """(R, L) of the config keys `lidar_rays` (0 = off, or a multiple of 4 in 4..32) and `lidar_range` (metres, > 0).
    Not part of the reference (it has no lidar): both keys are optional, and without them nothing changes."""
    rays, rng = cfg.get("lidar_rays", 0), cfg.get("lidar_range", 1.0)
    if isinstance(rays, bool) or not isinstance(rays, (int, np.integer)) or not (rays == 0 or (4 <= rays <= LIDAR_MAX_RAYS and rays % 4 == 0)):
        raise ValueError(f"lidar_rays must be 0 or a multiple of 4 in 4..{LIDAR_MAX_RAYS} (got {rays!r})")
    if isinstance(rng, bool) or not isinstance(rng, (int, float, np.integer, np.floating)):
        raise ValueError(f"lidar_range must be a positive finite number of metres (got {rng!r})")
    rng = float(rng)
    if not (rng > 0.0 and math.isfinite(rng) and math.isfinite(float(np.float32(rng)))):
        raise ValueError(f"lidar_range must be a positive finite number of metres (got {rng!r})")
    return int(rays), rng


def lidar_directions(rays):
    """The ray table [R][2]: cos, sin of 2 pi k / R computed in binary64, rounded to binary32 (ray 0 straight ahead, counter-clockwise)."""
    a = 2.0 * np.pi * np.arange(rays, dtype=np.float64) / rays
    return np.stack([np.cos(a), np.sin(a)], axis=1).astype(np.float32)


def lidar_params(scenario, cfg, params):
    """The rg_lidar_params block of a config (None when `lidar_rays` is 0 or absent): the lidar block is the last R columns of
    the row `params` (make_params(scenario, cfg)) describes."""
    if scenario not in SCENARIO_IDS:
        raise KeyError(f"scenario {scenario!r} is not built (have {sorted(SCENARIO_IDS)})")
    rays, rng = lidar_config(cfg)
    if rays == 0:
        return None
    lp = RgLidarParams()
    lp.rays = rays
    lp.offset = int(params.obs_dim) - rays
    lp.range = float(np.float32(rng))
    lp.inv_range = float(np.float32(1.0 / float(np.float32(rng))))
    d = lidar_directions(rays)
    for k in range(rays):
        lp.dir[k][0], lp.dir[k][1] = float(d[k, 0]), float(d[k, 1])
    return lp


# ------------------------------------------------------------------ pose disturbance (DESIGN.md "Pose disturbance")
def disturbance_config(cfg):
    """(sigma_xy, sigma_theta) of the config keys `pose_noise_xy` (metres, 0..0.1) and `pose_noise_theta` (radians, 0..0.5); both
    default to 0 = off.  Not part of the reference (its simulated robots are exact): without the keys nothing changes."""
    out = []
    for key, hi, unit in (("pose_noise_xy", DISTURB_MAX_SIGMA_XY, "metres"), ("pose_noise_theta", DISTURB_MAX_SIGMA_THETA, "radians")):
        v = cfg.get(key, 0.0)
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(float(v)) \
                or not 0.0 <= float(v) <= hi:
            raise ValueError(f"{key} must be a finite number of {unit} in [0, {hi}] (got {v!r})")
        out.append(float(v))
    return tuple(out)


def disturbance_params(scenario, cfg, params):
    """The rg_disturbance_params block of a config (None when both `pose_noise_xy` and `pose_noise_theta` are 0 or absent).
    The disturbance combines with neither the lidar nor a team pool."""
    if scenario not in SCENARIO_IDS:
        raise KeyError(f"scenario {scenario!r} is not built (have {sorted(SCENARIO_IDS)})")
    sxy, sth = disturbance_config(cfg)
    if sxy == 0.0 and sth == 0.0:
        return None
    refuse_second_block("disturbance", lambda b: b.configured(cfg), "pose_noise_xy / pose_noise_theta")
    dp = RgDisturbanceParams()
    # (a bound rounded to binary32 may lie above it -- 0.1 does: the library compares in binary32 too)
    dp.sigma_xy, dp.sigma_theta = float(np.float32(sxy)), float(np.float32(sth))
    return dp


# ------------------------------------------------------------------ team pool (DESIGN.md "Team pool")
# the capabilities a set may give, per scenario: config name -> the per-agent table it fills (rg_team_params)
TEAM_CAPABILITIES = {"PredatorCapturePrey": {"sensing_radius": "sensing_radius", "capture_radius": "capture_radius",
                                             "step_dist": "agent_step"},
                     "MaterialTransport": {"speed": "agent_step", "torque": "torque"},
                     "Warehouse": {"step_dist": "agent_step"},
                     "Simple": {"step_dist": "agent_step"}}
TEAM_SAMPLING = {"episode": TEAM_EPISODE, "fixed": TEAM_FIXED}


class TeamPool(object):
    """C capability sets of an N-agent scenario: [C][N] numpy tables agent_step, sensing_radius, capture_radius (float32) and
    torque (int32), and the sampling mode (TEAM_EPISODE | TEAM_FIXED).  Tables a scenario does not read hold its own values."""

    TABLES = ("agent_step", "sensing_radius", "capture_radius", "torque")

    def __init__(self, mode, agent_step, sensing_radius, capture_radius, torque):
        self.mode = int(mode)
        self.agent_step = np.ascontiguousarray(agent_step, np.float32)
        self.sensing_radius = np.ascontiguousarray(sensing_radius, np.float32)
        self.capture_radius = np.ascontiguousarray(capture_radius, np.float32)
        self.torque = np.ascontiguousarray(torque, np.int32)

    @property
    def n_sets(self):
        return int(self.agent_step.shape[0])

    @property
    def n_agents(self):
        return int(self.agent_step.shape[1])

    def __eq__(self, other):
        return isinstance(other, TeamPool) and self.mode == other.mode and all(
            np.array_equal(getattr(self, k), getattr(other, k)) for k in self.TABLES)

    def __repr__(self):
        return f"TeamPool(n_sets={self.n_sets}, n_agents={self.n_agents}, mode={self.mode})"


def _is_number(v):
    return not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating))


def team_pool(scenario, cfg, params):
    """The TeamPool of a config (None without a `teams` key): `teams` is a list of 1..64 mappings from a capability name of
    the scenario (TEAM_CAPABILITIES) to a list of N numbers; a capability a set leaves out takes the config's own per-agent
    value (make_params).  `team_sampling`: 'episode' (default: drawn at every episode start) or 'fixed' (env_offset + e mod C).
    Not part of the reference (it has no pool): without the keys nothing changes."""
    if scenario not in SCENARIO_IDS:
        raise KeyError(f"scenario {scenario!r} is not built (have {sorted(SCENARIO_IDS)})")
    sampling = cfg.get("team_sampling", "episode")
    if not isinstance(sampling, str) or sampling not in TEAM_SAMPLING:
        raise ValueError(f"team_sampling must be one of {sorted(TEAM_SAMPLING)} (got {sampling!r})")
    teams = cfg.get("teams")
    if teams is None:
        return None
    if scenario == "ArcticTransport":
        raise ValueError("teams: ArcticTransport's agent types are fixed by the scenario (ArcticTransport.py:26-33); it takes no team pool")
    refuse_second_block("teams", lambda b: b.configured(cfg), "teams")
    if isinstance(teams, (str, bytes)) or not isinstance(teams, (list, tuple)) or not 1 <= len(teams) <= TEAM_MAX_SETS:
        raise ValueError(f"teams must be a list of 1..{TEAM_MAX_SETS} capability sets (got {teams!r:.80})")
    N = int(params.n_agents)
    caps = TEAM_CAPABILITIES[scenario]
    own = {"agent_step": [params.agent_step[a] for a in range(N)], "sensing_radius": [params.sensing_radius[a] for a in range(N)],
           "capture_radius": [params.capture_radius[a] for a in range(N)], "torque": [params.torque[a] for a in range(N)]}
    tables = {k: np.tile(np.asarray(v, np.float64 if k != "torque" else np.int64), (len(teams), 1)) for k, v in own.items()}
    for t, st in enumerate(teams):
        if not isinstance(st, dict):
            raise ValueError(f"teams[{t}] must be a mapping from a capability name to a list of {N} numbers (got {st!r:.80})")
        for name, vals in st.items():
            key = f"teams[{t}].{name}"
            if name not in caps:
                raise ValueError(f"{key}: {name!r} is not a capability of {scenario} (have {sorted(caps)})")
            if isinstance(vals, (str, bytes)) or not hasattr(vals, "__len__") or len(vals) != N:
                raise ValueError(f"{key} must be a list of n_agents = {N} numbers (got {vals!r:.80})")
            vals = list(vals)
            if not all(_is_number(v) for v in vals):
                raise ValueError(f"{key} must hold numbers (got {vals!r:.80})")
            if name == "torque":
                if not all(math.isfinite(float(v)) and float(v) == int(v) and 0 <= int(v) < 2**31 for v in vals):
                    raise ValueError(f"{key} must hold integers >= 0 (got {vals!r:.80})")
                tables["torque"][t] = [int(v) for v in vals]
                continue
            fv = [float(v) for v in vals]
            with np.errstate(over="ignore"):   # (a value beyond binary32's range rounds to inf: refused below)
                finite = all(math.isfinite(v) and math.isfinite(float(np.float32(v))) for v in fv)
            if name in ("sensing_radius", "capture_radius"):
                if not finite or not all(v >= 0.0 for v in fv):
                    raise ValueError(f"{key} must hold finite radii >= 0 (got {vals!r:.80})")
            elif not finite or not all(v > 0.0 for v in fv):
                raise ValueError(f"{key} must hold finite values > 0 (got {vals!r:.80})")
            tables[caps[name]][t] = fv
    return TeamPool(TEAM_SAMPLING[sampling], tables["agent_step"], tables["sensing_radius"], tables["capture_radius"],
                    tables["torque"])


# ------------------------------------------------------------------ the side blocks
# What a handle can have on next to its parameter block -- at most ONE (the step kernels come in one family per block,
# csrc/launch_plan.h) -- a row each, in the order they were added:
#   attr        the keyword and attribute of VecRobotariumEnv that holds the block (None = off)
#   what, keys  how a message names the block, and the config keys that switch it on
#   one_launch  how evaluate.one_launch_refusals names it
#   configured  cfg -> the config switches it on;  read  (scenario, cfg, params) -> the block, or None
#   off         block -> it counts as None
#   setter      the C entry that takes it;  value_errors = (lo, hi): its return codes in (lo, hi] are a ValueError
SideBlock = collections.namedtuple("SideBlock", "attr what keys one_launch configured read off setter value_errors")
SIDE_BLOCKS = (
    SideBlock("lidar", "the lidar", "lidar_rays > 0", "the lidar observation (lidar_rays > 0)",
              lambda cfg: lidar_config(cfg)[0] > 0, lidar_params, lambda b: int(b.rays) == 0, "rg_set_lidar", (-60, -50)),
    SideBlock("teams", "a team pool", "teams", "a team pool (teams)",
              lambda cfg: cfg.get("teams") is not None, team_pool, lambda b: False, "rg_set_teams", (-70, -60)),
    SideBlock("disturbance", "the pose disturbance", "pose_noise_xy / pose_noise_theta",
              "the pose disturbance (pose_noise_xy / pose_noise_theta)", lambda cfg: any(disturbance_config(cfg)), disturbance_params,
              lambda b: float(b.sigma_xy) == 0.0 and float(b.sigma_theta) == 0.0, "rg_set_disturbance", (-80, -70)),
)


def refuse_second_block(attr, on, prefix):
    """At most one side block: ValueError if block `attr` is to go on next to a block of an earlier row for which on(row) holds.
    (A pair is refused once, in the name of its later block; `prefix` is how the caller addresses that one.)"""
    i = [b.attr for b in SIDE_BLOCKS].index(attr)
    for other in SIDE_BLOCKS[:i]:
        if on(other):
            raise ValueError(f"{prefix}: {SIDE_BLOCKS[i].what} does not combine with {other.what} ({other.keys})")


def params_to_bytes(p):
    return bytes(ctypes.string_at(ctypes.addressof(p), ctypes.sizeof(p)))


def params_from_bytes(b):
    p = RgScenarioParams()
    ctypes.memmove(ctypes.addressof(p), bytes(b), ctypes.sizeof(p))
    return p


if __name__ == "__main__":   # python -m marbler_amd.params <Scenario> <out.bin> [key=value ...]: the YAML as an rg_scenario_params blob
    import sys
    if len(sys.argv) < 3:
        raise SystemExit("usage: python -m marbler_amd.params <Scenario> <out.bin> [key=value ...]")
    ov = {}
    for kv in sys.argv[3:]:
        k, v = kv.split("=", 1)
        ov[k] = yaml.safe_load(v)
    if sys.argv[1] == "PredatorCapturePrey" and ("predator" in ov or "capture" in ov):
        cfg0 = load_config(sys.argv[1])
        ov.setdefault("n_agents", int(ov.get("predator", cfg0["predator"])) + int(ov.get("capture", cfg0["capture"])))
    with open(sys.argv[2], "wb") as fh:
        fh.write(params_to_bytes(make_params(sys.argv[1], load_config(sys.argv[1], overrides=ov))))
    print(f"wrote {sys.argv[2]} ({ctypes.sizeof(RgScenarioParams)} bytes)")
