"""The case tables of the physical-constants tier, shared by tests/test_gpu_physical_constants.py (GPU) and
tests/test_physical_regimes.py (CPU: every directed case reaches the regime it is named for, shown on the oracle alone).

The 13 rps constants of rg_scenario_params (include/robogym.h "rps constants") are config keys of their own names on both
sides: marbler_amd/params.py make_params writes them into the device's block, oracle/c_oracle.py params_from_config into the
oracle's.  NumPy only."""
import numpy as np

# the default point, restated: the tests hold both sides' blocks to these numbers
RPS_DEFAULTS = {"time_step": 0.033, "bound_x0": -1.6, "bound_y0": -1.0, "bound_w": 3.2, "bound_h": 2.0,
                "robot_diameter": 0.11, "wheel_radius": 0.016, "max_linear_velocity": 0.2,
                "collision_offset": 0.025, "collision_diameter": 0.135,
                "projection_distance": 0.05, "angular_velocity_limit": float(np.pi), "position_velocity_limit": 0.15}
SEED, ACTION_SEED = 99, 5                      # rollout_harness.rollout_bit_exact's own
STEPS, EPISODE = 30, 10

PCP4 = {"predator": 2, "capture": 2, "n_agents": 4}
PCP5 = {"predator": 3, "capture": 2, "n_agents": 5}
PCP12 = {"predator": 6, "capture": 6, "n_agents": 12, "num_prey": 10, "start_dist": 0.25, "num_neighbors": 4}
WH8 = {"n_agents": 8}
MT6 = {"n_agents": 6, "n_fast_agents": 3, "n_slow_agents": 3, "start_dist": 0.25}
N_ACT = {"MaterialTransport": 20}


def arena(x0, y0, w, h):
    return {"bound_x0": x0, "bound_y0": y0, "bound_w": w, "bound_h": h}


# PredatorCapturePrey in the large arena: the scenario's own rectangle moved next to the far wall, so that every robot lives at
# |x| in [6, 7.6] m, where binary16's spacing is 2^-8 m (the arena plus 0.25 m reaches 8.25 m: pre_margin takes 2^-7)
FAR_PCP = {"LEFT": -7.5, "RIGHT": 7.5, "ROBOT_INIT_RIGHT_THRESH": -6.5, "PREY_INIT_LEFT_THRESH": 6.5}

# PredatorCapturePrey in the tight arena: every reset cell inside it (x in [-1.25, 0.85], |y| <= 0.75) and spread towards the right
# wall, which the goals' own limit (RIGHT = 1.4) lies beyond: robots WALK through the wall at x = 1.3 within a few steps
TIGHT_PCP = {"LEFT": -1.25, "UP": -0.75, "DOWN": 0.75, "ROBOT_INIT_RIGHT_THRESH": 1.0}

# (id, constants, config overrides that go with them, the same per scenario).  `update_frequency` is dropped where a dispatch
# needs the scenario's own (the shaped kernels compile it in).
REGIMES = [
    ("wide-angle", {"time_step": 0.1}, {"update_frequency": 5}, {}),
    ("mixed-waves", {"time_step": 0.08, "angular_velocity_limit": 3.5}, {"update_frequency": 10}, {}),
    # (a safety radius above the collision limit: otherwise the barrier itself parks robots inside it)
    ("dense-only", {"collision_diameter": 0.3}, {"safety_radius": 0.36}, {}),
    # The issue's draft of this case (position_velocity_limit 0.4, time_step 0.05) cannot reach its regime: the position
    # controller's speed is the distance to the goal (step_dist, 0.2 m) capped at position_velocity_limit and thresholded at
    # magnitude_limit (0.2 m/s) before the barrier, and sparse_ok needs |dt v| + |offset| |dt w| >= (0.24 - lin_pre) / 4 =
    # 0.0255 m.  Replaced by one that does: goals 0.5 m away, both limits 0.5 m/s, 0.06 s, one controller period per step.
    ("fast-robots", {"max_linear_velocity": 0.5, "position_velocity_limit": 0.5, "time_step": 0.06},
     {"magnitude_limit": 0.5, "update_frequency": 10},
     {"PredatorCapturePrey": {"step_dist": 0.5, "PREY_INIT_LEFT_THRESH": -1.1}, "Warehouse": {"step_dist": 0.5}}),
    ("large-arena", arena(-8.0, -5.0, 16.0, 10.0), {}, {"PredatorCapturePrey": FAR_PCP}),
    ("off-centre-arena", arena(-1.6, -1.0, 4.8, 2.5), {}, {}),
    ("tight-arena", arena(-1.3, -0.8, 2.6, 1.6), {}, {"PredatorCapturePrey": TIGHT_PCP}),
    ("offset-0.06", {"collision_offset": 0.06}, {"collision_variant": "offset"}, {}),
    ("offset-negative", {"collision_offset": -0.025}, {"collision_variant": "offset"}, {}),
    ("offset-zero", {"collision_offset": 0.0}, {"collision_variant": "offset"}, {}),
    ("projection-0.02", {"projection_distance": 0.02}, {}, {}),
    ("projection-0.1", {"projection_distance": 0.1}, {}, {}),
    ("wide-robot", {"robot_diameter": 0.15, "wheel_radius": 0.03}, {}, {}),
]
REGIME_IDS = [r[0] for r in REGIMES]

# (id, scenario, overrides, step kernel, what rg_create reads from the environment, envs, solver, the form rg_step_form reports:
# "by-value" | "resident" | "shape" | None = the thread-per-env kernel, keeps `update_frequency`)
DISPATCHES = [
    ("gw4", "PredatorCapturePrey", PCP4, "group", {}, 65, "exact", "by-value", True),
    ("rows-by-value", "PredatorCapturePrey", PCP5, "group", {"RG_STEP_RESIDENT": "0"}, 65, "exact", "by-value", True),
    ("rows-resident", "PredatorCapturePrey", PCP5, "group", {"RG_STEP_SHAPE": "0"}, 65, "exact", "resident", True),
    ("rows-shape-pcp", "PredatorCapturePrey", PCP5, "group", {}, 65, "exact", "shape", False),
    ("rows-shape-pcp-1026", "PredatorCapturePrey", PCP5, "group", {}, 1026, "exact", "shape", False),
    ("rows-shape-warehouse", "Warehouse", WH8, "group", {}, 65, "exact", "shape", False),
    ("rows-shape-material", "MaterialTransport", MT6, "group", {}, 65, "exact", "shape", False),
    ("gw8-no-rows", "PredatorCapturePrey", PCP5, "group", {"RG_STEP_SPAN": "0"}, 65, "exact", "by-value", True),
    ("gw16", "PredatorCapturePrey", PCP12, "group", {}, 65, "exact", "by-value", True),
    ("tpe", "PredatorCapturePrey", PCP5, "tpe", {}, 65, "exact", None, True),
    ("ipm-gw4", "PredatorCapturePrey", PCP4, "group", {}, 65, "cvxopt", "by-value", True),
    ("ipm-gw8", "PredatorCapturePrey", PCP5, "group", {}, 65, "cvxopt", "by-value", True),
    ("ipm-tpe", "PredatorCapturePrey", PCP5, "tpe", {}, 65, "cvxopt", None, True),
]
DISPATCH_IDS = [d[0] for d in DISPATCHES]
# the dispatch tests/test_physical_regimes.py steps the oracle through (the oracle knows no dispatch: its configuration and batch)
REGIME_DISPATCH = "rows-resident"


def case_overrides(regime, dispatch):
    """The config overrides of a directed case, and its constants alone."""
    _, consts, extra, per_scenario = regime
    _, scenario, ov, _, _, _, solver, _, keeps_u = dispatch
    out = dict(ov, max_episode_steps=EPISODE, barrier_solver=solver, **consts)
    out.update({k: v for k, v in extra.items() if keeps_u or k != "update_frequency"})
    out.update(per_scenario.get(scenario, {}))
    return out, dict(consts)


def check_constants(block, consts):
    """`block` (either side's parameter block) holds the case's constants and the defaults elsewhere, as binary32."""
    for key, default in RPS_DEFAULTS.items():
        want = np.float32(consts.get(key, default))
        assert np.float32(getattr(block, key)) == want, (key, getattr(block, key), want)


# ---------------------------------------------------------------- the seeded fuzz
CHOICES = {"time_step": [0.01, 0.033, 0.05, 0.06, 0.08, 0.1],
           "robot_diameter": [0.11, 0.15], "wheel_radius": [0.016, 0.03],
           "max_linear_velocity": [0.2, 0.5], "position_velocity_limit": [0.15, 0.4, 0.5],
           "collision_offset": [0.025, 0.06, -0.025, 0.0], "collision_diameter": [0.135, 0.3],
           "projection_distance": [0.05, 0.02, 0.1], "angular_velocity_limit": [float(np.pi), 3.5]}
ARENAS = [(-1.6, -1.0, 3.2, 2.0), (-8.0, -5.0, 16.0, 10.0), (-1.6, -1.0, 4.8, 2.5), (-1.3, -0.8, 2.6, 1.6)]


def draw_constants(rng):
    """Every one of the 13 fields from a short list: its default and the directed table's values."""
    c = {k: float(v[rng.randint(len(v))]) for k, v in sorted(CHOICES.items())}
    c.update(arena(*ARENAS[rng.randint(len(ARENAS))]))
    return c


def draw_physical(rng, draw_config):
    scenario, ov, n_act, E, kernel = draw_config(rng)
    ov = dict(ov, **draw_constants(rng))
    ov["max_episode_steps"] = int(rng.choice([3, 7, 12]))
    return scenario, ov, n_act, E, kernel


def _fuzz_cases():
    from fuzz_cases import draw_config, draw_interior_point
    return ([draw_physical(np.random.RandomState(9000 + i), draw_config) for i in range(96)],
            [draw_physical(np.random.RandomState(9500 + i), draw_interior_point) for i in range(24)])


CASES, IPM_CASES = _fuzz_cases()          # the seeded fuzz over all 13 constants, exact and interior-point mode


# ---------------------------------------------------------------- binary16, as the collision pre-test rounds (csrc/kernel_args.h)
def half_toward_zero(v):
    """binary32 -> binary16 rounded toward zero (v_cvt_pkrtz_f16_f32), as float64; finite values saturate at 65504."""
    v = np.asarray(v, np.float32).astype(np.float64)
    a = np.abs(v)
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -14)))
    q = 2.0 ** (e - 10)
    return np.sign(v) * np.minimum(np.floor(a / q) * q, 65504.0)


def collision_points(poses, offset):
    """poses [E, 3, N] -> the collision points' x, y [E, N] in float64 (to within a binary32 rounding of the kernels' fma)."""
    p = np.asarray(poses, np.float32).astype(np.float64)
    return p[:, 0] + offset * np.cos(p[:, 2]), p[:, 1] + offset * np.sin(p[:, 2])


def rounded_distance(poses, offset, i=0, j=1):
    """The distance of robots i and j's collision points after both are rounded to binary16: what the pre-test looks at."""
    fx, fy = collision_points(poses, offset)
    hx, hy = half_toward_zero(fx), half_toward_zero(fy)
    return np.hypot(hx[:, i] - hx[:, j], hy[:, i] - hy[:, j])


def placed_pairs(base_poses, centre, gap, rng, pick=None, bearing=(-np.pi, np.pi), jitter=0.02):
    """base_poses [E, 3, N] with robots 0 and 1 of every env made a pair `gap` apart (centre to centre; one heading, so their
    collision points are as far apart), centred at `centre` +- jitter, at a random bearing and heading; the other robots stay.
    pick(poses) -> a score per env: 64 candidates are drawn per env and the E highest-scoring of them kept."""
    E = base_poses.shape[0]
    n_cand = 64 * E if pick is not None else E
    poses = np.ascontiguousarray(base_poses[np.arange(n_cand) % E], np.float32)
    b, heading = rng.uniform(bearing[0], bearing[1], n_cand), rng.uniform(-np.pi, np.pi, n_cand)
    cx, cy = centre[0] + rng.uniform(-jitter, jitter, n_cand), centre[1] + rng.uniform(-jitter, jitter, n_cand)
    for k, sgn in ((0, 0.5), (1, -0.5)):
        poses[:, 0, k] = cx + sgn * gap * np.cos(b)
        poses[:, 1, k] = cy + sgn * gap * np.sin(b)
        poses[:, 2, k] = heading
    if pick is not None:
        poses = poses[np.sort(np.argsort(-pick(poses), kind="stable")[:E])]
    return poses


# ---------------------------------------------------------------- stray poses (default constants, penalize_violations on)
STRAY_E = 64
STRAY_TEAMS = {4: PCP4, 5: PCP5, 8: {"predator": 4, "capture": 4, "n_agents": 8}, 12: PCP12}
GAP = RPS_DEFAULTS["collision_diameter"] - 0.001          # collision points 1 mm inside the collision distance
# (id, pair centre, the violation code the oracle must report; None = whatever it reports, asserted equal on both sides)
STRAY_POSES = [("x5", (5.0, 5.0), 3), ("x20", (20.0, 0.0), 3), ("ghost", (1018.0, -1000.0), 3), ("x1e5", (1e5, 0.0), 3),
               ("wall", (1.6, 0.0), None)]
NO_OP = 4                                                  # the action that keeps the goal where the robot is


def stray_poses(base_poses, pose_id, seed=7):
    """The loaded poses of a stray-pose case.  x5, x20: of 64 random placements per env the ones whose binary16 image is
    farthest apart -- where the pre-test's figure is least a bound.  (x5 is centred at y = 5 as well: with y inside the arena
    the x error alone, below 2^-8 m, stays 0.1 mm short of the default rounding bound.)  x1e5: binary32's own spacing there is 2^-7 m, so the pair
    lies along x, 17 / 128 m apart (the largest representable gap inside the collision distance less 1 mm) at one heading: both
    collision points round alike.  wall: the pair along x +- 0.5 rad across the wall x = 1.6, one robot on either side."""
    rng = np.random.RandomState(seed)
    centre = dict((p[0], p[1]) for p in STRAY_POSES)[pose_id]
    off = RPS_DEFAULTS["collision_offset"]
    if pose_id in ("x5", "x20"):
        return placed_pairs(base_poses, centre, GAP, rng, pick=lambda p: rounded_distance(p, off))
    if pose_id == "ghost":
        return placed_pairs(base_poses, centre, GAP, rng)
    if pose_id == "wall":
        return placed_pairs(base_poses, centre, GAP, rng, bearing=(-0.5, 0.5), jitter=0.0)
    poses = np.ascontiguousarray(base_poses, np.float32).copy()
    y, heading = rng.uniform(-0.5, 0.5, len(poses)), rng.uniform(-np.pi, np.pi, len(poses))
    for k, x in ((0, 1e5), (1, 1e5 + 17.0 / 128.0)):
        poses[:, 0, k], poses[:, 1, k], poses[:, 2, k] = x, y, heading
    return poses


# ---------------------------------------------------------------- a colliding pair inside the large arena
LARGE_ARENA = next(r for r in REGIMES if r[0] == "large-arena")
LARGE_ARENA_PAIR = (-6.0, -4.5)      # both coordinates in [4, 8) m: binary16 spacing 2^-8 m, four times the default arena's


def large_arena_poses(base_poses, seed=11):
    """Pairs 1 mm inside the collision distance, inside the arena: the ones a rounding bound for the default arena would miss."""
    return placed_pairs(base_poses, LARGE_ARENA_PAIR, GAP, np.random.RandomState(seed),
                        pick=lambda p: rounded_distance(p, RPS_DEFAULTS["collision_offset"]))
