"""The render cases the CPU and the GPU tier share (tests/test_render_cases.py, tests/test_gpu_render.py): scenario shapes, image
shapes, views, and seeded hand-made states.  The CPU tier asserts the twin's degenerate share on these very states; the GPU tier
loads them into an env and renders them, besides the env's own states after reset() and after some steps.

ArcticTransport's terrain squares have their sides on the lattice x = 0.25 j - 1.5, y = 1 - 0.25 i.  With the arena as the view,
whole pixel rows and columns have their centres ON that lattice (48 wide: column 16 lies at x = -0.5; 12 high: every third row;
84 high: rows 10, 31, 52, 73), and a centre on an edge is degenerate by definition: 2 - 33 % of the image, far above the 0.5 % cap
that keeps the comparison honest.  The same happens to the zone rectangles of Warehouse and MaterialTransport at 48 columns: their
inner sides x = +-(1.5 - width) = +-1.1 are the centres of columns 7 and 40.  Those cases (ON_LATTICE) therefore show the arena
through a view that is a little larger and off the lattice (OFF_LATTICE_VIEW); the image shapes stay, and the other cases of the
same scenarios render the arena itself (view None).  PredatorCapturePrey at 48 columns joins them for its reset states: the robots
start on a grid of spacing start_dist = 0.3 m or 0.2 m, 4.5 or 3 pixels of 1 / 15 m, so every ring of a class meets the pixel
centres in the same phase and what would be noise around 0.2 % becomes 0.4 % (N = 5) and 1.2 % (N = 16) in one image.
"""
import numpy as np

SCENARIOS = {"PredatorCapturePrey": {"predator": 3, "capture": 2, "n_agents": 5},
             "Warehouse": {"n_agents": 8},
             "MaterialTransport": {"n_agents": 6, "n_fast_agents": 3, "n_slow_agents": 3, "start_dist": 0.25},
             "Simple": {},
             "ArcticTransport": {}}
# further shapes: many prey, and sixteen agents (the exact-projection mode, the default barrier solver)
EXTRA = {"pcp-prey24": ("PredatorCapturePrey", dict(SCENARIOS["PredatorCapturePrey"], num_prey=24)),
         "pcp-n16": ("PredatorCapturePrey", {"predator": 8, "capture": 8, "n_agents": 16, "start_dist": 0.2})}

OFF_LATTICE_VIEW = (-1.6137, -1.0171, 3.2291, 2.0347)
ON_LATTICE = {("ArcticTransport", "48x32-k3"), ("ArcticTransport", "20x12"), ("ArcticTransport", "84x84"),
              ("Warehouse", "48x32-k3"), ("MaterialTransport", "48x32-k3"), ("PredatorCapturePrey", "48x32-k3")}
WIDE_VIEW = (-2.013, -1.507, 4.031, 3.017)
MAX_DEGENERATE_SHARE = 0.005
# the sampler key of a case's env where it is not 11: the states an env reaches are a function of the key, and a few keys put
# many edges within 1e-4 m of pixel centres at once (the reset grid's spacing is a whole number of pixels at some shapes)
ENV_SEED = {"PredatorCapturePrey-20x12": 12, "PredatorCapturePrey-zoom": 16, "pcp-n16-48x32-k3": 15, "pcp-n16-84x84": 15}

# (id, E, envs, (H, W), view): view None = the arena, "zoom" = 1 m x 1 m about robot 0 of the first rendered env
SHAPES = (("48x32-k3", 5, [4, 0, 2], (32, 48), None),
          ("20x12", 5, None, (12, 20), None),
          ("84x84", 2, None, (84, 84), None),
          ("zoom", 5, [1], (64, 96), "zoom"),
          ("wide", 5, [3, 1], (32, 48), WIDE_VIEW))


def all_cases():
    """(case id, group, scenario, overrides, shape id, E, envs, (H, W), view); a case's hand-made state has the seed len(case id)"""
    for scenario, ov in SCENARIOS.items():
        for shape in SHAPES:
            yield (scenario + "-" + shape[0], scenario, scenario, ov) + shape
    for name, (scenario, ov) in EXTRA.items():
        for shape in (SHAPES[0], SHAPES[2]):
            yield (name + "-" + shape[0], name, scenario, ov) + shape


def case_view(scenario, shape, view, poses_first):
    """the view tuple of a case (`shape`: its id in SHAPES): poses_first is [3, N] of the first rendered env (for the zoom)"""
    if isinstance(view, str):
        x, y = float(poses_first[0, 0]), float(poses_first[1, 0])
        return (x - 0.5, y - 0.5, 1.0, 1.0)
    if view is None and (scenario, shape) in ON_LATTICE:
        return OFF_LATTICE_VIEW
    return view


def synthetic_state(params, E, seed):
    """E hand-made env states (float32 / uint8 arrays with a leading E axis) for the parameter block: robots anywhere in the arena
    with any heading, prey anywhere with random flags, a random terrain."""
    r = np.random.RandomState(seed)
    N, P = int(params.n_agents), max(int(params.num_prey), 1)
    x0, y0, w, h = params.bound_x0, params.bound_y0, params.bound_w, params.bound_h
    poses = np.empty((E, 3, N), np.float32)
    poses[:, 0] = r.uniform(x0 + 0.05, x0 + w - 0.05, (E, N))
    poses[:, 1] = r.uniform(y0 + 0.05, y0 + h - 0.05, (E, N))
    poses[:, 2] = r.uniform(-np.pi, np.pi, (E, N))
    prey = np.stack([r.uniform(x0, x0 + w, (E, P)), r.uniform(y0, y0 + h, (E, P))], axis=-1).astype(np.float32)
    grid = r.randint(0, 4, (E, 96)).astype(np.uint8)
    return {"poses": poses, "prey_loc": prey, "prey_sensed": (r.rand(E, P) < 0.4).astype(np.uint8),
            "prey_captured": (r.rand(E, P) < 0.3).astype(np.uint8), "grid": grid}


def env_state(state, e):
    return {k: v[e] for k, v in state.items()}
