"""The pose disturbance's case tables, shared by tests/test_gpu_disturb_forms.py (GPU) and the CPU tests that keep them honest
(tests/test_disturb_forms_cases.py: the table covers the shipped kernels; tests/test_disturb_regimes.py: the inputs of the
sigma-bound cases reach the regime they are named for), and `Regime`, the bookkeeping both sides use for the latter: everything
it counts comes from the oracle's outputs and the twin's poses, never from the GPU's.  NumPy only."""
import numpy as np

SCN = {"PredatorCapturePrey": 0, "Warehouse": 1, "MaterialTransport": 2, "Simple": 3, "ArcticTransport": 4}
QPM = {"exact": 0, "cvxopt": 1}
N_ACT = {"MaterialTransport": 20}
LAUNCH_KINDS = ("step", "rollout", "gymma")          # (ROLLOUT, GYM) = (0, 0), (1, 0), (0, 1) of disturb_step_kernel
ARENA_X, ARENA_Y = 1.6, 1.0                          # the arena's half extents (oracle/c_oracle.py bound_x0 / bound_y0)

PCP4 = {"predator": 2, "capture": 2, "n_agents": 4}
PCP5 = {"predator": 3, "capture": 2, "n_agents": 5}
PCP9 = {"predator": 5, "capture": 4, "n_agents": 9, "start_dist": 0.25, "num_neighbors": 4}
MT6 = {"n_agents": 6, "n_fast_agents": 3, "n_slow_agents": 3, "start_dist": 0.25}
MT10 = {"n_agents": 10, "n_fast_agents": 5, "n_slow_agents": 5, "start_dist": 0.25}
WH10 = {"n_agents": 10, "start_dist": 0.3}           # at 0.25 the reset grid exceeds the device sampler's 64 cells
SIMPLE12 = {"n_agents": 12, "start_dist": 0.2}


def group_width(n_agents):
    return 4 if n_agents <= 4 else 8 if n_agents <= 8 else 16


def n_agents_of(scenario, ov):
    return int(ov.get("n_agents", 4))                # every shipped YAML has four agents (ArcticTransport: always)


# ---------------------------------------------------------------- 1. every (scenario, GW, solver) triple
# (id, scenario, overrides, solver, the launch kinds the case runs)
_PAIRS = [("pcp-n4", "PredatorCapturePrey", PCP4), ("pcp-n5", "PredatorCapturePrey", PCP5), ("pcp-n9", "PredatorCapturePrey", PCP9),
          ("warehouse-n4", "Warehouse", {"n_agents": 4}), ("warehouse-n6", "Warehouse", {"n_agents": 6}), ("warehouse-n10", "Warehouse", WH10),
          ("material-n4", "MaterialTransport", {}), ("material-n6", "MaterialTransport", MT6), ("material-n10", "MaterialTransport", MT10),
          ("simple-n4", "Simple", {}), ("simple-n8", "Simple", {"n_agents": 8}), ("simple-n12", "Simple", SIMPLE12),
          ("arctic-n4", "ArcticTransport", {})]
FORM_CASES = [(name, scenario, ov, "exact", LAUNCH_KINDS) for name, scenario, ov in _PAIRS] + \
             [("ipm-" + name, scenario, ov, "cvxopt", LAUNCH_KINDS) for name, scenario, ov in _PAIRS
              if group_width(n_agents_of(scenario, ov)) != 16]          # interior-point mode has GW 4 and GW 8 only


def triple(case):
    """(SCN, GW, QPM) of disturb_step_kernel<SCN, GW, ROLLOUT, GYM, QPM> the case launches."""
    _, scenario, ov, solver, _ = case
    return SCN[scenario], group_width(n_agents_of(scenario, ov)), QPM[solver]


# ---------------------------------------------------------------- 2. the admitted bounds and one-sided sigma
BOUNDS = (0.1, 0.5)
# (id, scenario, overrides, solver, sigma, envs, steps, episode steps).  tests/test_disturb_regimes.py steps the oracle alone
# through each (its own reset twin, the GPU test's seeds and action tensor: the same run) and observes, per case: violations /
# largest QP sweep (exact) or iteration (interior-point) count / closest displaced pair in m / displaced poses outside the
# arena / headings wrap_spec turned --
#   204 / 24 / 0.0076 / 125 / 127,  567 / 40 / 0.0053 / 224 / 52,  315 / 40 / 0.0192 / 315 / 496,  251 / 40 / 0.0082 / 139 / 63,
#   755 / 40 / 0.0042 / 314 / 21,  55 / 15 / 0.0206 / 29 / 26,  74 / 16 / 0.0032 / 77 / 131,  204 / 36 / 0.0095 / 115 / 0,
#   8 / 9 / 0.1379 / 1 / 148
# against the conditions of `check_regime`: at least E violations, a pose outside the arena, a pair closer than 0.05 m, and 40
# sweeps -- the QP's limit -- in some exact-mode case; theta alone: a heading that wraps.
REGIME_CASES = [
    ("pcp-n5", "PredatorCapturePrey", PCP5, "exact", BOUNDS, 67, 12, 5),
    ("pcp-n9", "PredatorCapturePrey", PCP9, "exact", BOUNDS, 67, 12, 5),
    ("warehouse-n8", "Warehouse", {"n_agents": 8}, "exact", BOUNDS, 67, 12, 5),
    ("material-n4", "MaterialTransport", {}, "exact", BOUNDS, 67, 12, 5),
    ("simple-n12", "Simple", SIMPLE12, "exact", BOUNDS, 67, 12, 5),
    ("ipm-pcp-n5", "PredatorCapturePrey", PCP5, "cvxopt", BOUNDS, 35, 6, 3),
    ("ipm-warehouse-n8", "Warehouse", {"n_agents": 8}, "cvxopt", BOUNDS, 35, 6, 3),
    ("pcp-n5-xy-only", "PredatorCapturePrey", PCP5, "exact", (0.1, 0.0), 67, 12, 5),
    ("pcp-n5-theta-only", "PredatorCapturePrey", PCP5, "exact", (0.0, 0.5), 67, 12, 5),
]
SEED, ACTION_SEED = 13, 3                            # disturbed_vs_oracle's own


class Regime(object):
    """What a run's inputs reached, from the oracle's outputs and the twin's poses."""

    def __init__(self):
        self.violations = self.outside = self.wrapped = self.episode_ends = 0
        self.max_sweeps = 0
        self.closest = np.inf

    def see_poses(self, before, displaced):
        """`before` [E, 3, N] the stored poses, `displaced` what the twin made of them."""
        before, displaced = np.asarray(before, np.float32), np.asarray(displaced, np.float32)
        self.outside += int(((np.abs(displaced[:, 0]) > ARENA_X) | (np.abs(displaced[:, 1]) > ARENA_Y)).sum())
        # a variate is bounded at 3.46 sigma <= 1.73 rad: the heading moved by more than pi only where wrap_spec took a turn off
        self.wrapped += int((np.abs(displaced[:, 2].astype(np.float64) - before[:, 2]) > np.pi).sum())
        xy = displaced[:, :2].astype(np.float64)
        d = np.sqrt(((xy[:, :, :, None] - xy[:, :, None, :]) ** 2).sum(axis=1))
        d[:, np.arange(d.shape[1]), np.arange(d.shape[1])] = np.inf
        self.closest = min(self.closest, float(d.min()))

    def see_step(self, done, violation, qp_sweeps):
        self.episode_ends += int(np.asarray(done).astype(bool).sum())
        self.violations += int((np.asarray(violation) > 0).sum())
        self.max_sweeps = max(self.max_sweeps, int(np.asarray(qp_sweeps).max()))

    def figures(self):
        return (self.violations, self.max_sweeps, round(self.closest, 4), self.outside, self.wrapped)


def check_regime(name, sigma, E, r):
    """The conditions of a sigma-bound case (the sweep cap is checked over the exact-mode cases together, by the caller)."""
    if sigma[0] == 0.0:
        assert r.wrapped >= 1, f"{name}: no heading crossed +-pi in the twin's update"
        return
    assert r.violations >= E, f"{name}: {r.violations} violations in a run of {E} envs"
    assert r.outside >= 1, f"{name}: no displaced pose outside the arena"
    assert r.closest < 0.05, f"{name}: the closest displaced pair is {r.closest:.4f} m apart"
