"""The directed cases of tests/test_gpu_physical_constants.py reach the regime they are named for -- shown without a GPU.

The float32 oracle alone, free-running with the reset twin of tests/helpers.py: the configuration, batch, seeds, length and
action stream of the GPU cases on the `rows-resident` dispatch (physical_cases.py), so -- the GPU being held to the oracle word
for word there -- the same run.  Per case, from the oracle's outputs and poses alone:

  ended episodes / violations with the collision bit / with the boundary bit / largest QP sweep count /
  agent-steps whose heading turned by more than 0.25 rad per sub-step / by less / env-steps that begin with a robot beyond
  2 m from the origin / env-steps in whose last controller period some robot's sub-step is long enough to switch the sparse
  pre-test off (lin_pre + 4 |dt v| >= 0.24, step_group.h sparse_ok) / in which no robot's can be / boundary violations in an
  episode's first step (a reset pose outside the arena, not a robot that walked out)

`FIGURES` holds them as exact numbers (python tests/test_physical_regimes.py prints the table): a drifting seed, helper or
constant shows up here first.  They were read off the oracle, never off the code under test."""
import numpy as np
import pytest

from oracle_check import FreeRunningOracle
from physical_cases import (ACTION_SEED, CASES, DISPATCHES, IPM_CASES, N_ACT, REGIME_DISPATCH, REGIMES, RPS_DEFAULTS, SEED, STEPS,
                            case_overrides, check_constants)

from marbler_amd.params import load_config, make_params

DISPATCH = next(d for d in DISPATCHES if d[0] == REGIME_DISPATCH)

FIGURES = {
    "wide-angle": (131, 1, 2, 11, 2497, 7238, 0, 0, 1945, 0),
    "mixed-waves": (159, 20, 26, 13, 203, 9317, 0, 0, 1904, 0),
    "dense-only": (713, 607, 7, 16, 0, 0, 0, 1336, 0, 0),
    "fast-robots": (245, 89, 91, 12, 0, 8855, 0, 1024, 390, 0),
    "large-arena": (130, 1, 0, 12, 0, 0, 1950, 0, 1949, 0),
    "off-centre-arena": (131, 1, 3, 12, 0, 0, 0, 0, 1946, 0),
    "tight-arena": (178, 1, 67, 8, 0, 0, 0, 0, 1882, 0),
    "offset-0.06": (131, 1, 3, 12, 0, 0, 0, 0, 1946, 0),
    "offset-negative": (152, 33, 3, 9, 0, 0, 0, 0, 1914, 0),
    "offset-zero": (137, 10, 3, 10, 0, 0, 0, 0, 1937, 0),
    "projection-0.02": (130, 0, 0, 11, 0, 0, 0, 0, 1950, 0),
    "projection-0.1": (174, 30, 49, 10, 0, 0, 0, 0, 1871, 0),
    "wide-robot": (131, 0, 1, 13, 0, 0, 0, 0, 1949, 0),
}


def wrap(d):
    return (d + np.pi) % (2.0 * np.pi) - np.pi


def oracle_alone(oracle_lib, regime, dispatch=DISPATCH, steps=STEPS):
    _, scenario, _, _, _, E, _, _, _ = dispatch
    ov, consts = case_overrides(regime, dispatch)
    cfg = load_config(scenario, overrides=ov)
    params = make_params(scenario, cfg)
    side = FreeRunningOracle(oracle_lib, scenario, cfg, E, params, SEED)
    orc = side.orc
    check_constants(orc.p, consts)
    check_constants(params, consts)
    side.reset()
    rng = np.random.RandomState(ACTION_SEED)
    U = int(cfg["update_frequency"])
    one_period = U <= 15 and not cfg.get("robotarium", False)
    ended = coll = bnd = sweeps = wide = narrow = far = fast = slow = fresh = 0
    c = dict(RPS_DEFAULTS, **consts)
    room = (0.24 - lin_pre(consts)) / 4.0            # sparse_ok: lin_pre + 4 max(|dt v| + |offset| |dt w|) < 0.24
    chord = abs(c["collision_offset"]) * c["time_step"] * c["angular_velocity_limit"]
    for t in range(steps):
        a = rng.randint(0, N_ACT.get(scenario, 5), size=(E, orc.N)).astype(np.int32)
        before = orc.poses.copy()
        far += int((np.hypot(before[:, 0], before[:, 1]) > 2.0).any(axis=1).sum())
        first_step = orc.steps == 0
        _, _, done, info = orc.step(a)
        viol = info["violation"]
        fresh += int((((viol & 2) != 0) & first_step).sum())
        if one_period:   # v, w held for the whole step: |delta theta| = U |dt w| up to one rounding
            ok = viol == 0
            turn = np.abs(wrap(orc.poses[ok, 2].astype(np.float64) - before[ok, 2])) / U
            wide += int((turn > 0.25).sum())
            narrow += int((turn <= 0.25).sum())
        # carry_dist is |dt v| of the step's last controller period: a lower bound of M (step_group.h mstep), and with the
        # largest chord term an upper bound
        last = orc.carry[viol == 0].astype(np.float64).max(axis=1, initial=0.0)
        fast += int((last >= 1.02 * room).sum())
        slow += int((last + chord < 0.98 * room).sum())
        ended += int(done.sum())
        coll += int(((viol & 1) != 0).sum())
        bnd += int(((viol & 2) != 0).sum())
        sweeps = max(sweeps, int(orc.qp_sweeps.max()))
        assert all(np.isfinite(x).all() for x in (orc.obs, orc.reward, orc.poses)), t
        side.reset_ended()
    return (ended, coll, bnd, sweeps, wide, narrow, far, fast, slow, fresh)


def pre_margin(max_abs_coordinate):
    """csrc/kernel_args.h pre_margin, restated."""
    spacing, lim = 2.0 ** -10, 2.0
    while lim <= max_abs_coordinate and lim < 1024.0:
        spacing, lim = 2.0 * spacing, 2.0 * lim
    return 1.05 * 1.41421356 * (2.0 * spacing + 2.0 ** -14)


def lin_pre(consts):
    c = dict(RPS_DEFAULTS, **consts)
    reach = max(abs(c["bound_x0"]), abs(c["bound_x0"] + c["bound_w"]), abs(c["bound_y0"]), abs(c["bound_y0"] + c["bound_h"]))
    return c["collision_diameter"] + pre_margin(reach + 0.25)


@pytest.fixture(scope="module")
def figures(oracle_lib):
    return {r[0]: oracle_alone(oracle_lib, r) for r in REGIMES}


@pytest.mark.parametrize("regime", REGIMES, ids=[r[0] for r in REGIMES])
def test_the_case_reaches_its_regime(regime, figures):
    name, consts = regime[0], regime[1]
    got = figures[name]
    print(f"{name}: ended / collision / boundary / max sweeps / wide / narrow / far / fast / slow / fresh = {got}")
    assert got == FIGURES[name], (name, got, FIGURES[name])
    ended, coll, bnd, sweeps, wide, narrow, far, fast, slow, fresh = got
    E = DISPATCH[5]
    assert ended >= E, "fewer than one ended episode per env"
    assert sweeps > 2, "no QP of more than two sweeps"
    c = dict(RPS_DEFAULTS, **consts)
    if name == "wide-angle":
        assert c["time_step"] * c["angular_velocity_limit"] > 0.25 and wide > 0
    if name == "mixed-waves":
        assert wide > 0 and narrow > 0
    if name == "dense-only":
        assert lin_pre(consts) >= 0.24            # sparse_ok (csrc/step_group.h) is false whatever the robots' travel
        assert coll > 0 and slow == 0
    if name == "fast-robots":
        assert fast > 0 and slow > 0             # sparse_ok false in some periods, true in others
    elif name != "dense-only":
        assert fast == 0                         # elsewhere the sparse pre-test stays on
    if name == "large-arena":
        assert pre_margin(8.25) == 1.05 * 1.41421356 * (2.0 * 2.0 ** -7 + 2.0 ** -14)           # the 2^-7 spacing of [8, 16) m
        assert far == STEPS * E and coll > 0 and bnd == 0
    if name == "off-centre-arena":
        assert c["bound_x0"] + 0.5 * c["bound_w"] != 0.0 and c["bound_y0"] + 0.5 * c["bound_h"] != 0.0
        assert coll > 0
    if name == "tight-arena":
        # boundary violations every few steps, every one of them by a robot that walked through a wall
        assert bnd >= STEPS // 3 and fresh == 0 and bnd > coll


# ---------------------------------------------------------------- the pre-test's bound, from the number formats alone
def pretest_figure(x0, y0, x1, y1):
    """What the collision pre-test computes of two collision points (csrc/step_group.h pair_min): both rounded toward zero to
    binary16, the packed difference rounded to nearest binary16, the squares summed."""
    from physical_cases import half_toward_zero
    dx = np.float16(half_toward_zero(x0) - half_toward_zero(x1)).astype(np.float64)
    dy = np.float16(half_toward_zero(y0) - half_toward_zero(y1)).astype(np.float64)
    return dx * dx + dy * dy


@pytest.mark.parametrize("reach", [1.6, 3.2, 8.0, 30.0, 100.0])
@pytest.mark.parametrize("lim", [0.11, 0.135, 0.3, 1.0])
def test_the_pretest_never_misses_inside_the_admitted_domain(reach, lim):
    """Pairs exactly `lim` apart, anywhere within the arena plus 0.25 m, for the largest arena and collision limits rg_create
    admits (include/robogym.h): the binary16 figure stays below thr_pre as make_consts computes it."""
    rng = np.random.RandomState(int(reach * 10) + int(lim * 1000))
    n = 200000
    # half of the pairs just below a power of two, where the spacing assumed is the tightest
    edge = 2.0 ** np.floor(np.log2(reach + 0.25))
    cx = np.where(rng.rand(n) < 0.5, rng.uniform(-reach - 0.25, reach + 0.25, n), rng.choice([-1.0, 1.0], n) * (edge - rng.uniform(0, 2 * lim, n)))
    cy = rng.uniform(-reach - 0.25, reach + 0.25, n)
    b = rng.uniform(-np.pi, np.pi, n)
    x0, y0 = np.float32(cx + 0.5 * lim * np.cos(b)), np.float32(cy + 0.5 * lim * np.sin(b))
    x1, y1 = np.float32(cx - 0.5 * lim * np.cos(b)), np.float32(cy - 0.5 * lim * np.sin(b))
    inside = (np.abs(np.stack([x0, x1, y0, y1])) <= reach + 0.25).all(axis=0)
    lp = np.float32(lim) + np.float32(pre_margin(reach + 0.25))
    thr = np.float32(np.float32(lp * lp) * np.float32(1.00001))
    fig = pretest_figure(x0, y0, x1, y1)[inside]
    assert inside.sum() > n // 2 and (fig <= float(thr)).all(), float(np.sqrt(fig.max()) - lp)


def _stray_oracle(oracle_lib, n_agents, pose_id):
    from physical_cases import STRAY_E, STRAY_TEAMS, stray_poses
    scenario = "PredatorCapturePrey"
    cfg = load_config(scenario, overrides=dict(STRAY_TEAMS[n_agents], penalize_violations=True))
    orc = FreeRunningOracle.at_reset(oracle_lib, scenario, cfg, STRAY_E, make_params(scenario, cfg), SEED)
    orc.poses[...] = stray_poses(orc.poses, pose_id)
    return cfg, orc


def test_stray_placements_defeat_the_binary16_figure(oracle_lib):
    """At x = 5 and x = 20 the loaded pairs collide, yet their binary16 image is farther apart than thr_pre allows: a replay that
    trusts the figure there reports no collision.  (What makes tests/test_gpu_physical_constants.py's stray poses bite.)"""
    from physical_cases import RPS_DEFAULTS as D, collision_points
    lp = np.float32(D["collision_diameter"]) + np.float32(pre_margin(1.6 + 0.25))
    thr = float(np.float32(np.float32(lp * lp) * np.float32(1.00001)))
    for pose_id, least in (("x5", 8), ("x20", 64)):
        _, orc = _stray_oracle(oracle_lib, 5, pose_id)
        fx, fy = collision_points(orc.poses, D["collision_offset"])
        assert (np.hypot(fx[:, 0] - fx[:, 1], fy[:, 0] - fy[:, 1]) < D["collision_diameter"] - 0.0005).all()
        missed = int((pretest_figure(fx[:, 0], fy[:, 0], fx[:, 1], fy[:, 1]) > thr).sum())
        print(pose_id, "envs whose binary16 figure exceeds thr_pre:", missed)
        assert missed >= least, (pose_id, missed)


@pytest.mark.parametrize("n_agents", [4, 5, 8, 12])
def test_the_oracle_judges_the_loaded_pairs_as_the_gpu_test_expects(n_agents, oracle_lib):
    """Violation 3 (collision and boundary) for every stray pose, the pair across the wall included; 1 (collision alone) for the
    pair inside the large arena.  The GPU test asserts the same before it steps the device."""
    from physical_cases import LARGE_ARENA, NO_OP, STRAY_E, STRAY_POSES, large_arena_poses
    for pose_id, _, _ in STRAY_POSES:
        _, orc = _stray_oracle(oracle_lib, n_agents, pose_id)
        _, _, done, info = orc.step(np.full((STRAY_E, orc.N), NO_OP, np.int32))
        assert set(info["violation"].tolist()) == {3} and done.all(), (pose_id, np.bincount(info["violation"]))
    if n_agents == 5:
        ov, _ = case_overrides(LARGE_ARENA, DISPATCH)
        cfg = load_config("PredatorCapturePrey", overrides=dict(ov, penalize_violations=True))
        orc = FreeRunningOracle.at_reset(oracle_lib, "PredatorCapturePrey", cfg, STRAY_E, make_params("PredatorCapturePrey", cfg), SEED)
        orc.poses[...] = large_arena_poses(orc.poses)
        # a bound sized for the default arena would miss some of these pairs; the large arena's own holds for all of them
        from physical_cases import RPS_DEFAULTS as D, collision_points
        fx, fy = collision_points(orc.poses, D["collision_offset"])
        fig = np.sqrt(pretest_figure(fx[:, 0], fy[:, 0], fx[:, 1], fy[:, 1]))
        assert (fig > D["collision_diameter"] + pre_margin(1.85)).sum() >= 8 and (fig < lin_pre(LARGE_ARENA[1])).all()
        _, _, done, info = orc.step(np.full((STRAY_E, orc.N), NO_OP, np.int32))
        assert set(info["violation"].tolist()) == {1}, np.bincount(info["violation"])


def test_every_fuzz_draw_lies_inside_the_admitted_domain():
    """rg_create refuses a block outside the domain before it looks for a device: no draw of the GPU fuzz may be refused for
    its constants (without a GPU the call then fails for want of a device; with one it succeeds)."""
    import ctypes
    from marbler_amd import _lib
    lib = _lib.load()
    lib.rg_create.restype = ctypes.c_void_p
    seen = {k: set() for k in RPS_DEFAULTS}
    for scenario, ov, _, E, _ in CASES + IPM_CASES:
        p = make_params(scenario, load_config(scenario, overrides=ov))
        for k in seen:
            seen[k].add(ov[k])
        h = lib.rg_create(ctypes.byref(p), E, 0, 0, None)
        if h:
            assert lib.rg_destroy(ctypes.c_void_p(h)) == 0
        else:
            assert b"HIP device" in lib.rg_last_error(), (scenario, ov, lib.rg_last_error())
    assert all(len(v) >= 2 for v in seen.values()), seen       # every one of the 13 fields varies over the draws
    assert {0.01, 0.033, 0.05, 0.1} <= seen["time_step"]


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import c_oracle
    c_oracle.build_library()
    for r in REGIMES:
        print(f'    "{r[0]}": {oracle_alone(c_oracle, r)},')
