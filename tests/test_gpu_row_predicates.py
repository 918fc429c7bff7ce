"""The 16-lane-row step kernels with their lane predicates held as wave masks (csrc/step_group.h step_once PM; csrc/device_common.h
lane_mask), word for word against the float32 oracle and against the same handle on 8-lane groups (RG_STEP_SPAN=0), 40 steps
each with auto-reset.  Every predicate is taken through both of its values:

  env_ok      E = 1, 3, 5, 9: at these batch sizes a wave carries ONE env (csrc/launch_plan.h wave_fill) and its other three rows
              are idle; E = 2050: four envs per wave, the last wave ragged (two envs, two idle rows);
  lane_ok     N = 5, 6 and 8 agents in the 8 lanes of a group: the three reference shapes, and a perturbed block of each that the
              generic resident kernel runs (update_frequency 23: periods of 15 and 8 sub-steps, a remainder chunk of 3);
  dead        a wave of four envs in the tight arena of tests/physical_cases.py, robots started close together: envs end by
              collision and by the wall while the other envs of their wave run on -- in the first, a middle and the last chunk of
              either controller period (`ended_in`: the oracle run with the step cut short says which) -- and, loaded: every env
              of wave 0 outside the arena (the wave leaves the period loop early), one env of wave 1 (its wave mates go on, and
              period 2 runs with its row dead);
  sparse_ok   false in the large-step case of tests/physical_cases.py ("fast-robots");
  penalize    penalize_violations off.
"""
import numpy as np
import pytest

import physical_cases as pc
from gpu_helpers import lane_group_kernel  # noqa: F401  (the fixture)
from oracle_check import FreeRunningOracle
from shape_kernel_harness import SHAPE_IDS, differing, make
from test_shape_kernels import REFERENCE

pytestmark = pytest.mark.gpu

STEPS = 40
N_ACT = {"PredatorCapturePrey": 5, "Warehouse": 5, "MaterialTransport": 20}
PCP6 = {"predator": 3, "capture": 3, "n_agents": 6}
PCP8 = pc.STRAY_TEAMS[8]
FAST = next(r for r in pc.REGIMES if r[0] == "fast-robots")
TIGHT = next(r for r in pc.REGIMES if r[0] == "tight-arena")
SHAPE_PCP = next(d for d in pc.DISPATCHES if d[0] == "rows-shape-pcp")
# (id, scenario, overrides, the form rg_step_form must report: "shape" | "resident")
CASES = [(s.lower() + "-shape", s, REFERENCE[s], "shape") for s in sorted(REFERENCE)] + \
        [(s.lower() + "-generic", s, dict(REFERENCE[s], update_frequency=23), "resident") for s in sorted(REFERENCE)] + \
        [("pcp6", "PredatorCapturePrey", PCP6, "resident"), ("pcp8", "PredatorCapturePrey", PCP8, "resident"),
         ("no-penalty", "PredatorCapturePrey", dict(pc.PCP5, penalize_violations=False), "resident"),
         ("fast-robots-shape", "PredatorCapturePrey", pc.case_overrides(FAST, SHAPE_PCP)[0], "shape"),
         ("fast-robots-generic", "PredatorCapturePrey", dict(pc.case_overrides(FAST, SHAPE_PCP)[0], update_frequency=23), "resident")]
TIGHT_OV = dict(pc.case_overrides(TIGHT, SHAPE_PCP)[0], start_dist=0.3, max_episode_steps=6)


def run(scenario, ov, E, want_form, oracle_lib, monkeypatch, load=None, each_step=None, seed=7):
    """The row kernel, the 8-lane-group kernel and the oracle from the same reset (and the same loaded poses), the same seeded
    actions: after every step the two handles agree in every output and state array, and the row kernel's agree with the oracle's."""
    import torch
    from marbler_amd import _lib
    rows = make(scenario, ov, E, monkeypatch, seed=seed)
    groups = make(scenario, ov, E, monkeypatch, env_vars=(("RG_STEP_SPAN", "0"),), seed=seed)
    side = FreeRunningOracle(oracle_lib, scenario, dict(rows.cfg), E, rows.params, seed, threads=8)
    side.reset()
    if load is not None:
        poses = load(side.orc.poses.copy())
        side.orc.poses[...] = poses
        for env in (rows, groups):
            env.poses.copy_(torch.as_tensor(poses))
    side.check_state(rows, scenario, "reset")
    rng = np.random.RandomState(11)
    for t in range(STEPS):
        a = rng.randint(0, N_ACT[scenario], size=(E, rows.N)).astype(np.int32)
        pre = side.orc.get_state(slice(None)) if each_step is not None else None
        for env in (rows, groups):
            env.step(torch.as_tensor(a, device=env.device))
        side.step(a)
        want = _lib.FORM_RESIDENT if want_form == "resident" else _lib.FORM_SHAPE + SHAPE_IDS[scenario]
        assert rows.step_form == want and groups.step_form == _lib.FORM_BY_VALUE, (t, rows.step_form, groups.step_form)
        bad = differing(rows, groups)
        assert not bad, f"step {t}: {bad} differ between the rows and the 8-lane groups"
        side.check_step(rows, scenario, t)
        if each_step is not None:
            each_step(t, pre, a, side.orc)
    side.check_statistics(rows, scenario)
    rows.close()
    groups.close()
    return side


@pytest.mark.parametrize("E", [1, 3, 5, 9])
@pytest.mark.parametrize("name,scenario,ov,form", CASES, ids=[c[0] for c in CASES])
def test_rows_against_the_oracle_and_the_groups(name, scenario, ov, form, E, oracle_lib, monkeypatch):
    # short episodes: resets, drawn-ahead copies and sampler runs within the 40 steps (max_episode_steps is no field of a shape)
    run(scenario, dict(ov, max_episode_steps=6), E, form, oracle_lib, monkeypatch)


# ---------------------------------------------------------------- where in the step an env ended
CUTS = (5, 10, 15, 20, 25)          # the chunk boundaries of 29 sub-steps in periods of 15: 5 5 5 | 5 5 4
CHUNKS = ("period 1, first", "period 1, middle", "period 1, last", "period 2, first", "period 2, middle", "period 2, remainder of 4")


class EndedIn(object):
    """The chunk in which an env's violation fell: the oracle steps the env's pre-step state with `update_frequency` cut to each
    chunk boundary, and the first cut that reports the violation names the chunk (an env stops at its first violation, so the
    cuts behind it report it too).  One small oracle per cut, loaded with the rows that ended."""

    def __init__(self, oracle_lib, scenario, cfg, cap=256):
        self.cap = cap
        self.cut = [oracle_lib.OracleVecEnv(scenario, dict(cfg, update_frequency=u), cap, dtype=np.float32) for u in CUTS]
        self.seen = set()          # (chunk, violation code)
        self.alone = set()         # ... of an env whose wave mates all went on

    def step(self, pre, actions, orc):
        ended = np.nonzero(orc.viol != 0)[0][:self.cap]
        if ended.size == 0:
            return
        chunk = np.zeros(ended.size, np.int64)
        for o in self.cut:
            for k, v in pre.items():
                getattr(o, k)[:ended.size] = v[ended]
            acts = np.full((self.cap, orc.N), pc.NO_OP, np.int32)
            acts[:ended.size] = actions[ended]
            o.step(acts)
            chunk += o.viol[:ended.size] == 0
        for e, c in zip(ended.tolist(), chunk.tolist()):
            self.seen.add((CHUNKS[c], int(orc.viol[e])))
            wave = slice(e // 4 * 4, e // 4 * 4 + 4)     # E = 2050: four consecutive envs per wave
            if int((orc.viol[wave] != 0).sum()) == 1 and int(orc.done[wave].sum()) == 1:
                self.alone.add((CHUNKS[c], int(orc.viol[e])))


def loaded_poses(poses):
    """Wave 0 (envs 0..3): every env has a robot outside the arena; wave 1 (envs 4..7): env 5 alone."""
    for e in (0, 1, 2, 3, 5):
        poses[e, 0, e % poses.shape[2]] = 5.0
    return poses


def test_envs_end_in_every_chunk_while_their_wave_mates_run_on(oracle_lib, monkeypatch):
    from marbler_amd.params import load_config
    scenario, E = "PredatorCapturePrey", 2050
    where = EndedIn(oracle_lib, scenario, load_config(scenario, overrides=TIGHT_OV))
    first = {}

    def each_step(t, pre, a, orc):
        if t == 0:
            first.update(viol=orc.viol.copy(), done=orc.done.copy())
        where.step(pre, a, orc)

    side = run(scenario, TIGHT_OV, E, "shape", oracle_lib, monkeypatch, load=loaded_poses, each_step=each_step)
    # the loaded waves: all four envs of wave 0 ended at the wall in the step's first sub-step; of wave 1 env 5 alone
    assert (first["viol"][:4] & 2).all() and first["viol"][5] & 2 and not first["viol"][[4, 6, 7]].any(), first["viol"][:8]
    print(f"{side.n_done} episodes ended, {side.n_viol} by a violation; chunks and codes seen with the wave mates running: {sorted(where.alone)}")
    for chunk in CHUNKS:
        for code, what in ((1, "a collision"), (2, "the wall")):
            assert any(c == chunk and v & code for c, v in where.alone), f"no env ended by {what} in `{chunk}` with its wave mates running"


@pytest.mark.parametrize("scenario", ["Warehouse", "MaterialTransport"])
def test_four_envs_per_wave_of_the_other_shapes(scenario, oracle_lib, monkeypatch):
    start = {"Warehouse": 0.3, "MaterialTransport": 0.2}[scenario]
    side = run(scenario, dict(REFERENCE[scenario], start_dist=start, max_episode_steps=8), 2050, "shape", oracle_lib, monkeypatch, load=loaded_poses)
    assert side.n_done > 2050 and side.n_viol > 0, (side.n_done, side.n_viol)
