"""What tests/test_gpu_shape_kernels.py and tests/test_gpu_launch_plan.py share: a handle made under the launch-form switches, the
seeded actions, and the word-for-word comparison of two handles."""
import numpy as np
import torch

import gpu_helpers
from gpu_helpers import guarded_class
from marbler_amd.gymma import N_ACTIONS
from test_shape_kernels import SCENARIOS, table

OUTS = ("obs", "reward", "done_u8", "dist_travelled", "violation", "remaining", "qp_sweeps")


class _ShapeIds(dict):   # scenario -> the id of its row of the library's table (read on first use, not at collection)
    def __missing__(self, scenario):
        self.update({SCENARIOS[r["scenario"]]: r["id"] for r in table()})
        return self[scenario]


SHAPE_IDS = _ShapeIds()


def make(scenario, ov, E, monkeypatch, env_vars=(), guarded=False, seed=7):
    from marbler_amd import VecRobotariumEnv
    with monkeypatch.context() as m:   # read by rg_create
        for k in ("RG_STEP_SHAPE", "RG_STEP_SPAN", "RG_STEP_RESIDENT"):
            m.delenv(k, raising=False)
        for k, v in env_vars:
            m.setenv(k, v)
        kw = dict(overrides=ov, seed=seed, auto_reset=True, collect_qp_stats=True)
        env = guarded_class()(scenario, E, slab_bytes=E * 8192 + (8 << 20), **kw) if guarded else VecRobotariumEnv(scenario, E, **kw)
    env.reset()
    assert env.step_kernel == "group"
    return env


def actions(env, scenario, count, seed=11):
    rng = np.random.RandomState(seed)
    return [torch.as_tensor(rng.randint(0, N_ACTIONS[scenario], size=(env.E, env.N)).astype(np.int32), device=env.device) for _ in range(count)]


def differing(a, b):
    return gpu_helpers.differing(a, b, OUTS + a.STATE_KEYS)
