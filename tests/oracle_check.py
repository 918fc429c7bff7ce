"""What "bit-exact against the float32 oracle" compares, stated once for every GPU tier.

Two kinds of harness hold the HIP step kernels to oracle/oracle.c:

  loaded-state  the oracle is loaded with the product's own state before a step (`load_oracle`), both step once: all seven outputs
                (`qp_sweeps` wherever the env collects it) and all 14 `STATE_KEYS`, on the rows the harness selects (the envs of a
                team, the envs that did not end);
  free-running  the oracle runs beside the product from the same reset stream with the reset twin (`FreeRunningOracle`): all
                seven outputs, `poses`, `carry`, `steps` and the arrays the scenario owns (`scenario_state`) after every step, the
                rollout statistics and `reset_count` at the end.  Arrays a scenario does not own are left out: nobody writes them,
                and the two sides fill them differently (`goal_col` is 1 in the product and 0 in the oracle outside ArcticTransport).

float32 arrays are compared as uint32 words, everything else as bytes (`assert_same_words`): -0.0 is not +0.0.
NumPy only: the CPU tier imports this module and tests it (tests/test_oracle_check.py)."""
import numpy as np

# the seven outputs of a step: (the oracle's attribute, the product's)
OUTPUTS = (("obs", "obs"), ("reward", "reward"), ("done", "done_u8"), ("dist", "dist_travelled"), ("viol", "violation"),
           ("remaining", "remaining"), ("qp_sweeps", "qp_sweeps"))
OUTPUT_KEYS = tuple(k for k, _ in OUTPUTS)
# the state arrays under the oracle's names, and the product's name where it differs
STATE_KEYS = ("poses", "carry", "steps", "prey_loc", "prey_sensed", "prey_captured", "loaded", "load",
              "zone_load", "messages", "grid", "goal_col", "pixel_type", "reached_goal")
GPU_NAME = {"carry": "carry_dist", "steps": "episode_steps"}
# what rg_bind_state requires for a scenario (robogym_capi.hip) next to poses, carry_dist and episode_steps
OWN_STATE = {"PredatorCapturePrey": ("prey_loc", "prey_sensed", "prey_captured"),
             "Warehouse": ("loaded",),
             "MaterialTransport": ("load", "zone_load", "messages"),
             "Simple": ("prey_loc",),
             "ArcticTransport": ("grid", "goal_col", "pixel_type", "reached_goal")}
STATISTICS = ("done_count", "done_return_sum", "ep_return", "reset_count")


def scenario_state(scenario):
    return ("poses", "carry", "steps") + OWN_STATE[scenario]


def _host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def gpu_outputs(env):
    """The env's output buffers on the host under the oracle's names; `qp_sweeps` exactly when the env collects it."""
    return {k: _host(getattr(env, g)) for k, g in OUTPUTS if getattr(env, g) is not None}


def gpu_state(env, keys=STATE_KEYS):
    return {k: _host(getattr(env, GPU_NAME.get(k, k))) for k in keys}


def load_oracle(orc, state):
    for k, v in state.items():
        arr = getattr(orc, k)
        arr[...] = np.asarray(v).astype(arr.dtype).reshape(arr.shape)


def assert_same_words(got, want, key, label="", step=None, rows=None):
    """got, want [E, ...]; rows: the envs to compare (all of them when None)."""
    got = np.asarray(got)
    want = np.asarray(want).astype(got.dtype).reshape(got.shape)
    if rows is not None:
        got, want = got[rows], want[rows]
    if got.size == 0:
        return
    word = np.uint32 if got.dtype == np.float32 else np.uint8
    a = np.ascontiguousarray(got).reshape(len(got), -1).view(word)
    b = np.ascontiguousarray(want).reshape(len(got), -1).view(word)
    if not np.array_equal(a, b):
        bad = np.nonzero((a != b).any(axis=1))[0]
        if rows is not None:
            rows = np.asarray(rows)
            bad = (np.nonzero(rows)[0] if rows.dtype == bool else rows)[bad]
        raise AssertionError(f"{label}: {key} differs at step {step} in {len(bad)} envs, first {bad[:8].tolist()}")


def assert_outputs(got, orc, label="", step=None, rows=None):
    """got: `gpu_outputs`.  Every output; `qp_sweeps` may be absent (an env that does not collect it), nothing else."""
    for k in OUTPUT_KEYS:
        if k != "qp_sweeps" or k in got:
            assert_same_words(got[k], getattr(orc, k), k, label, step, rows)


def assert_state(got, orc, keys=STATE_KEYS, label="", step=None, rows=None):
    """got: `gpu_state`."""
    for k in keys:
        assert_same_words(got[k], getattr(orc, k), k, label, step, rows)


class FreeRunningOracle(object):
    """The float32 oracle stepping beside an auto-resetting env: the reset twin (helpers.oracle_reset) in place of the fused
    reset, the per-env episode counters, and the float32 return accumulators of the rollout statistics (misc.py:178-185) in the
    kernels' order of additions: per-agent sum in agent order, agent 0 alone under `shared_reward`."""

    def __init__(self, oracle_lib, scenario, cfg, E, rg_params, seed, threads=1, dtype=np.float32):
        from helpers import oracle_reset_params
        self.lib, self.seed, self.threads = oracle_lib, seed, threads
        self.orc = oracle_lib.OracleVecEnv(scenario, cfg, E, dtype=dtype)
        self.rp = oracle_reset_params(oracle_lib, rg_params)
        self.shared = bool(rg_params.shared_reward)
        self.keys = scenario_state(scenario)
        self.episodes = np.zeros(E, np.int64)
        self.ret = np.zeros(E, np.float32)
        self.ret_sum = np.zeros(E, np.float32)
        self.n_done = self.n_viol = 0

    def _reset(self, e):
        from helpers import oracle_reset
        oracle_reset(self.lib, self.orc, self.rp, self.seed, e, int(self.episodes[e]))

    def reset(self):
        for e in range(self.orc.E):
            self._reset(e)

    def step(self, actions):
        """One step, then the twin's reset of the envs that ended: outputs of the step, state after the reset."""
        orc = self.orc
        orc.step(actions, threads=self.threads)
        if self.shared:
            self.ret = self.ret + orc.reward[:, 0]
        else:
            s = np.zeros(orc.E, np.float32)
            for k in range(orc.N):
                s = s + orc.reward[:, k]
            self.ret = self.ret + s
        ended = orc.done != 0
        self.ret_sum[ended] = self.ret_sum[ended] + self.ret[ended]
        self.ret[ended] = 0
        self.n_done += int(ended.sum())
        self.n_viol += int((orc.viol > 0).sum())
        self.reset_ended()

    def reset_ended(self):
        """The twin's reset of the envs the last step ended (for a caller that steps `orc` itself and looks in between)."""
        for e in np.nonzero(self.orc.done)[0]:
            self.episodes[e] += 1
            self._reset(e)

    @classmethod
    def at_reset(cls, *args, **kw):
        """-> the OracleVecEnv, every env in the reset twin's episode 0."""
        side = cls(*args, **kw)
        side.reset()
        return side.orc

    def check_state(self, env, label="", step=None):
        assert_state(gpu_state(env, self.keys), self.orc, self.keys, label, step)

    def check_step(self, env, label="", step=None):
        assert_outputs(gpu_outputs(env), self.orc, label, step)
        self.check_state(env, label, step)

    def check_statistics(self, env, label=""):
        """(`reset_count`: the explicit reset drew episode 0.)"""
        want = {"done_count": self.episodes, "done_return_sum": self.ret_sum, "ep_return": self.ret, "reset_count": self.episodes + 1}
        for k in STATISTICS:
            assert_same_words(_host(getattr(env, k)), want[k], k, label, "end")
