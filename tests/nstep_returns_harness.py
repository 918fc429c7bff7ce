"""The guarded batches and the case table of tests/test_gpu_nstep_returns.py (shared with tools/nstep_returns_probe.py): the scheme
of tests/td_targets_harness.py -- sentinel guard bands, sentinel-filled outputs, NaN in everything the rule says is not read,
episode kinds by b mod 5 -- for rg_nstep_returns."""
import itertools

import numpy as np
import torch

import nstep_returns_twin as tw
from td_targets_harness import DEV, NAN, SENTINELS, draw_episodes, guarded, guards_intact, words  # noqa: F401

OUTPUTS = ("returns", "values", "mask")


class Batch(object):
    """One guarded call.  extra = (obs, flag, out, value): rows an episode takes beyond the minimum in each group of arrays.
    `add` decides which rows are needed (row T only with add_value_last_step), hence which are poisoned."""

    def __init__(self, B, rows, N, D, add, extra=(0, 0, 0, 0), seed=0):
        rng = np.random.default_rng(200 + seed)
        self.B, self.rows, self.N, self.D, self.T, self.add = B, rows, N, D, rows - 1, bool(add)
        eo, ef, ex, ev = extra
        reward, terminated, filled = draw_episodes(B, rows, rng, seed)
        self.m = tw.mask_of(terminated, filled, rows)
        self.need = tw.needed_rows(self.m, add)
        obs = (rng.random((B, rows, N, D)) * 2 - 1).astype(np.float32)
        obs[~self.need] = NAN                                      # an obs row that is not needed is not read
        reward[:, :-1][~self.m] = NAN                              # nor the reward of a masked row
        reward[:, -1] = NAN                                        # nor reward[T]
        self.host = dict(obs=obs, reward=reward, terminated=terminated, filled=filled)
        self.guards, self.whole, self.dev = {}, {}, {}
        for name, arr, ext, fill in (("obs", obs, eo, NAN), ("reward", reward, ef, NAN), ("terminated", terminated, ef, 1), ("filled", filled, ef, 1)):
            shape = (B, rows + ext) + arr.shape[2:]
            self.guards[name], whole = guarded(shape, torch.from_numpy(arr).dtype)
            whole[:, rows:] = fill
            whole[:, :rows] = torch.from_numpy(arr).to(DEV)
            self.whole[name], self.dev[name] = whole, whole[:, :rows]
        self.used = {"returns": self.T, "mask": self.T, "values": rows}
        for name, n_rows, inner in (("returns", self.T + ex, (N,)), ("mask", self.T + ex, ()), ("values", rows + ev, (N,))):
            self.guards[name], self.whole[name] = guarded((B, n_rows) + inner, torch.float32)
        self.before = {k: v.clone() for k, v in self.whole.items() if k not in OUTPUTS}

    def outs(self):
        return {k + "_out": self.whole[k][:, :self.used[k]] for k in OUTPUTS}

    def run(self, critic, gamma, n, scale=1.0, shift=0.0, stream=None):
        from marbler_amd.returns import nstep_returns
        d = self.dev
        out = nstep_returns(d["obs"], d["reward"], d["terminated"], d["filled"], critic, gamma, n, self.add, scale, shift, stream=stream, **self.outs())
        torch.cuda.synchronize()
        self.check_untouched()
        assert all(out[k].data_ptr() == self.whole[k].data_ptr() for k in OUTPUTS)
        return {k: v.cpu().numpy() for k, v in out.items()}

    def check_untouched(self):
        for k, v in self.before.items():
            same = torch.equal(torch.nan_to_num(self.whole[k], nan=7.0), torch.nan_to_num(v, nan=7.0)) if v.dtype == torch.float32 else torch.equal(self.whole[k], v)
            assert same, (k, "an input changed")
        for k, g in self.guards.items():
            assert guards_intact(g), (k, "guard band damaged")
        for k in OUTPUTS:
            assert bool((self.whole[k][:, self.used[k]:] == SENTINELS[torch.float32]).all()), (k, "rows behind the last row were written")

    def values64(self, critic, scale=1.0, shift=0.0):
        h = self.host
        v64, need = tw.values64(critic.kind, {k: v.cpu().numpy() for k, v in critic.params.items()}, h["obs"], h["terminated"], h["filled"],
                                self.add, scale, shift)
        assert np.array_equal(need, self.need)
        return v64

    def torch_values(self, critic, scale=1.0, shift=0.0):
        """The torch float32 restatement of the values on the device, on the same inputs (the rows that are not needed hold NaN:
        they are zeroed for the critic and are not compared)."""
        obs = torch.nan_to_num(self.dev["obs"], nan=0.0).reshape(self.B, self.rows, self.N * self.D)
        v = critic.forward(obs)
        if scale != 1.0 or shift != 0.0:
            v = v * float(np.float32(scale)) + float(np.float32(shift))
        torch.cuda.synchronize()
        return v.cpu().numpy()

    def check_exact_parts(self, out, gamma, n):
        """Checks 1 and 2: the mask, the zero rows, and `returns` word for word against the float32 twin fed the kernel's OWN
        values."""
        assert np.array_equal(words(out["mask"]), words(self.m.astype(np.float32))), "mask"
        assert np.array_equal(words(out["values"][~self.need]), np.zeros(((~self.need).sum(), self.N), np.uint32)), "values of rows that are not needed"
        assert np.array_equal(words(out["returns"][~self.m]), np.zeros(((~self.m).sum(), self.N), np.uint32)), "returns of masked rows"
        ref = tw.returns32(out["values"], self.host["reward"], self.m, gamma, n, self.add)
        assert np.array_equal(words(out["returns"]), words(ref)), "returns against the float32 twin on the kernel's own values"
        return ref


def make_critic(kind, N, S, H, scale=1.0, seed=0):
    from marbler_amd.returns import TargetCritic
    critic = TargetCritic(kind, N, S, H, device=DEV, seed=seed)
    if scale != 1.0:
        critic.load_state_dict({k: v * scale for k, v in critic.state_dict().items()})
    return critic


SHAPES = [(2, 1), (5, 9), (4, 16), (8, 18)]                       # (N, D): S = 2, 45, 64, 144
GRID = list(itertools.product([1, 2, 3, 33], [2, 3, 12, 14]))     # (B, rows)
STEPS = (1, 5, 10, 20)                                            # 20 is above every T of the grid
EXTRA = lambda i: tuple(3 * ((i >> k) & 1) for k in range(4))     # noqa: E731  each pitch at its minimum and + 3
DEFAULTS, SCALED = (1.0, 0.0), (1.7, -0.3)                        # (value_scale, value_shift)


def _case(p, j):
    B, rows = GRID[j]
    return (("cv", "cv_ns")[p], (64, 128)[(j // 2 + p) % 2], B, rows) + SHAPES[(j + j // 4 + p) % 4] + \
           (STEPS[(j + j // 4 + 2 * p) % 4], (j + j // 8 + p) % 2 == 0, SCALED if (j + p) % 3 == 0 else DEFAULTS, EXTRA(j + 5 + 6 * p))


# kind, H, B, rows, N, D, n, add_value_last_step, (value_scale, value_shift), extra
CASES = [_case(p, j) for p in range(2) for j in range(len(GRID))] + \
        [("cv", 128, 2, 204, 8, 18, 10, True, DEFAULTS, (0, 0, 0, 0)),     # an episode's real length: seven tiles, the value store
         ("cv", 128, 3, 14, 5, 9, 5, True, DEFAULTS, (3, 0, 3, 0)),        # 14 rows x 5 agents: 70 (row, agent) pairs, a ragged tile
         ("cv_ns", 64, 2, 14, 5, 9, 10, False, SCALED, (0, 3, 0, 3)),
         ("cv_ns", 128, 2, 33, 4, 16, 5, True, DEFAULTS, (0, 3, 3, 0)),    # row T alone in a second tile
         ("cv", 64, 3, 65, 2, 1, 20, False, SCALED, (3, 3, 0, 3))]         # three tiles, the last one row T alone and not needed
