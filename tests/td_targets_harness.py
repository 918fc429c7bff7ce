"""The guarded batches and the case table of tests/test_gpu_td_targets.py (shared with tools/td_targets_probe.py): see that
module's docstring for the episode kinds and what is poisoned."""
import itertools

import numpy as np
import torch

import td_targets_twin as tw

DEV = "cuda:0"
GUARD = 256                                   # elements on either side of an array
SENTINELS = {torch.float32: -777.25, torch.int32: -77777, torch.uint8: 0xA5}
BAD_SEL = 1 << 30
NAN = float("nan")


def guarded(shape, dtype):
    """-> (the whole allocation, the array inside it): sentinels everywhere."""
    n = int(np.prod(shape))
    raw = torch.full((GUARD + n + GUARD + 3,), SENTINELS[dtype], dtype=dtype, device=DEV)
    lo = GUARD + (-(raw.data_ptr() // raw.element_size() + GUARD)) % 4
    return (raw, lo, n), raw[lo:lo + n].view(shape)


def guards_intact(g):
    raw, lo, n = g
    return bool((raw[:lo] == SENTINELS[raw.dtype]).all()) and bool((raw[lo + n:] == SENTINELS[raw.dtype]).all())


def words(x):
    x = x if isinstance(x, np.ndarray) else x.detach().cpu().contiguous().numpy()
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def draw_episodes(B, rows, rng, rotate):
    """-> reward, terminated, filled [B, rows] by the kinds of the module docstring (an episode of l transitions fills l + 1 rows)."""
    T = rows - 1
    terminated, filled = np.zeros((B, rows), np.uint8), np.zeros((B, rows), np.uint8)
    for b in range(B):
        kind = (b + rotate) % 5
        length = {0: 1, 1: T, 2: T, 3: 0}.get(kind, int(rng.integers(1, T + 1)))
        if length:
            filled[b, :length + 1] = 1
            if kind != 2:
                terminated[b, length - 1] = 1
    return rng.standard_normal((B, rows)).astype(np.float32), terminated, filled


class Batch(object):
    """One guarded call.  extra = (q, obs, flag, out): rows an episode takes beyond the minimum in each group of arrays."""

    def __init__(self, kind, B, rows, N, D, A, extra=(0, 0, 0, 0), with_sel=True, seed=0):
        rng = np.random.default_rng(100 + seed)
        self.kind, self.B, self.rows, self.N, self.D, self.A, self.T = kind, B, rows, N, D, A, rows - 1
        eq, eo, ef, ex = extra
        reward, terminated, filled = draw_episodes(B, rows, rng, seed)
        mask, live = tw.row_flags(terminated, filled, rows)
        read = np.zeros((B, rows), bool)
        read[:, 1:] = live                                         # row t + 1 of a live row t: the only rows of qt, sel, obs that are read
        qt = rng.standard_normal((B, rows, N, A)).astype(np.float32)
        obs = (rng.random((B, rows, N, D)) * 2 - 1).astype(np.float32)
        sel = rng.integers(0, A, (B, rows, N)).astype(np.int32)
        qt[~read], obs[~read], sel[~read] = NAN, NAN, BAD_SEL
        reward[:, :-1][~mask] = NAN
        reward[:, -1] = NAN
        self.host = dict(qt=qt, sel=sel if with_sel else None, obs=obs, reward=reward, terminated=terminated, filled=filled)
        self.mask, self.live = mask, live
        self.guards, self.whole, self.dev = {}, {}, {}
        for name, arr, ext, fill in (("qt", qt, eq, NAN), ("sel", sel, eq, BAD_SEL), ("obs", obs, eo, NAN), ("reward", reward, ef, NAN),
                                     ("terminated", terminated, ef, 1), ("filled", filled, ef, 1)):
            shape = (B, rows + ext) + arr.shape[2:]
            self.guards[name], whole = guarded(shape, torch.from_numpy(arr).dtype)
            whole[:, rows:] = fill
            whole[:, :rows] = torch.from_numpy(arr).to(DEV)
            self.whole[name], self.dev[name] = whole, whole[:, :rows]
        if not with_sel:
            self.dev["sel"] = None
        t_inner = (N,) if kind == "none" else ()
        for name, inner in (("targets", t_inner), ("mask", ()), ("agent_q", (N,))):
            self.guards[name], self.whole[name] = guarded((B, self.T + ex) + inner, torch.float32)
        self.before = {k: v.clone() for k, v in self.whole.items() if k not in ("targets", "mask", "agent_q")}

    def run(self, mixer, gamma, stream=None):
        from marbler_amd.targets import td_targets
        d, T = self.dev, self.T
        out = td_targets(
            d["qt"], d["obs"], d["reward"], d["terminated"], d["filled"], mixer, gamma, sel=d["sel"], targets_out=self.whole["targets"][:, :T],
            mask_out=self.whole["mask"][:, :T], agent_q_out=self.whole["agent_q"][:, :T], stream=stream)
        torch.cuda.synchronize()
        self.check_untouched()
        assert all(out[k].data_ptr() == self.whole[k].data_ptr() for k in ("targets", "mask", "agent_q"))
        return {k: v.cpu().numpy() for k, v in out.items()}

    def check_untouched(self):
        for k, v in self.before.items():
            same = torch.equal(torch.nan_to_num(self.whole[k], nan=7.0), torch.nan_to_num(v, nan=7.0)) if v.dtype == torch.float32 else torch.equal(self.whole[k], v)
            assert same, (k, "an input changed")
        for k, g in self.guards.items():
            assert guards_intact(g), (k, "guard band damaged")
        for k in ("targets", "mask", "agent_q"):
            assert bool((self.whole[k][:, self.T:] == SENTINELS[torch.float32]).all()), (k, "rows behind rows - 1 were written")

    def twin(self, gamma, params=None):
        h = self.host
        return tw.twin(self.kind, h["qt"], h["sel"], h["obs"], h["reward"], h["terminated"], h["filled"], gamma,
                       None if params is None else {k: v.cpu().numpy() for k, v in params.items()})

    def restatement(self, gamma, params):
        d = self.dev
        ref, ref_mask = tw.restatement(self.kind, d["qt"], d["sel"], d["obs"], d["reward"], d["terminated"], d["filled"], gamma, params)
        torch.cuda.synchronize()
        return ref[..., 0].cpu().numpy(), ref_mask[..., 0].cpu().numpy()


def make_mixer(kind, N, S, scale=1.0, seed=0):
    from marbler_amd.targets import TargetMixer
    mixer = TargetMixer(kind, N, S, device=DEV, seed=seed)
    if kind == "qmix" and scale != 1.0:
        mixer.load_state_dict({k: v * scale for k, v in mixer.state_dict().items()})
    return mixer


SHAPES = [(2, 1), (5, 9), (4, 16), (8, 18)]                       # (N, D): S = 2, 45, 64, 144
GRID = list(itertools.product([1, 2, 3, 33], [2, 3, 12, 14]))     # (B, rows): 1 .. 429 flat rows
EXTRA = lambda i: tuple(3 * ((i >> k) & 1) for k in range(4))     # noqa: E731  each pitch at its minimum and + 3
# kind, B, rows, N, D, A, extra, with_sel
CASES = [("qmix", B, rows) + SHAPES[(i + i // 4) % 4] + ((2, 5, 20)[i % 3], EXTRA(i + 5), i % 2 == 0) for i, (B, rows) in enumerate(GRID)] + \
        [("qmix", 2, 17, 4, 16, 5, (0, 3, 0, 3), True), ("qmix", 31, 2, 5, 9, 20, (3, 0, 3, 0), False)] + \
        [(("vdn", "none")[i % 2], B, rows) + SHAPES[(i + 1 + i // 4) % 4] + ((5, 20, 2)[i % 3], EXTRA(i), (i // 2) % 2 == 0)
         for i, (B, rows) in enumerate(GRID)]
