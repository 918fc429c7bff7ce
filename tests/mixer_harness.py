"""The case table, the chosen inputs and the guarded batches of tests/test_gpu_mixer.py (shared with tests/test_mixer_cases.py, which
shows without a device that the inputs can be chosen, and with tools/mixer_probe.py).

Inputs are CHOSEN, not filtered: the backward pass is discontinuous where a ReLU or |.| pre-activation is zero, so draw() redraws the
state of any live row in which some pre-activation, evaluated in float64, lies within the kink margin of zero (mixer_twin.kink_bounds),
at most MAX_DRAWS times per row, and no row is ever left out of a comparison.  Episodes are of td_targets_harness' five kinds, and every
q, actions and obs row that the rule says is not read -- masked rows and row T -- holds NaN or an out-of-range action."""
import itertools

import numpy as np
import torch

import mixer_twin as tw
import td_targets_twin as tdt
from td_targets_harness import DEV, NAN, SENTINELS, draw_episodes, guarded, guards_intact, words  # noqa: F401

BAD_ACTION = 1 << 30
MAX_DRAWS = 50

SHAPES = [(1, 3), (2, 1), (5, 9), (4, 16), (8, 18), (16, 16)]     # (N, D): S = 3, 2, 45, 64, 144, 256
GRID = list(itertools.product([1, 2, 3, 33], [2, 3, 12, 14]))     # (B, rows): 1 .. 429 flat rows
EXTRA = lambda i: tuple(3 * ((i >> k) & 1) for k in range(4))     # noqa: E731  (q, obs, out, aux): each pitch at its minimum and + 3
# kind, B, rows, N, D, A, extra; the widest shape (16, 256) goes with the small batches: its rows are the dearest to choose
QMIX_SHAPE = [5, 0, 1, 2, 3, 4, 5, 3, 4, 0, 5, 1, 2, 4, 3, 2]
CASES = [("qmix", B, rows) + SHAPES[QMIX_SHAPE[i]] + ((2, 5, 20)[i % 3], EXTRA(i + 5)) for i, (B, rows) in enumerate(GRID)] + \
        [("qmix", 31, 2, 4, 16, 5, (0, 3, 0, 3)), ("qmix", 32, 2, 5, 9, 20, (3, 0, 3, 0))] + \
        [(("vdn", "none")[i % 2], B, rows) + SHAPES[(i + 1 + i // 4) % 6] + ((5, 20, 2)[i % 3], EXTRA(i)) for i, (B, rows) in enumerate(GRID)]
SCALES = (1.0, 4.0)


def make_params(kind, N, S, scale=1.0, seed=0):
    """EPyMARL's state dict with torch's default initialisation (TargetMixer's, drawn on the host), times `scale`; {} for vdn / none."""
    if kind != "qmix":
        return {}
    from marbler_amd.targets import TargetMixer
    return {k: v * scale for k, v in TargetMixer(kind, N, S, device="cpu", seed=seed).state_dict().items()}


def draw(case, scale=1.0, seed=0, poison=True):
    """-> host arrays q, actions, obs, mask, d_mixed, live, params (numpy / torch CPU), and draws: the most draws a row needed."""
    kind, B, rows, N, D, A, _ = case
    rng = np.random.default_rng(1000 + seed)
    T, S = rows - 1, N * D
    _, terminated, filled = draw_episodes(B, rows, rng, seed)
    mask, _ = tdt.row_flags(terminated, filled, rows)
    live = mask != 0
    if not live.any():                                           # (a batch of empty slots alone shows nothing)
        mask[0, 0], live[0, 0] = 1.0, True
    q = rng.standard_normal((B, rows, N, A)).astype(np.float32)
    actions = rng.integers(0, A, (B, rows, N)).astype(np.int32)
    obs = (rng.random((B, rows, N, D)) * 2 - 1).astype(np.float32)
    params = make_params(kind, N, S, scale, seed)
    draws = 1
    if kind == "qmix":
        host = {k: v.numpy() for k, v in params.items()}
        idx = np.argwhere(live)
        todo = np.ones(len(idx), bool)
        for draws in range(1, MAX_DRAWS + 1):
            s = np.stack([obs[b, t].reshape(S) for b, t in idx[todo]])
            bad = tw.margin_violations(host, s)
            todo[np.nonzero(todo)[0][~bad]] = False
            if not todo.any():
                break
            for b, t in idx[todo]:
                obs[b, t] = (rng.random((N, D)) * 2 - 1).astype(np.float32)
        else:
            raise AssertionError(f"{case}: a row's state still violates the kink margin after {MAX_DRAWS} draws")
    unread = np.ones((B, rows), bool)
    unread[:, :T] = ~live
    if poison:
        q[unread], obs[unread], actions[unread] = NAN, NAN, BAD_ACTION
    d_mixed = rng.standard_normal((B, T, N) if kind == "none" else (B, T)).astype(np.float32)
    return dict(q=q, actions=actions, obs=obs, mask=mask.astype(np.float32), d_mixed=d_mixed, live=live, params=params, draws=draws)


class Batch(object):
    """One guarded call of both launches.  extra = (q, obs, out, aux): rows an episode takes beyond the minimum in each group."""

    def __init__(self, case, scale=1.0, seed=0, host=None):
        self.case = case
        kind, B, rows, N, D, A, extra = case
        self.kind, self.B, self.rows, self.N, self.D, self.A, self.T = kind, B, rows, N, D, A, rows - 1
        eq, eo, ex, ea = extra
        self.host = h = draw(case, scale, seed) if host is None else host
        self.guards, self.whole, self.dev = {}, {}, {}
        ins = (("q", h["q"], eq, NAN, rows), ("actions", h["actions"], eq, BAD_ACTION, rows), ("obs", h["obs"], eo, NAN, rows),
               ("mask", h["mask"], ex, NAN, self.T), ("d_mixed", h["d_mixed"], ex, NAN, self.T))
        for name, arr, ext, fill, r in ins:
            self.guards[name], whole = guarded((B, r + ext) + arr.shape[2:], torch.from_numpy(arr).dtype)
            whole[:, r:] = fill
            whole[:, :r] = torch.from_numpy(arr).to(DEV)
            self.whole[name], self.dev[name] = whole, whole[:, :r]
        tail = (N,) if kind == "none" else ()
        self.outs = {"mixed": ((B, self.T + ex) + tail, self.T), "d_q": ((B, rows + eq, N, A), rows)}
        if kind == "qmix":
            self.outs.update(d_pre=((B, rows + ea, 192), rows), d_p2=((B, rows + ea, 32 * N + 32), rows), g=((B, rows + ea, 160), rows))
        for name, (shape, _) in self.outs.items():
            self.guards[name], self.whole[name] = guarded(shape, torch.float32)
        self.before = {k: self.whole[k].clone() for k, *_ in ins}
        from marbler_amd.targets import TargetMixer
        self.mixer = TargetMixer(kind, N, N * D, h["params"] or None, device=DEV)

    def out(self, name):
        return self.whole[name][:, :self.outs[name][1]]

    def forward(self, stream=None):
        from marbler_amd.mixers import mixer_forward
        d = self.dev
        got = mixer_forward(d["q"], d["actions"], d["obs"], d["mask"], self.mixer, mixed_out=self.out("mixed"), stream=stream)
        assert got.data_ptr() == self.whole["mixed"].data_ptr()

    def backward(self, stream=None):
        from marbler_amd.mixers import mixer_backward
        d, qmix = self.dev, self.kind == "qmix"
        mixer_backward(d["q"], d["actions"], d["obs"], d["mask"], d["d_mixed"], self.mixer, d_q_out=self.out("d_q"),
                       d_pre_out=self.out("d_pre") if qmix else None, d_p2_out=self.out("d_p2") if qmix else None,
                       g_out=self.out("g") if qmix else None, stream=stream)

    def run(self):
        self.forward()
        self.backward()
        torch.cuda.synchronize()
        self.check_untouched()
        return {k: self.out(k).cpu().numpy() for k in self.outs}

    def check_untouched(self):
        for k, v in self.before.items():
            same = torch.equal(torch.nan_to_num(self.whole[k], nan=7.0), torch.nan_to_num(v, nan=7.0)) if v.dtype == torch.float32 else torch.equal(self.whole[k], v)
            assert same, (k, "an input changed")
        for k, g in self.guards.items():
            assert guards_intact(g), (k, "guard band damaged")
        for k, (_, r) in self.outs.items():
            assert bool((self.whole[k][:, r:] == SENTINELS[torch.float32]).all()), (k, "rows behind the last row were written")

    def twin(self):
        h = self.host
        params = {k: v.numpy() for k, v in h["params"].items()}
        return tw.twin(self.kind, h["q"], h["actions"], h["obs"], h["mask"], params, h["d_mixed"])

    def module(self, dtype=torch.float32):
        """A TrainableMixer with the batch's weights on the device."""
        from marbler_amd.mixers import TrainableMixer
        m = TrainableMixer(self.kind, self.N, self.N * self.D, device=DEV)
        if self.kind == "qmix":
            m.load_state_dict(self.host["params"])
        return m.to(dtype)

    def reference(self, dtype=torch.float32):
        """forward_reference under autograd on the device in `dtype` -> the same quantities as run(), and the parameter gradients."""
        B, rows, N, T = self.B, self.rows, self.N, self.T
        m, d = self.module(dtype), self.dev
        q = d["q"].to(dtype).clone().requires_grad_(True)
        parts = {} if self.kind == "qmix" else None
        mixed = m.forward_reference(q, d["actions"], d["obs"].to(dtype), d["mask"], parts)
        mixed.backward(d["d_mixed"].to(dtype))
        out = {"mixed": mixed.detach(), "d_q": torch.nan_to_num(q.grad, nan=0.0)}     # (the gather's backward leaves NaN rows alone: 0)
        if parts:
            live = (d["mask"] != 0).reshape(B * T, 1)
            for name, t in (("d_pre", parts["pre"].grad), ("d_p2", parts["p2"].grad), ("g", parts["g"].detach())):
                full = torch.zeros(B, rows, t.shape[1], dtype=dtype, device=DEV)
                full[:, :T] = torch.where(live, t, t.new_zeros(())).view(B, T, -1)
                out[name] = full
        grads = {k: p.grad for k, p in m.named_parameters()}
        return {k: v.cpu().numpy() for k, v in out.items()}, {k: v.cpu().numpy() for k, v in grads.items()}
