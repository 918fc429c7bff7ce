"""A trainable mixer: the ONLINE mixer's pass of a Q-learner's training step WITH gradients -- chosen_action_qvals =
mixer(gather(mac_out[:, :-1], actions), state[:, :-1]) -- in one HIP launch forward and one backward (rg_mixer_forward /
rg_mixer_backward, include/robogym_learn.h), and the weight gradients, which are sums over all rows, in torch's GEMMs.

    mixer = TrainableMixer.from_target(target_mixer)                  # or TrainableMixer("qmix", n_agents, n_agents * obs_dim)
    mixed = mixer(actor(obs), actions, obs, out["mask"])             # [B, rows - 1], with a graph through q and the parameters
    loss = (((mixed - out["targets"]) * out["mask"]) ** 2).sum() / out["mask"].sum()
    loss.backward(); optimizer.step()
    target_mixer.load_state_dict(mixer.state_dict())                  # the hard target update

The rule -- which rows are masked, what is read and what is not, the backward formulas at the kinks -- is stated once in
csrc/mixer_grad.h and DESIGN.md section 4 "Trainable mixer".  There is no host path: the launches need the library and a HIP device;
TrainableMixer.forward_reference() is the plain torch composition, on any device and in any floating-point dtype.
"""
import ctypes as C

import torch

from . import _args, _lib
from .targets import COLS, EMBED, FIRST_LAYERS, HYPER, KINDS, MAX_STATE, TargetMixer, qmix_shapes

_F32 = (torch.float32,)
G_COLS = 2 * HYPER + EMBED              # the columns of g: relu(a1), relu(af), relu(av)


def _check(who, q, actions, obs, mask, mixer):
    """The shared half of both launches' checks (everything but the device) -> (B, rows, N, A, D, q_pitch, obs_pitch)."""
    if not isinstance(mixer, TargetMixer):
        raise ValueError(f"{who}mixer must be a TargetMixer (the packed operands), got {type(mixer).__name__}")
    _args.check_tensor(who + "q", q, _F32, None, contiguous=False, errors=_args.VALUE)
    if q.dim() != 4:
        raise ValueError(f"{who}q must be [B, rows, N, A], got {tuple(q.shape)}")
    B, rows, N, A = q.shape
    if B < 1 or rows < 2:
        raise ValueError(f"{who}q must be [B, rows, N, A] with B >= 1 and rows >= 2, got {tuple(q.shape)}")
    if N != mixer.n_agents:
        raise ValueError(f"{who}q has {N} agents, the mixer {mixer.n_agents}")
    if not 1 <= A <= 32:
        raise ValueError(f"{who}n_actions must be in 1..32, q has {A}")
    dev = q.device
    _args.check_tensor(who + "actions", actions, (torch.int32,), (B, rows, N), dev, contiguous=False, errors=_args.VALUE)
    if not isinstance(obs, torch.Tensor) or obs.dim() != 4 or obs.shape[3] < 1:
        raise ValueError(f"{who}obs must be a float32 tensor [{B}, {rows}, {N}, D] with D >= 1")
    D = obs.shape[3]
    _args.check_tensor(who + "obs", obs, _F32, (B, rows, N, D), dev, contiguous=False, errors=_args.VALUE)
    if mixer.kind == "qmix" and N * D != mixer.state_dim:
        raise ValueError(f"{who}the mixer's state_dim is {mixer.state_dim}, obs provides {N} x {D}")
    _args.check_tensor(who + "mask", mask, _F32, (B, rows - 1), dev, contiguous=False, errors=_args.VALUE)
    if mixer.device != dev:
        raise ValueError(f"{who}the mixer is on {mixer.device}, q on {dev}")
    q_pitch = _args.shared_pitch(who, [("q", q, (N, A)), ("actions", actions, (N,))], rows)
    obs_pitch = _args.episode_pitch(who + "obs", obs, (N, D))
    return B, rows, N, A, D, q_pitch, obs_pitch


def _needs_hip(who, dev):
    """Every other check comes first: what is wrong with a call is said wherever its tensors live."""
    if dev.type != "cuda":
        raise ValueError(f"{who}q lives on {dev}; the launch runs on a HIP device and has no host path")


def _weights(mixer, w1b=None, wfb=None):
    w = _lib.RgMixerGradWeights()
    w.m = mixer.weights_struct()
    if mixer.kind == "qmix":
        w.w1b = (mixer.params["hyper_w_1.2.weight"] if w1b is None else w1b).data_ptr()
        w.wfb = (mixer.params["hyper_w_final.2.weight"] if wfb is None else wfb).data_ptr()
    return w


def _launch(entry, w, io, dev, stream):
    lib = _lib.load_mixer_grad()
    stream, hip_stream = _args.launch_stream(stream, dev)
    with torch.cuda.device(dev):
        rc = getattr(lib, entry)(C.byref(w), C.byref(io), hip_stream)
    if rc != 0:
        raise _args.launch_error(rc, lib.rg_mixer_grad_last_error().decode())


def _ptr(t):
    return t.data_ptr() if t is not None else None


def mixer_forward(q, actions, obs, mask, mixer, mixed_out=None, stream=None):
    """The mixed chosen-action values of an episode batch in ONE launch (rg_mixer_forward; the rule: csrc/mixer_grad.h).  q
    [B, rows, N, A] f32: the online actor's output; actions [B, rows, N] int32 (the same number of rows per episode as q); obs
    [B, rows, N, D] f32 (the state of a row is its N D floats; read with a qmix mixer only); mask [B, rows - 1] f32 (td_targets'
    mask); mixer: a TargetMixer, the packed operands.  Slices [:, :rows] of longer arrays are read in place.  Returns mixed
    [B, rows - 1] (a `none` mixer: [B, rows - 1, N]); mixed_out: the output to reuse, laid out with mask's number of rows per
    episode -- nothing is allocated when it is given, so the call can be captured.  ValueError for a wrong dtype, shape, stride or
    device and for what the launch refuses."""
    who = "mixer_forward: "
    B, rows, N, A, D, q_pitch, obs_pitch = _check(who, q, actions, obs, mask, mixer)
    dev, T = q.device, rows - 1
    tail = (N,) if mixer.kind == "none" else ()
    if mixed_out is not None:
        _args.check_tensor(who + "mixed_out", mixed_out, _F32, (B, T) + tail, dev, contiguous=False, errors=_args.VALUE)
    out_pitch = _args.episode_pitch(who + "mask", mask, ())
    if mixed_out is not None and _args.episode_pitch(who + "mixed_out", mixed_out, tail) != out_pitch and B > 1:
        raise ValueError(f"{who}mask and mixed_out must take the same number of rows per episode")
    _needs_hip(who, dev)
    if mixed_out is None:
        mixed_out = torch.empty((B, out_pitch) + tail, device=dev)[:, :T]
    io = _lib.RgMixerGradIO(q.data_ptr(), actions.data_ptr(), obs.data_ptr(), mask.data_ptr(), mixed_out.data_ptr(), None, None, None,
                            None, None, B, N, D, A, rows, q_pitch, obs_pitch, out_pitch, 0, 0)
    _launch("rg_mixer_forward", _weights(mixer), io, dev, stream)
    return mixed_out


def mixer_backward(q, actions, obs, mask, d_mixed, mixer, w1b=None, wfb=None, d_q_out=None, d_pre_out=None, d_p2_out=None, g_out=None,
                   stream=None):
    """The backward pass of mixer_forward in ONE launch (rg_mixer_backward; the rule: csrc/mixer_grad.h), which recomputes the
    forward pass.  q, actions, obs, mask, mixer as mixer_forward takes them; d_mixed: the gradient of mixed, laid out with mask's
    number of rows per episode; w1b / wfb: hyper_w_1.2.weight [32 N, 64] and hyper_w_final.2.weight [32, 64] as torch keeps them
    (None: the mixer's own copies).  Returns (d_q [B, rows, N, A], d_pre [B, rows, 192], d_p2 [B, rows, 32 N + 32], g
    [B, rows, 160]): d_q is written whole, zeros and row T included; the other three (None unless qmix) are the per-row arrays that
    the weight gradients are sums of, with zeros in masked rows and in row T.  d_q_out (laid out like q) / d_pre_out / d_p2_out /
    g_out (the same number of rows per episode in all three): outputs to reuse; nothing is allocated when they are given."""
    who = "mixer_backward: "
    B, rows, N, A, D, q_pitch, obs_pitch = _check(who, q, actions, obs, mask, mixer)
    dev, T, qmix = q.device, rows - 1, mixer.kind == "qmix"
    tail = (N,) if mixer.kind == "none" else ()
    _args.check_tensor(who + "d_mixed", d_mixed, _F32, (B, T) + tail, dev, contiguous=False, errors=_args.VALUE)
    out_pitch = _args.episode_pitch(who + "mask", mask, ())
    if _args.episode_pitch(who + "d_mixed", d_mixed, tail) != out_pitch and B > 1:
        raise ValueError(f"{who}mask and d_mixed must take the same number of rows per episode")
    if d_q_out is not None:
        _args.check_tensor(who + "d_q_out", d_q_out, _F32, (B, rows, N, A), dev, contiguous=False, errors=_args.VALUE)
        if _args.episode_pitch(who + "d_q_out", d_q_out, (N, A)) != q_pitch and B > 1:
            raise ValueError(f"{who}q and d_q_out must take the same number of rows per episode")
    aux = [("d_pre_out", d_pre_out, (COLS,)), ("d_p2_out", d_p2_out, (N * EMBED + EMBED,)), ("g_out", g_out, (G_COLS,))]
    for name, t, inner in aux:
        if t is not None:
            if not qmix:
                raise ValueError(f"{who}{name} is an output of the qmix mixer alone")
            _args.check_tensor(who + name, t, _F32, (B, rows) + inner, dev, contiguous=False, errors=_args.VALUE)
    aux_pitch = _args.shared_pitch(who, aux, rows)
    for name, t, shape in (("w1b", w1b, (N * EMBED, HYPER)), ("wfb", wfb, (EMBED, HYPER))):
        if t is not None:
            _args.check_tensor(who + name, t, _F32, shape, dev, errors=_args.VALUE)
    _needs_hip(who, dev)
    if d_q_out is None:
        d_q_out = torch.empty(B, q_pitch, N, A, device=dev)[:, :rows]
    if qmix:
        if d_pre_out is None:
            d_pre_out = torch.empty(B, aux_pitch, COLS, device=dev)[:, :rows]
        if d_p2_out is None:
            d_p2_out = torch.empty(B, aux_pitch, N * EMBED + EMBED, device=dev)[:, :rows]
        if g_out is None:
            g_out = torch.empty(B, aux_pitch, G_COLS, device=dev)[:, :rows]
    io = _lib.RgMixerGradIO(q.data_ptr(), actions.data_ptr(), obs.data_ptr(), mask.data_ptr(), None, d_mixed.data_ptr(), d_q_out.data_ptr(),
                            _ptr(d_pre_out), _ptr(d_p2_out), _ptr(g_out), B, N, D, A, rows, q_pitch, obs_pitch, out_pitch,
                            aux_pitch if qmix else 0, 0)
    _launch("rg_mixer_backward", _weights(mixer, w1b, wfb), io, dev, stream)
    return d_q_out, d_pre_out, d_p2_out, g_out


PARAM_NAMES = tuple(qmix_shapes(1, 1))     # EPyMARL's QMixer keys, in the order MixerFn takes the parameters


class MixerFn(torch.autograd.Function):
    """MixerFn.apply(q, actions, obs, mask, operands, *params) -> mixed: mixer_forward with a backward pass.  operands: the
    TargetMixer that holds the packed copy of `params` (the 14 QMixer tensors in PARAM_NAMES' order; none for vdn / none).  The
    backward pass is one launch (mixer_backward) and, for qmix, torch's GEMMs over all rows for the weight gradients:
    dW_in = d_pre^T state, dW1b = dp1^T g1, dWfb = dpf^T gf, dVb = sum dy gv, the biases as column sums.  The state of the masked
    rows is not read there either: the GEMM takes a copy of obs with zeros in them."""

    @staticmethod
    def forward(ctx, q, actions, obs, mask, operands, *params):
        q, mask = q.detach(), mask.detach()
        try:        # q and actions are addressed with one pitch: a copy of either only where their layouts differ
            same = _args.episode_pitch("q", q, q.shape[2:]) == _args.episode_pitch("actions", actions, actions.shape[2:])
        except (ValueError, AttributeError, IndexError, TypeError):
            same = False
        if not same and isinstance(actions, torch.Tensor):
            q, actions = q.contiguous(), actions.contiguous()
        mixed = mixer_forward(q, actions, obs, mask, operands)
        ctx.save_for_backward(q, actions, obs, mask, *[p.detach() for p in params])
        ctx.operands, ctx.version = operands, getattr(operands, "version", 0)
        return mixed

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_mixed):
        q, actions, obs, mask, *params = ctx.saved_tensors
        ops = ctx.operands
        B, rows, N, _ = q.shape
        T = rows - 1
        if params and getattr(ops, "version", 0) != ctx.version:     # another forward has re-packed since: pack this one's again
            ops._pack(dict(zip(PARAM_NAMES, params)))
            ops.version = ctx.version = getattr(ops, "version", 0) + 1
        # laid out as mask is (B T words: the one copy of the backward pass that is not a launch's own output)
        pitch = _args.episode_pitch("mask", mask, ())
        tail = (N,) if ops.kind == "none" else ()
        dm = torch.empty((B, pitch) + tail, device=q.device)[:, :T]
        dm.copy_(d_mixed)
        p = dict(zip(PARAM_NAMES, params))
        d_q, d_pre, d_p2, g = mixer_backward(q, actions, obs, mask, dm, ops, p.get("hyper_w_1.2.weight"), p.get("hyper_w_final.2.weight"))
        if ops.kind != "qmix":
            return (d_q, None, None, None, None)
        S, NE = ops.state_dim, N * EMBED
        live = torch.zeros(B, rows, dtype=torch.bool, device=q.device)
        live[:, :T] = mask != 0
        state = torch.where(live.unsqueeze(-1), obs.flatten(2), obs.new_zeros(())).view(B * rows, S)
        dy = torch.where(live[:, :T], dm, dm.new_zeros(())).reshape(1, B * T)
        d_pre, d_p2, g = d_pre.reshape(B * rows, COLS), d_p2.reshape(B * rows, NE + EMBED), g.reshape(B * rows, G_COLS)
        d_w_in, d_b_in = d_pre.t() @ state, d_pre.sum(dim=0)
        grads = {}
        for c, k, n in FIRST_LAYERS:
            grads[k + ".weight"], grads[k + ".bias"] = d_w_in[c:c + n], d_b_in[c:c + n]
        grads["hyper_w_1.2.weight"], grads["hyper_w_1.2.bias"] = d_p2[:, :NE].t() @ g[:, :HYPER], d_p2[:, :NE].sum(dim=0)
        grads["hyper_w_final.2.weight"], grads["hyper_w_final.2.bias"] = d_p2[:, NE:].t() @ g[:, HYPER:2 * HYPER], d_p2[:, NE:].sum(dim=0)
        gv = g.view(B, rows, G_COLS)[:, :T, 2 * HYPER:].reshape(B * T, EMBED)
        grads["V.2.weight"], grads["V.2.bias"] = dy @ gv, dy.sum(dim=1)
        return (d_q, None, None, None, None) + tuple(grads[k] for k in PARAM_NAMES)


class TrainableMixer(torch.nn.Module):
    """EPyMARL's mixer as a torch module whose pass over an episode batch is one launch forward and one backward.  kind: "qmix"
    (QMixer with mixing_embed_dim 32, hypernet_layers 2, hypernet_embed 64: parameters hyper_w_1.0 / .2, hyper_w_final.0 / .2,
    hyper_b_1, V.0 / .2 -- EPyMARL's own names and shapes, targets.qmix_shapes, so a checkpoint loads with load_state_dict and any
    torch optimiser works), "vdn" or "none" (no parameters).

    The launches read packed operands (include/robogym.h rg_mixer_weights); the parameters change with every optimiser step, so
    every forward() re-packs them under no_grad into ONE persistent buffer (a TargetMixer's): 14 small copies, no allocation.  The
    backward launch reads the second layers' weights in torch's own layout, straight from the parameters."""

    def __init__(self, kind, n_agents, state_dim, device=None):
        super().__init__()
        if kind not in KINDS:
            raise ValueError(f"kind must be one of {tuple(KINDS)}, got {kind!r}")
        for k, v in (("n_agents", n_agents), ("state_dim", state_dim)):
            if isinstance(v, bool) or not isinstance(v, int) or v < 1:
                raise ValueError(f"{k} must be an int >= 1, got {v!r}")
        if n_agents > _lib.MAX_AGENTS:
            raise ValueError(f"n_agents must be <= {_lib.MAX_AGENTS}, got {n_agents}")
        self.kind, self.n_agents, self.state_dim = kind, n_agents, state_dim
        self._operands = None
        if kind == "qmix":
            if (state_dim + 3) // 4 * 4 > MAX_STATE:
                raise ValueError(f"state_dim {state_dim} is above {MAX_STATE}: not supported by the launch")
            L, S = torch.nn.Linear, state_dim
            self.hyper_w_1 = torch.nn.Sequential(L(S, HYPER), torch.nn.ReLU(), L(HYPER, n_agents * EMBED))
            self.hyper_w_final = torch.nn.Sequential(L(S, HYPER), torch.nn.ReLU(), L(HYPER, EMBED))
            self.hyper_b_1 = L(S, EMBED)
            self.V = torch.nn.Sequential(L(S, EMBED), torch.nn.ReLU(), L(EMBED, 1))
        if device is not None:
            self.to(device)

    @classmethod
    def from_target(cls, target_mixer, device=None):
        """A TrainableMixer with the weights of a TargetMixer, on its device unless told otherwise."""
        if not isinstance(target_mixer, TargetMixer):
            raise ValueError(f"TrainableMixer: from_target needs a TargetMixer, got {type(target_mixer).__name__}")
        self = cls(target_mixer.kind, target_mixer.n_agents, target_mixer.state_dim, device=target_mixer.device if device is None else device)
        self.load_state_dict(target_mixer.state_dict())
        return self

    def _params(self):
        return [self.get_parameter(k) for k in PARAM_NAMES] if self.kind == "qmix" else []

    def _device(self):
        ps = self._params()
        return ps[0].device if ps else None

    def operands(self, device):
        """The TargetMixer that holds the packed operands, re-packed from the parameters as they are now."""
        ops = self._operands
        if ops is None or ops.device != device:
            with torch.no_grad():
                ops = self._operands = TargetMixer(self.kind, self.n_agents, self.state_dim,
                                                   {k: p.detach() for k, p in zip(PARAM_NAMES, self._params())}, device=device)
            ops.version = 0
        elif self.kind == "qmix":
            with torch.no_grad():
                ops._pack(dict(zip(PARAM_NAMES, self._params())))
            ops.version += 1
        return ops

    def forward(self, q, actions, obs, mask):
        """q [B, rows, N, A] f32 (TrainableActor's result is read in place), actions [B, rows, N] int32 or EPyMARL's
        [B, rows, N, 1], obs [B, rows, N, D] f32, mask [B, rows - 1] or [B, rows - 1, 1] f32 -> mixed [B, rows - 1] (`none`:
        [B, rows - 1, N]) with a graph through q and the parameters.  ValueError for a module that is not on a HIP device
        ("no host path"), not float32, or for tensors of a wrong dtype, shape or device."""
        who = "TrainableMixer: "
        ps = self._params()
        if ps and ps[0].dtype != torch.float32:
            raise ValueError(f"{who}the module must be float32, it is {ps[0].dtype}")
        if not isinstance(q, torch.Tensor):
            raise ValueError(f"{who}q must be a tensor, got {type(q).__name__}")
        if isinstance(actions, torch.Tensor) and actions.dim() == 4 and actions.shape[3] == 1:
            actions = actions[..., 0]
        if isinstance(actions, torch.Tensor) and actions.dtype == torch.int64:
            actions = actions.to(torch.int32)
        if isinstance(mask, torch.Tensor) and mask.dim() == 3 and mask.shape[2] == 1:
            mask = mask[..., 0]
        dev = self._device() or q.device
        if ps and q.device != dev:
            raise ValueError(f"{who}the module is on {dev}, q on {q.device}")
        if dev.type != "cuda":
            _check(who, q, actions, obs, mask, TargetMixer(self.kind, self.n_agents, self.state_dim, device=q.device))
            raise ValueError(f"{who}the module lives on {dev}; the launch runs on a HIP device and has no host path "
                             "(forward_reference is the torch composition)")
        return MixerFn.apply(q, actions, obs, mask, self.operands(dev), *ps)

    def forward_reference(self, q, actions, obs, mask, parts=None):
        """The same function as plain torch ops -- torch.gather, then TargetMixer.forward's lines on the parameters, times the
        live rows -- on any device and in any floating-point dtype: the baseline, and with .double() the float64 reference.
        parts: a dict that receives the intermediates the backward launch's per-row arrays are gradients of, over the B T flat
        rows -- "pre" [B T, 192] = (a1, af, av, b1), "p2" [B T, 32 N + 32] = (p1, pf), both with retain_grad(), and "g"
        [B T, 160] -- through which the result is then computed (qmix only)."""
        import torch.nn.functional as F
        if actions.dim() == 4:
            actions = actions[..., 0]
        if mask.dim() == 3:
            mask = mask[..., 0]
        B, rows, N, _ = q.shape
        T = rows - 1
        live = mask != 0
        act = torch.where(live.unsqueeze(-1), actions[:, :T].to(torch.int64), torch.zeros((), dtype=torch.int64, device=q.device))
        x = torch.gather(q[:, :T], 3, act.unsqueeze(-1)).squeeze(-1)
        x = torch.where(live.unsqueeze(-1), x, x.new_zeros(()))
        if self.kind == "none":
            return x
        if self.kind == "vdn":
            return x.sum(dim=-1)
        p = dict(zip(PARAM_NAMES, self._params()))
        s = obs[:, :T].reshape(B * T, self.state_dim)
        s = torch.where(live.reshape(B * T, 1), s, s.new_zeros(()))
        if parts is None:
            g1 = F.relu(F.linear(s, p["hyper_w_1.0.weight"], p["hyper_w_1.0.bias"]))
            gf = F.relu(F.linear(s, p["hyper_w_final.0.weight"], p["hyper_w_final.0.bias"]))
            gv = F.relu(F.linear(s, p["V.0.weight"], p["V.0.bias"]))
            b1 = F.linear(s, p["hyper_b_1.weight"], p["hyper_b_1.bias"])
            p1 = F.linear(g1, p["hyper_w_1.2.weight"], p["hyper_w_1.2.bias"])
            pf = F.linear(gf, p["hyper_w_final.2.weight"], p["hyper_w_final.2.bias"])
        else:
            pre = torch.cat([F.linear(s, p[k + ".weight"], p[k + ".bias"]) for _, k, _ in FIRST_LAYERS], dim=1)
            g = F.relu(pre[:, :G_COLS])
            g1, gf, gv, b1 = g[:, :HYPER], g[:, HYPER:2 * HYPER], g[:, 2 * HYPER:], pre[:, G_COLS:]
            p2 = torch.cat([F.linear(g1, p["hyper_w_1.2.weight"], p["hyper_w_1.2.bias"]),
                            F.linear(gf, p["hyper_w_final.2.weight"], p["hyper_w_final.2.bias"])], dim=1)
            p1, pf = p2[:, :N * EMBED], p2[:, N * EMBED:]
            if pre.requires_grad:
                pre.retain_grad(), p2.retain_grad()
            parts.update(pre=pre, p2=p2, g=g)
        w1 = torch.abs(p1).view(-1, N, EMBED)
        hidden = F.elu(torch.bmm(x.reshape(-1, 1, N), w1) + b1.view(-1, 1, EMBED))
        v = F.linear(gv, p["V.2.weight"], p["V.2.bias"]).view(-1, 1, 1)
        y = (torch.bmm(hidden, torch.abs(pf).view(-1, EMBED, 1)) + v).view(B, T)
        return torch.where(live, y, y.new_zeros(()))
