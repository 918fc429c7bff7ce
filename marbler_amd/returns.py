"""N-step returns: what a PPO learner computes under no_grad every epoch -- the episode mask, the TARGET CRITIC over every row of
the episode batch, and EPyMARL's nstep_returns -- in one HIP launch (rg_nstep_returns, include/robogym_returns.h).

    critic = TargetCritic("cv", n_agents, n_agents * obs_dim, 128, target_critic.state_dict(), device="cuda:0")
    out = nstep_returns(obs, reward, terminated, filled, critic, gamma=0.99, nstep=10)
    out["returns"], out["values"], out["mask"]      # [B, rows - 1, N], [B, rows, N], [B, rows - 1]

The rule -- the mask, which rows are needed, what is read and what is not, the order of the scan's arithmetic, the one deliberate
difference from EPyMARL -- is stated once in csrc/nstep_returns.h and DESIGN.md section 4 "N-step returns".  There is no host path:
nstep_returns() needs the library and a HIP device; TargetCritic.forward() is the plain torch composition of the critic (EPyMARL's
CentralVCritic / CentralVCriticNS), on any device.
"""
import ctypes as C
import math

import torch

from . import _args, _lib

KINDS = {"cv": _lib.CRITIC_CV, "cv_ns": _lib.CRITIC_CV_NS}
HIDDEN = (64, 128)                      # the kernel's two instantiations
MAX_STATE = 256                         # the padded state width the kernel's LDS image holds
LAYERS = ("fc1", "fc2", "fc3")


def critic_shapes(kind, n_agents, state_dim, hidden_dim):
    """One network's state dict (EPyMARL's CentralVCritic: fc1 sees [state, onehot(agent)]; one of CentralVCriticNS's critics:
    fc1 sees the state alone): key -> shape."""
    H, wide = hidden_dim, state_dim + (n_agents if kind == "cv" else 0)
    return {"fc1.weight": (H, wide), "fc1.bias": (H,), "fc2.weight": (H, H), "fc2.bias": (H,), "fc3.weight": (1, H), "fc3.bias": (1,)}


def packed_layout(kind, n_agents, state_dim, hidden_dim):
    """name -> (offset, shape) of ONE network's packed arrays (float32 elements; every offset a multiple of 4, so every array is
    16-byte aligned), and the network's length: the layout of include/robogym_returns.h rg_critic_weights.  A cv_ns critic is
    n_agents such networks back to back."""
    sp, H = (state_dim + 7) // 8 * 8, hidden_dim
    arrays = [("w1", (sp, H))] + ([("w1_id", (n_agents, H))] if kind == "cv" else []) + \
             [("b1", (H,)), ("w2", (H, H)), ("b2", (H,)), ("w3", (H,)), ("b3", (1,))]
    out, off = {}, 0
    for name, shape in arrays:
        out[name] = (off, shape)
        off += (math.prod(shape) + 3) // 4 * 4
    return out, off


class TargetCritic(object):
    """A centralised V critic whose weights are packed once for rg_nstep_returns.  kind: "cv" (one network, the agent's one-hot id
    behind the state) or "cv_ns" (n_agents networks on the state alone).  state_dict: EPyMARL's (cv: fc1.weight .. fc3.bias; cv_ns:
    critics.{i}.fc1.weight .., or a list of n_agents per-network dicts; None: torch's default initialisation of the same layers,
    drawn from `seed`).  load_state_dict() re-packs into the same storage: a soft or hard target update allocates nothing."""

    def __init__(self, kind, n_agents, state_dim, hidden_dim=128, state_dict=None, device="cuda:0", seed=0):
        if kind not in KINDS:
            raise ValueError(f"kind must be one of {tuple(KINDS)}, got {kind!r}")
        for k, v in (("n_agents", n_agents), ("state_dim", state_dim), ("hidden_dim", hidden_dim)):
            if isinstance(v, bool) or not isinstance(v, int) or v < 1:
                raise ValueError(f"{k} must be an int >= 1, got {v!r}")
        if n_agents > _lib.MAX_AGENTS:
            raise ValueError(f"n_agents must be <= {_lib.MAX_AGENTS}, got {n_agents}")
        if hidden_dim not in HIDDEN:
            raise ValueError(f"hidden_dim must be one of {HIDDEN}, got {hidden_dim}")
        if (state_dim + 7) // 8 * 8 > MAX_STATE:
            raise ValueError(f"state_dim {state_dim} is above {MAX_STATE}: not supported by the launch")
        self.kind, self.n_agents, self.state_dim, self.hidden_dim = kind, n_agents, state_dim, hidden_dim
        self.n_nets = 1 if kind == "cv" else n_agents
        self.device = torch.device(device)
        self.layout, self.net_len = packed_layout(kind, n_agents, state_dim, hidden_dim)
        self.params = {k: torch.zeros(s, device=self.device) for k, s in self._shapes().items()}
        self.packed = torch.zeros(self.n_nets * self.net_len, device=self.device)
        if state_dict is None:
            g = torch.Generator().manual_seed(seed)
            state_dict, shapes = {}, self._shapes()
            for k, s in shapes.items():     # nn.Linear's default: U(-1 / sqrt(fan_in), 1 / sqrt(fan_in))
                fan_in = shapes[k.rsplit(".", 1)[0] + ".weight"][1]
                state_dict[k] = (torch.rand(s, generator=g) * 2 - 1) / math.sqrt(fan_in)
        self.load_state_dict(state_dict)

    def _prefix(self, i):
        return "" if self.kind == "cv" else f"critics.{i}."

    def _shapes(self):
        one = critic_shapes(self.kind, self.n_agents, self.state_dim, self.hidden_dim)
        return {self._prefix(i) + k: s for i in range(self.n_nets) for k, s in one.items()}

    def load_state_dict(self, state_dict):
        """Checks and re-packs: ValueError for missing keys, wrong shapes, tensors that are not floating-point or not finite.  A
        refused state dict leaves the packed weights alone.  Nothing is allocated on the critic's device beyond the copies of the
        incoming tensors."""
        if self.kind == "cv_ns" and isinstance(state_dict, (list, tuple)):
            if len(state_dict) != self.n_agents:
                raise ValueError(f"a cv_ns critic of {self.n_agents} agents needs {self.n_agents} state dicts, got {len(state_dict)}")
            state_dict = {f"critics.{i}.{k}": v for i, sd in enumerate(state_dict) for k, v in sd.items()}
        if not isinstance(state_dict, dict):
            raise ValueError(f"state_dict must be a dict{' or a list of dicts' if self.kind == 'cv_ns' else ''}, got {type(state_dict).__name__}")
        shapes = self._shapes()
        missing = [k for k in shapes if k not in state_dict]
        if missing:
            raise ValueError(f"the state dict lacks {missing}")
        for k, s in shapes.items():
            t = state_dict[k]
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != s:
                raise ValueError(f"state_dict[{k!r}] must be a tensor {s} (kind {self.kind}, hidden_dim {self.hidden_dim}, n_agents "
                                 f"{self.n_agents}, state_dim {self.state_dim}), got {tuple(getattr(t, 'shape', ()))}")
            if not t.is_floating_point():
                raise ValueError(f"state_dict[{k!r}] must be a floating-point tensor, got {t.dtype}")
        for k in shapes:
            if not bool(torch.isfinite(state_dict[k]).all()):
                raise ValueError(f"state_dict[{k!r}] holds a value that is not finite")
        for k in shapes:
            self.params[k].copy_(state_dict[k].detach())
        self._pack()

    def state_dict(self):
        return {k: v.clone() for k, v in self.params.items()}

    def _view(self, name, net=0):
        off, shape = self.layout[name]
        off += net * self.net_len
        return self.packed[off:off + math.prod(shape)].view(shape)

    def _pack(self):
        S = self.state_dim
        for i in range(self.n_nets):
            p = {k: self.params[self._prefix(i) + k] for k in critic_shapes(self.kind, self.n_agents, S, self.hidden_dim)}
            w1 = self._view("w1", i)
            w1[:S].copy_(p["fc1.weight"][:, :S].t())
            w1[S:].zero_()
            if self.kind == "cv":
                self._view("w1_id", i).copy_(p["fc1.weight"][:, S:].t())
            self._view("b1", i).copy_(p["fc1.bias"])
            self._view("w2", i).copy_(p["fc2.weight"].t())
            self._view("b2", i).copy_(p["fc2.bias"])
            self._view("w3", i).copy_(p["fc3.weight"][0])
            self._view("b3", i).copy_(p["fc3.bias"])

    def unpack(self):
        """The state dict read back out of the packed arrays (what the launch sees)."""
        S, out = self.state_dim, {}
        for i in range(self.n_nets):
            w1 = self._view("w1", i)[:S].t()
            if self.kind == "cv":
                w1 = torch.cat([w1, self._view("w1_id", i).t()], dim=1)
            pre = self._prefix(i)
            out[pre + "fc1.weight"], out[pre + "fc1.bias"] = w1.clone(), self._view("b1", i).clone()
            out[pre + "fc2.weight"], out[pre + "fc2.bias"] = self._view("w2", i).t().clone(), self._view("b2", i).clone()
            out[pre + "fc3.weight"], out[pre + "fc3.bias"] = self._view("w3", i).clone().view(1, -1), self._view("b3", i).clone()
        return out

    def forward(self, state):
        """The critic in plain torch ops: state [..., S] -> values [..., N].  EPyMARL's CentralVCritic.forward (the inputs are
        [state, onehot(agent)] per agent) / CentralVCriticNS.forward (one network per agent on the state)."""
        import torch.nn.functional as F
        p, N = self.params, self.n_agents

        def net(x, pre):
            x = F.relu(F.linear(x, p[pre + "fc1.weight"], p[pre + "fc1.bias"]))
            x = F.relu(F.linear(x, p[pre + "fc2.weight"], p[pre + "fc2.bias"]))
            return F.linear(x, p[pre + "fc3.weight"], p[pre + "fc3.bias"])
        if self.kind == "cv":
            lead = state.shape[:-1]
            eye = torch.eye(N, device=state.device, dtype=state.dtype).expand(*lead, N, N)
            inputs = torch.cat([state.unsqueeze(-2).expand(*lead, N, self.state_dim), eye], dim=-1)
            return net(inputs, "").squeeze(-1)
        return torch.cat([net(state, self._prefix(i)) for i in range(N)], dim=-1)

    def weights_struct(self):
        """include/robogym_returns.h rg_critic_weights over the packed storage."""
        w = _lib.RgCriticWeights()
        w.kind, w.n_agents, w.state_dim, w.hidden_dim = KINDS[self.kind], self.n_agents, self.state_dim, self.hidden_dim
        w.net_stride = 0 if self.kind == "cv" else self.net_len
        for name, (off, _) in self.layout.items():
            setattr(w, name, self.packed.data_ptr() + 4 * off)
        return w


def _number(name, v, lo=None, hi=None):
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or (lo is not None and not lo <= v <= hi):
        raise ValueError(f"nstep_returns: {name} must be a finite number{'' if lo is None else f' in [{lo}, {hi}]'}, got {v!r}")


def nstep_returns(obs, reward, terminated, filled, critic, gamma, nstep, add_value_last_step=True, value_scale=1.0, value_shift=0.0,
                  returns_out=None, values_out=None, mask_out=None, stream=None):
    """The target critic's values and the n-step returns of an episode batch in ONE launch (rg_nstep_returns; the rule:
    csrc/nstep_returns.h).  obs [B, rows, N, D] f32 (the state of a row is its N D floats); reward [B, rows] f32, terminated and
    filled [B, rows] uint8 or bool; critic: a TargetCritic; nstep in 1..32; value_scale / value_shift: the de-normalisation
    v * scale + shift of a learner that standardises returns.  Slices [:, :rows] of longer arrays are read in place: the dimensions
    behind the batch must be contiguous, and reward, terminated and filled must take the same number of rows per episode.
    Returns {"returns" [B, rows - 1, N], "values" [B, rows, N], "mask" [B, rows - 1]}, float32; returns_out / values_out /
    mask_out: outputs to reuse (returns_out and mask_out the same number of rows per episode); nothing is allocated when all three
    are given, so the call can be captured.  ValueError for a wrong dtype, shape, stride or device and for what the launch refuses."""
    if not isinstance(critic, TargetCritic):
        raise ValueError(f"nstep_returns: critic must be a TargetCritic, got {type(critic).__name__}")
    _args.check_tensor("nstep_returns: obs", obs, (torch.float32,), None, contiguous=False, errors=_args.VALUE)
    if obs.dim() != 4:
        raise ValueError(f"nstep_returns: obs must be [B, rows, N, D], got {tuple(obs.shape)}")
    B, rows, N, D = obs.shape
    if B < 1 or rows < 2 or D < 1:
        raise ValueError(f"nstep_returns: obs must be [B, rows, N, D] with B >= 1, rows >= 2 and D >= 1, got {tuple(obs.shape)}")
    if rows > _lib.RETURNS_MAX_ROWS:
        raise ValueError(f"nstep_returns: rows must be <= {_lib.RETURNS_MAX_ROWS}, obs has {rows}")
    if N != critic.n_agents:
        raise ValueError(f"nstep_returns: obs has {N} agents, the critic {critic.n_agents}")
    if N * D != critic.state_dim:
        raise ValueError(f"nstep_returns: the critic's state_dim is {critic.state_dim}, obs provides {N} x {D}")
    _number("gamma", gamma, 0.0, 1.0)
    if isinstance(nstep, bool) or not isinstance(nstep, int) or not 1 <= nstep <= _lib.NSTEP_MAX:
        raise ValueError(f"nstep_returns: nstep must be an int in 1..{_lib.NSTEP_MAX}, got {nstep!r}")
    if not isinstance(add_value_last_step, (bool, int)) or add_value_last_step not in (0, 1):
        raise ValueError(f"nstep_returns: add_value_last_step must be a bool, got {add_value_last_step!r}")
    _number("value_scale", value_scale)
    _number("value_shift", value_shift)
    dev = obs.device
    T = rows - 1
    flags = (torch.uint8, torch.bool)
    f32 = (torch.float32,)
    # (name, tensor, dtypes, shape), grouped as the launch addresses them: one pitch per group
    obs_arg = ("obs", obs, f32, (B, rows, N, D))
    flag_args = [("reward", reward, f32, (B, rows)), ("terminated", terminated, flags, (B, rows)), ("filled", filled, flags, (B, rows))]
    out_args = [("returns_out", returns_out, f32, (B, T, N)), ("mask_out", mask_out, f32, (B, T))]
    value_args = [("values_out", values_out, f32, (B, rows, N))]
    for name, t, dtypes, shape in flag_args + [a for a in out_args + value_args if a[1] is not None]:
        _args.check_tensor("nstep_returns: " + name, t, dtypes, shape, dev, contiguous=False, errors=_args.VALUE)
    if critic.device != dev:
        raise ValueError(f"nstep_returns: the critic is on {critic.device}, obs on {dev}")
    pitch = lambda args, dense: _args.shared_pitch("nstep_returns: ", [(n, t, shape[2:]) for n, t, _, shape in args], dense)  # noqa: E731
    obs_pitch, flag_pitch = pitch([obs_arg], rows), pitch(flag_args, rows)
    out_pitch, value_pitch = pitch(out_args, T), pitch(value_args, rows)
    if dev.type != "cuda":
        raise ValueError(f"nstep_returns: obs lives on {dev}; the launch runs on a HIP device and has no host path")
    lib = _lib.load_returns()
    if returns_out is None:
        returns_out = torch.empty(B, out_pitch, N, device=dev)[:, :T]
    if mask_out is None:
        mask_out = torch.empty(B, out_pitch, device=dev)[:, :T]
    if values_out is None:
        values_out = torch.empty(B, rows, N, device=dev)
    stream, hip_stream = _args.launch_stream(stream, dev)
    w = critic.weights_struct()
    as_u8 = lambda t: t.view(torch.uint8) if t.dtype == torch.bool else t  # noqa: E731
    io = _lib.RgNstepReturnsIO(obs.data_ptr(), reward.data_ptr(), as_u8(terminated).data_ptr(), as_u8(filled).data_ptr(),
                               returns_out.data_ptr(), values_out.data_ptr(), mask_out.data_ptr(), B, N, D, rows, nstep,
                               int(add_value_last_step), obs_pitch, flag_pitch, out_pitch, value_pitch, float(gamma),
                               float(value_scale), float(value_shift), 0)
    with torch.cuda.device(dev):
        rc = lib.rg_nstep_returns(C.byref(w), C.byref(io), hip_stream)
    if rc != 0:
        raise _args.launch_error(rc, lib.rg_nstep_returns_last_error().decode())
    return {"returns": returns_out, "values": values_out, "mask": mask_out}
