"""TD targets: the gradient-free half of a Q-learner's training step -- episode mask, double-Q gather, TARGET MIXER,
reward + gamma (1 - terminated) mixed -- in one HIP launch (rg_td_targets, include/robogym.h).

    mixer = TargetMixer("qmix", n_agents, n_agents * obs_dim, target_mixer.state_dict(), device="cuda:0")
    out = td_targets(qt, obs, reward, terminated, filled, mixer, gamma=0.99, sel=greedy)
    out["targets"], out["mask"], out["agent_q"]     # [B, rows - 1], [B, rows - 1], [B, rows - 1, N]

The rule -- which rows are masked, which are terminal, what is read and what is not, the order of the arithmetic -- is stated once
in csrc/td_targets.h and DESIGN.md section 4 "TD targets".  There is no host path: td_targets() needs the library and a HIP device;
TargetMixer.forward() is the plain torch composition of the mixer (EPyMARL's QMixer / VDNMixer), on any device.
"""
import ctypes as C
import math

import torch

from . import _args, _lib

KINDS = {"none": _lib.MIXER_NONE, "vdn": _lib.MIXER_VDN, "qmix": _lib.MIXER_QMIX}
EMBED, HYPER = 32, 64                   # mixing_embed_dim, hypernet_embed (hypernet_layers: 2): the one instantiation
MAX_STATE = 256                         # the padded state width the kernel's LDS image holds
COLS = 2 * HYPER + 2 * EMBED            # the four first layers side by side: 192 columns
# (first column, state-dict prefix, width) of each in w_in / b_in
FIRST_LAYERS = ((0, "hyper_w_1.0", HYPER), (HYPER, "hyper_w_final.0", HYPER), (2 * HYPER, "V.0", EMBED), (2 * HYPER + EMBED, "hyper_b_1", EMBED))


def qmix_shapes(n_agents, state_dim):
    """EPyMARL's QMixer state dict (mixing_embed_dim 32, hypernet_layers 2, hypernet_embed 64): key -> shape."""
    S, N = state_dim, n_agents
    return {"hyper_w_1.0.weight": (HYPER, S), "hyper_w_1.0.bias": (HYPER,),
            "hyper_w_1.2.weight": (N * EMBED, HYPER), "hyper_w_1.2.bias": (N * EMBED,),
            "hyper_w_final.0.weight": (HYPER, S), "hyper_w_final.0.bias": (HYPER,),
            "hyper_w_final.2.weight": (EMBED, HYPER), "hyper_w_final.2.bias": (EMBED,),
            "hyper_b_1.weight": (EMBED, S), "hyper_b_1.bias": (EMBED,),
            "V.0.weight": (EMBED, S), "V.0.bias": (EMBED,), "V.2.weight": (1, EMBED), "V.2.bias": (1,)}


def packed_layout(n_agents, state_dim):
    """name -> (offset, shape) of the packed arrays in TargetMixer.packed (float32 elements; every offset a multiple of 4, so every
    array is 16-byte aligned), and the total length.  The layout of include/robogym.h rg_mixer_weights."""
    sp = (state_dim + 3) // 4 * 4
    out, off = {}, 0
    for name, shape in (("w_in", (sp, COLS)), ("b_in", (COLS,)), ("w_w1", (HYPER, n_agents * EMBED)), ("b_w1", (n_agents * EMBED,)),
                        ("w_wf", (HYPER, EMBED)), ("b_wf", (EMBED,)), ("w_v", (EMBED,)), ("b_v", (1,))):
        out[name] = (off, shape)
        off += (math.prod(shape) + 3) // 4 * 4
    return out, off


class TargetMixer(object):
    """A mixer whose weights are packed once for rg_td_targets.  kind: "none", "vdn" or "qmix".  state_dict: EPyMARL's QMixer
    state dict (qmix only; None: torch's default initialisation of the same layers, drawn from `seed`).  load_state_dict()
    re-packs into the same storage: a soft or hard target update allocates nothing."""

    def __init__(self, kind, n_agents, state_dim, state_dict=None, device="cuda:0", seed=0):
        if kind not in KINDS:
            raise ValueError(f"kind must be one of {tuple(KINDS)}, got {kind!r}")
        for k, v in (("n_agents", n_agents), ("state_dim", state_dim)):
            if isinstance(v, bool) or not isinstance(v, int) or v < 1:
                raise ValueError(f"{k} must be an int >= 1, got {v!r}")
        if n_agents > _lib.MAX_AGENTS:
            raise ValueError(f"n_agents must be <= {_lib.MAX_AGENTS}, got {n_agents}")
        self.kind, self.n_agents, self.state_dim = kind, n_agents, state_dim
        self.device = torch.device(device)
        self.params, self.packed = None, None
        if kind != "qmix":
            if state_dict:
                raise ValueError(f"a {kind!r} mixer has no weights, got a state dict of {len(state_dict)} entries")
            return
        if (state_dim + 3) // 4 * 4 > MAX_STATE:
            raise ValueError(f"state_dim {state_dim} is above {MAX_STATE}: not supported by the launch")
        self.layout, total = packed_layout(n_agents, state_dim)
        self.params = {k: torch.zeros(s, device=self.device) for k, s in qmix_shapes(n_agents, state_dim).items()}
        self.packed = torch.zeros(total, device=self.device)
        if state_dict is None:
            g = torch.Generator().manual_seed(seed)
            state_dict = {}
            for k, s in qmix_shapes(n_agents, state_dim).items():     # nn.Linear's default: U(-1 / sqrt(fan_in), 1 / sqrt(fan_in))
                fan_in = qmix_shapes(n_agents, state_dim)[k.rsplit(".", 1)[0] + ".weight"][1]
                state_dict[k] = (torch.rand(s, generator=g) * 2 - 1) / math.sqrt(fan_in)
        self.load_state_dict(state_dict)

    def load_state_dict(self, state_dict):
        """Checks and re-packs (qmix): ValueError for missing keys, wrong shapes, the shapes of hypernet_layers: 1, weights that are
        not finite.  Nothing is allocated on the mixer's device beyond the copies of the incoming tensors."""
        if self.kind != "qmix":
            if state_dict:
                raise ValueError(f"a {self.kind!r} mixer has no weights")
            return
        shapes = qmix_shapes(self.n_agents, self.state_dim)
        if "hyper_w_1.weight" in state_dict or "hyper_w_final.weight" in state_dict:
            raise ValueError("the state dict is a QMixer with hypernet_layers: 1 (hyper_w_1.weight); only hypernet_layers: 2 is supported")
        missing = [k for k in shapes if k not in state_dict]
        if missing:
            raise ValueError(f"the state dict lacks {missing}")
        for k, s in shapes.items():
            t = state_dict[k]
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != s:
                raise ValueError(f"state_dict[{k!r}] must be a tensor {s} (mixing_embed_dim {EMBED}, hypernet_embed {HYPER}, n_agents "
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
        return {} if self.params is None else {k: v.clone() for k, v in self.params.items()}

    def _view(self, name):
        off, shape = self.layout[name]
        return self.packed[off:off + math.prod(shape)].view(shape)

    def _pack(self, params=None):
        """params: the tensors to pack in place of self.params (mixers.TrainableMixer hands its parameters over with this)."""
        p, S = self.params if params is None else params, self.state_dim
        w_in = self._view("w_in")
        for c, k, n in FIRST_LAYERS:
            w_in[:S, c:c + n].copy_(p[k + ".weight"].t())
            self._view("b_in")[c:c + n].copy_(p[k + ".bias"])
        w_in[S:].zero_()
        self._view("w_w1").copy_(p["hyper_w_1.2.weight"].t())
        self._view("b_w1").copy_(p["hyper_w_1.2.bias"])
        self._view("w_wf").copy_(p["hyper_w_final.2.weight"].t())
        self._view("b_wf").copy_(p["hyper_w_final.2.bias"])
        self._view("w_v").copy_(p["V.2.weight"][0])
        self._view("b_v").copy_(p["V.2.bias"])

    def unpack(self):
        """The state dict read back out of the packed arrays (what the launch sees)."""
        S = self.state_dim
        w_in, b_in = self._view("w_in"), self._view("b_in")
        out = {}
        for c, k, n in FIRST_LAYERS:
            out[k + ".weight"] = w_in[:S, c:c + n].t().clone()
            out[k + ".bias"] = b_in[c:c + n].clone()
        out["hyper_w_1.2.weight"], out["hyper_w_1.2.bias"] = self._view("w_w1").t().clone(), self._view("b_w1").clone()
        out["hyper_w_final.2.weight"], out["hyper_w_final.2.bias"] = self._view("w_wf").t().clone(), self._view("b_wf").clone()
        out["V.2.weight"], out["V.2.bias"] = self._view("w_v").clone().view(1, EMBED), self._view("b_v").clone()
        return out

    def forward(self, agent_q, state):
        """The mixer in plain torch ops: agent_q [..., N], state [..., S] -> [..., 1] (`none`: agent_q itself).  EPyMARL's
        QMixer.forward / VDNMixer.forward."""
        import torch.nn.functional as F
        if self.kind == "none":
            return agent_q
        if self.kind == "vdn":
            return agent_q.sum(dim=-1, keepdim=True)
        p, N = self.params, self.n_agents
        lead = agent_q.shape[:-1]
        s = state.reshape(-1, self.state_dim)
        q = agent_q.reshape(-1, 1, N)
        w1 = torch.abs(F.linear(F.relu(F.linear(s, p["hyper_w_1.0.weight"], p["hyper_w_1.0.bias"])), p["hyper_w_1.2.weight"],
                                p["hyper_w_1.2.bias"])).view(-1, N, EMBED)
        b1 = F.linear(s, p["hyper_b_1.weight"], p["hyper_b_1.bias"]).view(-1, 1, EMBED)
        hidden = F.elu(torch.bmm(q, w1) + b1)
        wf = torch.abs(F.linear(F.relu(F.linear(s, p["hyper_w_final.0.weight"], p["hyper_w_final.0.bias"])),
                                p["hyper_w_final.2.weight"], p["hyper_w_final.2.bias"])).view(-1, EMBED, 1)
        v = F.linear(F.relu(F.linear(s, p["V.0.weight"], p["V.0.bias"])), p["V.2.weight"], p["V.2.bias"]).view(-1, 1, 1)
        return (torch.bmm(hidden, wf) + v).view(*lead, 1)

    def weights_struct(self):
        """include/robogym.h rg_mixer_weights over the packed storage."""
        w = _lib.RgMixerWeights()
        w.kind, w.n_agents, w.state_dim = KINDS[self.kind], self.n_agents, self.state_dim
        if self.kind == "qmix":
            w.embed_dim, w.hypernet_embed = EMBED, HYPER
            for name, (off, _) in self.layout.items():
                setattr(w, name, self.packed.data_ptr() + 4 * off)
        return w


def td_targets(qt, obs, reward, terminated, filled, mixer, gamma, sel=None, targets_out=None, mask_out=None, agent_q_out=None,
               stream=None):
    """TD targets of an episode batch in ONE launch (rg_td_targets; the rule: csrc/td_targets.h).  qt [B, rows, N, A] f32: the
    target actor's unroll; sel [B, rows, N] int32 or None: the online actor's greedy actions (double-Q; None: the maximum over the
    actions); obs [B, rows, N, D] f32 (the state of a row is its N D floats; read with a qmix mixer only); reward [B, rows] f32,
    terminated and filled [B, rows] uint8 or bool.  Slices [:, :rows] of longer arrays are read in place: the dimensions behind the
    batch must be contiguous, qt and sel must take the same number of rows per episode, and so must reward, terminated and filled.
    Returns {"targets" [B, rows - 1] (a `none` mixer: [B, rows - 1, N]), "mask" [B, rows - 1], "agent_q" [B, rows - 1, N]}, float32;
    targets_out / mask_out / agent_q_out: outputs to reuse (the same number of rows per episode in all three); nothing is allocated
    when all three are given, so the call can be captured.  ValueError for a wrong dtype, shape, stride or device and for what the
    launch refuses."""
    if not isinstance(mixer, TargetMixer):
        raise ValueError(f"td_targets: mixer must be a TargetMixer, got {type(mixer).__name__}")
    _args.check_tensor("td_targets: qt", qt, (torch.float32,), None, contiguous=False, errors=_args.VALUE)
    if qt.dim() != 4:
        raise ValueError(f"td_targets: qt must be [B, rows, N, A], got {tuple(qt.shape)}")
    B, rows, N, A = qt.shape
    if B < 1 or rows < 2:
        raise ValueError(f"td_targets: qt must be [B, rows, N, A] with B >= 1 and rows >= 2, got {tuple(qt.shape)}")
    if N != mixer.n_agents:
        raise ValueError(f"td_targets: qt has {N} agents, the mixer {mixer.n_agents}")
    if not 1 <= A <= 32:
        raise ValueError(f"td_targets: n_actions must be in 1..32, qt has {A}")
    if not isinstance(obs, torch.Tensor) or obs.dim() != 4 or obs.shape[3] < 1:
        raise ValueError(f"td_targets: obs must be a float32 tensor [{B}, {rows}, {N}, D] with D >= 1")
    D = obs.shape[3]
    if mixer.kind == "qmix" and N * D != mixer.state_dim:
        raise ValueError(f"td_targets: the mixer's state_dim is {mixer.state_dim}, obs provides {N} x {D}")
    if isinstance(gamma, bool) or not isinstance(gamma, (int, float)) or not math.isfinite(gamma) or not 0.0 <= gamma <= 1.0:
        raise ValueError(f"td_targets: gamma must be a finite number in [0, 1], got {gamma!r}")
    dev = qt.device
    T = rows - 1
    flags = (torch.uint8, torch.bool)
    f32, t_shape = (torch.float32,), ((B, T, N) if mixer.kind == "none" else (B, T))
    # (name, tensor, dtypes, shape), grouped as the launch addresses them: one pitch per group
    qt_arg, sel_arg = ("qt", qt, f32, (B, rows, N, A)), ("sel", sel, (torch.int32,), (B, rows, N))
    obs_arg = ("obs", obs, f32, (B, rows, N, D))
    flag_args = [("reward", reward, f32, (B, rows)), ("terminated", terminated, flags, (B, rows)), ("filled", filled, flags, (B, rows))]
    out_args = [("targets_out", targets_out, f32, t_shape), ("mask_out", mask_out, f32, (B, T)), ("agent_q_out", agent_q_out, f32, (B, T, N))]
    for name, t, dtypes, shape in [obs_arg] + flag_args + [a for a in [sel_arg] + out_args if a[1] is not None]:
        _args.check_tensor("td_targets: " + name, t, dtypes, shape, dev, contiguous=False, errors=_args.VALUE)
    if mixer.device != dev:
        raise ValueError(f"td_targets: the mixer is on {mixer.device}, qt on {dev}")
    pitch = lambda args, dense: _args.shared_pitch("td_targets: ", [(n, t, shape[2:]) for n, t, _, shape in args], dense)  # noqa: E731
    q_pitch, obs_pitch = pitch([qt_arg, sel_arg], rows), pitch([obs_arg], rows)
    flag_pitch, out_pitch = pitch(flag_args, rows), pitch(out_args, T)
    if dev.type != "cuda":
        raise ValueError(f"td_targets: qt lives on {dev}; the launch runs on a HIP device and has no host path")
    lib = _lib.load()
    if targets_out is None:
        targets_out = torch.empty((B, out_pitch) + t_shape[2:], device=dev)[:, :T]
    if mask_out is None:
        mask_out = torch.empty(B, out_pitch, device=dev)[:, :T]
    if agent_q_out is None:
        agent_q_out = torch.empty(B, out_pitch, N, device=dev)[:, :T]
    stream, hip_stream = _args.launch_stream(stream, dev)
    m = mixer.weights_struct()
    as_u8 = lambda t: t.view(torch.uint8) if t.dtype == torch.bool else t  # noqa: E731
    io = _lib.RgTdTargetsIO(qt.data_ptr(), sel.data_ptr() if sel is not None else None, obs.data_ptr(), reward.data_ptr(),
                            as_u8(terminated).data_ptr(), as_u8(filled).data_ptr(), targets_out.data_ptr(), mask_out.data_ptr(),
                            agent_q_out.data_ptr(), B, N, D, A, rows, q_pitch, obs_pitch, flag_pitch, out_pitch, float(gamma), 0)
    with torch.cuda.device(dev):
        rc = lib.rg_td_targets(C.byref(m), C.byref(io), hip_stream)
    if rc != 0:
        raise _args.launch_error(rc, lib.rg_td_targets_last_error().decode())
    return {"targets": targets_out, "mask": mask_out, "agent_q": agent_q_out}
