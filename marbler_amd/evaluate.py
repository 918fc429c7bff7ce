"""Batched greedy evaluation of EPyMARL actors on the device.

The reference evaluates a trained model with `python -m robotarium_gym.main` -> `run_env`
(utilities/misc.py:134-221): one env, one step at a time, actor forward on the CPU.  Here the
same loop runs for E envs at once: observations never leave the GPU, the actor
(utilities/rnn_agent.py:5-29 `RNNAgent`: fc1 -> ReLU -> GRUCell -> fc2, or the non-shared
`RNNNSAgent` of rnn_ns_agent.py:5-36 with one such network per agent) is evaluated for all
E x N agents with a handful of batched GEMMs (torch -> rocBLAS/hipBLASLt: plain library GEMMs),
actions are the arg-max Q (misc.py:170), and the episode statistics accumulate in the env's
on-device counters.  `load_actor` reads the reference's model zoo (`scenarios/*/models/*.th`
state dicts + sacred `.json` configs, misc.py:65-91) unchanged.
"""
import ctypes as C
import json

import torch

from . import _args, _lib
from .params import SIDE_BLOCKS


DEFAULT_PACK_GRU = "f16x2"   # what pack_gru=True means


class BatchedActor(object):
    """RNNAgent / RNNNSAgent weights stacked as [A, ...] with A = 1 (shared) or N (one per agent)."""

    def __init__(self, state_dict, n_agents, use_rnn=True, device="cpu", pack_gru=True):
        keys = list(state_dict.keys())
        self.non_shared = keys[0].startswith("agents.")
        self.use_rnn = bool(use_rnn)
        self.n_agents = int(n_agents)
        # fused kernel: how the two GRU matrices are handed over -- True / "f16x2": two binary16 planes (three plane products per float32
        # product on the binary16 matrix cores, error at the level of a float32 GEMM's own roundings; activations above 65 504
        # saturate); "bf16x3": three bfloat16 planes (six plane products, float32's exponent range, error below a float32 GEMM's
        # own; 1.2 x the launch time); "f32": float32 in the kernel's streaming order (f32-input MFMA, 16 x slower per product);
        # False: torch's layout as it is (f32-input MFMA)
        self.pack_gru = {True: DEFAULT_PACK_GRU, False: None, None: None}.get(pack_gru, pack_gru)
        if self.pack_gru not in (None, "bf16x3", "f16x2", "f32"):
            raise ValueError("pack_gru must be True, 'f16x2', 'bf16x3', 'f32' or False")

        def stack(name):
            if self.non_shared:
                return torch.stack([state_dict[f"agents.{i}.{name}"] for i in range(self.n_agents)]).float().to(device)
            return state_dict[name].float().unsqueeze(0).to(device)

        self.w1, self.b1 = stack("fc1.weight"), stack("fc1.bias")          # [A,H,I], [A,H]
        self.w2, self.b2 = stack("fc2.weight"), stack("fc2.bias")          # [A,O,H], [A,O]
        if self.use_rnn:
            self.wih, self.whh = stack("rnn.weight_ih"), stack("rnn.weight_hh")   # [A,3H,H]
            self.bih, self.bhh = stack("rnn.bias_ih"), stack("rnn.bias_hh")
        else:
            self.wr, self.br = stack("rnn.weight"), stack("rnn.bias")
        self.hidden_dim = self.w1.shape[1]
        self.input_dim = self.w1.shape[2]
        self.n_actions = self.w2.shape[1]

    def init_hidden(self, num_envs):
        return torch.zeros(num_envs, self.n_agents, self.hidden_dim, device=self.w1.device)

    def _lin(self, x, w, b):
        # x [E,N,I]; w [A,O,I]; b [A,O] -> [E,N,O]
        if w.shape[0] == 1:
            return torch.matmul(x, w[0].t()) + b[0]
        return torch.einsum("eni,noi->eno", x, w) + b

    def forward(self, inputs, hidden):
        """inputs [E,N,input_dim], hidden [E,N,H] -> (q [E,N,n_actions], new hidden [E,N,H])."""
        x = torch.relu(self._lin(inputs, self.w1, self.b1))
        if self.use_rnn:   # torch.nn.GRUCell: r, z, n gates in that order
            gi = self._lin(x, self.wih, self.bih)
            gh = self._lin(hidden, self.whh, self.bhh)
            H = self.hidden_dim
            r = torch.sigmoid(gi[..., :H] + gh[..., :H])
            z = torch.sigmoid(gi[..., H:2 * H] + gh[..., H:2 * H])
            n = torch.tanh(gi[..., 2 * H:] + r * gh[..., 2 * H:])
            h = (1.0 - z) * n + z * hidden
        else:
            h = torch.relu(self._lin(x, self.wr, self.br))
        return self._lin(h, self.w2, self.b2), h

    # ------------------------------------------------------------------ fused HIP kernel (csrc/actor_mfma.hip)
    def fused_supported(self):
        return (self.w1.is_cuda and self.hidden_dim in (64, 128) and self.n_actions <= 32 and self.input_dim <= 64)

    def _weights_struct(self):
        if getattr(self, "_ws", None) is None:
            t = {k: getattr(self, k).contiguous() for k in ("w1", "b1", "w2", "b2")}
            packed = 0
            if self.use_rnn:
                t.update({k: getattr(self, k).contiguous() for k in ("wih", "bih", "whh", "bhh")})
            if self.use_rnn and self.pack_gru:
                packed = self._pack_gru(t, {})
            if not self.use_rnn:
                t.update({"wih": self.wr.contiguous(), "bih": self.br.contiguous()})
            ptr = lambda k: t[k].data_ptr() if k in t else None  # noqa: E731
            self._ws_tensors = t   # keep the contiguous copies alive
            self._ws = _lib.RgActorWeights(ptr("w1"), ptr("b1"), ptr("wih"), ptr("bih"), ptr("whh"), ptr("bhh"),
                                           ptr("w2"), ptr("b2"), self.w1.shape[0], self.input_dim, self.hidden_dim,
                                           self.n_actions, 1 if self.use_rnn else 0, packed)
        return self._ws

    def _pack_gru(self, src, dst):
        """The two GRU matrices src["wih"], src["whh"] into the kernel's streaming order on the current stream: into dst[k], or into
        new buffers where dst has none; src[k] becomes the packed buffer.  Records the event weights_for orders every launch behind.
        -> rg_actor_weights.gru_packed"""
        lib = _lib.load()
        stream = C.c_void_p(torch.cuda.current_stream(self.w1.device).cuda_stream)
        for k in ("wih", "whh"):
            if self.pack_gru == "bf16x3":
                out = dst[k] if k in dst else torch.empty(src[k].numel() * 3, dtype=torch.int16, device=src[k].device)   # 6 bytes per weight
                rc = lib.rg_actor_pack_gru_bf16x3(src[k].data_ptr(), self.w1.shape[0], self.hidden_dim, out.data_ptr(), stream)
            elif self.pack_gru == "f16x2":
                out = dst[k] if k in dst else torch.empty(src[k].numel() * 2, dtype=torch.int16, device=src[k].device)   # 4 bytes per weight
                rc = lib.rg_actor_pack_gru_f16x2(src[k].data_ptr(), self.w1.shape[0], self.hidden_dim, out.data_ptr(), stream)
            else:
                out = dst[k] if k in dst else torch.empty_like(src[k])
                rc = lib.rg_actor_pack_gru(src[k].data_ptr(), self.w1.shape[0], self.hidden_dim, out.data_ptr(), stream)
            if rc != 0:
                raise _lib.RobogymError("rg_actor_pack_gru: " + lib.rg_actor_last_error().decode())
            src[k] = out
        # a first launch on ANOTHER stream must not overtake the two pack kernels (weights_for orders every launch behind this)
        self._pack_done = torch.cuda.Event()
        self._pack_done.record(torch.cuda.current_stream(self.w1.device))
        return {"bf16x3": 2, "f16x2": 3}.get(self.pack_gru, 1)

    _FC1, _FC2 = (("fc1.weight", "w1"), ("fc1.bias", "b1")), (("fc2.weight", "w2"), ("fc2.bias", "b2"))
    _GRU = (("rnn.weight_ih", "wih"), ("rnn.weight_hh", "whh"), ("rnn.bias_ih", "bih"), ("rnn.bias_hh", "bhh"))
    _RNN = (("rnn.weight", "wr"), ("rnn.bias", "br"))

    def _keys(self):
        """(EPyMARL's parameter name, the attribute that holds it stacked), in the module's own order."""
        return self._FC1 + (self._GRU if self.use_rnn else self._RNN) + self._FC2

    def state_dict(self):
        """The weights under EPyMARL's names (agents.{i}. in front with one network per agent): copies."""
        keys = self._keys()
        if self.non_shared:
            return {f"agents.{i}.{k}": getattr(self, a)[i].clone() for i in range(self.n_agents) for k, a in keys}
        return {k: getattr(self, a)[0].clone() for k, a in keys}

    def load_state_dict(self, state_dict):
        """New weights into the SAME storages (a learner's update: collect -> learn -> collect): every tensor is copied into the
        array it replaces and, where the actor has handed its weights to a launch before, the GRU matrices are packed again into
        the same packed buffers on the current stream and the event weights_for orders launches behind is recorded anew -- so the
        cached weights struct, and every graph captured around a launch of this actor, stay valid and see the new weights.
        ValueError for a state dict that is not a dict, lacks keys, changes a shape, or holds a tensor that is not floating-point
        or not finite; a refused state dict leaves the actor alone."""
        if not isinstance(state_dict, dict):
            raise ValueError(f"state_dict must be a dict, got {type(state_dict).__name__}")
        keys = self._keys()
        A = self.w1.shape[0]
        names = [((f"agents.{i}." if self.non_shared else "") + k, a, i) for i in range(A) for k, a in keys]
        missing = [n for n, _, _ in names if n not in state_dict]
        if missing:
            raise ValueError(f"the state dict lacks {missing}")
        for n, a, i in names:
            t, want = state_dict[n], tuple(getattr(self, a).shape[1:])
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != want:
                raise ValueError(f"state_dict[{n!r}] must be a tensor {want}, got {tuple(getattr(t, 'shape', ()))}")
            if not t.is_floating_point():
                raise ValueError(f"state_dict[{n!r}] must be a floating-point tensor, got {t.dtype}")
        for n, _, _ in names:
            if not bool(torch.isfinite(state_dict[n]).all()):
                raise ValueError(f"state_dict[{n!r}] holds a value that is not finite")
        with torch.no_grad():
            for n, a, i in names:
                getattr(self, a)[i].copy_(state_dict[n].detach())
        if getattr(self, "_ws", None) is not None and self.use_rnn and self.pack_gru:
            self._pack_gru({"wih": self.wih, "whh": self.whh}, {k: self._ws_tensors[k] for k in ("wih", "whh")})

    def weights_for(self, stream):
        """The weights struct for a launch on `stream` (a torch stream).  The weights were packed (once) on the then-current
        stream: until that has finished, a launch on any stream is ordered behind it here."""
        ws = self._weights_struct()
        ev = getattr(self, "_pack_done", None)
        if ev is not None:
            if ev.query():
                self._pack_done = None
            else:
                stream.wait_event(ev)
        return ws

    def forward_fused(self, obs, hidden, append_agent_id=True, restart=None, q_out=None, actions_out=None, stream=None,
                      explore_u=None, epsilon=0.0, sample_u=None, prob_out=None):
        """One actor step for all E x N agents in one launch (rg_actor_forward: the matrix cores; GRU on bfloat16 planes unless pack_gru says otherwise).
        obs [E,N,D] f32; hidden [E,N,H] f32 updated IN PLACE; restart [E] uint8 (nonzero = start that
        env's hidden state from zero) or None; stream: a torch.cuda.Stream (default: the device's current stream).
        explore_u [E,N] f32 uniforms in [0, 1) with epsilon > 0: epsilon-greedy actions (rg_actor_forward_explore; the rule is
        `explore_select` below).  sample_u [E,N] f32 uniforms in [0, 1): soft-policies actions, SAMPLED from softmax(q)
        (rg_actor_forward_sample; the rule is `soft_select` below), and prob_out [E,N] f32 (or None) receives the probability of the
        sampled action; not together with explore_u.  Returns (q [E,N,A], actions [E,N] int32)."""
        lib = _lib.load()
        E, N, D = obs.shape
        if q_out is None:
            q_out = torch.empty(E, N, self.n_actions, device=obs.device)
        if actions_out is None:
            actions_out = torch.empty(E, N, dtype=torch.int32, device=obs.device)
        stream, hip_stream = _args.launch_stream(stream, obs.device)
        args = [C.byref(self.weights_for(stream)), E, N, obs.data_ptr(), D, 1 if append_agent_id else 0,
                restart.data_ptr() if restart is not None else None, hidden.data_ptr(), q_out.data_ptr(), actions_out.data_ptr()]
        if sample_u is not None and explore_u is not None:
            raise ValueError("sample_u (soft policies) and explore_u (epsilon-greedy) do not combine")
        if prob_out is not None and sample_u is None:
            raise ValueError("prob_out needs sample_u")
        if sample_u is not None:
            _args.check_tensor("sample_u", sample_u, (torch.float32,), (E, N), errors=_args.VALUE)
            if prob_out is not None:
                _args.check_tensor("prob_out", prob_out, (torch.float32,), (E, N), errors=_args.VALUE)
            rc = lib.rg_actor_forward_sample(*args, sample_u.data_ptr(), prob_out.data_ptr() if prob_out is not None else None, hip_stream)
        elif explore_u is not None:
            _args.check_tensor("explore_u", explore_u, (torch.float32,), (E, N), errors=_args.VALUE)
            rc = lib.rg_actor_forward_explore(*args, explore_u.data_ptr(), float(epsilon), hip_stream)
        else:
            rc = lib.rg_actor_forward(*args, hip_stream)
        if rc != 0:
            raise _lib.RobogymError("rg_actor_forward: " + lib.rg_actor_last_error().decode())
        return q_out, actions_out

    # ------------------------------------------------------------------ whole episode batches (csrc/actor_unroll.h)
    def unroll(self, obs, append_agent_id=True, hidden=None, q_out=None, actions_out=None, hidden_out=None, stream=None):
        """The actor over every time step of an episode batch in ONE launch (rg_actor_unroll; the rule: csrc/actor_unroll.h):
        what `init_hidden(B)` and `rows` calls of forward_fused on the time slices compute, bit for bit, with the hidden state kept
        on the chip.  obs [B, rows, N, D] f32 on the actor's device, its last three dimensions contiguous and its batch stride a
        multiple of N D (EpisodeBuffer.obs[:, :rows] is read in place); the observation at t = 0 is read as stored.  hidden
        [B, N, H] f32 or None (zeros); hidden_out [B, N, H] or None receives the state after the last step (it may be `hidden`).
        q_out [B, rows, N, A] f32 / actions_out [B, rows, N] int32: outputs to reuse, laid out like obs (the same number of rows
        per episode in both); nothing is allocated when both are given, so the call can be captured.  Every one of the `rows`
        steps is computed: there are no masks.  Returns (q, greedy actions).  ValueError for a wrong dtype, shape, stride or
        device and for an actor the launch refuses."""
        if not (self.use_rnn and self.pack_gru == "f16x2"):
            raise ValueError("unroll: the actor must be a GRU packed as two binary16 planes (pack_gru=True / 'f16x2')")
        if self.hidden_dim not in (64, 128):
            raise ValueError(f"unroll: hidden size must be 64 or 128, the actor's is {self.hidden_dim}")
        if not 1 <= self.n_actions <= 32:
            raise ValueError(f"unroll: n_actions must be in 1..32, the actor's is {self.n_actions}")
        if (self.input_dim + 7) // 8 * 8 > 64:
            raise ValueError(f"unroll: an input width above 64 is not supported, the actor's is {self.input_dim}")
        dev, N, H, A = self.w1.device, self.n_agents, self.hidden_dim, self.n_actions
        _args.check_tensor("unroll: obs", obs, (torch.float32,), None, dev, contiguous=False, errors=_args.VALUE)
        if obs.dim() != 4 or obs.shape[0] < 1 or obs.shape[1] < 1 or obs.shape[2] != N:
            raise ValueError(f"unroll: obs must be [B, rows, {N}, D] with B, rows >= 1, got {tuple(obs.shape)}")
        B, rows, _, D = obs.shape
        if D + (N if append_agent_id else 0) != self.input_dim:
            raise ValueError(f"unroll: the actor expects {self.input_dim} inputs per agent, obs provides "
                             f"{D + (N if append_agent_id else 0)}")
        obs_pitch = _args.episode_pitch("unroll: obs", obs, (N, D))
        outs = (("q_out", q_out, (N, A)), ("actions_out", actions_out, (N,)))
        for (name, t, inner), dtype in zip(outs, (torch.float32, torch.int32)):
            if t is not None:
                _args.check_tensor("unroll: " + name, t, (dtype,), (B, rows) + inner, dev, contiguous=False, errors=_args.VALUE)
        out_pitch = _args.shared_pitch("unroll: ", outs, rows)
        for name, t in (("hidden", hidden), ("hidden_out", hidden_out)):
            if t is not None:
                _args.check_tensor("unroll: " + name, t, (torch.float32,), (B, N, H), dev, errors=_args.VALUE)
        if dev.type != "cuda":
            raise ValueError(f"unroll: the actor lives on {dev}; the launch runs on a HIP device and has no host path")
        lib = _lib.load()
        if q_out is None:
            q_out = torch.empty(B, out_pitch, N, A, device=dev)[:, :rows]
        if actions_out is None:
            actions_out = torch.empty(B, out_pitch, N, dtype=torch.int32, device=dev)[:, :rows]
        stream, hip_stream = _args.launch_stream(stream, dev)
        ws = self.weights_for(stream)
        io = _lib.RgActorUnrollIO(obs.data_ptr(), q_out.data_ptr(), actions_out.data_ptr(),
                                  hidden.data_ptr() if hidden is not None else None,
                                  hidden_out.data_ptr() if hidden_out is not None else None,
                                  B, N, D, rows, obs_pitch, out_pitch, 1 if append_agent_id else 0, 0)
        with torch.cuda.device(dev):
            rc = lib.rg_actor_unroll(C.byref(ws), C.byref(io), hip_stream)
        if rc != 0:
            raise _args.launch_error(rc, lib.rg_actor_unroll_last_error().decode())
        return q_out, actions_out


def one_launch_refusals(env, actor=None, append_agent_id=True):
    """ValueError for what rg_policy_rollout refuses, said before anything is launched: first the env's part (read from its
    attributes alone), then the actor's.  actor=None: the env's part only, for a caller that has not looked at its actor yet."""
    if int(env.params.qp_mode) != 0:
        raise ValueError("one launch: the interior-point mode (barrier_solver: cvxopt) is not supported")
    for b in sorted(SIDE_BLOCKS, key=lambda b: b.attr != "teams"):   # (the pool is asked first, the others in the table's order)
        if getattr(env, b.attr, None) is not None:
            raise ValueError(f"one launch: an env with {b.one_launch} is not supported; use the two-launch path")
    if actor is None:
        return
    if not (actor.use_rnn and actor.pack_gru == "f16x2"):
        raise ValueError("one launch: the actor must be a GRU packed as two binary16 planes (pack_gru=True / 'f16x2')")
    if actor.hidden_dim not in (64, 128):
        raise ValueError("one launch: hidden size must be 64 or 128")
    in_dim = env.D + (env.N if append_agent_id else 0)
    if in_dim != actor.input_dim:
        raise ValueError(f"one launch: the actor expects {actor.input_dim} inputs per agent, the env provides {in_dim}")


def policy_rollout(env, actor, T, io, hidden, actions, restart=None, append_agent_id=True, restart_on_done=False, explore_u=None,
                   epsilon=0.0, obs=None, reward_sum=None, ended=None, dist_sum=None, sample_u=None, prob=None):
    """rg_policy_rollout: T time steps of actor -> action -> env step in ONE launch on the env's handle (csrc/policy_rollout.h).
    env: a VecRobotariumEnv; io: the rg_step_io it steps with (it must carry the gymma block); the tensors are device tensors in
    the layouts of include/robogym.h rg_policy_io (None = NULL).  sample_u [T, E, N] f32 uniforms: soft-policies actions
    (rg_policy_rollout_sample), prob [T, E, N] f32 or None the probability each had; not together with explore_u.
    Raises ValueError for a configuration the launch refuses."""
    lib = _lib.load()
    one_launch_refusals(env, actor, append_agent_id)
    ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    if explore_u is not None:
        _args.check_tensor("explore_u", explore_u, (torch.float32,), None, errors=_args.VALUE)
    if sample_u is not None and explore_u is not None:
        raise ValueError("sample_u (soft policies) and explore_u (epsilon-greedy) do not combine")
    if prob is not None and sample_u is None:
        raise ValueError("prob needs sample_u")
    for name, t in (("sample_u", sample_u), ("prob", prob)):
        if t is not None:
            _args.check_tensor(name, t, (torch.float32,), (int(T), env.E, env.N), errors=_args.VALUE)
    env._sync_stream()   # the handle launches on torch's current stream
    ws = actor.weights_for(torch.cuda.current_stream(env.device))
    pio = _lib.RgPolicyIO(ptr(hidden), ptr(restart), 1 if append_agent_id else 0, 1 if restart_on_done else 0, ptr(explore_u),
                          float(epsilon), ptr(actions), ptr(obs), ptr(reward_sum), ptr(ended), ptr(dist_sum))
    if sample_u is not None:
        ps = _lib.RgPolicySample(ptr(sample_u), ptr(prob))
        rc = lib.rg_policy_rollout_sample(env._h, C.byref(ws), int(T), C.byref(pio), C.byref(ps), C.byref(io),
                                          1 if env.auto_reset else 0, env.seed)
    else:
        rc = lib.rg_policy_rollout(env._h, C.byref(ws), int(T), C.byref(pio), C.byref(io), 1 if env.auto_reset else 0, env.seed)
    if rc != 0:
        msg = f"rg_policy_rollout ({rc}): {lib.rg_last_error().decode()}"
        raise (_lib.RobogymError if rc <= -30 and rc > -40 or rc == -100 else ValueError)(msg)


def explore_select(greedy, u, epsilon, n_actions, out=None):
    """The epsilon-greedy rule of rg_actor_forward_explore in torch ops (the composed runner path and the tests use it): with
    k = int(u * (n_actions / epsilon)) in float32, the action is k where k < n_actions (u < epsilon; k uniform), else greedy."""
    import numpy as np
    scale = float(np.float32(n_actions) / np.float32(epsilon))
    k = (u * torch.tensor(scale, dtype=torch.float32, device=u.device)).to(torch.int32)
    return torch.where(k < n_actions, k, greedy, out=out)


# soft_exp's constants (csrc/actor_common.h states them once; tests/soft_twin.py is the numpy twin)
_SOFT_LOG2E, _SOFT_LN2_HI, _SOFT_LN2_LO, _SOFT_CUT = 1.4426950408889634, 0.693359375, -2.12194440e-4, -87.336
_SOFT_POLY = (1.9875691500e-4, 1.3981999507e-3, 8.3334519073e-3, 4.1665795894e-2, 1.6666665459e-1, 5.0000001201e-1)


def soft_exp(x):
    """exp(x) for float32 x <= 0 as the explicit float32 operation sequence of csrc/actor_common.h `soft_exp` (no library or
    hardware exponential: each torch op below is one correctly rounded IEEE operation); 0 below the underflow cut."""
    f = lambda v: torch.tensor(v, dtype=torch.float32, device=x.device)  # noqa: E731
    k = torch.round(x * f(_SOFT_LOG2E))                       # round to nearest even
    r = (x - k * f(_SOFT_LN2_HI)) - k * f(_SOFT_LN2_LO)
    p = f(_SOFT_POLY[0])
    for c in _SOFT_POLY[1:]:
        p = p * r + f(c)
    y = ((p * (r * r)) + r) + f(1.0)
    live = x >= f(_SOFT_CUT)
    ki = torch.where(live, k, f(0.0)).to(torch.int32)
    scaled = (y.view(torch.int32) + (ki << 23)).view(torch.float32)   # 2^k through the exponent field
    return torch.where(live, scaled, f(0.0))


def soft_select(q, u, out_actions=None, out_prob=None):
    """The soft-policies rule of rg_actor_forward_sample in torch elementwise ops (the composed runner path and the tests use it;
    CPU or GPU tensors): q [..., A] float32 logits, u [...] float32 uniforms in [0, 1).  With m the row maximum,
    e_c = soft_exp(q_c - m), the partial sums c_k of ((e_0 + e_1) + e_2) + ... and Z the last of them, the action is the first k
    with u * Z < c_k (none: the last k with e_k > 0) and prob = e_action / Z.  A row whose maximum is not finite takes
    torch.argmax's action and prob = NaN.  Returns (actions int32 [...], prob float32 [...])."""
    A = q.shape[-1]
    m = q.max(dim=-1).values                                  # (a NaN anywhere gives NaN)
    ok = torch.isfinite(m)
    e = soft_exp(q - m.unsqueeze(-1))
    run = torch.zeros_like(m)
    cs = []
    for k in range(A):                                        # the ordered sum (0 + e_0 is e_0)
        run = run + e[..., k]
        cs.append(run)
    t = u * run
    act = torch.full(m.shape, -1, dtype=torch.int32, device=q.device)
    e_act = torch.zeros_like(m)
    last = torch.zeros_like(act)
    e_last = torch.zeros_like(m)
    for k in range(A):
        hit = (t < cs[k]) & (act < 0)
        act = torch.where(hit, k, act)
        e_act = torch.where(hit, e[..., k], e_act)
        pos = e[..., k] > 0
        last = torch.where(pos, k, last)
        e_last = torch.where(pos, e[..., k], e_last)
    none = act < 0
    act = torch.where(none, last, act)
    e_act = torch.where(none, e_last, e_act)
    act = torch.where(ok, act, q.argmax(dim=-1).to(torch.int32))
    prob = torch.where(ok, e_act / run, torch.tensor(float("nan"), dtype=torch.float32, device=q.device))
    if out_actions is not None:
        out_actions.copy_(act)
        act = out_actions
    if out_prob is not None:
        out_prob.copy_(prob)
        prob = out_prob
    return act, prob


def load_actor(model_file, model_config, n_agents, device="cuda:0"):
    """model_file: a `.th` state dict of the reference's model zoo; model_config: its sacred `.json`
    (path or dict).  Returns (BatchedActor, config dict) -- misc.py:65-91 without the env part."""
    cfg = model_config if isinstance(model_config, dict) else json.load(open(model_config))
    sd = torch.load(model_file, map_location="cpu")
    return BatchedActor(sd, n_agents, use_rnn=cfg.get("use_rnn", True), device=device), cfg


@torch.no_grad()
def run_eval(env, actor, steps, obs_agent_id=True, use_graph=False, fused=None, one_launch=False):
    """Greedy rollout of `actor` on a VecRobotariumEnv (auto_reset on) for `steps` env steps.
    Mirrors run_env's per-step body (misc.py:160-172): optional one-hot agent id appended to the
    observation, actor forward, arg-max, env.step; hidden states restart at zero with each episode.
    Returns the statistics run_env prints, from the env's on-device accumulators.

    use_graph: record one iteration (a dozen small GEMM / elementwise launches plus the env step)
    into a hipGraph on a side stream and replay it `steps` times -- the loop is launch-bound, the
    replay is one launch per step.  Same arithmetic, same results.
    fused (default: when the actor's shape allows): the whole policy step in one launch of the MFMA
    kernel (csrc/actor_mfma.hip) -- an iteration is then three launches (actor, env step, distance
    sum); float32 like the torch path, sums in a different order (action values agree to 1e-5).
    one_launch: the fused loop with the actor and the env step inside ONE launch per (up to) 64 steps (rg_policy_rollout):
    the same statistics as fused=True bit for bit, and the env left in the same state.  Needs an actor packed as two binary16
    planes and the exact barrier QP; anything else raises ValueError."""
    if one_launch:
        one_launch_refusals(env, actor, obs_agent_id)
    E, N = env.E, env.N
    dev = env.device
    eye = torch.eye(N, device=dev).unsqueeze(0).expand(E, N, N)
    in_dim = env.D + (N if obs_agent_id else 0)
    if in_dim != actor.input_dim:
        raise ValueError(f"actor expects {actor.input_dim} inputs per agent, the env provides {in_dim}")
    # loop-carried state lives in fixed buffers, updated in place (what a graph replay needs)
    obs_in = env.reset().clone()
    hidden = actor.init_hidden(E)
    dist = torch.zeros(E, N, device=dev)
    actions = torch.zeros(E, N, dtype=torch.int32, device=dev)

    def body():
        inp = torch.cat([obs_in, eye], dim=2) if obs_agent_id else obs_in
        q, h = actor.forward(inp, hidden)
        actions.copy_(q.argmax(dim=2))
        obs, reward, done, info = env.step(actions)
        dist.add_(info["dist_travelled"])
        keep = (~done)[:, None, None]
        hidden.copy_(torch.where(keep, h, 0.0))
        obs_in.copy_(torch.where(keep, obs, 0.0))   # a finished env restarts from the reference's reset() observation (zeros)

    if one_launch:
        if use_graph:
            raise ValueError("one_launch and use_graph are two different ways to cut launches: pick one")
        if env.elapsed is None:   # the launch always runs the gymma block: give it a TimeLimit that never fires
            io = _lib.RgStepIO.from_buffer_copy(env._io)
            scratch = [torch.zeros(E, dtype=torch.int32, device=dev), torch.zeros(E, dtype=torch.uint8, device=dev),
                       torch.zeros(E, dtype=torch.uint8, device=dev), torch.zeros(E, device=dev)]
            io.elapsed, io.truncated, io.ended, io.reward_sum = (t.data_ptr() for t in scratch)
            io.time_limit = 2 ** 31 - 1
        else:
            io = env._io
        chunk = min(int(steps), 64)
        act = torch.empty(chunk, E, N, dtype=torch.int32, device=dev)
        done = 0
        while done < steps:
            k = min(chunk, steps - done)
            # like the fused loop: the actor reads env.obs and restarts after env.done_u8, the step rewrites both
            policy_rollout(env, actor, k, io, hidden, act, restart=env.done_u8, append_agent_id=obs_agent_id, restart_on_done=True,
                           dist_sum=dist)
            done += k
        torch.cuda.synchronize(dev)
        return _eval_stats(env, dist, steps)
    if fused is None:
        fused = actor.fused_supported()
    if fused:
        q_buf = torch.empty(E, N, actor.n_actions, device=dev)

        def body():  # noqa: F811 - the fused form of the loop body above
            # env.obs / env.done_u8 are the previous step's outputs (zeros after reset()): a finished env is
            # seen through a zero observation and a zero hidden state, inside the kernel
            actor.forward_fused(env.obs, hidden, append_agent_id=obs_agent_id, restart=env.done_u8, q_out=q_buf,
                                actions_out=actions)
            env.step(actions)
            dist.add_(env.dist_travelled)

    if not use_graph:
        for _ in range(steps):
            body()
    else:
        side = torch.cuda.Stream(device=dev)
        prev = env._stream
        side.wait_stream(torch.cuda.current_stream(dev))
        try:
            env.set_stream(side)
            with torch.cuda.stream(side):
                n_warm = min(steps, 3)   # library handles and workspaces exist before the capture
                for _ in range(n_warm):
                    body()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, stream=side):
                    body()
                for _ in range(steps - n_warm):
                    graph.replay()
            torch.cuda.current_stream(dev).wait_stream(side)
        finally:
            env.set_stream(prev)
        torch.cuda.synchronize(dev)
    return _eval_stats(env, dist, steps)


def _eval_stats(env, dist, steps):
    """run_eval's return value (the statistics the reference's run_env prints, misc.py:134-221): from the env's on-device
    accumulators and the per-agent distance sums `dist` of `steps` steps."""
    ret_sum, episodes, ep_steps = env.episode_stats()
    n = max(int(episodes), 1)
    return {"episodes": int(episodes), "mean_return": float(ret_sum) / n, "mean_steps": float(ep_steps) / n,
            "mean_dist_per_step": float(dist.sum()) / (steps * env.E * env.N)}


def main(argv=None):
    """`python -m marbler_amd.evaluate --scenario PredatorCapturePrey --model-file qmix.th --model-config qmix.json`
    -- the batched counterpart of `python -m robotarium_gym.main --scenario X` (main.py / misc.py:93-221):
    loads a model of the reference's zoo, rolls it out greedily on --envs envs for --steps steps, prints
    the statistics run_env prints (mean return, mean episode length) as one JSON line."""
    import argparse
    from .params import load_config
    from .vec_env import VecRobotariumEnv
    ap = argparse.ArgumentParser(prog="python -m marbler_amd.evaluate")
    ap.add_argument("--scenario", required=True)
    ap.add_argument("--model-file", required=True, help="a .th state dict of the model zoo")
    ap.add_argument("--model-config", required=True, help="its sacred .json config")
    ap.add_argument("--config", default=None, help="scenario YAML (default: this package's copy of the reference's)")
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--torch-actor", action="store_true", help="evaluate the policy with torch ops instead of the fused kernel")
    args = ap.parse_args(argv)
    cfg = load_config(args.scenario, config_path=args.config)
    env = VecRobotariumEnv(args.scenario, args.envs, overrides=cfg, device=args.device, seed=args.seed)
    actor, mcfg = load_actor(args.model_file, args.model_config, env.N, device=args.device)
    out = run_eval(env, actor, args.steps, obs_agent_id=bool(mcfg.get("obs_agent_id", True)),
                   fused=False if args.torch_actor else None)
    out.update({"scenario": args.scenario, "envs": args.envs, "steps": args.steps})
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
