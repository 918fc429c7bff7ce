"""A trainable actor: EPyMARL's recurrent agent over whole episode batches WITH gradients, the recurrence in two HIP launches
(rg_gru_scan_forward / rg_gru_scan_backward, include/robogym_learn.h) and everything that is batched over all rows in torch's GEMMs.

    actor = TrainableActor.from_actor(batched_actor)                 # or TrainableActor(n_agents, input_dim, 128, n_actions)
    q = actor(batch["obs"])                                           # [B, rows, N, A], with a graph
    loss.backward(); optimizer.step()
    batched_actor.load_state_dict(actor.state_dict())                 # collect with the new weights

The rule of the two launches -- torch.nn.GRUCell's recurrence and its hand-written backward pass -- is stated once in
csrc/gru_scan.h and DESIGN.md section 4 "Trainable actor".  There is no host path: the launches need the library and a HIP device;
TrainableActor.forward_reference() is the plain per-step torch loop, on any device and in any floating-point dtype.
"""
import ctypes as C

import torch

from . import _args, _lib

HIDDEN = (64, 128)                      # the kernels' two instantiations
_F32 = (torch.float32,)


def _weights(who, w_hh, b_hh, dev):
    """w_hh [3H, H] or [A, 3H, H], b_hh [3H] or [A, 3H] (None: not needed) -> (w_hh [A, 3H, H], b_hh [A, 3H] or None, A, H)."""
    _args.check_tensor(who + "w_hh", w_hh, _F32, None, dev, errors=_args.VALUE)
    if w_hh.dim() == 2:
        w_hh = w_hh.unsqueeze(0)
    if w_hh.dim() != 3 or w_hh.shape[1] != 3 * w_hh.shape[2] or w_hh.shape[0] < 1:
        raise ValueError(f"{who}w_hh must be [3H, H] or [A, 3H, H], got {tuple(w_hh.shape)}")
    A, _, H = w_hh.shape
    if H not in HIDDEN:
        raise ValueError(f"{who}the hidden size must be one of {HIDDEN}, w_hh has {H}")
    if b_hh is not None:
        _args.check_tensor(who + "b_hh", b_hh, _F32, None, dev, errors=_args.VALUE)
        if b_hh.dim() == 1:
            b_hh = b_hh.unsqueeze(0)
        if tuple(b_hh.shape) != (A, 3 * H):
            raise ValueError(f"{who}b_hh must be {(A, 3 * H)} (or [3H] with one weight set), got {tuple(b_hh.shape)}")
    return w_hh, b_hh, A, H


def _sets(who, A, N):
    if N > _lib.MAX_AGENTS:
        raise ValueError(f"{who}at most {_lib.MAX_AGENTS} agents, got {N}")
    if A not in (1, N):
        raise ValueError(f"{who}w_hh holds {A} weight sets: must be 1 or the number of agents, {N}")


def _rows(who, name, t, dev, inner=None):
    """t: [B, rows, N, *] float32 on dev -> its shape."""
    _args.check_tensor(who + name, t, _F32, None, dev, contiguous=False, errors=_args.VALUE)
    if t.dim() != 4 or min(t.shape) < 1:
        raise ValueError(f"{who}{name} must be [B, rows, N, {'*' if inner is None else inner}] with every dimension >= 1, got {tuple(t.shape)}")
    if t.shape[1] > _lib.GRU_SCAN_MAX_ROWS:
        raise ValueError(f"{who}rows must be <= {_lib.GRU_SCAN_MAX_ROWS}, {name} has {t.shape[1]}")
    return tuple(t.shape)


def _device(who, name, t):
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{who}{name} must be a tensor, got {type(t).__name__}")
    return t.device


def _needs_hip(who, dev):
    """Every other check comes first: what is wrong with a call is said wherever its tensors live."""
    if dev.type != "cuda":
        raise ValueError(f"{who}the tensors live on {dev}; the launch runs on a HIP device and has no host path")


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _launch(entry, who, w, io, dev, stream):
    lib = _lib.load_learn()
    stream, hip_stream = _args.launch_stream(stream, dev)
    with torch.cuda.device(dev):
        rc = getattr(lib, entry)(C.byref(w), C.byref(io), hip_stream)
    if rc != 0:
        raise _args.launch_error(rc, lib.rg_gru_scan_last_error().decode())


def gru_scan_forward(gi, w_hh, b_hh, hidden=None, h_out=None, gates_out=None, hidden_out=None, stream=None):
    """torch.nn.GRUCell's recurrence over every row of an episode batch in ONE launch (rg_gru_scan_forward; the rule:
    csrc/gru_scan.h).  gi [B, rows, N, 3H] f32, the input half of the gates (x W_ih^T + b_ih, torch's order r, z, n), its last two
    dimensions contiguous; w_hh [3H, H] / b_hh [3H] (shared) or [N, 3H, H] / [N, 3H] (one set per agent), H in {64, 128}; hidden
    [B, N, H] or None (zeros).  Returns (h [B, rows, N, H], gates [B, rows, N, 4H] = (r, z, n, gh_n) for the backward launch).
    h_out / gates_out: outputs to reuse (the same number of rows per episode in both; gates_out=False: no gates are written and
    None is returned for them); hidden_out [B, N, H] or None receives the last state.  Nothing is allocated when h_out and
    gates_out are given, so the call can be captured.  ValueError for a wrong dtype, shape, stride or device."""
    who = "gru_scan_forward: "
    dev = _device(who, "gi", gi)
    w_hh, b_hh, A, H = _weights(who, w_hh, b_hh, dev)
    if b_hh is None:
        raise ValueError(who + "b_hh is needed")
    B, rows, N, G = _rows(who, "gi", gi, dev)
    if G != 3 * H:
        raise ValueError(f"{who}gi must be [B, rows, N, {3 * H}], got {tuple(gi.shape)}")
    _sets(who, A, N)
    gi_pitch = _args.episode_pitch(who + "gi", gi, (N, 3 * H))
    want_gates = gates_out is not False
    outs = [("h_out", h_out, (N, H))] + ([("gates_out", gates_out, (N, 4 * H))] if want_gates else [])
    for name, t, inner in outs:
        if t is not None:
            _args.check_tensor(who + name, t, _F32, (B, rows) + inner, dev, contiguous=False, errors=_args.VALUE)
    save_pitch = _args.shared_pitch(who, outs, rows)
    for name, t in (("hidden", hidden), ("hidden_out", hidden_out)):
        if t is not None:
            _args.check_tensor(who + name, t, _F32, (B, N, H), dev, errors=_args.VALUE)
    _needs_hip(who, dev)
    if h_out is None:
        h_out = torch.empty(B, save_pitch, N, H, device=dev)[:, :rows]
    if want_gates and gates_out is None:
        gates_out = torch.empty(B, save_pitch, N, 4 * H, device=dev)[:, :rows]
    w = _lib.RgGruScanWeights(w_hh.data_ptr(), b_hh.data_ptr(), None, A, H)
    io = _lib.RgGruScanIO(gi.data_ptr(), _ptr(hidden), h_out.data_ptr(), _ptr(gates_out) if want_gates else None, _ptr(hidden_out),
                          None, None, None, None, None, B, N, rows, gi_pitch, save_pitch, rows)
    _launch("rg_gru_scan_forward", who, w, io, dev, stream)
    return h_out, (gates_out if want_gates else None)


def gru_scan_backward(h, gates, w_hh, dh_ext, hidden=None, d_hidden_out=None, dgi_out=None, dghn_out=None, d_hidden_in_out=None,
                      stream=None):
    """The backward pass of gru_scan_forward in ONE launch (rg_gru_scan_backward; the rule: csrc/gru_scan.h).  h [B, rows, N, H] and
    gates [B, rows, N, 4H] as the forward launch wrote them (the same number of rows per episode in both), w_hh and hidden as it
    was given them; dh_ext [B, rows, N, H]: the gradient that reaches every h_t from outside the recurrence; d_hidden_out [B, N, H]
    or None: the gradient of the last state.  Returns (dgi [B, rows, N, 3H], dghn [B, rows, N, H], d_hidden_in [B, N, H]): the
    gradient of gi, the n third of the gradient of gh = h_{t-1} W_hh^T + b_hh (its r and z thirds are dgi's), and the gradient of
    hidden.  dgi_out / dghn_out (laid out like dh_ext: the same number of rows per episode in all three) / d_hidden_in_out: outputs
    to reuse; nothing is allocated when all three are given.  ValueError for a wrong dtype, shape, stride or device."""
    who = "gru_scan_backward: "
    dev = _device(who, "h", h)
    w_hh, _, A, H = _weights(who, w_hh, None, dev)
    B, rows, N, Hh = _rows(who, "h", h, dev)
    if Hh != H:
        raise ValueError(f"{who}h must be [B, rows, N, {H}], got {tuple(h.shape)}")
    _sets(who, A, N)
    _args.check_tensor(who + "gates", gates, _F32, (B, rows, N, 4 * H), dev, contiguous=False, errors=_args.VALUE)
    save_pitch = _args.shared_pitch(who, [("h", h, (N, H)), ("gates", gates, (N, 4 * H))], rows)
    grads = [("dh_ext", dh_ext, (N, H)), ("dgi_out", dgi_out, (N, 3 * H)), ("dghn_out", dghn_out, (N, H))]
    for name, t, inner in grads:
        if t is not None or name == "dh_ext":
            _args.check_tensor(who + name, t, _F32, (B, rows) + inner, dev, contiguous=False, errors=_args.VALUE)
    grad_pitch = _args.shared_pitch(who, grads, rows)
    for name, t in (("hidden", hidden), ("d_hidden_out", d_hidden_out), ("d_hidden_in_out", d_hidden_in_out)):
        if t is not None:
            _args.check_tensor(who + name, t, _F32, (B, N, H), dev, errors=_args.VALUE)
    _needs_hip(who, dev)
    if dgi_out is None:
        dgi_out = torch.empty(B, grad_pitch, N, 3 * H, device=dev)[:, :rows]
    if dghn_out is None:
        dghn_out = torch.empty(B, grad_pitch, N, H, device=dev)[:, :rows]
    if d_hidden_in_out is None:
        d_hidden_in_out = torch.empty(B, N, H, device=dev)
    w = _lib.RgGruScanWeights(w_hh.data_ptr(), None, None, A, H)
    io = _lib.RgGruScanIO(None, _ptr(hidden), h.data_ptr(), gates.data_ptr(), None, dh_ext.data_ptr(), _ptr(d_hidden_out),
                          dgi_out.data_ptr(), dghn_out.data_ptr(), d_hidden_in_out.data_ptr(), B, N, rows, rows, save_pitch, grad_pitch)
    _launch("rg_gru_scan_backward", who, w, io, dev, stream)
    return dgi_out, dghn_out, d_hidden_in_out


class GruScan(torch.autograd.Function):
    """GruScan.apply(gi, w_hh, b_hh, hidden) -> h [B, rows, N, H]: gru_scan_forward with a backward pass.  gi [B, rows, N, 3H];
    w_hh [3H, H] / b_hh [3H] or [N, 3H, H] / [N, 3H]; hidden [B, N, H] or None.  The backward pass is one launch for what is
    sequential (gru_scan_backward) and torch's GEMMs for the weight gradients: dW_hh = dgh^T h_prev summed over every row, with
    h[:, :-1] read in place (the rows are shifted through the flat view, the t = 0 term comes from `hidden`), db_hh = sum dgh."""

    @staticmethod
    def forward(ctx, gi, w_hh, b_hh, hidden):
        w_hh_c = w_hh.detach().contiguous()
        gi = gi.detach()
        if gi.dim() == 4 and gi.stride()[1:] != (gi.shape[2] * gi.shape[3], gi.shape[3], 1):   # (einsum hands back a permuted view)
            gi = gi.contiguous()
        h, gates = gru_scan_forward(gi, w_hh_c, b_hh.detach().contiguous(), None if hidden is None else hidden.detach().contiguous())
        ctx.save_for_backward(h, gates, w_hh_c, hidden)
        ctx.shapes = (tuple(w_hh.shape), tuple(b_hh.shape))
        return h

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dh):
        h, gates, w_hh, hidden = ctx.saved_tensors
        B, rows, N, H = h.shape
        if dh.stride()[1:] != (N * H, H, 1):
            dh = dh.contiguous()
        hid = None if hidden is None else hidden.detach().contiguous()
        # the gradient of gh for every row in one array: dgi's r and z thirds, and dghn
        dgi, dghn, d_hidden = gru_scan_backward(h, gates, w_hh, dh, hid)
        dgh = torch.cat([dgi[..., :2 * H], dghn], dim=3)
        per_agent = w_hh.dim() == 3 and w_hh.shape[0] > 1
        d_b = dgh.sum(dim=(0, 1)) if per_agent else dgh.sum(dim=(0, 1, 2))
        # t = 0 pairs with `hidden`; every other row (b, t, n) with row (b, t - 1, n), which lies N rows before it in the flat view
        # -- once the t = 0 rows of dgh are zero, the shifted product over ALL flat rows is the sum over t >= 1
        if per_agent:
            d_w = torch.einsum("bng,bnh->ngh", dgh[:, 0], hid) if hid is not None else torch.zeros_like(w_hh)
            dgh[:, 0].zero_()
            if B * rows > 1:
                g3, h3 = dgh.view(B * rows, N, 3 * H)[1:], h.view(B * rows, N, H)[:-1]
                d_w = d_w + torch.bmm(g3.permute(1, 2, 0), h3.permute(1, 0, 2))
        else:
            d_w = dgh[:, 0].reshape(-1, 3 * H).t() @ hid.view(-1, H) if hid is not None else torch.zeros(3 * H, H, device=h.device)
            dgh[:, 0].zero_()
            if B * rows * N > N:
                d_w = d_w + dgh.view(-1, 3 * H)[N:].t() @ h.view(-1, H)[:-N]
        w_shape, b_shape = ctx.shapes
        return dgi, d_w.view(w_shape), d_b.view(b_shape), (d_hidden if hidden is not None else None)


class _Agent(torch.nn.Module):
    """EPyMARL's RNNAgent: fc1 -> ReLU -> GRUCell -> fc2, under its own parameter names."""

    def __init__(self, input_dim, hidden_dim, n_actions):
        super().__init__()
        self.fc1 = torch.nn.Linear(input_dim, hidden_dim)
        self.rnn = torch.nn.GRUCell(hidden_dim, hidden_dim)
        self.fc2 = torch.nn.Linear(hidden_dim, n_actions)


class TrainableActor(torch.nn.Module):
    """EPyMARL's recurrent actor as a torch module whose forward pass over an episode batch is three batched GEMMs and one GRU scan
    launch, and whose backward pass is the mirror image.  shared=True: RNNAgent, parameters fc1.*, rnn.weight_ih / weight_hh /
    bias_ih / bias_hh, fc2.*; shared=False: RNNNSAgent, one such network per agent under agents.{i}. -- EPyMARL's own names, so a
    checkpoint or a zoo model loads with load_state_dict and any torch optimiser works."""

    def __init__(self, n_agents, input_dim, hidden_dim, n_actions, shared=True, device=None):
        super().__init__()
        for k, v in (("n_agents", n_agents), ("input_dim", input_dim), ("hidden_dim", hidden_dim), ("n_actions", n_actions)):
            if isinstance(v, bool) or not isinstance(v, int) or v < 1:
                raise ValueError(f"{k} must be an int >= 1, got {v!r}")
        if n_agents > _lib.MAX_AGENTS:
            raise ValueError(f"n_agents must be <= {_lib.MAX_AGENTS}, got {n_agents}")
        if hidden_dim not in HIDDEN:
            raise ValueError(f"hidden_dim must be one of {HIDDEN}, got {hidden_dim}")
        self.n_agents, self.input_dim, self.hidden_dim, self.n_actions, self.shared = n_agents, input_dim, hidden_dim, n_actions, bool(shared)
        if self.shared:
            one = _Agent(input_dim, hidden_dim, n_actions)
            self.fc1, self.rnn, self.fc2 = one.fc1, one.rnn, one.fc2
        else:
            self.agents = torch.nn.ModuleList([_Agent(input_dim, hidden_dim, n_actions) for _ in range(n_agents)])
        if device is not None:
            self.to(device)

    @classmethod
    def from_actor(cls, actor, device=None):
        """A TrainableActor with the weights of a BatchedActor (marbler_amd.evaluate), on its device unless told otherwise."""
        if not getattr(actor, "use_rnn", False):
            raise ValueError("TrainableActor: the actor must be a GRU actor (use_rnn=True)")
        self = cls(actor.n_agents, actor.input_dim, actor.hidden_dim, actor.n_actions, shared=not actor.non_shared,
                   device=actor.w1.device if device is None else device)
        names = (("fc1.weight", "w1"), ("fc1.bias", "b1"), ("rnn.weight_ih", "wih"), ("rnn.weight_hh", "whh"), ("rnn.bias_ih", "bih"),
                 ("rnn.bias_hh", "bhh"), ("fc2.weight", "w2"), ("fc2.bias", "b2"))
        sd = {(f"agents.{i}." if actor.non_shared else "") + k: getattr(actor, a)[i] for i in range(actor.w1.shape[0]) for k, a in names}
        self.load_state_dict(sd)
        return self

    def _nets(self):
        return [self] if self.shared else list(self.agents)

    def _stack(self, get):
        """One parameter of every network: [..] with shared weights, [N, ..] otherwise."""
        nets = self._nets()
        return get(nets[0]) if self.shared else torch.stack([get(a) for a in nets])

    def _check(self, who, obs, append_agent_id, hidden):
        p = self._nets()[0].fc1.weight
        N, H = self.n_agents, self.hidden_dim
        _args.check_tensor(who + "obs", obs, (p.dtype,), None, p.device, contiguous=False, errors=_args.VALUE)
        if obs.dim() != 4 or obs.shape[0] < 1 or obs.shape[1] < 1 or obs.shape[2] != N:
            raise ValueError(f"{who}obs must be [B, rows, {N}, D] with B, rows >= 1, got {tuple(obs.shape)}")
        D = obs.shape[3]
        if D + (N if append_agent_id else 0) != self.input_dim:
            raise ValueError(f"{who}the actor expects {self.input_dim} inputs per agent, obs provides {D + (N if append_agent_id else 0)}")
        if hidden is not None:
            _args.check_tensor(who + "hidden", hidden, (p.dtype,), (obs.shape[0], N, H), p.device, contiguous=False, errors=_args.VALUE)
        return D

    def _lin(self, x, w, b):
        # x [..., N, I]; w [O, I] / b [O], or [N, O, I] / [N, O]
        if self.shared:
            return torch.matmul(x, w.t()) + b
        return torch.einsum("...ni,noi->...no", x, w) + b

    def forward(self, obs, append_agent_id=True, hidden=None):
        """obs [B, rows, N, D] f32 on the module's HIP device (its last two dimensions contiguous; buf.batch(slots)["obs"] is read in
        place), hidden [B, N, H] or None (zeros) -> q [B, rows, N, A] with a graph.  fc1, the input half of the GRU and fc2 are
        torch's GEMMs over all B rows N rows at once; the recurrence is GruScan.  The one-hot agent id is never materialised: its
        columns of fc1.weight are added as a per-agent bias.  There is no limit on D or A.  ValueError for a module that is not on
        a HIP device ("no host path"), not float32, or for obs / hidden of a wrong dtype, shape or device."""
        who = "TrainableActor: "
        p = self._nets()[0].fc1.weight
        if p.dtype != torch.float32:
            raise ValueError(f"{who}the module must be float32, it is {p.dtype}")
        D = self._check(who, obs, append_agent_id, hidden)
        if obs.stride(3) != 1 and obs.shape[3] > 1 or obs.stride(2) != obs.shape[3] and obs.shape[2] > 1:
            raise ValueError(f"{who}the last two dimensions of obs must be contiguous (shape {tuple(obs.shape)}, strides {obs.stride()})")
        if p.device.type != "cuda":
            raise ValueError(f"{who}the module lives on {p.device}; the scan runs on a HIP device and has no host path "
                             "(forward_reference is the torch loop)")
        w1, b1 = self._stack(lambda a: a.fc1.weight), self._stack(lambda a: a.fc1.bias)
        if append_agent_id:   # [obs, onehot(n)] W1^T = obs W1[:, :D]^T + W1[:, D + n]
            b1 = b1 + (w1[..., D:].t() if self.shared else torch.diagonal(w1[..., D:], dim1=0, dim2=2).t())
            w1 = w1[..., :D]
        x = torch.relu(self._lin(obs, w1, b1))
        gi = self._lin(x, self._stack(lambda a: a.rnn.weight_ih), self._stack(lambda a: a.rnn.bias_ih))
        h = GruScan.apply(gi, self._stack(lambda a: a.rnn.weight_hh), self._stack(lambda a: a.rnn.bias_hh), hidden)
        return self._lin(h, self._stack(lambda a: a.fc2.weight), self._stack(lambda a: a.fc2.bias))

    def forward_reference(self, obs, append_agent_id=True, hidden=None, return_hidden=False):
        """The same function as the plain per-step torch loop (EPyMARL's mac.forward(batch, t) for every t; BatchedActor.forward's
        composition): the baseline, and with .double() the float64 reference.  Any device."""
        who = "TrainableActor.forward_reference: "
        self._check(who, obs, append_agent_id, hidden)
        B, rows, N, _ = obs.shape
        H = self.hidden_dim
        st = lambda get: self._stack(get)  # noqa: E731
        w1, b1, w2, b2 = st(lambda a: a.fc1.weight), st(lambda a: a.fc1.bias), st(lambda a: a.fc2.weight), st(lambda a: a.fc2.bias)
        wih, bih, whh, bhh = (st(lambda a: a.rnn.weight_ih), st(lambda a: a.rnn.bias_ih), st(lambda a: a.rnn.weight_hh),
                              st(lambda a: a.rnn.bias_hh))
        eye = torch.eye(N, device=obs.device, dtype=obs.dtype).unsqueeze(0).expand(B, N, N)
        h = hidden if hidden is not None else torch.zeros(B, N, H, device=obs.device, dtype=obs.dtype)
        qs = []
        for t in range(rows):
            inp = torch.cat([obs[:, t], eye], dim=2) if append_agent_id else obs[:, t]
            x = torch.relu(self._lin(inp, w1, b1))
            gi, gh = self._lin(x, wih, bih), self._lin(h, whh, bhh)
            r = torch.sigmoid(gi[..., :H] + gh[..., :H])
            z = torch.sigmoid(gi[..., H:2 * H] + gh[..., H:2 * H])
            n = torch.tanh(gi[..., 2 * H:] + r * gh[..., 2 * H:])
            h = (1.0 - z) * n + z * h
            qs.append(self._lin(h, w2, b2))
        q = torch.stack(qs, dim=1)
        return (q, h) if return_hidden else q
