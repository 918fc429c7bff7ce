"""The rule of rg_td_targets (csrc/td_targets.h) in NumPy, and EPyMARL's own lines in torch.

twin(): the rule as stated -- float32 in the stated order for `none` / `vdn` (every bit is fixed), float64 for qmix (the kernel's
float32 arithmetic has a summation order of its own; the float64 result is what both it and torch's float32 are measured against).
Rows the rule says are not read are not read here either: they may hold NaN.

restatement(): a torch float32 restatement of q_learner.train's target lines and of QMixer.forward, written from EPyMARL's
definition (mask[:, 1:] *= 1 - terminated[:, :-1]; the double-Q gather of target_mac_out[:, 1:]; target_mixer(., state[:, 1:]);
rewards + gamma (1 - terminated) target_max_qvals).  It computes every row, padding included, so what it gives on a row that holds
NaN is NaN: it is compared on the unmasked rows only.  The yardstick for the qmix tolerance.
"""
import numpy as np

EMBED, HYPER = 32, 64


def row_flags(terminated, filled, rows):
    """-> (mask, live) [B, T] bool: mask as the rule states it; live = unmasked and not terminal (row t + 1 is read)."""
    term, fill = np.asarray(terminated).astype(bool)[:, :rows], np.asarray(filled).astype(bool)[:, :rows]
    mask = fill[:, :-1].copy()
    mask[:, 1:] &= ~term[:, :-2]
    return mask, mask & ~term[:, :-1]


def agent_values(qt, sel, live):
    """agent_q [B, T, N] float32 of the live rows (zero elsewhere): the gather by sel (out of range: NaN) or the first maximum
    with a NaN counting as the largest value."""
    q = np.asarray(qt, np.float32)[:, 1:]
    A = q.shape[-1]
    with np.errstate(invalid="ignore"):
        if sel is not None:
            a = np.asarray(sel)[:, 1:q.shape[1] + 1].astype(np.int64)
            ok = (a >= 0) & (a < A)
            v = np.take_along_axis(q, np.clip(a, 0, A - 1)[..., None], axis=-1)[..., 0]
            v = np.where(ok, v, np.float32("nan"))
        else:
            v = q[..., 0].copy()
            for c in range(1, A):
                x = q[..., c]
                v = np.where((x > v) | (np.isnan(x) & ~np.isnan(v)), x, v)
    return np.where(live[..., None], v, np.float32(0.0)).astype(np.float32)


def qmix64(params, agent_q, state):
    """QMixer.forward in float64: agent_q [R, N], state [R, S] -> y [R]."""
    p = {k: np.asarray(v, np.float64) for k, v in params.items()}
    lin = lambda x, k: x @ p[k + ".weight"].T + p[k + ".bias"]  # noqa: E731
    relu = lambda x: np.maximum(x, 0.0)  # noqa: E731
    R, N = agent_q.shape
    w1 = np.abs(lin(relu(lin(state, "hyper_w_1.0")), "hyper_w_1.2")).reshape(R, N, EMBED)
    b1 = lin(state, "hyper_b_1")
    x = np.einsum("rn,rne->re", agent_q, w1) + b1
    hidden = np.where(x > 0, x, np.expm1(np.minimum(x, 0.0)))
    wf = np.abs(lin(relu(lin(state, "hyper_w_final.0")), "hyper_w_final.2"))
    v = lin(relu(lin(state, "V.0")), "V.2")[:, 0]
    return (hidden * wf).sum(-1) + v


def twin(kind, qt, sel, obs, reward, terminated, filled, gamma, params=None):
    """-> (targets, mask, agent_q): [B, T] ([B, T, N] for `none`), [B, T] float32, [B, T, N] float32.  targets is float32 for
    none / vdn and float64 for qmix."""
    rows = np.asarray(qt).shape[1]
    T = rows - 1
    mask, live = row_flags(terminated, filled, rows)
    aq = agent_values(qt, sel, live)
    N = aq.shape[-1]
    r = np.asarray(reward, np.float32)[:, :T]
    g = np.float32(gamma)
    with np.errstate(invalid="ignore", over="ignore"):
        if kind == "qmix":
            S = N * np.asarray(obs).shape[-1]
            state = np.asarray(obs, np.float64)[:, 1:rows].reshape(-1, S)
            state = np.where(live.reshape(-1, 1), state, 0.0)
            y = qmix64(params, aq.astype(np.float64).reshape(-1, N), state).reshape(live.shape)
            t = np.where(live, r.astype(np.float64) + np.float64(g) * y, np.where(mask, r.astype(np.float64), 0.0))
        elif kind == "vdn":
            y = aq[..., 0].copy()
            for n in range(1, N):
                y = (y + aq[..., n]).astype(np.float32)
            t = np.where(live, (r + (g * y).astype(np.float32)).astype(np.float32), np.where(mask, r, np.float32(0.0))).astype(np.float32)
        else:
            full = (r[..., None] + (g * aq).astype(np.float32)).astype(np.float32)
            t = np.where(live[..., None], full, np.where(mask, r, np.float32(0.0))[..., None]).astype(np.float32)
    return t, mask.astype(np.float32), aq


def qmixer_torch(params, agent_qs, states):
    """EPyMARL's QMixer.forward (hypernet_layers: 2), from its definition: agent_qs [B, T, N], states [B, T, S] -> [B, T, 1]."""
    import torch
    import torch.nn.functional as F
    bs, N = agent_qs.size(0), agent_qs.size(-1)
    states = states.reshape(-1, states.size(-1))
    agent_qs = agent_qs.reshape(-1, 1, N)
    w1 = torch.abs(F.linear(F.relu(F.linear(states, params["hyper_w_1.0.weight"], params["hyper_w_1.0.bias"])),
                            params["hyper_w_1.2.weight"], params["hyper_w_1.2.bias"]))
    b1 = F.linear(states, params["hyper_b_1.weight"], params["hyper_b_1.bias"])
    w1, b1 = w1.view(-1, N, EMBED), b1.view(-1, 1, EMBED)
    hidden = F.elu(torch.bmm(agent_qs, w1) + b1)
    w_final = torch.abs(F.linear(F.relu(F.linear(states, params["hyper_w_final.0.weight"], params["hyper_w_final.0.bias"])),
                                 params["hyper_w_final.2.weight"], params["hyper_w_final.2.bias"])).view(-1, EMBED, 1)
    v = F.linear(F.relu(F.linear(states, params["V.0.weight"], params["V.0.bias"])), params["V.2.weight"], params["V.2.bias"]).view(-1, 1, 1)
    return (torch.bmm(hidden, w_final) + v).view(bs, -1, 1)


def restatement(kind, qt, sel, obs, reward, terminated, filled, gamma, params=None):
    """q_learner.train's target lines on torch tensors of any device/dtype: -> (targets [B, T, 1] or [B, T, N], mask [B, T, 1]).
    sel is clamped into [0, A): rows the rule does not read may hold anything, and torch.gather checks its index."""
    B, rows, N, A = qt.shape
    rewards = reward[:, :-1].unsqueeze(-1)
    term = terminated[:, :-1].to(qt.dtype).unsqueeze(-1)
    mask = filled[:, :-1].to(qt.dtype).unsqueeze(-1).clone()
    mask[:, 1:] = mask[:, 1:] * (1 - term[:, :-1])
    target_mac_out = qt[:, 1:]
    if sel is not None:
        cur_max_actions = sel[:, 1:].long().clamp(0, A - 1).unsqueeze(-1)
        target_max_qvals = target_mac_out.gather(3, cur_max_actions).squeeze(3)
    else:
        target_max_qvals = target_mac_out.max(dim=3)[0]
    if kind == "qmix":
        target_max_qvals = qmixer_torch(params, target_max_qvals, obs[:, 1:].reshape(B, rows - 1, -1))
    elif kind == "vdn":
        target_max_qvals = target_max_qvals.sum(dim=2, keepdim=True)
    return rewards + gamma * (1 - term) * target_max_qvals, mask


def rel_err(x, ref64, where):
    """max |x - ref| / (1 + |ref|) over the rows `where` (0.0 when there is none)."""
    x, ref64 = np.asarray(x, np.float64)[where], np.asarray(ref64, np.float64)[where]
    return float(np.max(np.abs(x - ref64) / (1.0 + np.abs(ref64)))) if x.size else 0.0
