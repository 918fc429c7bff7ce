"""The rule of rg_nstep_returns (csrc/nstep_returns.h) in NumPy, and EPyMARL's own lines in torch.

twin: mask_of() / needed_rows() as the rule states them; values64() the critic in float64 on the needed rows (the kernel's float32
arithmetic has a summation order of its own; the float64 result is what both it and torch's float32 are measured against);
returns32() the n-step pass in float32 in the stated order -- given `values`, every bit is fixed.  Rows the rule says are not read
are not read here either: they may hold NaN.

restatement: a torch restatement of ppo_learner's no_grad lines, written from EPyMARL's definition -- mask[:, 1:] *= 1 -
terminated[:, :-1], repeated over the agents; target_critic(batch) * sqrt(var) + mean; and nstep_returns' double loop over t_start
and step, which adds `gamma ** step * rewards[:, t] * mask[:, t]`, at step == nsteps `gamma ** step * values[:, t] * mask[:, t]`,
and at the last row with add_value_last_step `gamma ** (step + 1) * values[:, t + 1]` WITHOUT a mask.  It computes every row, padding
included, so it wants finite inputs, and is compared on the unmasked rows only.
"""
import numpy as np


def mask_of(terminated, filled, rows):
    """-> m [B, T] bool."""
    term, fill = np.asarray(terminated).astype(bool)[:, :rows], np.asarray(filled).astype(bool)[:, :rows]
    m = fill[:, :-1].copy()
    m[:, 1:] &= ~term[:, :-2]
    return m


def needed_rows(m, add_value_last_step):
    """-> [B, T + 1] bool: row t < T iff m[t]; row T iff add_value_last_step and m[T - 1]."""
    last = m[:, -1:] & bool(add_value_last_step)
    return np.concatenate([m, last], axis=1)


def discounts(gamma, n):
    """g[0 .. n + 1] float32: (float) pow((double) (float) gamma, k)."""
    g = float(np.float32(gamma))
    return np.array([g ** k for k in range(n + 2)], np.float64).astype(np.float32)


def critic64(kind, params, state, N):
    """The critic in float64: state [R, S] -> [R, N].  params: name -> array (cv: fc1.weight ..; cv_ns: critics.{i}.fc1.weight ..)."""
    p = {k: np.asarray(v, np.float64) for k, v in params.items()}
    state = np.asarray(state, np.float64)

    def net(x, pre):
        x = np.maximum(x @ p[pre + "fc1.weight"].T + p[pre + "fc1.bias"], 0.0)
        x = np.maximum(x @ p[pre + "fc2.weight"].T + p[pre + "fc2.bias"], 0.0)
        return (x @ p[pre + "fc3.weight"].T + p[pre + "fc3.bias"])[:, 0]
    if kind == "cv":
        eye = np.eye(N)
        return np.stack([net(np.concatenate([state, np.broadcast_to(eye[a], (state.shape[0], N))], axis=1), "") for a in range(N)], axis=1)
    return np.stack([net(state, f"critics.{a}.") for a in range(N)], axis=1)


def values64(kind, params, obs, terminated, filled, add_value_last_step, value_scale=1.0, value_shift=0.0):
    """-> (values [B, rows, N] float64: scale c + shift on the needed rows, 0 elsewhere; needed [B, rows] bool)."""
    obs = np.asarray(obs)
    B, rows, N, D = obs.shape
    need = needed_rows(mask_of(terminated, filled, rows), add_value_last_step)
    out = np.zeros((B, rows, N), np.float64)
    if need.any():
        c = critic64(kind, params, obs[need].reshape(-1, N * D), N)
        out[need] = float(np.float32(value_scale)) * c + float(np.float32(value_shift))
    return out, need


def returns32(values, reward, m, gamma, n, add_value_last_step):
    """The n-step pass of the rule, float32, products rounded before sums: values [B, T + 1, N] float32, reward [B, >= T], m [B, T]
    bool -> returns [B, T, N] float32.  Reads values and rewards only where the rule does (what it does not read may be NaN)."""
    values, reward = np.asarray(values, np.float32), np.asarray(reward, np.float32)
    B, T = m.shape
    N = values.shape[2]
    g = discounts(gamma, n)
    last = m[:, T - 1] & bool(add_value_last_step)
    out = np.zeros((B, T, N), np.float32)
    f32 = np.float32
    with np.errstate(invalid="ignore", over="ignore"):
        for t0 in range(T):
            ret = np.zeros((B, N), np.float32)
            for k in range(n + 1):
                t = t0 + k
                if t >= T:
                    break
                on = (m[:, t0] & m[:, t])[:, None]
                if k == n:
                    ret = np.where(on, (ret + (g[k] * values[:, t]).astype(f32)).astype(f32), ret)
                else:
                    ret = np.where(on, (ret + (g[k] * reward[:, t, None]).astype(f32)).astype(f32), ret)
                    if t == T - 1:
                        ret = np.where((m[:, t0] & last)[:, None], (ret + (g[k + 1] * values[:, T]).astype(f32)).astype(f32), ret)
            out[:, t0] = ret
    return out


def epymarl_nstep_returns(rewards, mask, values, nsteps, gamma, add_value_last_step):
    """EPyMARL's PPOLearner.nstep_returns, from its definition: rewards [B, T, 1], mask [B, T, N], values [B, T + 1, N] (torch,
    any device / dtype) -> [B, T, N].  gamma is a Python float: `gamma ** step` is a binary64 power, as in EPyMARL."""
    import torch as th
    nstep_values = th.zeros_like(values[:, :-1])
    for t_start in range(rewards.size(1)):
        nstep_return_t = th.zeros_like(values[:, 0])
        for step in range(nsteps + 1):
            t = t_start + step
            if t >= rewards.size(1):
                break
            elif step == nsteps:
                nstep_return_t += gamma ** (step) * values[:, t] * mask[:, t]
            elif t == rewards.size(1) - 1 and add_value_last_step:
                nstep_return_t += gamma ** (step) * rewards[:, t] * mask[:, t]
                nstep_return_t += gamma ** (step + 1) * values[:, t + 1]
            else:
                nstep_return_t += gamma ** (step) * rewards[:, t] * mask[:, t]
        nstep_values[:, t_start, :] = nstep_return_t
    return nstep_values


def restatement(critic_forward, obs, reward, terminated, filled, gamma, nstep, add_value_last_step, value_scale=1.0, value_shift=0.0):
    """ppo_learner's no_grad lines on torch tensors of any device: -> (returns [B, T, N], values [B, T + 1, N], mask [B, T, N]).
    critic_forward: state [B, rows, S] -> [B, rows, N] (TargetCritic.forward).  gamma is taken as the float32 the launch is given."""
    B, rows, N, D = obs.shape
    rewards = reward[:, :-1].unsqueeze(-1)
    term = terminated[:, :-1].to(obs.dtype).unsqueeze(-1)
    mask = filled[:, :-1].to(obs.dtype).unsqueeze(-1).clone()
    mask[:, 1:] = mask[:, 1:] * (1 - term[:, :-1])
    mask = mask.repeat(1, 1, N)
    values = critic_forward(obs.reshape(B, rows, N * D))
    if value_scale != 1.0 or value_shift != 0.0:
        values = values * float(np.float32(value_scale)) + float(np.float32(value_shift))
    ret = epymarl_nstep_returns(rewards, mask, values, nstep, float(np.float32(gamma)), add_value_last_step)
    return ret, values, mask


def differing_rows(m, n, add_value_last_step):
    """-> (where [B, T] bool, k [B, T]): the rows the rule's one difference from EPyMARL covers -- m[t0] == 1, the flag on,
    m[T - 1] == 0 and the window reaches row T - 1 (k = T - 1 - t0 < n): EPyMARL adds fl(g[k + 1] values[T]) there, the rule
    does not."""
    B, T = m.shape
    k = (T - 1) - np.arange(T)[None].repeat(B, 0)
    where = m & ~m[:, -1:] & bool(add_value_last_step) & (k < n)
    return where, k


def rel_err(x, ref64, where):
    """max |x - ref| / (1 + |ref|) over the rows `where` (0.0 when there is none)."""
    x, ref64 = np.asarray(x, np.float64)[where], np.asarray(ref64, np.float64)[where]
    return float(np.max(np.abs(x - ref64) / (1.0 + np.abs(ref64)))) if x.size else 0.0
