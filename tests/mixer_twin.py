"""The rule of rg_mixer_forward / rg_mixer_backward (csrc/mixer_grad.h) in NumPy float64: the forward pass, the hand-written backward
pass with the weight-gradient sums, a float32 twin of vdn / none that fixes every bit, and the a-priori float32 error bound of every
pre-activation that has a kink behind it (the kink margin of DESIGN.md section 4 "Trainable mixer")."""
import numpy as np

EMBED, HYPER = 32, 64
U = 2.0 ** -24                          # the unit roundoff of binary32
MARGIN = 8.0                            # a pre-activation must lie further from zero than MARGIN x its bound


def live_rows(mask):
    return np.asarray(mask) != 0.0


def chosen(q, actions, live):
    """x [B, T, N] of the live rows (zero elsewhere); an action outside [0, A) gives NaN."""
    B, rows, N, A = q.shape
    T = rows - 1
    x = np.zeros((B, T, N), q.dtype)
    for b, t in zip(*np.nonzero(live)):
        for n in range(N):
            a = int(actions[b, t, n])
            x[b, t, n] = q[b, t, n, a] if 0 <= a < A else np.nan
    return x


def gather_twin(kind, q, actions, mask, d_mixed):
    """vdn / none in float32, every bit fixed -> (mixed, d_q [B, rows, N, A])."""
    q = np.asarray(q, np.float32)
    B, rows, N, A = q.shape
    T, live = rows - 1, live_rows(mask)
    x = chosen(q, actions, live)
    d_q = np.zeros((B, rows, N, A), np.float32)
    if kind == "none":
        mixed = x.copy()
    else:
        mixed = x[..., 0].copy()
        for n in range(1, N):
            mixed = (mixed + x[..., n]).astype(np.float32)
    for b, t in zip(*np.nonzero(live)):
        for n in range(N):
            a = int(actions[b, t, n])
            if 0 <= a < A:
                d_q[b, t, n, a] = d_mixed[b, t, n] if kind == "none" else d_mixed[b, t]
    return mixed, d_q


def _f64(params):
    return {k: np.asarray(v, np.float64) for k, v in params.items()}


def pre_activations(params, s):
    """s [R, S] float64 -> a1 [R, 64], af [R, 64], av [R, 32], p1 [R, 32 N], pf [R, 32], b1 [R, 32]."""
    p = _f64(params)
    a1 = s @ p["hyper_w_1.0.weight"].T + p["hyper_w_1.0.bias"]
    af = s @ p["hyper_w_final.0.weight"].T + p["hyper_w_final.0.bias"]
    av = s @ p["V.0.weight"].T + p["V.0.bias"]
    p1 = np.maximum(a1, 0) @ p["hyper_w_1.2.weight"].T + p["hyper_w_1.2.bias"]
    pf = np.maximum(af, 0) @ p["hyper_w_final.2.weight"].T + p["hyper_w_final.2.bias"]
    b1 = s @ p["hyper_b_1.weight"].T + p["hyper_b_1.bias"]
    return a1, af, av, p1, pf, b1


def kink_bounds(params, s):
    """The a-priori float32 forward error bound of every pre-activation with a kink behind it, by absolute-value sums through
    both layers.  A sum of K products and a bias, in which every term passes through at most C + 2 roundings, is off by at most
    (C + 2) 2^-24 (sum |w input| + |b|); the launches deal the K steps of every sum out to two chains in turn and add the chains,
    so C = K / 2:
        first layer,  a = W s + b, K = S:              e(a) = (S / 2 + 2) 2^-24 (sum_k |W_k s_k| + |b|)
        second layer, p = W2 relu(a) + b2, K = 64:     e(p) = (32 + 2) 2^-24 (sum_c |W2_c| relu(a_c) + |b2|) + sum_{c: a_c > 0} |W2_c| e(a_c)
    relu is 1-Lipschitz, so the error of a first-layer unit is carried with the weight's absolute value; a unit with a_c < -e(a_c)
    -- and every unit is checked to lie outside its own margin -- is 0.0 in float32 as it is in float64 and carries nothing.
    -> (values, bounds), each the concatenation [R, 64 + 64 + 32 + 32 N + 32] of (a1, af, av, p1, pf)."""
    p = _f64(params)
    s = np.asarray(s, np.float64)
    S = s.shape[1]
    a1, af, av, p1, pf, _ = pre_activations(params, s)
    first = lambda k: (S / 2 + 2) * U * (np.abs(s) @ np.abs(p[k + ".weight"]).T + np.abs(p[k + ".bias"]))   # noqa: E731
    e1, ef, ev = first("hyper_w_1.0"), first("hyper_w_final.0"), first("V.0")
    second = lambda k, a, e: ((HYPER / 2 + 2) * U * (np.maximum(a, 0) @ np.abs(p[k + ".weight"]).T + np.abs(p[k + ".bias"]))   # noqa: E731
                              + (e * (a > 0)) @ np.abs(p[k + ".weight"]).T)
    return (np.concatenate([a1, af, av, p1, pf], axis=1),
            np.concatenate([e1, ef, ev, second("hyper_w_1.2", a1, e1), second("hyper_w_final.2", af, ef)], axis=1))


def margin_violations(params, s):
    """[R] bool: some pre-activation of the row lies within MARGIN x its bound of zero."""
    values, bounds = kink_bounds(params, s)
    return (np.abs(values) <= MARGIN * bounds).any(axis=1)


def qmix_forward(params, x, s):
    """x [R, N], s [R, S] float64 -> a dict of every intermediate; y [R]."""
    p = _f64(params)
    R, N = x.shape
    a1, af, av, p1, pf, b1 = pre_activations(params, s)
    w1, wf = np.abs(p1).reshape(R, N, EMBED), np.abs(pf)
    u = np.einsum("rn,rne->re", x, w1) + b1
    with np.errstate(over="ignore", invalid="ignore"):
        hidden = np.where(u > 0, u, np.expm1(np.minimum(u, 0)))
    hidden = np.where(np.isnan(u), np.nan, hidden)
    v = np.maximum(av, 0) @ p["V.2.weight"][0] + p["V.2.bias"][0]
    y = (hidden * wf).sum(axis=1) + v
    return dict(a1=a1, af=af, av=av, p1=p1, pf=pf, w1=w1, wf=wf, u=u, hidden=hidden, y=y)


def twin(kind, q, actions, obs, mask, params=None, d_mixed=None):
    """The whole rule in float64.  q [B, rows, N, A], actions [B, rows, N], obs [B, rows, N, D], mask [B, T]; d_mixed [B, T]
    ([B, T, N] for none) or None (forward only).  -> dict: mixed, and with d_mixed: d_q [B, rows, N, A]; for qmix d_pre [B, rows, 192],
    d_p2 [B, rows, 32 N + 32], g [B, rows, 160] and grads {EPyMARL's key: array}.  Rows that are not live are never read."""
    q = np.asarray(q, np.float64)
    B, rows, N, A = q.shape
    T, live = rows - 1, live_rows(mask)
    x = chosen(q, actions, live)
    out = {}
    if kind != "qmix":
        out["mixed"] = x if kind == "none" else x.sum(axis=-1)
        if d_mixed is not None:
            d_q = np.zeros((B, rows, N, A))
            for b, t in zip(*np.nonzero(live)):
                for n in range(N):
                    a = int(actions[b, t, n])
                    if 0 <= a < A:
                        d_q[b, t, n, a] = d_mixed[b, t, n] if kind == "none" else d_mixed[b, t]
            out["d_q"] = d_q
        return out
    p = _f64(params)
    S = N * obs.shape[3]
    idx = np.nonzero(live)
    s = np.asarray(obs, np.float64).reshape(B, rows, S)[:, :T][idx]
    f = qmix_forward(params, x[idx], s)
    mixed = np.zeros((B, T))
    mixed[idx] = f["y"]
    out["mixed"] = mixed
    if d_mixed is None:
        return out
    R = s.shape[0]
    dy = np.asarray(d_mixed, np.float64)[idx]
    xs = x[idx]
    d_hidden, d_wf = dy[:, None] * f["wf"], dy[:, None] * f["hidden"]
    du = d_hidden * np.where(f["u"] > 0, 1.0, f["hidden"] + 1.0)
    dx = np.einsum("re,rne->rn", du, f["w1"])
    d_w1 = xs[:, :, None] * du[:, None, :]
    dp1 = (d_w1 * np.sign(f["p1"]).reshape(R, N, EMBED)).reshape(R, N * EMBED)
    dpf = d_wf * np.sign(f["pf"])
    da1 = (dp1 @ p["hyper_w_1.2.weight"]) * (f["a1"] > 0)
    daf = (dpf @ p["hyper_w_final.2.weight"]) * (f["af"] > 0)
    dav = dy[:, None] * p["V.2.weight"][0] * (f["av"] > 0)
    g1, gf, gv = np.maximum(f["a1"], 0), np.maximum(f["af"], 0), np.maximum(f["av"], 0)
    d_q = np.zeros((B, rows, N, A))
    for r, (b, t) in enumerate(zip(*idx)):
        for n in range(N):
            a = int(actions[b, t, n])
            if 0 <= a < A:
                d_q[b, t, n, a] = dx[r, n]
    d_pre, d_p2, g = np.zeros((B, rows, 192)), np.zeros((B, rows, N * EMBED + EMBED)), np.zeros((B, rows, 160))
    d_pre[:, :T][idx] = np.concatenate([da1, daf, dav, du], axis=1)
    d_p2[:, :T][idx] = np.concatenate([dp1, dpf], axis=1)
    g[:, :T][idx] = np.concatenate([g1, gf, gv], axis=1)
    grads = {"hyper_w_1.0.weight": da1.T @ s, "hyper_w_1.0.bias": da1.sum(0), "hyper_w_final.0.weight": daf.T @ s,
             "hyper_w_final.0.bias": daf.sum(0), "V.0.weight": dav.T @ s, "V.0.bias": dav.sum(0), "hyper_b_1.weight": du.T @ s,
             "hyper_b_1.bias": du.sum(0), "hyper_w_1.2.weight": dp1.T @ g1, "hyper_w_1.2.bias": dp1.sum(0),
             "hyper_w_final.2.weight": dpf.T @ gf, "hyper_w_final.2.bias": dpf.sum(0), "V.2.weight": (dy @ gv)[None, :],
             "V.2.bias": np.array([dy.sum()])}
    out.update(d_q=d_q, d_pre=d_pre, d_p2=d_p2, g=g, grads=grads)
    return out
