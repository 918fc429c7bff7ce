"""The NumPy twin of the GRU scan rule (marbler_amd/csrc/gru_scan.h): the forward recurrence and a HAND-WRITTEN backward pass, line for
line as the rule states them, in whatever dtype it is handed (float64 in the tests).  tests/test_gru_scan_cases.py holds its backward
pass to torch.autograd through a float64 GRUCell composition; tests/test_gpu_gru_scan.py holds the kernels to it."""
import numpy as np


def sigmoid(x):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-x))


def _sets(w, N):
    """w [A, ...] with A = 1 or N -> [N, ...] (agent n's set)."""
    w = np.asarray(w)
    return np.broadcast_to(w, (N,) + w.shape[1:]) if w.shape[0] == 1 else w


def forward(gi, w_hh, b_hh, hidden=None):
    """gi [B, rows, N, 3H], w_hh [A, 3H, H], b_hh [A, 3H], hidden [B, N, H] or None -> h [B, rows, N, H], gates [B, rows, N, 4H] =
    (r, z, n, gh_n), hidden_out [B, N, H]."""
    B, rows, N, G = gi.shape
    H = G // 3
    w, b = _sets(w_hh, N), _sets(b_hh, N)
    hp = np.zeros((B, N, H), gi.dtype) if hidden is None else np.asarray(hidden, gi.dtype)
    h, gates = np.empty((B, rows, N, H), gi.dtype), np.empty((B, rows, N, 4 * H), gi.dtype)
    for t in range(rows):
        gh = np.einsum("bnk,ngk->bng", hp, w) + b
        r = sigmoid(gi[:, t, :, :H] + gh[..., :H])
        z = sigmoid(gi[:, t, :, H:2 * H] + gh[..., H:2 * H])
        n = np.tanh(gi[:, t, :, 2 * H:] + r * gh[..., 2 * H:])
        hp = (1.0 - z) * n + z * hp
        h[:, t], gates[:, t] = hp, np.concatenate([r, z, n, gh[..., 2 * H:]], axis=-1)
    return h, gates, hp


def backward(h, gates, w_hh, dh_ext, hidden=None, d_hidden_out=None):
    """The rule's backward pass on saved h and gates -> dgi [B, rows, N, 3H], dghn [B, rows, N, H], d_hidden_in [B, N, H]."""
    B, rows, N, H = h.shape
    w = _sets(w_hh, N)
    carry = np.zeros((B, N, H), h.dtype) if d_hidden_out is None else np.asarray(d_hidden_out, h.dtype)
    h0 = np.zeros((B, N, H), h.dtype) if hidden is None else np.asarray(hidden, h.dtype)
    dgi, dghn = np.empty((B, rows, N, 3 * H), h.dtype), np.empty((B, rows, N, H), h.dtype)
    for t in range(rows - 1, -1, -1):
        r, z, n, ghn = (gates[:, t, :, k * H:(k + 1) * H] for k in range(4))
        hp = h[:, t - 1] if t > 0 else h0
        dh = dh_ext[:, t] + carry
        dn = dh * (1.0 - z)
        dz = dh * (hp - n)
        da_n = dn * (1.0 - n * n)
        da_r = (da_n * ghn) * r * (1.0 - r)
        da_z = dz * z * (1.0 - z)
        dgi[:, t] = np.concatenate([da_r, da_z, da_n], axis=-1)
        dghn[:, t] = da_n * r
        dgh = np.concatenate([da_r, da_z, dghn[:, t]], axis=-1)
        carry = dh * z + np.einsum("bng,ngk->bnk", dgh, w)
    return dgi, dghn, carry


def weight_grads(h, dgi, dghn, hidden, n_sets):
    """dW_hh [A, 3H, H] and db_hh [A, 3H] from the scan's outputs: dgh^T h_prev and the sum of dgh over every row."""
    B, rows, N, H = h.shape
    dgh = np.concatenate([dgi[..., :2 * H], dghn], axis=-1)
    hp = np.concatenate([(np.zeros((B, 1, N, H), h.dtype) if hidden is None else np.asarray(hidden, h.dtype)[:, None]), h[:, :-1]], axis=1)
    dw, db = np.einsum("btng,btnk->ngk", dgh, hp), dgh.sum(axis=(0, 1))
    return (dw.sum(axis=0, keepdims=True), db.sum(axis=0, keepdims=True)) if n_sets == 1 else (dw, db)


def err(x, x64):
    """The tests' metric: max |x - x64| / (1 + |x64|)."""
    x64 = np.asarray(x64, np.float64)
    return float(np.max(np.abs(np.asarray(x, np.float64) - x64) / (1.0 + np.abs(x64))))
