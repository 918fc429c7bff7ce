"""The soft-policies selection rule (csrc/actor_common.h `soft_exp` / `soft_select_row`, marbler_amd.evaluate.soft_select) in
numpy float32, operation for operation, plus a float64 inverse-CDF reference.  Every float32 operation below is one correctly
rounded IEEE operation (numpy does not contract), in the order the header states, so the kernel, the torch restatement and this
file give the same action and the same `prob` word for the same (q, u)."""
import numpy as np

F = np.float32
LOG2E = F(1.4426950408889634)          # 0x3FB8AA3B
LN2_HI = F(0.693359375)                # 355 / 512: nine significant bits, k * LN2_HI is exact for |k| <= 2^15
LN2_LO = F(-2.12194440e-4)             # ln 2 - LN2_HI
POLY = (F(1.9875691500e-4), F(1.3981999507e-3), F(8.3334519073e-3), F(4.1665795894e-2), F(1.6666665459e-1), F(5.0000001201e-1))
CUT = F(-87.336)                       # below it exp(x) < 1.001 x 2^-126, the edge of the normal float32 range: soft_exp is 0 there


def soft_exp(x):
    """exp(x) for float32 x <= 0 (any shape); 0 for x < CUT (and for -inf)."""
    x = np.asarray(x, F)
    with np.errstate(invalid="ignore", over="ignore"):
        k = np.rint(x * LOG2E)                      # round to nearest even
        r = (x - k * LN2_HI) - k * LN2_LO
        p = POLY[0]
        for c in POLY[1:]:
            p = p * r + c                           # one multiply, one add
        y = ((p * (r * r)) + r) + F(1.0)
        ki = np.where(x >= CUT, k, F(0.0)).astype(np.int32)
        scaled = (y.view(np.int32) + (ki << 23)).view(F)   # 2^k through the exponent field
    return np.where(x >= CUT, scaled, F(0.0)).astype(F)


def greedy(q):
    """torch.argmax's answer per row: the first maximum, a NaN counting as the largest value (the first NaN wins)."""
    q = np.asarray(q, F)
    nan = np.isnan(q)
    return np.where(nan.any(-1), nan.argmax(-1), np.where(nan, -np.inf, q).argmax(-1)).astype(np.int32)


def soft_select(q, u):
    """q [..., A] float32 logits, u [...] float32 uniforms in [0, 1) -> (actions int32 [...], prob float32 [...])."""
    q, u = np.asarray(q, F), np.asarray(u, F)
    A = q.shape[-1]
    with np.errstate(invalid="ignore"):
        m = q.max(-1)                               # (a NaN anywhere gives NaN)
        ok = np.isfinite(m)
        e = soft_exp(q - m[..., None])
        c = np.empty_like(e)
        run = np.zeros(q.shape[:-1], F)
        for k in range(A):                          # ((e_0 + e_1) + e_2) + ...   (0 + e_0 is e_0)
            run = run + e[..., k]
            c[..., k] = run
        Z = run
        t = u * Z
        cross = t[..., None] < c
        first = np.where(cross.any(-1), cross.argmax(-1), -1)
        pos = e > 0
        last = A - 1 - pos[..., ::-1].argmax(-1)
        act = np.where(first >= 0, first, last)
        prob = np.take_along_axis(e, act[..., None], -1)[..., 0] / Z
    act = np.where(ok, act, greedy(q)).astype(np.int32)
    prob = np.where(ok, prob, F(np.nan)).astype(F)
    return act, prob


def softmax64(q):
    """float64 softmax of float32 logits (np.exp in binary64); rows must have a finite maximum."""
    q = np.asarray(q, np.float64)
    e = np.exp(q - q.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def inverse_cdf64(q, u):
    """float64 reference: (action, distance of u to the nearest CDF boundary of its row)."""
    p = softmax64(q)
    cdf = np.cumsum(p, -1)
    cdf[..., -1] = 1.0
    u = np.asarray(u, np.float64)
    act = (u[..., None] >= cdf).sum(-1).astype(np.int32)
    dist = np.abs(u[..., None] - cdf[..., :-1]).min(-1) if q.shape[-1] > 1 else np.ones_like(u)
    return act, dist
