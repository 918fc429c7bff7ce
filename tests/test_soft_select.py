"""The soft-policies selection rule on the CPU tier: marbler_amd.evaluate.soft_select (torch) and tests/soft_twin.py (numpy) agree
word for word, and the rule is accurate against a float64 reference (np.exp in binary64).

soft_exp's measured error (this file, numpy float32 on the CPU): 1.37 x 2^-24 relative over 2^24 random arguments and every
reduction boundary; the bound asserted is 4 x 2^-24.  The arguments cover [-88, 0]; the relative bound is asserted from the
underflow cut (-87.336, just above ln 2^-126 = -87.3365) up: below it exp(x) < 1.001 x 2^-126 is at or under the edge of the normal
float32 range, where no float32 function can meet a relative bound, and the rule returns 0 -- asserted as such, together with the
size of what is dropped (an absolute error below 1.001 x 2^-126 = 1.18e-38)."""
import numpy as np
import pytest
import torch

import soft_twin
from marbler_amd.evaluate import soft_select

ONE_BELOW = np.nextafter(np.float32(1), np.float32(0))


def _logits(rng, rows, A, scale):
    q = (rng.standard_normal((rows, A)) * scale).astype(np.float32)
    q[rng.random(q.shape) < 0.05] = -np.inf              # rows with -inf columns
    q[: rows // 10, A - 1] = q[: rows // 10, 0]          # rows with ties
    q[rows // 10: rows // 5] = np.float32(0.25)          # all columns equal
    return q


@pytest.mark.parametrize("A", [2, 5, 7, 32])
@pytest.mark.parametrize("scale", [0.1, 1.0, 10.0, 50.0])
def test_torch_and_numpy_agree_word_for_word(A, scale):
    rng = np.random.default_rng(1000 * A + int(10 * scale))
    rows = 20000
    q = _logits(rng, rows, A, scale)
    q[-30:-20] = np.nan
    q[-20:-10, A // 2] = np.inf
    q[-10:] = -np.inf
    u = rng.random(rows, dtype=np.float32)
    u[::7] = 0.0
    u[3::7] = ONE_BELOW
    a, p = soft_twin.soft_select(q, u)
    ta, tp = soft_select(torch.from_numpy(q), torch.from_numpy(u))
    assert ta.dtype == torch.int32 and tp.dtype == torch.float32
    assert np.array_equal(a, ta.numpy())
    assert np.array_equal(p.view(np.uint32), tp.numpy().view(np.uint32))
    assert ((a >= 0) & (a < A)).all()
    # a column with e = 0 (a -inf logit) is never chosen on a row with a finite maximum
    fin = np.isfinite(q.max(-1))
    assert np.isfinite(np.take_along_axis(q, a[:, None].astype(np.int64), 1)[:, 0][fin]).all()
    # out= forms write in place
    oa, op = torch.empty(rows, dtype=torch.int32), torch.empty(rows)
    ra, rp = soft_select(torch.from_numpy(q), torch.from_numpy(u), out_actions=oa, out_prob=op)
    assert ra is oa and rp is op and torch.equal(oa, ta) and np.array_equal(op.numpy().view(np.uint32), p.view(np.uint32))


def test_soft_exp_against_binary64():
    rng = np.random.default_rng(7)
    x = rng.uniform(-88.0, 0.0, 1 << 24).astype(np.float32)
    # every reduction boundary (k + 1/2) ln 2 with four neighbours on either side, the ends and the cut
    b = ((np.arange(-127, 1)[:, None] + 0.5) * np.log(2.0)).astype(np.float32)
    near = [b]
    for direction in (np.float32(-np.inf), np.float32(np.inf)):
        w = b
        for _ in range(4):
            w = np.nextafter(w, direction)
            near.append(w)
    edge = np.array([0.0, -0.0, -88.0, soft_twin.CUT, np.nextafter(soft_twin.CUT, np.float32(-np.inf)), -1e-30, -1e-8], np.float32)
    x = np.concatenate([x] + [w.ravel() for w in near] + [edge])
    x = x[(x <= 0) & (x >= -88.0)]
    assert x.size >= 1 << 24
    y = soft_twin.soft_exp(x)
    ref = np.exp(x.astype(np.float64))
    live = x >= soft_twin.CUT
    rel = np.abs(y[live].astype(np.float64) - ref[live]) / ref[live]
    print(f"soft_exp: max relative error {rel.max() * 2 ** 24:.3f} x 2^-24 at x = {x[live][rel.argmax()]!r} over {live.sum()} arguments")
    assert rel.max() <= 4 * 2.0 ** -24
    assert (y[~live] == 0).all() and ref[~live].max() < 1.001 * 2.0 ** -126 and (~live).sum() > 1000
    assert soft_twin.soft_exp(np.float32(0.0)) == 1.0 and soft_twin.soft_exp(np.float32(-np.inf)) == 0.0
    # the torch restatement of soft_exp is the same function
    from marbler_amd.evaluate import soft_exp
    sub = np.concatenate([x[: 1 << 20]] + [w.ravel() for w in near] + [edge])
    assert np.array_equal(soft_exp(torch.from_numpy(sub)).numpy().view(np.uint32), soft_twin.soft_exp(sub).view(np.uint32))


@pytest.mark.parametrize("A", [2, 5, 7, 32])
def test_prob_and_actions_against_float64(A):
    rng = np.random.default_rng(50 + A)
    rows = 200000
    q = np.concatenate([_logits(rng, rows // 4, A, s) for s in (0.1, 1.0, 10.0, 50.0)])
    q[np.isinf(q).all(-1), 0] = 0.0                    # (rows with no finite maximum have no float64 reference: their own test)
    u = rng.random(rows, dtype=np.float32)
    a, p = soft_twin.soft_select(q, u)
    p64 = soft_twin.softmax64(q)
    # prob: 31 ordered additions (<= 31 x 2^-24 = 1.9e-6), the exponential's 2.4e-7 twice, one division
    pa = np.take_along_axis(p64, a[:, None].astype(np.int64), 1)[:, 0]
    normal = pa > 2.0 ** -100                          # (far above float32's underflow: the quotient of normal numbers)
    rel = np.abs(p[normal].astype(np.float64) - pa[normal]) / pa[normal]
    print(f"A = {A}: prob max relative error {rel.max():.3e}")
    assert rel.max() <= 4e-6
    # actions: identical wherever u is farther than 1e-5 from every float64 CDF boundary of its row
    a64, dist = soft_twin.inverse_cdf64(q, u)
    far = dist > 1e-5
    print(f"A = {A}: {(~far).mean():.2e} of the rows within 1e-5 of a boundary")
    assert (~far).mean() <= 1e-3
    assert np.array_equal(a[far], a64[far])


def test_frequencies():
    rng = np.random.default_rng(11)
    n = 1 << 20
    for q in (np.array([0.3, -1.2, 2.0, 0.0, 1.1], np.float32), rng.standard_normal(20).astype(np.float32) * 2):
        u = rng.random(n, dtype=np.float32)
        a, p = soft_twin.soft_select(np.broadcast_to(q, (n, q.size)), u)
        p64 = soft_twin.softmax64(q)
        freq = np.bincount(a, minlength=q.size) / n
        sd = np.sqrt(p64 * (1 - p64) / n)
        assert (np.abs(freq - p64) <= 5 * sd).all(), (freq, p64)


def test_degenerate_rows_take_the_greedy_action():
    q = np.array([[0.0, np.nan, 1.0, 2.0], [np.nan, np.nan, 0.0, 1.0], [0.0, np.inf, 1.0, np.inf], [-np.inf] * 4,
                  [1.0, np.inf, np.nan, 0.0]], np.float32)
    tq = torch.from_numpy(q)
    for u in (0.0, 0.37, float(ONE_BELOW)):
        uu = np.full(len(q), u, np.float32)
        a, p = soft_twin.soft_select(q, uu)
        ta, tp = soft_select(tq, torch.from_numpy(uu))
        want = tq.argmax(dim=1).to(torch.int32)
        assert np.array_equal(a, want.numpy()) and torch.equal(ta, want)
        assert np.isnan(p).all() and torch.isnan(tp).all()
    assert want.tolist() == [1, 0, 1, 0, 2]


def test_no_crossing_takes_the_last_positive_column():
    # the rule's fallback: when no partial sum is above the threshold the last column with e > 0 is taken, never a -inf one.
    # For u <= nextafter(1, 0) the float32 product u * Z stays below Z, so the fallback is reached only by u = 1 -- outside the
    # contract of sample_u, and still an action inside the row's support rather than an index past it.
    q = np.array([[0.0, 0.0, 0.0, -np.inf], [1.0, -np.inf, -200.0, -np.inf], [0.5, 1.5, -1.0, 2.0]], np.float32)
    for uv, want in ((1.0, [2, 0, 3]), (float(ONE_BELOW), [2, 0, 3])):
        u = np.full(3, uv, np.float32)
        a, p = soft_twin.soft_select(q, u)
        assert a.tolist() == want and p[1] == 1.0
        ta, tp = soft_select(torch.from_numpy(q), torch.from_numpy(u))
        assert ta.tolist() == want and np.array_equal(tp.numpy().view(np.uint32), p.view(np.uint32))
