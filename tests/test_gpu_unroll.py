"""rg_actor_unroll on the GPU (csrc/actor_unroll.h) against the launch it replaces: `rows` forward_fused launches on contiguous time
slices, restart=None, the hidden state carried through memory.  The claim is bit identity, so every comparison is on the words
(NaNs compare) and nothing here has a tolerance.  Every array the launch touches lies between sentinel guard bands; the outputs
start out full of sentinels, and the rows of an episode behind `rows` must keep them; the observation rows behind `rows` are NaN:
a launch that read one would show it."""
import numpy as np
import pytest
import torch

from gpu_helpers import random_actor

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 256                                   # elements on either side of an array
SENTINELS = {torch.float32: -777.25, torch.int32: -77777}


def guarded(shape, dtype):
    """-> (the whole allocation, the array inside it): sentinels everywhere."""
    n = int(np.prod(shape))
    raw = torch.full((GUARD + n + GUARD + 3,), SENTINELS[dtype], dtype=dtype, device=DEV)
    lo = GUARD + (-(raw.data_ptr() // raw.element_size() + GUARD)) % 4           # the array 16-byte aligned
    return (raw, lo, n), raw[lo:lo + n].view(shape)


def guards_intact(g):
    raw, lo, n = g
    return bool((raw[:lo] == SENTINELS[raw.dtype]).all()) and bool((raw[lo + n:] == SENTINELS[raw.dtype]).all())


def words(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t.contiguous()


def make_actor(n_sets, N, D, append, H, A, seed=3):
    from marbler_amd.evaluate import BatchedActor
    return BatchedActor(random_actor(n_sets, D + (N if append else 0), H, A, True, seed), N, device=DEV)


def per_step_launches(actor, obs, append, hidden=None):
    """The oracle: forward_fused on every time slice -> (q [B, rows, N, A], actions [B, rows, N], the last hidden state)."""
    B, rows = obs.shape[:2]
    h = actor.init_hidden(B) if hidden is None else hidden.clone()
    qs, acts = [], []
    for t in range(rows):
        q, a = actor.forward_fused(obs[:, t].contiguous(), h, append_agent_id=append, restart=None)
        qs.append(q)
        acts.append(a)
    return torch.stack(qs, 1), torch.stack(acts, 1), h


class Call(object):
    """One guarded unroll call: obs [B, rows + obs_extra, N, D] (NaN behind `rows`), outputs with out_extra more rows."""

    def __init__(self, B, N, D, H, A, rows, obs_extra=0, out_extra=0, with_hidden=False, seed=0):
        g = torch.Generator(device=DEV).manual_seed(1000 + seed)
        self.rows = rows
        self.g_obs, self.obs_all = guarded((B, rows + obs_extra, N, D), torch.float32)
        self.obs_all.copy_(torch.rand(B, rows + obs_extra, N, D, generator=g, device=DEV) * 3 - 1.5)    # (obs[:, 0] nonzero)
        self.obs_all[:, rows:] = float("nan")
        self.obs = self.obs_all[:, :rows]
        self.g_q, self.q_all = guarded((B, rows + out_extra, N, A), torch.float32)
        self.g_act, self.act_all = guarded((B, rows + out_extra, N), torch.int32)
        self.g_hout, self.hidden_out = guarded((B, N, H), torch.float32)
        self.hidden = None
        if with_hidden:
            self.g_hin, self.hidden = guarded((B, N, H), torch.float32)
            self.hidden.copy_(torch.rand(B, N, H, generator=g, device=DEV) * 2 - 1)

    def run(self, actor, append):
        obs_before = self.obs_all.clone()
        h_before = None if self.hidden is None else self.hidden.clone()
        q, act = actor.unroll(self.obs, append_agent_id=append, hidden=self.hidden, q_out=self.q_all[:, :self.rows],
                              actions_out=self.act_all[:, :self.rows], hidden_out=self.hidden_out)
        torch.cuda.synchronize()
        assert q.data_ptr() == self.q_all.data_ptr() and act.data_ptr() == self.act_all.data_ptr()
        assert torch.equal(words(torch.nan_to_num(self.obs_all, nan=7.0)), words(torch.nan_to_num(obs_before, nan=7.0))), "obs changed"
        assert h_before is None or torch.equal(words(self.hidden), words(h_before)), "hidden_in changed"
        for name in ("g_obs", "g_q", "g_act", "g_hout", "g_hin"):
            assert not hasattr(self, name) or guards_intact(getattr(self, name)), (name, "guard band damaged")
        assert bool((self.q_all[:, self.rows:] == SENTINELS[torch.float32]).all()), "q rows behind `rows` were written"
        assert bool((self.act_all[:, self.rows:] == SENTINELS[torch.int32]).all()), "action rows behind `rows` were written"
        return q, act


# B, N, one set per agent, H, D, one-hot id, A, rows, obs rows behind `rows`, output rows behind `rows`, hidden_in
# Tiles: shared weights B N = 4, 28, 32, 36, 45, 132, 165 flat rows (part of a tile, one exactly, one row into a second, several);
# per agent B = 1, 7, 8, 9, 33 episodes per agent index (B = 33: a second tile with ONE valid row).  Padded input widths: 16, 24,
# 32 (staged in LDS; 32 is the last that is) and 40, 48, 64 (read from memory as they lie).
CASES = [
    (1, 4, False, 128, 12, True, 5, 13, 0, 0, False),
    (7, 4, False, 128, 12, True, 5, 2, 3, 0, True),
    (8, 4, False, 128, 12, True, 5, 13, 0, 3, False),
    (9, 4, False, 64, 12, True, 5, 13, 3, 3, True),
    (9, 5, False, 128, 18, True, 20, 2, 0, 0, False),
    (33, 4, False, 128, 12, True, 5, 2, 3, 3, True),
    (33, 5, False, 64, 11, False, 32, 13, 0, 3, False),
    (8, 4, False, 64, 28, True, 20, 1, 3, 3, True),            # width 32: the widest staged input
    (1, 5, False, 64, 40, True, 5, 1, 0, 0, False),            # the wide path
    (8, 5, False, 128, 40, False, 20, 13, 3, 0, True),
    (33, 4, False, 128, 29, True, 32, 2, 0, 3, False),         # width 33 -> 40: the narrowest wide input
    (7, 4, False, 64, 60, True, 5, 2, 3, 3, True),             # width 64: the widest
    (1, 4, True, 128, 12, True, 5, 13, 3, 3, True),
    (7, 5, True, 64, 11, True, 20, 2, 0, 0, False),
    (8, 4, True, 128, 12, False, 32, 13, 0, 3, True),
    (9, 4, True, 64, 12, True, 5, 2, 3, 0, False),
    (9, 5, True, 128, 18, True, 5, 13, 0, 0, True),
    (33, 4, True, 128, 12, True, 5, 13, 3, 3, False),
    (33, 5, True, 64, 11, False, 20, 2, 3, 3, True),
    (33, 5, True, 128, 40, True, 32, 2, 0, 3, False),          # the wide path with one set per agent
    (8, 4, True, 64, 40, False, 5, 1, 3, 0, True),
    (33, 4, True, 64, 28, True, 20, 1, 0, 0, False),
    (1, 5, True, 128, 59, True, 32, 1, 0, 3, True),
    (7, 4, True, 128, 29, False, 20, 13, 3, 3, False),
]


def test_the_case_table_covers_what_it_is_meant_to():
    col = lambda i: {c[i] for c in CASES}  # noqa: E731
    assert 20 <= len(CASES) <= 28 and len(set(CASES)) == len(CASES)
    assert {c[0] * c[1] for c in CASES if not c[2]} >= {4, 28, 32, 36, 45, 132, 165}
    assert {c[0] for c in CASES if c[2]} == {1, 7, 8, 9, 33} and col(1) == {4, 5} and col(3) == {64, 128}
    assert col(6) == {5, 20, 32} and col(7) == {1, 2, 13} and col(8) == col(9) == {0, 3} and col(5) == col(10) == {False, True}
    widths = {(c[4] + (c[1] if c[5] else 0) + 7) // 8 * 8 for c in CASES}
    assert {32, 40, 64} <= widths and min(widths) <= 16
    for shared in (False, True):        # every path, both hidden sizes, with both kinds of weights
        assert {(c[3], (c[4] + (c[1] if c[5] else 0)) > 32) for c in CASES if c[2] != shared} == {(64, False), (64, True), (128, False), (128, True)}


@pytest.mark.parametrize("i", range(len(CASES)))
def test_unroll_equals_the_per_step_launches_bit_for_bit(i):
    B, N, per_agent, H, D, append, A, rows, obs_extra, out_extra, with_hidden = CASES[i]
    actor = make_actor(N if per_agent else 1, N, D, append, H, A, seed=i)
    call = Call(B, N, D, H, A, rows, obs_extra, out_extra, with_hidden, seed=i)
    q_ref, act_ref, h_ref = per_step_launches(actor, call.obs, append, call.hidden)
    q, act = call.run(actor, append)
    assert tuple(q.shape) == (B, rows, N, A) and tuple(act.shape) == (B, rows, N) and act.dtype == torch.int32
    assert torch.equal(words(q), words(q_ref)), CASES[i]
    assert torch.equal(act, act_ref), CASES[i]
    assert torch.equal(words(call.hidden_out), words(h_ref)), CASES[i]
    assert bool(((act >= 0) & (act < A)).all())
    assert float(call.obs[:, 0].abs().min()) > 0.0            # not the restart flag's zero observation


def test_outputs_are_optional_and_allocated_outputs_are_plain_tensors():
    B, N, D, H, A, rows = 9, 4, 12, 128, 5, 3
    actor = make_actor(1, N, D, True, H, A)
    call = Call(B, N, D, H, A, rows, obs_extra=2)
    q_ref, act_ref, h_ref = per_step_launches(actor, call.obs, True)
    q, act = actor.unroll(call.obs)
    assert q.is_contiguous() and act.is_contiguous() and torch.equal(words(q), words(q_ref)) and torch.equal(act, act_ref)
    # the C entry point with one output at a time
    import ctypes as C
    from marbler_amd import _lib
    lib, ws = _lib.load(), actor._weights_struct()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for keep in ("q", "actions", "hidden_out"):
        again = Call(B, N, D, H, A, rows, obs_extra=2)
        ptr = lambda name, t: t.data_ptr() if name == keep else None  # noqa: E731
        io = _lib.RgActorUnrollIO(again.obs_all.data_ptr(), ptr("q", again.q_all), ptr("actions", again.act_all), None,
                                  ptr("hidden_out", again.hidden_out), B, N, D, rows, rows + 2, rows, 1, 0)
        assert lib.rg_actor_unroll(C.byref(ws), C.byref(io), stream) == 0, lib.rg_actor_unroll_last_error()
        torch.cuda.synchronize()
        for name, got, want in (("q", again.q_all, q_ref), ("actions", again.act_all, act_ref), ("hidden_out", again.hidden_out, h_ref)):
            if name == keep:
                assert torch.equal(words(got), words(want)), keep
            else:
                assert bool((got == SENTINELS[got.dtype]).all()), (keep, name, "an output that was not asked for was written")
        assert all(guards_intact(g) for g in (again.g_q, again.g_act, again.g_hout, again.g_obs))


@pytest.mark.parametrize("per_agent", [False, True])
def test_two_chunks_of_time_equal_one_call(per_agent):
    """unroll(12) = unroll(5) then unroll(7) from its hidden_out, on the same storage; the second call's hidden_out IS its hidden."""
    B, N, D, H, A = 33, 4, 12, 128, 5
    actor = make_actor(N if per_agent else 1, N, D, True, H, A)
    whole = Call(B, N, D, H, A, 12, seed=5)
    q_ref, act_ref = whole.run(actor, True)
    parts = Call(B, N, D, H, A, 12, seed=5)
    assert torch.equal(parts.obs_all, whole.obs_all)
    _, h = guarded((B, N, H), torch.float32)
    actor.unroll(parts.obs[:, :5], q_out=parts.q_all[:, :5], actions_out=parts.act_all[:, :5], hidden_out=h)
    actor.unroll(parts.obs[:, 5:], hidden=h, q_out=parts.q_all[:, 5:], actions_out=parts.act_all[:, 5:], hidden_out=h)
    torch.cuda.synchronize()
    assert torch.equal(words(parts.q_all), words(q_ref)) and torch.equal(parts.act_all, act_ref)
    assert torch.equal(words(h), words(whole.hidden_out))
    assert guards_intact(parts.g_q) and guards_intact(parts.g_act) and guards_intact(parts.g_obs)


def test_a_nan_stays_in_its_own_row():
    B, N, D, H, A, rows = 9, 4, 12, 64, 5, 6
    b0, t0, n0 = 4, 2, 1
    actor = make_actor(1, N, D, True, H, A)
    clean = Call(B, N, D, H, A, rows, seed=8)
    q_clean, act_clean, _ = per_step_launches(actor, clean.obs, True)
    call = Call(B, N, D, H, A, rows, seed=8)
    call.obs[b0, t0, n0, 3] = float("nan")
    q_ref, act_ref, h_ref = per_step_launches(actor, call.obs, True)
    q, act = call.run(actor, True)
    assert torch.equal(words(q), words(q_ref)) and torch.equal(act, act_ref) and torch.equal(words(call.hidden_out), words(h_ref))
    hit = torch.zeros(B, rows, N, dtype=torch.bool, device=DEV)
    hit[b0, t0:, n0] = True
    assert bool(torch.isnan(q[hit]).all()) and bool(torch.isnan(call.hidden_out[b0, n0]).all())
    assert bool((act[hit] == 0).all())                                    # the first NaN is the maximum
    assert bool(torch.isfinite(q[~hit]).all())
    assert torch.equal(words(q[~hit]), words(q_clean[~hit])) and torch.equal(act[~hit], act_clean[~hit])


def test_a_captured_unroll_replays_to_the_same_bits():
    B, N, D, H, A, rows = 33, 4, 12, 128, 5, 7
    actor = make_actor(1, N, D, True, H, A)
    eager, graphed = Call(B, N, D, H, A, rows, 3, 3, True, seed=2), Call(B, N, D, H, A, rows, 3, 3, True, seed=2)
    eager.run(actor, True)                                         # (the weights are packed by now)
    side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(graph, stream=side):                     # one node, one branch
        actor.unroll(graphed.obs, hidden=graphed.hidden, q_out=graphed.q_all[:, :rows], actions_out=graphed.act_all[:, :rows],
                     hidden_out=graphed.hidden_out)
    torch.cuda.synchronize()
    graph.replay()                                                 # (a capture records; the replay is what runs)
    torch.cuda.synchronize()
    for name in ("q_all", "act_all", "hidden_out"):
        assert torch.equal(words(getattr(graphed, name)), words(getattr(eager, name))), name
    assert all(guards_intact(g) for g in (graphed.g_q, graphed.g_act, graphed.g_hout, graphed.g_hin, graphed.g_obs))


# ---------------------------------------------------------------- end to end: what the runner collected
def _collect(selector, one_launch, H):
    from marbler_amd.episodes import EpisodeBuffer
    from marbler_amd.evaluate import BatchedActor
    from marbler_amd.gymma import BatchedRunner, GymmaVecEnv
    v = GymmaVecEnv("robotarium_gym:PredatorCapturePrey-v0", 40, time_limit=12, seed=18)
    actor = BatchedActor(random_actor(1, v.obs_size + v.n_agents, H, v.n_actions, True, seed=4), v.n_agents, device=DEV)
    runner = BatchedRunner(v, actor, epsilon=0.0, seed=9, action_selector=selector)
    buf = EpisodeBuffer.for_runner(runner)
    runner.run(30, one_launch=one_launch, into=buf)
    out, batch = buf.unroll(actor), buf.batch()
    again = buf.unroll(actor, trim=True)
    torch.cuda.synchronize()
    B, rows = batch["length"].numel(), int(batch["length"].max()) + 1
    assert B >= 1, "no episode completed"
    assert tuple(out["q"].shape) == (B, buf.L + 1, buf.N, buf.A) and tuple(out["greedy"].shape) == (B, buf.L + 1, buf.N)
    assert tuple(again["q"].shape) == (B, rows, buf.N, buf.A) and torch.equal(words(again["q"]), words(out["q"][:, :rows]))
    assert torch.equal(again["greedy"], out["greedy"][:, :rows])
    data = torch.arange(buf.L + 1, device=DEV)[None, :] < batch["length"][:, None]          # t < length
    v.close()
    return out, batch, data


@pytest.mark.parametrize("one_launch", [False, True])
def test_unrolled_greedy_actions_are_the_actions_the_runner_took(one_launch):
    out, batch, data = _collect("epsilon_greedy", one_launch, 128)
    assert int(data.sum()) >= 12
    assert torch.equal(out["greedy"][data].to(torch.int64), batch["actions"][..., 0][data])


@pytest.mark.parametrize("one_launch", [False, True])
def test_unrolled_logits_give_the_probabilities_the_runner_stored(one_launch):
    """prob of the stored action from the unrolled q by the rule of evaluate.soft_select, written out: e_c = soft_exp(q_c - m),
    Z the sum ((e_0 + e_1) + e_2) + ... in column order, prob = e_action / Z -- the words the collection stored."""
    from marbler_amd.evaluate import soft_exp
    out, batch, data = _collect("soft_policies", one_launch, 64)
    q = out["q"]
    e = soft_exp(q - q.max(dim=-1, keepdim=True).values)
    Z = torch.zeros_like(e[..., 0])
    for k in range(q.shape[-1]):
        Z = Z + e[..., k]
    prob = e.gather(-1, batch["actions"].clamp(0, q.shape[-1] - 1))[..., 0] / Z
    assert int(data.sum()) >= 12
    assert torch.equal(words(prob[data]), words(batch["probs"][data]))
    assert not torch.equal(out["greedy"][data].to(torch.int64), batch["actions"][..., 0][data]), "the runner sampled: some action is not the greedy one"
