"""The fused actor kernel (csrc/actor_mfma.hip, f32 MFMA) against the torch float32 evaluation of the
same weights (marbler_amd.evaluate.BatchedActor.forward, itself pinned to the reference's RNNAgent /
RNNNSAgent modules by tests/test_evaluate.py): action values and hidden state within 1e-5, greedy
actions equal wherever the top two action values are more than 1e-4 apart."""
import os

import numpy as np
import pytest
import torch

from gpu_helpers import fused_actor_random_shape, random_actor

pytestmark = pytest.mark.gpu
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("shared,H,E,N,D,A,use_rnn,append", [
    (True, 128, 300, 5, 16, 5, True, True),      # the PredatorCapturePrey model zoo shape (qmix.json)
    (True, 128, 70, 5, 16, 5, True, None),       # the same on torch-layout GRU weights (no packing: f32-input MFMA)
    (True, 128, 70, 5, 16, 5, True, "f32"),      # ... and on the float32 streaming order of rg_actor_pack_gru (f32-input MFMA)
    (False, 128, 40, 4, 30, 5, True, "f32"),
    (True, 64, 77, 4, 9, 20, True, True),        # MaterialTransport: 20 actions
    (False, 64, 130, 5, 16, 5, True, False),     # rnn_ns: one network per agent, no agent id
    (True, 128, 33, 8, 18, 5, False, True),      # use_rnn = False
    (False, 128, 1, 3, 30, 5, True, False),      # a single env, ragged tile
    (False, 128, 50, 4, 9, 20, False, False),    # the zoo's MaterialTransport mappo_ns: one MLP-layer network per agent (round 4: its weight stride)
    (True, 128, 65, 4, 28, 5, True, True),       # input width exactly 32: the widest layer fc1 stages through LDS
    (False, 64, 65, 3, 32, 7, True, False),      # ... per-agent weights, no agent id, two wavefronts per tile
    (True, 64, 65, 4, 29, 5, True, True),        # input width 33: the first one fc1 reads straight from memory
    (False, 128, 35, 2, 62, 3, True, True),      # input width 64: the widest supported
    (True, 128, 35, 3, 1, 2, True, False),       # input width 1
])
def test_fused_actor_matches_torch(shared, H, E, N, D, A, use_rnn, append):
    from marbler_amd.evaluate import BatchedActor
    dev = "cuda:0"
    pack = {None: False, "f32": "f32"}.get(append, True)     # True: the default, three bfloat16 planes (rg_actor_pack_gru_bf16x3)
    append = True if append in (None, "f32") else append
    I = D + (N if append else 0)
    sd = random_actor(1 if shared else N, I, H, A, use_rnn, seed=H + E)
    actor = BatchedActor(sd, N, use_rnn=use_rnn, device=dev, pack_gru=pack)
    assert actor.fused_supported()
    g = torch.Generator(device=dev).manual_seed(1)
    hidden = (torch.rand(E, N, H, generator=g, device=dev) * 2 - 1)
    eye = torch.eye(N, device=dev).unsqueeze(0).expand(E, N, N)
    h_ref = hidden.clone()
    for step in range(3):   # the hidden state feeds back
        obs = torch.rand(E, N, D, generator=g, device=dev) * 3 - 1.5
        restart = (torch.rand(E, generator=g, device=dev) < 0.2).to(torch.uint8)
        fresh = restart.bool()[:, None, None]      # a new episode: zero observation, zero hidden state
        obs_seen = torch.where(fresh, torch.zeros_like(obs), obs)
        inp = torch.cat([obs_seen, eye], dim=2) if append else obs_seen
        h_in = torch.where(restart.bool()[:, None, None], torch.zeros_like(h_ref), h_ref)
        q_ref, h_ref = actor.forward(inp, h_in)
        q, act = actor.forward_fused(obs, hidden, append_agent_id=append, restart=restart)
        torch.cuda.synchronize()
        assert float((q - q_ref).abs().max()) < 1e-5, step
        assert float((hidden - h_ref).abs().max()) < 1e-5, step
        top2 = q_ref.topk(2, dim=2).values
        clear = (top2[..., 0] - top2[..., 1]) > 1e-4
        assert torch.equal(act[clear].long(), q_ref.argmax(dim=2)[clear])
        assert bool(clear.float().mean() > 0.9)


@pytest.mark.parametrize("name", ["actor_shared_gru_h64", "actor_ns_gru_h64"])
def test_fused_actor_on_the_reference_vectors(name):
    """Golden vectors from the reference's own RNNAgent / RNNNSAgent (tests/golden/make_actor_golden.py)."""
    from marbler_amd.evaluate import BatchedActor
    g = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
    sd = {k[3:]: torch.as_tensor(g[k]) for k in g.files if k.startswith("sd_")}
    T, N, I = g["inputs"].shape
    actor = BatchedActor(sd, N, use_rnn=bool(g["use_rnn"]), device="cuda:0")
    E = 3                                            # the same env three times: batching must not mix rows
    hidden = actor.init_hidden(E)
    for t in range(T):
        x = torch.as_tensor(g["inputs"][t]).unsqueeze(0).expand(E, N, I).contiguous().cuda()   # carries the agent id already
        q, _ = actor.forward_fused(x, hidden, append_agent_id=False)
        for e in range(E):
            assert np.abs(q[e].cpu().numpy() - g["q"][t]).max() < 1e-5
            assert np.abs(hidden[e].cpu().numpy() - g["h"][t]).max() < 1e-5


@pytest.mark.parametrize("seed", range(96))
def test_fused_actor_random_shapes(seed):
    """Shapes nobody listed: every input width up to 64 (ragged fc1 rows, agent id on or off), 1 ... 32 actions (fc2's padded tile,
    the all-thread arg-max), ragged and tiny batches, shared / per-agent weights, GRU in all three weight forms / the MLP layer --
    against the torch evaluation: 1e-5 on q and hidden, greedy actions equal where the top two values are 1e-4 apart."""
    fused_actor_random_shape(seed)


@pytest.mark.parametrize("A", [1, 5, 20, 32])
def test_greedy_action_is_a_valid_index_on_non_finite_rows(A):
    """Rows whose action values are all NaN, all -inf, or mixed: the greedy action is what torch.argmax gives (a NaN counts as the
    largest value, the first one wins; an all -inf row gives column 0) and ALWAYS an index in [0, A) -- the batched runner feeds it
    straight back into env.step and into gathers.  The non-finite values are put in through fc2's bias (per agent: non-shared
    weights), so every other stage of the kernel runs on ordinary numbers."""
    from marbler_amd.evaluate import BatchedActor
    dev = "cuda:0"
    N, H, D = 6, 64, 7
    sd = random_actor(N, D, H, A, True, 5)
    b2 = [k for k in sd if k.endswith("fc2.bias")]
    assert len(b2) == N, sorted(sd)
    nan, ninf = float("nan"), float("-inf")
    for a, k in enumerate(sorted(b2)):
        b = sd[k].clone()
        if a == 0:
            b[:] = nan                       # every column NaN
        elif a == 1:
            b[:] = ninf                      # every column -inf
        elif a == 2 and A > 2:
            b[A // 2] = nan                  # one NaN among finite values: it wins
        elif a == 3 and A > 2:
            b[:] = ninf
            b[A - 1] = -3.2e38               # below the old sentinel -3.0e38, but the only finite value
        elif a == 4 and A > 3:
            b[1] = nan
            b[A - 2] = nan                   # two NaNs: the first
        sd[k] = b
    actor = BatchedActor(sd, N, use_rnn=True, device=dev)
    g = torch.Generator(device=dev).manual_seed(3)
    E = 70
    hidden = torch.rand(E, N, H, generator=g, device=dev) * 2 - 1
    obs = torch.rand(E, N, D, generator=g, device=dev)
    q_ref, _ = actor.forward(obs, hidden.clone())
    q, act = actor.forward_fused(obs, hidden, append_agent_id=False)
    torch.cuda.synchronize()
    assert int(act.min()) >= 0 and int(act.max()) < A
    assert torch.equal(torch.isnan(q), torch.isnan(q_ref))
    want = q_ref.argmax(dim=2)
    for a in range(5):                       # the rows made non-finite: exactly torch's answer
        assert torch.equal(act[:, a].long(), want[:, a]), (a, act[:3, a], want[:3, a])


@pytest.mark.parametrize("shared,H,A,eps", [(True, 128, 5, 0.25), (False, 64, 20, 0.05), (True, 64, 5, 1.0), (True, 64, 32, 1e-6)])
def test_epsilon_greedy_selection_inside_the_launch(shared, H, A, eps):
    """rg_actor_forward_explore: the same launch with EPyMARL's epsilon-greedy selection folded in.  Everything but the actions is
    identical to the plain launch; the actions equal the rule in torch ops (evaluate.explore_select) applied to the plain launch's
    greedy actions and the same uniforms; the explored share is epsilon and the explored actions are uniform."""
    from marbler_amd import _lib
    from marbler_amd.evaluate import BatchedActor, explore_select
    dev = "cuda:0"
    E, N, D = 3000, 4, 9
    actor = BatchedActor(random_actor(1 if shared else N, D + N, H, A, True, 8), N, use_rnn=True, device=dev)
    g = torch.Generator(device=dev).manual_seed(11)
    hidden = torch.rand(E, N, H, generator=g, device=dev) * 2 - 1
    obs = torch.rand(E, N, D, generator=g, device=dev)
    u = torch.rand(E, N, generator=g, device=dev)
    u[0, 0], u[0, 1] = 0.0, float(np.nextafter(np.float32(1.0), np.float32(0.0)))    # the ends of the range
    h0, h1 = hidden.clone(), hidden.clone()
    q0, greedy = actor.forward_fused(obs, h0)
    q1, act = actor.forward_fused(obs, h1, explore_u=u, epsilon=eps)
    torch.cuda.synchronize()
    assert torch.equal(q0, q1) and torch.equal(h0, h1)
    want = explore_select(greedy, u, eps, A)
    assert torch.equal(act, want)
    assert int(act.min()) >= 0 and int(act.max()) < A
    assert int(act[0, 0]) == 0 and (eps == 1.0 or int(act[0, 1]) == int(greedy[0, 1]))
    explored = u < eps
    if eps >= 0.05:
        share = float(explored.float().mean())
        assert abs(share - eps) < 4 * (eps * (1 - eps) / (E * N)) ** 0.5 + 1e-3
        counts = torch.bincount(act[explored].long(), minlength=A).float()
        expect = float(explored.sum()) / A
        assert float(((counts - expect) ** 2 / expect).sum()) < 3 * A + 20      # chi-square, loose
    # what is not explored is the greedy action (the boundary u ~ epsilon is decided by the float32 product: skip one ulp of it)
    clear = (u >= eps * 1.0001) | (u <= eps * 0.9999)
    assert torch.equal(act[clear & ~explored], greedy[clear & ~explored])
    assert bool((act[clear & explored] == (u[clear & explored] / eps * A).floor().clamp(max=A - 1).int()).float().mean() > 0.999)
    # argument checks
    with pytest.raises(_lib.RobogymError):
        actor.forward_fused(obs, h1, explore_u=u, epsilon=0.0)
    with pytest.raises(ValueError):
        actor.forward_fused(obs, h1, explore_u=u[:, :2], epsilon=eps)


@pytest.mark.parametrize("shared,H,E,N,D,A", [(True, 128, 300, 5, 16, 5), (False, 64, 130, 5, 16, 5), (True, 64, 77, 4, 9, 20),
                                                (False, 128, 33, 3, 30, 7)])
def test_two_binary16_planes_match_torch_and_the_three_plane_form(shared, H, E, N, D, A):
    """gru_packed = 3 (rg_actor_pack_gru_f16x2): three plane products per float32 product.  Against torch's float32 evaluation to the
    same 1e-5 as every other form over a few recurrent steps, and against the three-bfloat16-plane form (error far below float32's
    own) to 3e-6 -- a float32 GEMM's own roundings are of that size."""
    from marbler_amd.evaluate import BatchedActor
    dev = "cuda:0"
    sd = random_actor(1 if shared else N, D + N, H, A, True, seed=H + E)
    fast, fine = (BatchedActor(sd, N, use_rnn=True, device=dev, pack_gru=p) for p in ("f16x2", "bf16x3"))
    g = torch.Generator(device=dev).manual_seed(2)
    hidden = torch.rand(E, N, H, generator=g, device=dev) * 2 - 1
    h_fine, h_ref = hidden.clone(), hidden.clone()
    eye = torch.eye(N, device=dev).unsqueeze(0).expand(E, N, N)
    worst = 0.0
    for step in range(4):
        obs = torch.rand(E, N, D, generator=g, device=dev) * 3 - 1.5
        q_ref, h_ref = fast.forward(torch.cat([obs, eye], dim=2), h_ref)
        q, act = fast.forward_fused(obs, hidden)
        q3, act3 = fine.forward_fused(obs, h_fine)
        torch.cuda.synchronize()
        assert float((q - q_ref).abs().max()) < 1e-5 and float((hidden - h_ref).abs().max()) < 1e-5, step
        worst = max(worst, float((q - q3).abs().max()), float((hidden - h_fine).abs().max()))
        top2 = q_ref.topk(2, dim=2).values
        clear = (top2[..., 0] - top2[..., 1]) > 1e-4
        assert torch.equal(act[clear], act3[clear])
    assert worst < 3e-6, worst


def test_two_binary16_planes_on_values_outside_binary16s_normal_range():
    """Activations and weights below 2^-14 (binary16's smallest normal number) travel in the scaled low plane alone; the result must
    not lose them: a network whose recurrent weights and hidden state are mostly tiny, against the three-plane form."""
    from marbler_amd.evaluate import BatchedActor
    dev = "cuda:0"
    E, N, D, H, A = 64, 4, 12, 128, 5
    sd = random_actor(1, D + N, H, A, True, seed=21)
    g0 = torch.Generator().manual_seed(4)
    for k in ("rnn.weight_hh", "rnn.weight_ih"):
        w = sd[k]
        tiny = torch.rand(w.shape, generator=g0) < 0.5
        scale = 10.0 ** (-4 - 4 * torch.rand(w.shape, generator=g0))       # 1e-4 ... 1e-8
        sd[k] = torch.where(tiny, w * scale, w)
    fast, fine = (BatchedActor(sd, N, use_rnn=True, device=dev, pack_gru=p) for p in ("f16x2", "bf16x3"))
    g = torch.Generator(device=dev).manual_seed(6)
    for amp in (1.0, 3e-5, 1e-7):
        hidden = (torch.rand(E, N, H, generator=g, device=dev) * 2 - 1) * amp
        # large recurrent products on purpose: tiny h x weights scaled UP would show a lost hi plane
        obs = torch.rand(E, N, D, generator=g, device=dev) * amp
        h2 = hidden.clone()
        q, _ = fast.forward_fused(obs, hidden)
        q3, _ = fine.forward_fused(obs, h2)
        torch.cuda.synchronize()
        assert float((q - q3).abs().max()) < 2e-6 and float((hidden - h2).abs().max()) < 2e-6, amp
    # the lost-plane check proper: gh = h W_hh with h ~ 3e-5 and W_hh ~ 3e3 (products of order 1 from operands below 2^-14)
    sd2 = dict(sd)
    sd2["rnn.weight_hh"] = sd["rnn.weight_hh"].sign() * 3e3 * torch.rand(sd["rnn.weight_hh"].shape, generator=g0)
    fast, fine = (BatchedActor(sd2, N, use_rnn=True, device=dev, pack_gru=p) for p in ("f16x2", "bf16x3"))
    hidden = (torch.rand(E, N, H, generator=g, device=dev) * 2 - 1) * 3e-5
    obs = torch.rand(E, N, D, generator=g, device=dev)
    h2 = hidden.clone()
    q, _ = fast.forward_fused(obs, hidden)
    q3, _ = fine.forward_fused(obs, h2)
    torch.cuda.synchronize()
    assert float((q - q3).abs().max()) < 1e-5 and float((hidden - h2).abs().max()) < 1e-5


def test_two_binary16_planes_saturate_beyond_binary16s_range_and_keep_nans():
    """An activation beyond 65 504 (here: a hidden unit of fc1 whose bias is 1e5, its weights zero) would convert to infinity and its
    low plane to NaN; the two-plane form saturates it instead -- the outputs are finite and bit-identical to those of the same
    network with that bias AT 65 504 -- and a NaN observation still gives NaN action values, in its own rows only."""
    from marbler_amd.evaluate import BatchedActor
    dev = "cuda:0"
    E, N, D, H, A = 40, 4, 12, 128, 5
    outs = []
    for bias in (1e5, 65504.0):
        sd = random_actor(1, D + N, H, A, True, seed=31)
        sd["fc1.weight"][3] = 0.0
        sd["fc1.bias"][3] = bias
        sd["rnn.weight_ih"][:, 3] *= 1e-3          # (keeps the gates' pre-activations in a range where the outputs still move)
        actor = BatchedActor(sd, N, use_rnn=True, device=dev, pack_gru="f16x2")
        g = torch.Generator(device=dev).manual_seed(8)
        hidden = torch.rand(E, N, H, generator=g, device=dev) * 2 - 1
        obs = torch.rand(E, N, D, generator=g, device=dev)
        q, act = actor.forward_fused(obs, hidden)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(q).all()) and bool(torch.isfinite(hidden).all()), bias
        outs.append((q.clone(), hidden.clone(), act.clone()))
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    obs[5, 2, 0] = float("nan")
    hidden = torch.rand(E, N, H, generator=g, device=dev) * 2 - 1
    q, act = actor.forward_fused(obs, hidden)
    torch.cuda.synchronize()
    bad = torch.isnan(q).any(dim=2)
    assert bool(bad[5, 2]) and int(bad.sum()) == 1
    assert int(act.min()) >= 0 and int(act.max()) < A


@pytest.mark.parametrize("entry", ["forward_fused", "unroll", "policy_rollout"])
def test_first_launch_on_a_side_stream_is_ordered_behind_the_weight_pack(entry):
    """The GRU matrices are packed once, by two kernels queued on the stream that is current when the weights struct is first
    built.  A first launch on ANOTHER stream must be ordered behind them (BatchedActor.weights_for): a freshly constructed actor,
    its pack queued on the current stream behind a few large products, goes straight to a side stream through each entry that
    takes the weights, and must give, bit for bit, what an actor that was packed and synchronised first gives for the same call.
    The memory the unsynchronised actor packs into must not already hold the answer: the reference actor stays alive until the
    comparison (its packed planes are not handed out again), a decoy actor of the same shapes and OTHER weights is packed and
    dropped right before (what the allocator hands out next holds the decoy's planes), and each entry has its own weights.
    A guard, not a proof: a launch that missed the wait would read weights that are not packed yet, which shows as wrong values
    (never as a fault) -- unless the pack happened to finish first, and then the test passes by luck."""
    from marbler_amd.evaluate import BatchedActor
    from marbler_amd.gymma import BatchedRunner, GymmaVecEnv
    dev = torch.device("cuda:0")
    E, N, D, H, A, T = 8, 3, 5, 64, 6, 2
    g = torch.Generator().manual_seed(11)
    obs = (torch.rand(E, 3, N, D, generator=g) * 3 - 1.5).to(dev)                 # unroll: B = 8 episodes of 3 rows
    hidden0 = (torch.rand(E, N, H, generator=g) * 2 - 1).to(dev)
    obs0 = obs[:, 0].contiguous()
    busy = torch.rand(4096, 4096, device=dev)
    side = torch.cuda.Stream(device=dev)

    seed = {"forward_fused": 3, "unroll": 13, "policy_rollout": 23}[entry]

    def call(synchronised, seed):
        """-> (the outputs, the actor: whoever holds it keeps its packed planes from being handed out again)"""
        v = GymmaVecEnv("robotarium_gym:PredatorCapturePrey-v0", E, time_limit=10, seed=5) if entry == "policy_rollout" else None
        n, width, n_act = (v.n_agents, v.obs_size + v.n_agents, v.n_actions) if v is not None else (N, D + N, A)
        actor = BatchedActor(random_actor(1, width, H, n_act, True, seed=seed), n, device=dev)
        runner = BatchedRunner(v, actor, seed=9) if v is not None else None
        hidden = hidden0.clone()
        torch.cuda.synchronize()
        if not synchronised:
            for _ in range(4):                      # the pack kernels queue up behind these
                torch.mm(busy, busy)
        actor._weights_struct()
        if synchronised:
            torch.cuda.synchronize()
        if entry == "forward_fused":
            q, act = actor.forward_fused(obs0, hidden, stream=side)
            out = [q, act, hidden]
        elif entry == "unroll":
            h_out = torch.empty_like(hidden)
            q, act = actor.unroll(obs, hidden=hidden, hidden_out=h_out, stream=side)
            out = [q, act, h_out]
        else:
            with torch.cuda.stream(side):           # (the env's handle launches on torch's current stream)
                batch = runner.run(T, one_launch=True)
            out = [batch[k] for k in ("obs", "actions", "reward", "terminated")] + [runner.hidden]
        torch.cuda.synchronize()
        out = [t.clone() for t in out]
        if v is not None:
            v.close()
        return out, actor

    want, reference = call(True, seed)
    decoy, _ = call(True, seed + 1)
    del _                                           # the decoy's planes go back to the allocator; the reference's stay out
    got, _ = call(False, seed)
    assert reference._ws is not None and len(want) == len(got) and all(torch.equal(a, b) for a, b in zip(want, got))
    assert bool(torch.isfinite(want[0]).all()) and bool(want[0].abs().sum() > 0)
    assert not all(torch.equal(a, b) for a, b in zip(want, decoy))             # (other weights do give other values)
