"""Torch-side helpers shared by the GPU test modules, the soak scripts and tools/ (no test module imports another)."""
import numpy as np
import pytest
import torch

from marbler_amd.gymma import N_ACTIONS

SENTINEL = 0xA5
ZONE = 1024
# what the row-kernel tests stack per step (the results of env.step, then qp_sweeps), and the state and statistics arrays of the
# scenarios that have row kernels
STEP_OUTS = ("obs", "reward", "done", "dist_travelled", "violation", "remaining", "qp_sweeps")
ROW_STATE = ("poses", "carry_dist", "episode_steps", "reset_count", "prey_loc", "prey_sensed", "prey_captured", "loaded", "load",
             "zone_load", "messages", "ep_return", "done_return_sum", "done_count", "done_steps_sum")


@pytest.fixture(autouse=True)
def lane_group_kernel(monkeypatch):
    """Imported by the modules whose every test runs the lane-group kernel (an imported fixture belongs to the importing module)."""
    monkeypatch.setenv("RG_STEP_KERNEL", "group")


def same_bits(a, b):
    """torch.equal on the words: float32 as int32, everything else as it is."""
    a, b = (t.detach().cpu().contiguous() for t in (a, b))
    return torch.equal(*(t.view(torch.int32) if t.dtype == torch.float32 else t for t in (a, b)))


def random_actions(env, T, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randint(0, N_ACTIONS[env.scenario], (T, env.E, env.N), generator=g, dtype=torch.int32).to(env.device)


def random_actor(n_sets, I, H, A, use_rnn, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: (torch.rand(*s, generator=g) * 2 - 1) * 0.3  # noqa: E731
    sd = {}
    for i in range(n_sets):
        pre = f"agents.{i}." if n_sets > 1 else ""
        sd[pre + "fc1.weight"], sd[pre + "fc1.bias"] = r(H, I), r(H)
        if use_rnn:
            sd[pre + "rnn.weight_ih"], sd[pre + "rnn.weight_hh"] = r(3 * H, H), r(3 * H, H)
            sd[pre + "rnn.bias_ih"], sd[pre + "rnn.bias_hh"] = r(3 * H), r(3 * H)
        else:
            sd[pre + "rnn.weight"], sd[pre + "rnn.bias"] = r(H, H), r(H)
        sd[pre + "fc2.weight"], sd[pre + "fc2.bias"] = r(A, H), r(A)
    return sd


def draw_actor_case(rng):
    H = int(rng.choice([64, 128]))
    shared = bool(rng.rand() < 0.6)
    N = int(rng.randint(1, 9))
    append = bool(rng.rand() < 0.6)
    D = int(rng.randint(1, 64 - (N if append else 0) + 1))          # input width D (+ N) <= 64
    A = int(rng.choice([1, 2, 5, 7, 20, 31, 32]))
    E = int(rng.choice([1, 2, 31, 32, 33, 100, 257]))
    use_rnn = bool(rng.rand() < 0.8)
    pack = [True, "f32", False][int(rng.randint(0, 3))]
    if rng.rand() < 0.4:     # (drawn after everything else: the cases of earlier rounds keep their shapes)
        pack = "f16x2" if pack is True else "bf16x3" if pack == "f32" else pack
    return shared, H, E, N, D, A, use_rnn, append, pack


def fused_actor_random_shape(seed):
    """One draw of tests/test_gpu_actor.py::test_fused_actor_random_shapes (tests/actor_soak.py runs many more)."""
    from marbler_amd.evaluate import BatchedActor
    rng = np.random.RandomState(7000 + seed)
    shared, H, E, N, D, A, use_rnn, append, pack = draw_actor_case(rng)
    dev = "cuda:0"
    I = D + (N if append else 0)
    actor = BatchedActor(random_actor(1 if shared else N, I, H, A, use_rnn, seed), N, use_rnn=use_rnn, device=dev, pack_gru=pack)
    g = torch.Generator(device=dev).manual_seed(seed)
    hidden = torch.rand(E, N, H, generator=g, device=dev) * 2 - 1
    h_ref = hidden.clone()
    eye = torch.eye(N, device=dev).unsqueeze(0).expand(E, N, N)
    for step in range(2):
        obs = torch.rand(E, N, D, generator=g, device=dev) * 3 - 1.5
        restart = (torch.rand(E, generator=g, device=dev) < 0.3).to(torch.uint8)
        fresh = restart.bool()[:, None, None]
        obs_seen = torch.where(fresh, torch.zeros_like(obs), obs)
        q_ref, h_ref = actor.forward(torch.cat([obs_seen, eye], dim=2) if append else obs_seen, torch.where(fresh, torch.zeros_like(h_ref), h_ref))
        q, act = actor.forward_fused(obs, hidden, append_agent_id=append, restart=restart)
        torch.cuda.synchronize()
        case = (shared, H, E, N, D, A, use_rnn, append, pack, step)
        assert float((q - q_ref).abs().max()) < 1e-5, case
        assert float((hidden - h_ref).abs().max()) < 1e-5, case
        if A > 1:
            top2 = q_ref.topk(2, dim=2).values
            clear = (top2[..., 0] - top2[..., 1]) > 1e-4
            assert torch.equal(act[clear].long(), q_ref.argmax(dim=2)[clear]), case
        else:
            assert int(act.abs().sum()) == 0, case


def rollout_equals_single_steps(s, r, acts, more_state=()):
    """`r` through one rg_rollout launch, its twin `s` through single steps: every output of every step, then the state.  -> the rollout"""
    out = r.rollout(acts)
    for t in range(len(acts)):
        s.step(acts[t])
        for k in ("obs", "reward", "done_u8", "dist_travelled", "violation", "remaining"):
            assert same_bits(getattr(s, k), out["done" if k == "done_u8" else k][t]), (t, k)
    for k in s.STATE_KEYS + tuple(more_state):
        assert same_bits(getattr(s, k), getattr(r, k)), k
    return out


def runner_batch_replays(out, key, E, T, ov, columns=slice(None)):
    """A BatchedRunner batch `out` against a twin gymma env stepped with the recorded actions: terminations and observations."""
    from marbler_amd.gymma import GymmaVecEnv
    w = GymmaVecEnv(key, E, time_limit=5, seed=3, overrides=ov)
    w.reset()
    for t in range(T):
        _, ended, _ = w.step(out["actions"][t])
        obs = w.get_obs()
        torch.cuda.synchronize()
        assert torch.equal(ended, out["terminated"][t])
        assert torch.equal(obs[..., columns], out["obs"][t + 1][..., columns]) and torch.equal(obs, out["obs"][t + 1])


def runners_agree(r1, r2):
    """(GymmaVecEnv, BatchedRunner) twice: the actors' recurrent state, what the envs show next, statistics and whole state."""
    (v1, a), (v2, b) = r1, r2
    torch.cuda.synchronize()
    assert torch.equal(a.hidden, b.hidden) and torch.equal(a._restart, b._restart)
    assert torch.equal(v1.get_obs(), v2.get_obs()) and torch.equal(v1._ended, v2._ended)
    assert torch.equal(v1.env.done_count, v2.env.done_count)
    assert v1.get_stats() == v2.get_stats()
    s1, s2 = v1.env.state_dict(), v2.env.state_dict()
    for k in s1:
        assert torch.equal(s1[k], s2[k]), k


def differing(a, b, keys):
    """The names among `keys` of the arrays of two handles that differ in any word (compared on the device)."""
    return [k for k in keys if not torch.equal(getattr(a, k).contiguous().view(torch.uint8), getattr(b, k).contiguous().view(torch.uint8))]


def expected_slots(N, E):
    """wave_fill's rule (csrc/launch_plan.h), restated: halve the env slots per wave while the batch still fits 1024 waves."""
    gw = 4 if N <= 4 else 8 if N <= 8 else 16
    epw = 64 // gw
    while epw >= 2 and (E + epw // 2 - 1) // (epw // 2) <= 1024:
        epw //= 2
    return epw


def guarded_class():
    from marbler_amd import VecRobotariumEnv

    class GuardedEnv(VecRobotariumEnv):
        """All arrays from one slab, red zones between them."""

        def __init__(self, *a, slab_bytes=1 << 26, **kw):
            dev = torch.device(kw.get("device", "cuda:0"))
            self._slab = torch.full((slab_bytes,), SENTINEL, dtype=torch.uint8, device=dev)
            self._cursor = 0
            self._regions = []
            super().__init__(*a, **kw)

        def _alloc(self, shape, dtype, fill=0):
            nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
            lo = (self._cursor + ZONE + 255) // 256 * 256
            hi = lo + nbytes
            if hi + ZONE > self._slab.numel():
                raise MemoryError("guard slab too small")
            self._cursor = hi
            self._regions.append((lo, hi))
            t = self._slab[lo:hi].view(dtype).view(tuple(shape))
            t.fill_(fill)
            return t

        def _alloc_outputs(self):   # one array each (the product packs them into one arena, 16-byte aligned, no gaps)
            E, N, D = self.E, self.N, self.D
            f32, i32, u8 = torch.float32, torch.int32, torch.uint8
            self.obs = self._alloc((E, N, D), f32)
            self.reward = self._alloc((E, N), f32)
            self.dist_travelled = self._alloc((E, N), f32)
            self.remaining = self._alloc((E,), i32, fill=-1)
            self.done_u8 = self._alloc((E,), u8)
            self.done = self.done_u8.view(torch.bool)
            self.violation = self._alloc((E,), u8)
            self._out_arena, self._out_offsets = None, {}

        def red_zones_intact(self):
            keep = torch.ones(self._slab.numel(), dtype=torch.bool, device=self._slab.device)
            for lo, hi in self._regions:
                keep[lo:hi] = False
            bad = torch.nonzero(keep & (self._slab != SENTINEL)).flatten()
            return bad.cpu().numpy()

        def owner_of(self, off):
            """Nearest array below a damaged byte (diagnostics)."""
            names = {}
            for k, v in self.__dict__.items():
                if isinstance(v, torch.Tensor) and v.device == self._slab.device and v.untyped_storage().data_ptr() == self._slab.untyped_storage().data_ptr():
                    names[v.data_ptr() - self._slab.data_ptr()] = k
            below = [o for o in names if o <= off]
            return names[max(below)] if below else "<slab start>"

    return GuardedEnv


def fused_time_limit_vs_composed(key, ov, n_act, limit, E, steps):
    """(RG_STEP_KERNEL is the caller's business.)"""
    from marbler_amd.gymma import GymmaVecEnv
    a = GymmaVecEnv(key, E, time_limit=limit, overrides=ov, seed=5, fused=True)
    b = GymmaVecEnv(key, E, time_limit=limit, overrides=ov, seed=5, fused=False)
    assert a.env.time_limit == limit and b.env.time_limit == 0
    a.reset()
    b.reset()
    g = torch.Generator(device=a.env.device)
    g.manual_seed(3)
    n_trunc = n_done = 0
    for t in range(steps):
        act = torch.randint(0, n_act, (E, a.n_agents), generator=g, device=a.env.device, dtype=torch.int32)
        ra, ta, ia = a.step(act)
        rb, tb, ib = b.step(act)
        assert torch.equal(ta, tb) and torch.equal(ia["TimeLimit.truncated"], ib["TimeLimit.truncated"]), t
        assert torch.allclose(ra, rb, rtol=0, atol=1e-5), t
        assert torch.equal(a.get_obs().view(torch.int32), b.get_obs().view(torch.int32)), t
        assert torch.equal(a.get_state(), a.get_obs().reshape(E, -1))
        for k in ("violation", "remaining", "dist_travelled"):
            assert torch.equal(ia[k], ib[k]), (t, k)
        assert torch.equal(a.env.poses.view(torch.int32), b.env.poses.view(torch.int32)), t
        assert torch.equal(a.env.episode_steps, b.env.episode_steps) and torch.equal(a.env.reset_count, b.env.reset_count)
        n_trunc += int(ia["TimeLimit.truncated"].sum())
        n_done += int(ta.sum())
    sa, sb = a.get_stats(), b.get_stats()
    assert sa["episodes"] == sb["episodes"] == n_done and sa["steps"] == sb["steps"]
    assert abs(sa["return_sum"] - sb["return_sum"]) < 1e-3 * max(1.0, abs(sb["return_sum"]))
    assert n_done > E // 2 and (n_trunc > E if limit < 50 else n_trunc == 0)
    a.close()
    b.close()
