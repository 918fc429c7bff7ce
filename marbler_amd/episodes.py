"""Episode buffer: BatchedRunner.run(T)'s time-major stream as episode-major batches padded to episode_limit + 1, the layout of
EPyMARL's EpisodeBatch / ReplayBuffer, kept on the device and filled by one HIP launch per collection (rg_episodes_append,
include/robogym.h).

    buf = EpisodeBuffer.for_runner(runner)          # E x 2 slots of episode_limit + 1 rows, allocated once
    runner.run(64, one_launch=True, into=buf)       # collect, then ONE launch cuts the stream into the slots
    new = buf.take_new()                            # the slots completed since the last call
    batch = buf.batch(new)                          # obs [B, L + 1, N, D], actions, reward, terminated, filled, ...

The rule -- where an episode opens, which row takes what, what happens to an episode that is cut off or does not fit -- is
stated once in csrc/episodes.h and DESIGN.md section 4 "Episode buffer".  There is no host path: append() needs the library and a
HIP device.
"""
import ctypes as C

import torch

from . import _args, _lib

# name -> (dtype name, shape as a function of (E, R, L, N, D)); `prob` only with with_prob
ARRAYS = {"obs": ("float32", lambda E, R, L, N, D: (E * R, L + 1, N, D)),
          "actions": ("int32", lambda E, R, L, N, D: (E * R, L + 1, N)),
          "reward": ("float32", lambda E, R, L, N, D: (E * R, L + 1)),
          "terminated": ("uint8", lambda E, R, L, N, D: (E * R, L + 1)),
          "filled": ("uint8", lambda E, R, L, N, D: (E * R, L + 1)),
          "prob": ("float32", lambda E, R, L, N, D: (E * R, L + 1, N)),
          "length": ("int32", lambda E, R, L, N, D: (E * R,)),
          "episode_return": ("float32", lambda E, R, L, N, D: (E * R,)),
          "complete": ("uint8", lambda E, R, L, N, D: (E * R,)),
          "fresh": ("uint8", lambda E, R, L, N, D: (E * R,)),
          "episode_index": ("int32", lambda E, R, L, N, D: (E * R,)),
          "cursor": ("int32", lambda E, R, L, N, D: (E, 4))}
INT32_MAX = 2 ** 31 - 1


class EpisodeBuffer(object):
    """E x slots_per_env episode slots of episode_limit + 1 rows on `device`; all storage is allocated here, zero-filled, and
    nothing is allocated afterwards by append().  Slot e * slots_per_env + r is env e's r-th ring entry: an env's episodes go
    round its own ring, so with slots_per_env = 2 the episode an env has just completed stays readable while its next one fills.
    storage: the arrays themselves (name -> tensor, ARRAYS' dtypes and shapes, contiguous), for a caller that owns the memory."""

    def __init__(self, num_envs, n_agents, obs_dim, n_actions, episode_limit, slots_per_env=2, with_prob=False, device="cuda:0",
                 storage=None):
        dims = {"num_envs": num_envs, "n_agents": n_agents, "obs_dim": obs_dim, "n_actions": n_actions,
                "episode_limit": episode_limit, "slots_per_env": slots_per_env}
        for k, v in dims.items():
            if isinstance(v, bool) or not isinstance(v, int):
                raise TypeError(f"{k} must be an int, got {v!r}")
            if v < 1:
                raise ValueError(f"{k} must be >= 1, got {v}")
        self.E, self.N, self.D, self.A = num_envs, n_agents, obs_dim, n_actions
        self.L, self.R = episode_limit, slots_per_env
        self.with_prob = bool(with_prob)
        self.device = torch.device(device)
        if self.E * self.R * (self.L + 1) * self.N * self.D > INT32_MAX:
            raise ValueError("num_envs * slots_per_env * (episode_limit + 1) * n_agents * obs_dim exceeds 2^31 - 1 elements")
        shape_args = (self.E, self.R, self.L, self.N, self.D)
        self.names = tuple(k for k in ARRAYS if k != "prob" or self.with_prob)
        if storage is None:
            storage = {k: torch.zeros(ARRAYS[k][1](*shape_args), dtype=getattr(torch, ARRAYS[k][0]), device=self.device)
                       for k in self.names}
            storage["cursor"][:, 0] = -1           # no env has an open episode
        elif set(storage) != set(self.names):
            raise ValueError(f"storage must hold exactly {self.names}, got {tuple(storage)}")
        for k in self.names:
            _args.check_tensor(f"storage[{k!r}]", storage[k], (getattr(torch, ARRAYS[k][0]),), ARRAYS[k][1](*shape_args), self.device)
            setattr(self, k, storage[k])
        if not self.with_prob:
            self.prob = None
        self._c_buffer = _lib.RgEpisodeBuffer(
            self.obs.data_ptr(), self.actions.data_ptr(), self.reward.data_ptr(), self.terminated.data_ptr(), self.filled.data_ptr(),
            self.prob.data_ptr() if self.with_prob else None, self.length.data_ptr(), self.episode_return.data_ptr(),
            self.complete.data_ptr(), self.fresh.data_ptr(), self.episode_index.data_ptr(), self.cursor.data_ptr(),
            self.E, self.R, self.L, self.N, self.D, 0)

    @classmethod
    def for_runner(cls, runner, slots_per_env=2):
        """A buffer that fits `runner` (a BatchedRunner): its venv's shapes and episode limit, `prob` if it samples soft policies."""
        v = runner.venv
        soft = runner.action_selector == "soft_policies" and not runner.test_mode
        return cls(v.E, v.n_agents, v.obs_size, v.n_actions, v.episode_limit, slots_per_env=slots_per_env, with_prob=soft,
                   device=v.env.device)

    @property
    def num_slots(self):
        return self.E * self.R

    # -- filling
    def check_fits(self, num_envs, n_agents, obs_dim, episode_limit, with_prob):
        """ValueError unless a collector of these shapes can append to this buffer (BatchedRunner.run(into=) asks before it
        collects): the same E, N, D, an episode limit the slots can hold, the same `prob` setting."""
        for name, have, want in (("num_envs", self.E, num_envs), ("n_agents", self.N, n_agents), ("obs_dim", self.D, obs_dim)):
            if have != want:
                raise ValueError(f"the buffer was built for {name} = {have}, the collector has {want}")
        if self.L < episode_limit:
            raise ValueError(f"the buffer's episode_limit {self.L} is below the collector's {episode_limit}: its episodes would overflow")
        if self.with_prob != bool(with_prob):
            raise ValueError("the buffer was built with_prob=%s, the collector %s `prob`" %
                             (self.with_prob, "returns" if with_prob else "does not return"))

    def check_stream(self, batch):
        """batch: run()'s dict.  Checks names, dtypes, shapes, contiguity and devices; returns T.  Touches no device."""
        if not isinstance(batch, dict):
            raise TypeError("batch must be the dict BatchedRunner.run returns")
        need = ("obs", "actions", "reward", "terminated", "episode_start")
        missing = [k for k in need if k not in batch]
        if missing:
            raise ValueError(f"batch lacks {missing}")
        if self.with_prob and batch.get("prob") is None:
            raise ValueError("the buffer was built with_prob=True, the batch has no 'prob'")
        if not self.with_prob and batch.get("prob") is not None:
            raise ValueError("the batch has 'prob', the buffer was built with_prob=False")
        if not isinstance(batch["actions"], torch.Tensor) or batch["actions"].dim() != 3 or batch["actions"].shape[0] < 1:
            raise ValueError("batch['actions'] must be a tensor [T, E, N] with T >= 1")
        T = int(batch["actions"].shape[0])
        if (T + 1) * self.E * self.N * self.D > INT32_MAX:
            raise ValueError("(T + 1) * num_envs * n_agents * obs_dim exceeds 2^31 - 1 elements")
        f32, flags = (torch.float32,), (torch.bool, torch.uint8)
        for k, dtypes, shape in (("obs", f32, (T + 1, self.E, self.N, self.D)), ("actions", (torch.int32,), (T, self.E, self.N)),
                                 ("reward", f32, (T, self.E)), ("terminated", flags, (T, self.E)), ("episode_start", flags, (T, self.E)),
                                 ("prob", f32, (T, self.E, self.N))):
            if k != "prob" or self.with_prob:
                _args.check_tensor(f"batch[{k!r}]", batch[k], dtypes, shape, self.device)
        return T

    def append(self, batch, stream=None):
        """Cut run()'s dict into the slots: one launch on `stream` (a torch stream; None: the current one), no host
        synchronisation, nothing allocated -- safe inside a torch.cuda.graph capture.  Returns nothing."""
        T = self.check_stream(batch)
        if self.device.type != "cuda":
            raise ValueError(f"the buffer lives on {self.device}: append() runs on a HIP device and has no host path")
        lib = _lib.load()
        s = _lib.RgEpisodeStream(batch["obs"].data_ptr(), batch["actions"].data_ptr(), batch["reward"].data_ptr(),
                                 batch["terminated"].data_ptr(), batch["episode_start"].data_ptr(),
                                 batch["prob"].data_ptr() if self.with_prob else None, T, 0)
        with torch.cuda.device(self.device):
            rc = lib.rg_episodes_append(C.byref(self._c_buffer), C.byref(s), _args.launch_stream(stream, self.device)[1])
        if rc != 0:
            raise _args.launch_error(rc, "rg_episodes_append: " + lib.rg_episodes_last_error().decode(), refuses=False)

    # -- reading
    def take_new(self):
        """The slots completed since the last call: int64, ascending.  Clears `fresh`."""
        new = torch.nonzero(self.fresh).flatten()
        self.fresh.zero_()
        return new

    def _slots(self, slots):
        if slots is None:
            return torch.nonzero(self.complete).flatten()
        if isinstance(slots, torch.Tensor):
            if slots.dtype not in (torch.int64, torch.int32):
                raise ValueError(f"slots must be an int64 or int32 tensor, got {slots.dtype}")
            if slots.dim() != 1:
                raise ValueError(f"slots must be one-dimensional, got {tuple(slots.shape)}")
            if slots.device.type == "cpu":
                host = slots.tolist()
            else:
                return slots.to(device=self.device, dtype=torch.int64)    # device data: taken as it is (torch checks the index)
        else:
            try:
                host = [int(v) for v in slots]
            except TypeError:
                raise ValueError(f"slots must be None, an int tensor or a sequence of ints, got {slots!r}") from None
        bad = [v for v in host if not 0 <= v < self.num_slots]
        if bad:
            raise ValueError(f"slots {bad[:4]} outside [0, {self.num_slots})")
        return torch.tensor(host, dtype=torch.int64).to(self.device)

    def _select(self, slots, trim, min_rows):
        """(idx, B, rows, length) of a read of `slots`: their indices, how many, and the rows of the time axis -- L + 1, or under
        `trim` those of the longest episode selected (one host read), at least `min_rows`.  length: the slots' lengths where
        trimming gathered them, else None (only batch() returns them: nothing is gathered twice, or for nobody)."""
        idx = self._slots(slots)
        B, rows, length = int(idx.numel()), self.L + 1, None
        if trim and B > 0:
            length = self.length[idx]
            rows = max(int(length.max()) + 1, min_rows)
        return idx, B, rows, length

    def _check_fits(self, actor, obs_agent_id, mixer=None):
        """ValueError unless `actor` (a BatchedActor) and `mixer` (a targets.TargetMixer, if given) fit this buffer's episodes."""
        fits = [("actor's n_agents", getattr(actor, "n_agents", None), self.N), ("actor's n_actions", getattr(actor, "n_actions", None), self.A),
                ("actor's input_dim", getattr(actor, "input_dim", None), self.D + (self.N if obs_agent_id else 0))]
        if mixer is not None:
            fits.append(("mixer's n_agents", mixer.n_agents, self.N))
            if mixer.kind == "qmix":
                fits.append(("mixer's state_dim", mixer.state_dim, self.N * self.D))
        for name, have, want in fits:
            if have != want:
                raise ValueError(f"the {name} is {have}, the buffer's episodes need {want}")
        if actor.w1.device != self.device:
            raise ValueError(f"the actor is on {actor.w1.device}, the buffer on {self.device}")
        if mixer is not None and mixer.device != self.device:
            raise ValueError(f"the mixer is on {mixer.device}, the buffer on {self.device}")

    def batch(self, slots=None, trim=False):
        """EPyMARL's episode batch of `slots` (None: every complete slot, ascending), B episodes: obs [B, L + 1, N, D], state
        [B, L + 1, N D] (gymma's state is the concatenated observations), actions [B, L + 1, N, 1] int64, avail_actions
        [B, L + 1, N, A] int32 ones, reward [B, L + 1, 1], terminated [B, L + 1, 1] uint8, filled [B, L + 1, 1] int64, probs
        [B, L + 1, N] (a buffer with_prob), length [B] int32, episode_return [B].  trim: the time axis is cut to the longest
        episode selected, max(length) + 1 rows (one host read)."""
        idx, B, rows, length = self._select(slots, trim, 1)
        obs = self.obs[idx, :rows]
        out = {"obs": obs, "state": obs.reshape(B, rows, self.N * self.D),
               "actions": self.actions[idx, :rows].to(torch.int64).unsqueeze(-1),
               "avail_actions": torch.ones(B, rows, self.N, self.A, dtype=torch.int32, device=self.device),
               "reward": self.reward[idx, :rows].unsqueeze(-1),
               "terminated": self.terminated[idx, :rows].unsqueeze(-1),
               "filled": self.filled[idx, :rows].to(torch.int64).unsqueeze(-1),
               "length": self.length[idx] if length is None else length, "episode_return": self.episode_return[idx]}
        if self.with_prob:
            out["probs"] = self.prob[idx, :rows]
        return out

    def unroll(self, actor, slots=None, trim=False, obs_agent_id=True):
        """A learner's first pass over batch(slots, trim): `actor` (a BatchedActor) from a zero hidden state over every row of
        every selected episode, in ONE launch (BatchedActor.unroll; the rule: csrc/actor_unroll.h).  Returns q [B, rows, N, A]
        and greedy [B, rows, N] int32 over the same rows as batch(slots, trim).  Every row is computed, the padding behind an
        episode's end included (there are no masks: `filled` says which rows are data); q of the taken action and max q stay
        torch.gather / max on q.  ValueError for an actor that does not fit the buffer or that the launch refuses."""
        self._check_fits(actor, obs_agent_id)
        idx, B, rows, _ = self._select(slots, trim, 1)
        if B == 0:
            return {"q": torch.empty(0, rows, self.N, self.A, device=self.device),
                    "greedy": torch.empty(0, rows, self.N, dtype=torch.int32, device=self.device)}
        q, greedy = actor.unroll(self.obs[idx][:, :rows], append_agent_id=obs_agent_id)   # (the gathered copy is read in place)
        return {"q": q, "greedy": greedy}

    def td_targets(self, target_actor, mixer, greedy=None, slots=None, trim=False, gamma=0.99, obs_agent_id=True):
        """Everything a Q-learner computes under detach() for batch(slots, trim), in two launches: `target_actor` (a BatchedActor)
        unrolled over the selected episodes (BatchedActor.unroll), then the episode mask, the double-Q gather, `mixer` (a
        targets.TargetMixer) and reward + gamma (1 - terminated) mixed (targets.td_targets; the rule: csrc/td_targets.h), both on
        ONE gathered copy of the slots' observations.  greedy: unroll(online_actor)["greedy"] over the same slots and trim, which
        is double-Q; None: the target network's own maximum.  Returns targets [B, rows - 1, 1] (a `none` mixer:
        [B, rows - 1, N]), mask [B, rows - 1, 1] and agent_q [B, rows - 1, N] over the rows of batch(slots, trim)[:, :-1].
        ValueError for an actor, a mixer or a `greedy` that does not fit the buffer or that a launch refuses."""
        from . import targets
        if not isinstance(mixer, targets.TargetMixer):
            raise ValueError(f"mixer must be a TargetMixer, got {type(mixer).__name__}")
        self._check_fits(target_actor, obs_agent_id, mixer)
        idx, B, rows, _ = self._select(slots, trim, 2)
        if greedy is not None:      # (unroll(online_actor)["greedy"] of the same slots and trim has this shape)
            _args.check_tensor("greedy", greedy, (torch.int32,), (B, rows, self.N), contiguous=False, errors=_args.VALUE)
        if B == 0:
            t_shape = (0, rows - 1, self.N if mixer.kind == "none" else 1)
            return {"targets": torch.empty(t_shape, device=self.device), "mask": torch.empty(0, rows - 1, 1, device=self.device),
                    "agent_q": torch.empty(0, rows - 1, self.N, device=self.device)}
        obs = self.obs[idx][:, :rows]                             # the one gathered copy both launches read in place
        qt, _ = target_actor.unroll(obs, append_agent_id=obs_agent_id)
        out = targets.td_targets(qt, obs, self.reward[idx][:, :rows], self.terminated[idx][:, :rows], self.filled[idx][:, :rows],
                                 mixer, gamma, sel=greedy)
        return {"targets": out["targets"] if mixer.kind == "none" else out["targets"].unsqueeze(-1),
                "mask": out["mask"].unsqueeze(-1), "agent_q": out["agent_q"]}

    def mixed_q(self, mixer, q, mask, slots=None, trim=False):
        """The online mixer's pass over batch(slots, trim) with gradients: `mixer` (a mixers.TrainableMixer) on q [B, rows, N, A]
        (TrainableActor's output over the same slots and trim) with the buffer's own actions and observations of the selected
        slots, and mask [B, rows - 1] or [B, rows - 1, 1] (td_targets' mask).  Returns mixed [B, rows - 1, 1] (a `none` mixer:
        [B, rows - 1, N]) with a graph through q and the mixer's parameters (the rule: csrc/mixer_grad.h).  ValueError for a mixer
        that does not fit the buffer, or a q or mask that does not fit the selection."""
        from . import mixers
        if not isinstance(mixer, mixers.TrainableMixer):
            raise ValueError(f"mixer must be a TrainableMixer, got {type(mixer).__name__}")
        fits = [("mixer's n_agents", mixer.n_agents, self.N)] + ([("mixer's state_dim", mixer.state_dim, self.N * self.D)] if mixer.kind == "qmix" else [])
        for name, have, want in fits:
            if have != want:
                raise ValueError(f"the {name} is {have}, the buffer's episodes need {want}")
        idx, B, rows, _ = self._select(slots, trim, 2)
        _args.check_tensor("q", q, (torch.float32,), (B, rows, self.N, self.A), contiguous=False, errors=_args.VALUE)
        if not isinstance(mask, torch.Tensor) or tuple(mask.shape) not in ((B, rows - 1), (B, rows - 1, 1)):
            raise ValueError(f"mask must be a tensor {(B, rows - 1)} or {(B, rows - 1, 1)}, got {tuple(getattr(mask, 'shape', ()))}")
        if B == 0:
            return torch.empty(0, rows - 1, self.N if mixer.kind == "none" else 1, device=self.device)
        mixed = mixer(q, self.actions[idx, :rows], self.obs[idx][:, :rows], mask)
        return mixed if mixer.kind == "none" else mixed.unsqueeze(-1)

    def nstep_returns(self, target_critic, slots=None, trim=False, gamma=0.99, nstep=10, add_value_last_step=True, value_scale=1.0,
                      value_shift=0.0, reward=None):
        """Everything a PPO learner computes under no_grad for batch(slots, trim), in one launch: the episode mask, `target_critic`
        (a returns.TargetCritic) over every needed row, and the n-step returns (returns.nstep_returns; the rule:
        csrc/nstep_returns.h).  reward: an optional [B, rows] float32 replacement for the slots' rewards (a learner that
        standardises rewards), over the same rows as batch(slots, trim).  Returns returns [B, rows - 1, N], values [B, rows, N] and
        mask [B, rows - 1, 1].  ValueError for a critic or a `reward` that does not fit the buffer or that the launch refuses."""
        from . import returns
        if not isinstance(target_critic, returns.TargetCritic):
            raise ValueError(f"target_critic must be a TargetCritic, got {type(target_critic).__name__}")
        for name, have, want in (("critic's n_agents", target_critic.n_agents, self.N), ("critic's state_dim", target_critic.state_dim, self.N * self.D)):
            if have != want:
                raise ValueError(f"the {name} is {have}, the buffer's episodes need {want}")
        if target_critic.device != self.device:
            raise ValueError(f"the critic is on {target_critic.device}, the buffer on {self.device}")
        idx, B, rows, _ = self._select(slots, trim, 2)
        if reward is not None:
            _args.check_tensor("reward", reward, (torch.float32,), (B, rows), self.device, contiguous=False, errors=_args.VALUE)
        if B == 0:
            return {"returns": torch.empty(0, rows - 1, self.N, device=self.device), "values": torch.empty(0, rows, self.N, device=self.device),
                    "mask": torch.empty(0, rows - 1, 1, device=self.device)}
        cut = lambda x: x[idx][:, :rows]  # noqa: E731  (the gathered copy is read in place)
        if reward is not None:      # (a replacement has its own pitch: the flags then go dense beside it)
            reward, flags = reward.contiguous(), (cut(self.terminated).contiguous(), cut(self.filled).contiguous())
        else:
            reward, flags = cut(self.reward), (cut(self.terminated), cut(self.filled))
        out = returns.nstep_returns(cut(self.obs), reward, flags[0], flags[1], target_critic, gamma, nstep, add_value_last_step,
                                    value_scale, value_shift)
        return {"returns": out["returns"], "values": out["values"], "mask": out["mask"].unsqueeze(-1)}

    def sample(self, n, generator=None):
        """n slots drawn uniformly, without replacement, among the complete ones (int64); ValueError if fewer are complete."""
        if isinstance(n, bool) or not isinstance(n, int) or n < 1:
            raise ValueError(f"sample(n) draws n >= 1 slots, got {n!r}")
        if n > self.num_slots:
            raise ValueError(f"sample({n}): the buffer has {self.num_slots} slots")
        done = torch.nonzero(self.complete).flatten()
        if int(done.numel()) < n:
            raise ValueError(f"sample({n}): only {int(done.numel())} slots hold a complete episode")
        pick = torch.randperm(int(done.numel()), generator=generator, device=generator.device if generator is not None else "cpu")
        return done[pick[:n].to(done.device)]

    def overflowed(self):
        """How many episodes were cut at the buffer's episode_limit (rule 5), over all envs: a device scalar (int64)."""
        return self.cursor[:, 3].sum()

    # -- checkpoints
    def state_dict(self):
        """Every array, cursors included (an open episode goes on after load_state_dict), as a plain dict of tensor copies."""
        out = {k: getattr(self, k).clone() for k in self.names}
        out["dims"] = torch.tensor([self.E, self.R, self.L, self.N, self.D, self.A], dtype=torch.int64)
        return out

    def load_state_dict(self, state):
        want = torch.tensor([self.E, self.R, self.L, self.N, self.D, self.A], dtype=torch.int64)
        if "dims" not in state or not torch.equal(state["dims"].cpu().to(torch.int64), want):
            raise ValueError(f"the checkpoint's dims {state.get('dims')} differ from this buffer's {want.tolist()} (E, R, L, N, D, A)")
        missing = [k for k in self.names if k not in state]
        if missing or ("prob" in state) != self.with_prob:
            raise ValueError(f"the checkpoint lacks {missing}" if missing else "the checkpoint and the buffer differ in with_prob")
        for k in self.names:
            mine = getattr(self, k)
            if state[k].dtype != mine.dtype or tuple(state[k].shape) != tuple(mine.shape):
                raise ValueError(f"checkpoint[{k!r}] is {state[k].dtype} {tuple(state[k].shape)}, the buffer's {mine.dtype} {tuple(mine.shape)}")
        for k in self.names:
            getattr(self, k).copy_(state[k])
