"""The episode buffer's rule (csrc/episodes.h) in NumPy, written from the rule's text: one env and one time step after the other,
episode_return as binary32 additions in step order.  The GPU tier compares every array of the buffer with this word for word."""
import numpy as np

DTYPES = {"obs": np.float32, "actions": np.int32, "reward": np.float32, "terminated": np.uint8, "filled": np.uint8,
          "prob": np.float32, "length": np.int32, "episode_return": np.float32, "complete": np.uint8, "fresh": np.uint8,
          "episode_index": np.int32, "cursor": np.int32}


def shapes(E, R, L, N, D):
    S = E * R
    return {"obs": (S, L + 1, N, D), "actions": (S, L + 1, N), "reward": (S, L + 1), "terminated": (S, L + 1),
            "filled": (S, L + 1), "prob": (S, L + 1, N), "length": (S,), "episode_return": (S,), "complete": (S,),
            "fresh": (S,), "episode_index": (S,), "cursor": (E, 4)}


class TwinBuffer(object):
    def __init__(self, E, R, L, N, D, with_prob=False, arrays=None):
        """arrays: initial contents (name -> array, copied); default: zeros, no env with an open episode."""
        self.E, self.R, self.L, self.N, self.D, self.with_prob = E, R, L, N, D, with_prob
        self.names = tuple(k for k in DTYPES if k != "prob" or with_prob)
        for k in self.names:
            shape = shapes(E, R, L, N, D)[k]
            if arrays is None:
                a = np.zeros(shape, DTYPES[k])
            else:
                a = np.array(arrays[k], dtype=DTYPES[k]).reshape(shape)
            setattr(self, k, a)
        if arrays is None:
            self.cursor[:, 0] = -1

    def arrays(self):
        return {k: getattr(self, k) for k in self.names}

    def _open(self, e):
        open_, _, opened, _ = self.cursor[e]
        if open_ >= 0:
            opened -= 1                                   # abandoned: not complete, its slot and index go to the new episode
        s = e * self.R + opened % self.R
        self.filled[s] = 0
        self.terminated[s] = 0
        self.reward[s] = 0
        self.length[s] = 0
        self.episode_return[s] = 0
        self.complete[s] = 0
        self.fresh[s] = 0
        self.episode_index[s] = opened
        self.cursor[e, 0], self.cursor[e, 1], self.cursor[e, 2] = s, 0, opened + 1

    def _close(self, e, s, p, obs_next):
        self.obs[s, p + 1] = obs_next
        self.filled[s, p + 1] = 1
        self.length[s] = p + 1
        self.complete[s] = 1
        self.fresh[s] = 1
        self.cursor[e, 0], self.cursor[e, 1] = -1, 0

    def append(self, batch):
        """batch: run()'s dict as NumPy arrays (obs [T + 1, E, N, D], actions, reward, terminated, episode_start, prob)."""
        obs, actions, reward = batch["obs"], batch["actions"], np.asarray(batch["reward"], np.float32)
        term, start = np.asarray(batch["terminated"]).astype(bool), np.asarray(batch["episode_start"]).astype(bool)
        T = actions.shape[0]
        for e in range(self.E):
            for t in range(T):
                if start[t, e]:
                    self._open(e)
                s, p = int(self.cursor[e, 0]), int(self.cursor[e, 1])
                if s < 0:
                    continue
                self.obs[s, p] = obs[t, e]
                self.actions[s, p] = actions[t, e]
                self.reward[s, p] = reward[t, e]
                self.terminated[s, p] = 1 if term[t, e] else 0
                if self.with_prob:
                    self.prob[s, p] = batch["prob"][t, e]
                self.filled[s, p] = 1
                self.episode_return[s] = np.float32(self.episode_return[s]) + np.float32(reward[t, e])
                if term[t, e]:
                    self._close(e, s, p, obs[t + 1, e])
                elif p + 1 == self.L:
                    self._close(e, s, p, obs[t + 1, e])
                    self.cursor[e, 3] += 1
                else:
                    self.cursor[e, 1] = p + 1

    def take_new(self):
        new = np.flatnonzero(self.fresh)
        self.fresh[:] = 0
        return new
