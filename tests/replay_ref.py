"""NumPy restatement of DeviceReplayBuffer's push and sample (csrc/replay.hip; the rule of include/trajopt_grpo_hip.h, tg_replay),
written slot by slot and row by row, and the brute-force per-row definition of an n-step transition the in-place rule must equal.

Arithmetic: the discount table is float32(gamma ** j) with the power formed in float64; a row's return grows by
float32(float32(g[j] * r) + rew) -- one float32 multiply and one float32 add, each rounded on its own, in push order."""
import numpy as np

from philox_fp64 import draw_np


def discount_table(gamma, n_step):
    return np.array([float(gamma) ** j for j in range(n_step + 1)], dtype=np.float64).astype(np.float32)


def index_map(w, R):
    """Row of a draw's first word w among R stored rows: (uint64(w) * R) >> 32."""
    return (np.asarray(w, dtype=np.uint64) * np.uint64(R)) >> np.uint64(32)


class ReplayRef:
    def __init__(self, S, A, n, K, n_step=1, gamma=0.99, seed=0):
        self.S, self.A, self.n, self.K, self.n_step, self.seed = S, A, n, K, n_step, seed
        self.g = discount_table(gamma, n_step)
        self.obs = np.zeros((K * n, S), np.float32)
        self.act = np.zeros((K * n, A), np.float32)
        self.next_obs = np.zeros((K * n, S), np.float32)
        self.rew = np.zeros(K * n, np.float32)
        self.disc = np.zeros(K * n, np.float32)
        self.nstep = np.zeros(K * n, np.uint8)
        self.last_obs = np.zeros((n, S), np.float32)
        self.cursor = np.zeros(n, np.int32)
        self.filled = np.zeros(n, np.int32)
        self.open = np.zeros(n, np.int32)
        self.ordinal = 0

    def start(self, obs):
        self.last_obs[:] = obs
        self.open[:] = 0

    def clear(self):
        self.cursor[:] = 0
        self.filled[:] = 0
        self.open[:] = 0

    def push(self, actions, obs, reward, terminated, truncated, final_obs):
        n, K, g = self.n, self.K, self.g
        for i in range(n):
            c, o = int(self.cursor[i]), int(self.open[i])
            term, done = bool(terminated[i]), bool(terminated[i]) or bool(truncated[i])
            nx = final_obs[i] if done else obs[i]
            r = np.float32(reward[i])
            row = c * n + i
            self.obs[row] = self.last_obs[i]
            self.act[row] = actions[i]
            self.rew[row] = r
            self.next_obs[row] = nx
            self.disc[row] = np.float32(0.0) if term else g[1]
            self.nstep[row] = 1
            for j in range(1, o + 1):
                row = ((c - j) % K) * n + i
                self.rew[row] = np.float32(self.rew[row] + np.float32(g[j] * r))
                self.next_obs[row] = nx
                self.disc[row] = np.float32(0.0) if term else g[j + 1]
                self.nstep[row] = j + 1
            self.open[i] = 0 if done else min(o + 1, self.n_step - 1)
            self.cursor[i] = (c + 1) % K
            self.filled[i] = min(int(self.filled[i]) + 1, K)
            self.last_obs[i] = obs[i]

    @property
    def rows(self):
        return int(self.filled[0]) * self.n

    def sample_indices(self, batch):
        """The rows the next sample(batch) without `indices` takes (does not advance the ordinal)."""
        w = draw_np(self.seed, np.arange(batch, dtype=np.uint64), (self.ordinal >> 32) & 0xFFFFFFFF, self.ordinal & 0xFFFFFFFF)[0]
        return index_map(w, self.rows).astype(np.int64)

    def sample(self, batch=None, indices=None):
        """-> (obs, act, rew, next_obs, disc, idx); a row outside [0, R) is NaN in every float."""
        idx = self.sample_indices(batch) if indices is None else np.asarray(indices, dtype=np.int64)
        self.ordinal += 1
        ok = (idx >= 0) & (idx < self.rows)
        safe = np.where(ok, idx, 0)
        out = [self.obs[safe].copy(), self.act[safe].copy(), self.rew[safe].copy(), self.next_obs[safe].copy(), self.disc[safe].copy()]
        for a in out:
            a[~ok] = np.nan
        return (*out, idx)

    def arrays(self):
        return {"obs": self.obs, "act": self.act, "next_obs": self.next_obs, "rew": self.rew, "disc": self.disc, "nstep": self.nstep,
                "last_obs": self.last_obs, "cursor": self.cursor, "filled": self.filled, "open": self.open}


def brute_force_rows(history, n, K, n_step, g):
    """The per-row definition.  `history[i]` is slot i's list of pushes, oldest first, each a dict(obs, act, rew, term, trunc, nx,
    cut) -- `obs` the observation the action was applied to, `nx` the successor (final_obs where the episode ended), `cut` True when
    a start() followed the push (nothing extends across it).  The row stored for push t is the k-step transition that starts there:
    the return is accumulated left to right in float32 and stops at the first done, at a cut, at n_step steps or at the newest push.
    -> {row index: (obs, act, rew, next_obs, disc, nstep)} for the rows the ring still holds."""
    rows = {}
    for i in range(n):
        h = history[i]
        T = len(h)
        for t in range(max(0, T - K), T):
            ret, k = np.float32(h[t]["rew"]), 1
            while not (h[t + k - 1]["term"] or h[t + k - 1]["trunc"] or h[t + k - 1]["cut"]) and k < n_step and t + k < T:
                ret = np.float32(ret + np.float32(g[k] * np.float32(h[t + k]["rew"])))
                k += 1
            last = h[t + k - 1]
            rows[(t % K) * n + i] = (h[t]["obs"], h[t]["act"], ret, last["nx"], np.float32(0.0) if last["term"] else g[k], k)
    return rows
