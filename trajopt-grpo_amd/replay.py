"""DeviceReplayBuffer: n-step replay for off-policy loops (SAC, TD3, DQN-style) on DeviceVecEnv.

A ring of `capacity_steps` time slots of `num_envs` transitions each, in device memory.  `add()` takes the action just applied and
`DeviceVecEnv.step`'s five results and is ONE kernel launch (tg_replay_push, csrc/replay.hip); `sample()` is ONE gather launch
(tg_replay_sample).  What SAME_STEP autoreset makes easy to get wrong is done in the kernel: the successor state of a row is
`info["final_obs"]` where the episode ended, not the already-reset `obs`; a row bootstraps through `truncated` and not through
`terminated`; an n-step return never runs across an episode boundary.  Every stored row is at all times a consistent k-step
transition for its own k = nstep <= n_step, with the target

    rew + disc * Q(next_obs)            (rew = sum_j gamma^j r_j, disc = gamma^k, or 0 behind a termination)

so no row is ever "not ready" and sampling needs no exclusion window.  INTEGRATION.md, "Replay buffer", states the rule;
tests/replay_ref.py restates it in NumPy, bit for bit.  tools/vec_env_sac.py is a complete example.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _native as N

MAX_N_STEP, MAX_OBS_DIM, MAX_ACT_DIM = 16, 32, 8


def discount_table(gamma: float, n_step: int) -> np.ndarray:
    """g[j] = float32(gamma ** j), j = 0 .. n_step: each power formed in float64 and rounded once."""
    return np.array([float(gamma) ** j for j in range(int(n_step) + 1)], dtype=np.float64).astype(np.float32)


class DeviceReplayBuffer:
    """n-step replay storage for `num_envs` auto-resetting env slots on one GPU.

    capacity_steps  K: time slots of the ring; the buffer holds up to K * num_envs transitions (K >= n_step, K * num_envs < 2^31)
    n_step          longest return a row accumulates, in [1, 16]; gamma in (0, 1]
    seed            of sample()'s draws (unsigned 64-bit)

    Storage is float32, row-major, row = slot * num_envs + i: `obs`, `act`, `next_obs`, `rew`, `disc`, `nstep` (uint8).

    The tensors sample() returns are the object's own buffers, overwritten by the next sample(): clone what you keep."""

    def __init__(self, obs_dim: int, act_dim: int, num_envs: int, capacity_steps: int, *, n_step: int = 1, gamma: float = 0.99,
                 seed: int = 0, device=None):
        S, A, n, K, n_step, gamma = int(obs_dim), int(act_dim), int(num_envs), int(capacity_steps), int(n_step), float(gamma)
        if not 1 <= S <= MAX_OBS_DIM or not 1 <= A <= MAX_ACT_DIM:
            raise ValueError(f"DeviceReplayBuffer: obs_dim={S} must be in [1, {MAX_OBS_DIM}] and act_dim={A} in [1, {MAX_ACT_DIM}]")
        if n <= 0:
            raise ValueError(f"DeviceReplayBuffer: num_envs={n} must be positive")
        if not 1 <= n_step <= MAX_N_STEP:
            raise ValueError(f"DeviceReplayBuffer: n_step={n_step} outside [1, {MAX_N_STEP}]")
        if K < n_step:
            raise ValueError(f"DeviceReplayBuffer: capacity_steps={K} < n_step={n_step}")
        if K * n >= 2 ** 31:
            raise ValueError(f"DeviceReplayBuffer: capacity_steps {K} x num_envs {n} = {K * n} rows >= 2^31")
        if not 0.0 < gamma <= 1.0:
            raise ValueError(f"DeviceReplayBuffer: gamma={gamma} not in (0, 1]")
        self.seed = self._checked_seed(seed)
        self.device = torch.device(device) if device is not None else torch.device("cuda", 0)
        if self.device.type != "cuda":
            raise N.NativeLibraryError("DeviceReplayBuffer needs an MI355X (cuda) device; there is no CPU fallback")
        self.lib = N.load()
        self.obs_dim, self.act_dim, self.num_envs, self.capacity_steps, self._n_step, self._gamma = S, A, n, K, n_step, gamma
        dev, rows = self.device, K * n
        self.obs = torch.zeros(rows, S, dtype=torch.float32, device=dev)
        self.act = torch.zeros(rows, A, dtype=torch.float32, device=dev)
        self.next_obs = torch.zeros(rows, S, dtype=torch.float32, device=dev)
        self.rew = torch.zeros(rows, dtype=torch.float32, device=dev)
        self.disc = torch.zeros(rows, dtype=torch.float32, device=dev)
        self.nstep = torch.zeros(rows, dtype=torch.uint8, device=dev)
        # per-slot state, all of it on the device: a push takes nothing by value that changes from push to push
        self._last_obs = torch.zeros(n, S, dtype=torch.float32, device=dev)
        self._slots = torch.zeros(3, n, dtype=torch.int32, device=dev)
        self.cursor, self.filled, self.open = self._slots[0], self._slots[1], self._slots[2]
        self.discount = discount_table(gamma, n_step)
        r = N.Replay()
        r.d_obs, r.d_act, r.d_next_obs = self.obs.data_ptr(), self.act.data_ptr(), self.next_obs.data_ptr()
        r.d_rew, r.d_disc, r.d_nstep = self.rew.data_ptr(), self.disc.data_ptr(), self.nstep.data_ptr()
        r.d_last_obs, r.d_cursor, r.d_filled, r.d_open = (self._last_obs.data_ptr(), self.cursor.data_ptr(), self.filled.data_ptr(),
                                                          self.open.data_ptr())
        r.n, r.capacity_steps, r.obs_dim, r.act_dim, r.n_step = n, K, S, A, n_step
        for j, g in enumerate(self.discount):
            r.discount[j] = float(g)
        self._native = r
        self._pushes = 0                 # add() calls since the last clear(): the host mirror of `filled` and `cursor`
        self._ordinal = 0                # sample() calls so far: the stream of the next call's draws
        self._started = False
        self._out, self._out_rows = None, 0

    @classmethod
    def for_env(cls, venv, capacity_steps: int, **kwargs):
        """The buffer that fits a DeviceVecEnv: its obs / action widths, slot count and device."""
        kwargs.setdefault("device", venv.device)
        return cls(venv.S, venv.A, venv.num_envs, capacity_steps, **kwargs)

    @staticmethod
    def _checked_seed(seed) -> int:
        seed = int(seed)
        if not 0 <= seed < 2 ** 64:
            raise ValueError(f"DeviceReplayBuffer: seed {seed} is not an unsigned 64-bit integer")
        return seed

    # ---- properties (host mirrors: no synchronisation) ---------------------------------------------------------------------------
    def __len__(self) -> int:
        return min(self._pushes, self.capacity_steps) * self.num_envs

    @property
    def capacity(self) -> int:
        """Transitions the ring holds when full: capacity_steps * num_envs."""
        return self.capacity_steps * self.num_envs

    @property
    def n_step(self) -> int:
        return self._n_step

    @property
    def gamma(self) -> float:
        return self._gamma

    # ---- writing -----------------------------------------------------------------------------------------------------------------
    def _rows(self, t, name, width, dtypes=(torch.float32,)):
        """`t` as a valid argument: a CUDA tensor [n] (width None) or [n][width] of one of `dtypes`, made contiguous if it is not."""
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"DeviceReplayBuffer: {name} must be a torch tensor, got {type(t).__name__}")
        shape = (self.num_envs,) if width is None else (self.num_envs, width)
        if t.dtype not in dtypes or tuple(t.shape) != shape:
            raise ValueError(f"DeviceReplayBuffer: {name} must be {' / '.join(str(d) for d in dtypes)} "
                             f"{list(shape)}, got {t.dtype} {list(t.shape)}")
        if not t.is_cuda:
            raise ValueError(f"DeviceReplayBuffer: {name} must be a CUDA tensor (there is no CPU fallback)")
        return t if t.is_contiguous() else t.contiguous()

    def start(self, obs):
        """Call after venv.reset(): `obs` [n][S] becomes the observation the next add()'s action was applied to, and no stored row
        is extended any further.  Stored rows stay."""
        obs = self._rows(obs, "obs", self.obs_dim)
        with torch.cuda.device(self.device):
            N.check(self.lib.tg_replay_start(C.byref(self._native), obs.data_ptr(), N.stream_ptr(self.device)), "tg_replay_start")
        self._started = True

    def clear(self):
        """Drop every stored row: cursor, filled and open go to 0.  Call start() again before the next add()."""
        self._slots.zero_()
        self._pushes = 0
        self._started = False

    def add(self, actions, obs, reward, terminated, truncated, info):
        """Store one step of every slot: the action just applied and venv.step's five results.  One launch, no copy of a contiguous
        argument, no host read: the buffer keeps its own copy of the last observation, so DeviceVecEnv's reused buffers can be handed
        over as they are.  `info["final_obs"]` is read only in rows where terminated | truncated."""
        if not self._started:
            raise RuntimeError("DeviceReplayBuffer: add() before start()")
        if not isinstance(info, dict) or "final_obs" not in info:
            raise ValueError('DeviceReplayBuffer: info["final_obs"] is missing (the successor state of a row whose episode ended)')
        flags = (torch.bool, torch.uint8)
        actions = self._rows(actions, "actions", self.act_dim)
        obs = self._rows(obs, "obs", self.obs_dim)
        reward = self._rows(reward, "reward", None)
        terminated = self._rows(terminated, "terminated", None, flags)
        truncated = self._rows(truncated, "truncated", None, flags)
        final_obs = self._rows(info["final_obs"], 'info["final_obs"]', self.obs_dim)
        with torch.cuda.device(self.device):
            N.check(self.lib.tg_replay_push(C.byref(self._native), actions.data_ptr(), obs.data_ptr(), reward.data_ptr(),
                                            terminated.data_ptr(), truncated.data_ptr(), final_obs.data_ptr(),
                                            N.stream_ptr(self.device)), "tg_replay_push")
        self._pushes += 1

    # ---- reading -----------------------------------------------------------------------------------------------------------------
    def _outputs(self, batch):
        if batch > self._out_rows:
            dev = self.device
            self._out = (torch.empty(batch, self.obs_dim, dtype=torch.float32, device=dev),
                         torch.empty(batch, self.act_dim, dtype=torch.float32, device=dev),
                         torch.empty(batch, dtype=torch.float32, device=dev),
                         torch.empty(batch, self.obs_dim, dtype=torch.float32, device=dev),
                         torch.empty(batch, dtype=torch.float32, device=dev),
                         torch.empty(batch, dtype=torch.int64, device=dev))
            self._out_rows = batch
        return tuple(t[:batch] for t in self._out)

    def sample(self, batch=None, indices=None):
        """-> (obs [B][S], act [B][A], rew [B], next_obs [B][S], disc [B], idx int64 [B]) in one launch; the TD target of row b is
        rew[b] + disc[b] * Q(next_obs[b]).

        Without `indices`, element b takes row (w * R) >> 32 of the R = filled * num_envs stored rows (R is read on the device), w the
        first word of the Philox draw (seed, idx = b, sub = ordinal >> 32, stream = ordinal & 0xffffffff); `ordinal` counts this
        object's sample() calls and is passed by value, so a captured graph repeats its draws: inside a graph pass `indices=` (a
        tensor you refill in place).  With `indices` (int64 device tensor [B]) those rows are gathered; an index outside [0, R) is
        not read and gives a row of NaNs.

        The six tensors are this object's buffers, reallocated only when B grows: the next sample() overwrites them."""
        if indices is not None:
            if (not isinstance(indices, torch.Tensor) or indices.dtype != torch.int64 or indices.dim() != 1 or indices.numel() == 0
                    or (batch is not None and int(batch) != indices.numel())):
                raise ValueError("DeviceReplayBuffer: indices must be a non-empty int64 tensor [B] (and batch, if given, its length)")
            if not indices.is_cuda:
                raise ValueError("DeviceReplayBuffer: indices must be a CUDA tensor (there is no CPU fallback)")
            indices = indices if indices.is_contiguous() else indices.contiguous()
            batch = indices.numel()
        elif batch is None or int(batch) <= 0:
            raise ValueError(f"DeviceReplayBuffer: batch={batch} must be a positive integer")
        batch = int(batch)
        if self._pushes == 0:
            raise RuntimeError("DeviceReplayBuffer: sample() on an empty buffer (no add() yet)")
        out = self._outputs(batch)
        with torch.cuda.device(self.device):
            N.check(self.lib.tg_replay_sample(C.byref(self._native), batch, N.ptr(indices), self.seed, self._ordinal,
                                              *(t.data_ptr() for t in out), N.stream_ptr(self.device)), "tg_replay_sample")
        self._ordinal += 1
        return out

    # ---- checkpointing -----------------------------------------------------------------------------------------------------------
    _TENSORS = ("obs", "act", "next_obs", "rew", "disc", "nstep", "_last_obs", "_slots")

    def state_dict(self):
        """Copies of the storage and the per-slot state, the counters, the seed and the sample ordinal."""
        sd = {name.lstrip("_"): getattr(self, name).clone() for name in self._TENSORS}
        sd.update(obs_dim=self.obs_dim, act_dim=self.act_dim, num_envs=self.num_envs, capacity_steps=self.capacity_steps,
                  n_step=self._n_step, gamma=self._gamma, seed=self.seed, ordinal=self._ordinal, pushes=self._pushes,
                  started=self._started)
        return sd

    def load_state_dict(self, sd):
        """Take over a state_dict() of an object of the same shape: later add() and sample() calls agree bit for bit with the
        original's."""
        for key in ("obs_dim", "act_dim", "num_envs", "capacity_steps", "n_step"):
            if int(sd[key]) != getattr(self, key):
                raise ValueError(f"DeviceReplayBuffer: state_dict has {key}={sd[key]}, this object {getattr(self, key)}")
        if float(sd["gamma"]) != self._gamma:
            raise ValueError(f"DeviceReplayBuffer: state_dict has gamma={sd['gamma']}, this object {self._gamma}")
        slots = sd["slots"].to("cpu")
        K = self.capacity_steps
        if (tuple(slots.shape) != (3, self.num_envs) or bool((slots[0] < 0).any()) or bool((slots[0] >= K).any())
                or bool((slots[1] < 0).any()) or bool((slots[1] > K).any()) or bool((slots[2] < 0).any())
                or bool((slots[2] > self._n_step - 1).any())):
            raise ValueError("DeviceReplayBuffer: state_dict's cursor / filled / open are outside the ring")
        for name in self._TENSORS:
            src, dst = sd[name.lstrip("_")], getattr(self, name)
            if tuple(src.shape) != tuple(dst.shape) or src.dtype != dst.dtype:
                raise ValueError(f"DeviceReplayBuffer: state_dict's {name.lstrip('_')} is {src.dtype} {list(src.shape)}, "
                                 f"expected {dst.dtype} {list(dst.shape)}")
        for name in self._TENSORS:
            getattr(self, name).copy_(sd[name.lstrip("_")])
        self.seed, self._ordinal = self._checked_seed(sd["seed"]), int(sd["ordinal"])
        self._pushes, self._started = int(sd["pushes"]), bool(sd["started"])
