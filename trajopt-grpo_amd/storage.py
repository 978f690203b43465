"""DeviceRolloutStorage: fixed-length rollout segments for on-policy loops (PPO, A2C-style) on DeviceVecEnv.

`steps` time rows of `num_envs` slots each, in device memory.  `add()` takes what the policy and the critic gave for a step and
`DeviceVecEnv.step`'s results and is ONE kernel launch (tg_segment_push, csrc/segment.hip); `compute_returns()` is ONE launch for GAE
over the whole segment (tg_segment_gae), `shuffle()` ONE launch for a fresh permutation of the L * n rows (tg_segment_permute, no
sort), `minibatch()` ONE gather launch (tg_segment_gather).  The slots sit anywhere in their episodes -- an episode may end and
restart in the middle of a column -- and what that makes easy to get wrong is done in the kernels: a step that `truncated` ended
(and `terminated` did not) bootstraps from the critic's value of the state the clock cut off, a terminated one from nothing, and
neither passes anything on from the episode behind it.  INTEGRATION.md, "Rollout storage", states the rule and the order of the
arithmetic; tests/segment_ref.py restates it in NumPy, bit for bit.  tools/vec_env_ppo.py --storage is a complete example.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _native as N
from .replay import MAX_ACT_DIM, MAX_OBS_DIM

PERMUTE_BLOCK = 256                      # TG_SEGMENT_PERMUTE_BLOCK: one shuffle counter per workgroup of the permutation launch


class DeviceRolloutStorage:
    """On-policy storage for `num_envs` auto-resetting env slots on one GPU: `steps` = L rows per segment.

    gamma, lam      in (0, 1]; the kernels use float32(gamma) and float32(gamma * lam), the product formed in float64
    seed            of shuffle()'s permutations (unsigned 64-bit)

    Storage is float32, [L][n]-major: `obs` [L + 1][n][S] (row t is what the action of step t was applied to, row L the observation
    behind the last step -- and row 0 of the next segment, written by the same launch), `act` [L][n][A], `logp`, `val`, `rew` (the
    effective reward), `adv`, `ret` [L][n], `flags` uint8 [L][n] (bit 0 terminated, bit 1 truncated), `idx` int64 [L * n].
    `obs[t]` is a stable view for the policy to read: DeviceVecEnv's own observation buffer is overwritten by the next step.
    `first_obs` [n][S] is row 0 as step 0 of the segment saw it: once the segment's last add() has put the next segment's first
    observation into row 0, the stored observations of the finished segment are first_obs and obs[1:L], and minibatch() reads those.

    The step counter and the shuffle counter live on the device and add() / shuffle() take nothing by value that changes, so
    venv.step + add, or a shuffle, captured into a hipGraph do the next thing at every replay.  The host keeps no mirror of them:
    calling compute_returns() only after a whole number of segments is the caller's side of the contract.

    The tensors compute_returns() and minibatch() return are the object's own buffers, overwritten by the next call: clone what
    you keep."""

    def __init__(self, obs_dim: int, act_dim: int, num_envs: int, steps: int, *, gamma: float = 0.99, lam: float = 0.95,
                 seed: int = 0, device=None):
        S, A, n, L, gamma, lam = int(obs_dim), int(act_dim), int(num_envs), int(steps), float(gamma), float(lam)
        if not 1 <= S <= MAX_OBS_DIM or not 1 <= A <= MAX_ACT_DIM:
            raise ValueError(f"DeviceRolloutStorage: obs_dim={S} must be in [1, {MAX_OBS_DIM}] and act_dim={A} in [1, {MAX_ACT_DIM}]")
        if n <= 0 or L <= 0:
            raise ValueError(f"DeviceRolloutStorage: num_envs={n} and steps={L} must be positive")
        if (L + 1) * n >= 2 ** 31:
            raise ValueError(f"DeviceRolloutStorage: (steps {L} + 1) x num_envs {n} = {(L + 1) * n} rows >= 2^31")
        if not 0.0 < gamma <= 1.0 or not 0.0 < lam <= 1.0:
            raise ValueError(f"DeviceRolloutStorage: gamma={gamma} or lam={lam} not in (0, 1]")
        self.seed = self._checked_seed(seed)
        self.device = torch.device(device) if device is not None else torch.device("cuda", 0)
        if self.device.type != "cuda":
            raise N.NativeLibraryError("DeviceRolloutStorage needs an MI355X (cuda) device; there is no CPU fallback")
        if self.device.index is None:    # ("cuda" -> the current device, spelled out: arguments are compared against it)
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.lib = N.load()
        self.obs_dim, self.act_dim, self.num_envs, self.steps, self.gamma, self.lam = S, A, n, L, gamma, lam
        dev, f32 = self.device, torch.float32
        self.obs = torch.zeros(L + 1, n, S, dtype=f32, device=dev)
        self.act = torch.zeros(L, n, A, dtype=f32, device=dev)
        self.logp, self.val, self.rew, self.adv, self.ret = (torch.zeros(L, n, dtype=f32, device=dev) for _ in range(5))
        self.flags = torch.zeros(L, n, dtype=torch.uint8, device=dev)
        self.idx = torch.arange(L * n, dtype=torch.int64, device=dev)        # (the identity until the first shuffle())
        self.first_obs = torch.zeros(n, S, dtype=f32, device=dev)
        self._step = torch.zeros(n, dtype=torch.int32, device=dev)
        self._shuffles = torch.zeros(-(-L * n // PERMUTE_BLOCK), dtype=torch.int64, device=dev)   # (read as unsigned)
        s = N.Segment()
        s.d_obs, s.d_act, s.d_logp, s.d_val, s.d_rew = (t.data_ptr() for t in (self.obs, self.act, self.logp, self.val, self.rew))
        s.d_flags, s.d_adv, s.d_ret, s.d_idx = (t.data_ptr() for t in (self.flags, self.adv, self.ret, self.idx))
        s.d_step, s.d_shuffles, s.d_first_obs = self._step.data_ptr(), self._shuffles.data_ptr(), self.first_obs.data_ptr()
        s.n, s.seed, s.steps, s.obs_dim, s.act_dim = n, self.seed, L, S, A
        s.gamma, s.gamma_lam = float(np.float32(gamma)), float(np.float32(gamma * lam))
        self._native = s
        self._started = False
        self._out, self._out_rows = None, 0

    @classmethod
    def for_env(cls, venv, steps: int, **kwargs):
        """The storage that fits a DeviceVecEnv: its obs / action widths, slot count and device."""
        kwargs.setdefault("device", venv.device)
        return cls(venv.S, venv.A, venv.num_envs, steps, **kwargs)

    @staticmethod
    def _checked_seed(seed) -> int:
        seed = int(seed)
        if not 0 <= seed < 2 ** 64:
            raise ValueError(f"DeviceRolloutStorage: seed {seed} is not an unsigned 64-bit integer")
        return seed

    @property
    def rows(self) -> int:
        """Rows of a segment: steps * num_envs."""
        return self.steps * self.num_envs

    @property
    def done(self) -> torch.Tensor:
        """bool [L][n]: terminated | truncated."""
        return self.flags != 0

    def _rows(self, t, name, width, dtypes=(torch.float32,), align=False):
        """`t` as a valid argument: a CUDA tensor [n] (width None) or [n][width] of one of `dtypes`, made contiguous (and, for the
        two row arrays the kernel reads 16 bytes at a time, 16-byte aligned) if it is not."""
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"DeviceRolloutStorage: {name} must be a torch tensor, got {type(t).__name__}")
        shape = (self.num_envs,) if width is None else (self.num_envs, width)
        if t.dtype not in dtypes or tuple(t.shape) != shape:
            raise ValueError(f"DeviceRolloutStorage: {name} must be {' / '.join(str(d) for d in dtypes)} "
                             f"{list(shape)}, got {t.dtype} {list(t.shape)}")
        if t.device != self.device:
            raise ValueError(f"DeviceRolloutStorage: {name} is on {t.device}, the storage on {self.device} (there is no CPU fallback)")
        t = t.detach()
        t = t if t.is_contiguous() else t.contiguous()
        return t.clone() if align and t.data_ptr() % 16 else t

    def _stream(self):
        return N.stream_ptr(self.device)

    # ---- writing -----------------------------------------------------------------------------------------------------------------
    def start(self, obs):
        """Call after venv.reset(): `obs` [n][S] becomes row 0 and the step counter goes to 0.  (Between two segments nothing is to
        be called: the last add() of a segment wrote row 0 of the next.)"""
        obs = self._rows(obs, "obs", self.obs_dim)
        self.obs[0].copy_(obs)
        self._step.zero_()
        self._started = True

    def add(self, actions, logp, value, obs, reward, terminated, truncated, final_value):
        """Store one step of every slot in one launch, no host read: the action applied and its log-probability, the critic's value
        of the observation it was applied to (`obs[t]`), venv.step's obs / reward / terminated / truncated as they are, and
        `final_value` [n], the critic's value of info["final_obs"] -- read ONLY in slots where truncated and not terminated (its
        other rows may hold anything, NaN included): there the stored reward is reward + gamma * final_value."""
        if not self._started:
            raise RuntimeError("DeviceRolloutStorage: add() before start()")
        flags = (torch.bool, torch.uint8)
        args = (self._rows(actions, "actions", self.act_dim, align=True), self._rows(logp, "logp", None),
                self._rows(value, "value", None), self._rows(obs, "obs", self.obs_dim, align=True),
                self._rows(reward, "reward", None), self._rows(terminated, "terminated", None, flags),
                self._rows(truncated, "truncated", None, flags), self._rows(final_value, "final_value", None))
        with torch.cuda.device(self.device):
            N.check(self.lib.tg_segment_push(C.byref(self._native), *(t.data_ptr() for t in args), self._stream()), "tg_segment_push")

    def compute_returns(self, last_value):
        """-> (adv, ret), both [L][n], in one launch: GAE(gamma, lam) backwards over the segment, `last_value` [n] the critic's
        value of obs[L].  Float32, every operation rounded on its own, in the order INTEGRATION.md states."""
        last_value = self._rows(last_value, "last_value", None)
        with torch.cuda.device(self.device):
            N.check(self.lib.tg_segment_gae(C.byref(self._native), last_value.data_ptr(), self._stream()), "tg_segment_gae")
        return self.adv, self.ret

    # ---- reading -----------------------------------------------------------------------------------------------------------------
    def shuffle(self):
        """`idx` becomes a fresh permutation of the L * n rows, in one launch and without a sort; -> idx.  The count of shuffles is
        on the device: a captured shuffle() draws a new permutation at every replay."""
        with torch.cuda.device(self.device):
            N.check(self.lib.tg_segment_permute(C.byref(self._native), self._stream()), "tg_segment_permute")
        return self.idx

    def minibatch(self, k: int, num_minibatches: int):
        """-> (obs [B][S], act [B][A], logp, adv, ret, val [B]): rows idx[k B .. (k + 1) B) of the segment in one gather launch,
        B = ceil(L n / num_minibatches); the last minibatch is shorter.  Row r = t * num_envs + i is step t of slot i.

        The six tensors are this object's buffers, reallocated only when B grows: the next minibatch() overwrites them."""
        k, m = int(k), int(num_minibatches)
        if not 1 <= m <= self.rows:
            raise ValueError(f"DeviceRolloutStorage: num_minibatches={m} outside [1, {self.rows}]")
        B = -(-self.rows // m)
        first = k * B
        if k < 0 or first >= self.rows:
            raise ValueError(f"DeviceRolloutStorage: minibatch {k} of {m} is empty ({self.rows} rows in minibatches of {B})")
        count = min(B, self.rows - first)
        if B > self._out_rows:
            dev, f32 = self.device, torch.float32
            self._out = (torch.empty(B, self.obs_dim, dtype=f32, device=dev), torch.empty(B, self.act_dim, dtype=f32, device=dev),
                         *(torch.empty(B, dtype=f32, device=dev) for _ in range(4)))
            self._out_rows = B
        out = tuple(t[:count] for t in self._out)
        with torch.cuda.device(self.device):
            N.check(self.lib.tg_segment_gather(C.byref(self._native), first, count, *(t.data_ptr() for t in out), self._stream()),
                    "tg_segment_gather")
        return out

    # ---- checkpointing -----------------------------------------------------------------------------------------------------------
    _TENSORS = ("obs", "first_obs", "act", "logp", "val", "rew", "flags", "adv", "ret", "idx", "_step", "_shuffles")

    def state_dict(self):
        """Copies of the storage, the results and the two device counters, and what fixes the object."""
        sd = {name.lstrip("_"): getattr(self, name).clone() for name in self._TENSORS}
        sd.update(obs_dim=self.obs_dim, act_dim=self.act_dim, num_envs=self.num_envs, steps=self.steps, gamma=self.gamma,
                  lam=self.lam, seed=self.seed, started=self._started)
        return sd

    def load_state_dict(self, sd):
        """Take over a state_dict() of an object of the same shape, mid-segment or not: later calls agree bit for bit with the
        original's.  The seed comes with it."""
        for key in ("obs_dim", "act_dim", "num_envs", "steps"):
            if int(sd[key]) != getattr(self, key):
                raise ValueError(f"DeviceRolloutStorage: state_dict has {key}={sd[key]}, this object {getattr(self, key)}")
        if float(sd["gamma"]) != self.gamma or float(sd["lam"]) != self.lam:
            raise ValueError(f"DeviceRolloutStorage: state_dict has gamma={sd['gamma']} lam={sd['lam']}, this object {self.gamma} {self.lam}")
        for name in self._TENSORS:
            src, dst = sd[name.lstrip("_")], getattr(self, name)
            if tuple(src.shape) != tuple(dst.shape) or src.dtype != dst.dtype:
                raise ValueError(f"DeviceRolloutStorage: state_dict's {name.lstrip('_')} is {src.dtype} {list(src.shape)}, "
                                 f"expected {dst.dtype} {list(dst.shape)}")
        step = sd["step"].to("cpu")
        if bool((step < 0).any()) or bool((step >= self.steps).any()):
            raise ValueError("DeviceRolloutStorage: state_dict's step counter is outside the segment")
        for name in self._TENSORS:
            getattr(self, name).copy_(sd[name.lstrip("_")])
        self.seed = self._native.seed = self._checked_seed(sd["seed"])
        self._started = bool(sd["started"])
