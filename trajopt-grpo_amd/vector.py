"""DeviceVecEnv: the HIP environments behind the batched, auto-resetting `VectorEnv` contract of Isaac Gym / gymnasium.

`step(actions)` takes a float32 device tensor [n][A] and returns (obs [n][S], reward [n], terminated [n], truncated [n], info) as
device tensors; a slot whose episode ended comes back already reset (gymnasium's SAME_STEP autoreset mode) with the state the
step produced in `info["final_obs"]`.  One step is ONE kernel launch (tg_vec_env_step, csrc/vec_env.hip): no allocation, no host
read, no synchronisation, so any PyTorch RL loop -- CleanRL, rsl_rl, an SB3-style collector, a SAC of your own -- can drive
CartPole / Pendulum / QuadPole2D / QuadPole with `Env.substeps`, `Env.motor_time_constant` and `Env.randomize` without one of this
package's policy classes.  tools/vec_env_ppo.py is a complete example; INTEGRATION.md, "Vector env", states the semantics.

The kernel calls the env's own step / reset code, so episode k of slot i equals, bit for bit, what DeviceRollout's kernels make of the
same initial state (tg_env_reset with stream id k, key env_offset + i) and actions.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _native as N
from .environments import Box


def batched_space(space: Box, n: int) -> Box:
    """The space of n stacked samples of `space`: shape (n,) + space.shape, the bounds repeated."""
    shape = (int(n),) + tuple(space.shape)
    return Box(low=np.broadcast_to(space.low, shape), high=np.broadcast_to(space.high, shape), shape=shape, dtype=space.dtype)


def vector_spaces(env, num_envs: int):
    """(single_observation_space, single_action_space, observation_space, action_space) of `num_envs` copies of `env`."""
    return (env.observation_space, env.action_space, batched_space(env.observation_space, num_envs),
            batched_space(env.action_space, num_envs))


class DeviceVecEnv:
    """`num_envs` auto-resetting copies of `env` on one GPU.

    env         an Env instance; its parameters, `substeps`, `motor_time_constant` and `randomize(...)` ranges are read here and
                again at every reset().  Swarm envs raise ValueError.
    seed        of the reset draws: slot i starts its k-th episode from tg_env_reset(seed, stream_id = k, key_offset = env_offset + i).
    dtype       arithmetic type of the state (float32 / float64); observations and rewards come back as float32 either way.
    env_offset  global index of slot 0: objects with consecutive offsets are, bit for bit, the slots of one larger object.

    The tensors step() and reset() return are the object's own buffers, overwritten by the next step(): clone what you keep."""

    def __init__(self, env, num_envs: int, *, seed: int = 0, dtype=torch.float32, device=None, env_offset: int = 0):
        if int(getattr(env, "n_agents", 1)) > 1:
            raise ValueError("DeviceVecEnv: swarm envs (n_agents > 1) are not supported")
        if int(num_envs) <= 0 or int(env_offset) < 0:
            raise ValueError(f"DeviceVecEnv: num_envs={num_envs} must be positive and env_offset={env_offset} non-negative")
        self.env, self.num_envs, self.env_offset = env, int(num_envs), int(env_offset)
        (self.single_observation_space, self.single_action_space, self.observation_space,
         self.action_space) = vector_spaces(env, self.num_envs)
        self.device = torch.device(device) if device is not None else getattr(env, "_device", torch.device("cuda", 0))
        if self.device.type != "cuda":
            raise N.NativeLibraryError("DeviceVecEnv needs an MI355X (cuda) device; there is no CPU fallback")
        self.lib = N.load()
        self.dtype, self._dtype_code = dtype, N.dtype_code(dtype)
        self.seed = self._checked_seed(seed)
        n, S, A, dev = self.num_envs, env.obs_dim, env.act_dim, self.device
        self.S, self.A = S, A
        # per-slot state (struct of arrays, env fastest: include/trajopt_grpo_hip.h, tg_vec_env)
        self._state = torch.zeros(S, n, dtype=dtype, device=dev)
        self._steps = torch.zeros(n, dtype=torch.int32, device=dev)
        self._balanced = torch.zeros(n, dtype=torch.int32, device=dev)
        self._ep_return = torch.zeros(n, dtype=torch.float64, device=dev)
        self._episode = torch.zeros(n, dtype=torch.int32, device=dev)             # (the bits of a u32)
        self._motor = None                                                        # f32 [A][n] while the env has an actuator lag
        self.env_params = None                                                    # f64 [12][n] while Env.randomize is on
        # what a step returns
        self._obs = torch.zeros(n, S, dtype=torch.float32, device=dev)
        self._reward = torch.zeros(n, dtype=torch.float32, device=dev)
        self._terminated = torch.zeros(n, dtype=torch.uint8, device=dev)
        self._truncated = torch.zeros(n, dtype=torch.uint8, device=dev)
        self._final_obs = torch.zeros(n, S, dtype=torch.float32, device=dev)
        self._final_return = torch.zeros(n, dtype=torch.float32, device=dev)
        self._final_length = torch.zeros(n, dtype=torch.int32, device=dev)
        self._term_b, self._trunc_b = self._terminated.view(torch.bool), self._truncated.view(torch.bool)
        self._resets = 0                 # reset() calls since the seed was set: the stream id of the parameter draw
        self._started = False
        self._closed = False
        self._read_env()

    @staticmethod
    def _checked_seed(seed) -> int:
        seed = int(seed)
        if not 0 <= seed < 2 ** 64:
            raise ValueError(f"DeviceVecEnv: seed {seed} is not an unsigned 64-bit integer")
        return seed

    def _read_env(self):
        """The env's parameters as the next steps run them (DeviceRollout._read_env's rule): with substeps != 1 or a lag those of the
        physics clock; the motor state exists while the lag is on; the randomisation spec while Env.randomize is on."""
        env = self.env
        self.substeps = int(getattr(env, "substeps", 1))
        self.horizon = int(env.max_steps)
        self.params = env.native_params() if self.substeps == 1 else env.physics_params()
        self.lag = float(getattr(env, "motor_time_constant", 0.0)) > 0.0
        if not self.lag:
            self._motor = None
        elif self._motor is None:
            self._motor = torch.zeros(self.A, self.num_envs, dtype=torch.float32, device=self.device)
        self._rand_spec = env.randomize_spec()
        if self._rand_spec is None:
            self.env_params = None
        elif self.env_params is None:
            self.env_params = torch.empty(12, self.num_envs, dtype=torch.float64, device=self.device)
        v = N.VecEnv()
        v.d_state, v.d_steps, v.d_balanced = self._state.data_ptr(), self._steps.data_ptr(), self._balanced.data_ptr()
        v.d_ep_return, v.d_episode = self._ep_return.data_ptr(), self._episode.data_ptr()
        v.n, v.env_offset, v.seed, v.horizon, v.dtype = self.num_envs, self.env_offset, self.seed, self.horizon, self._dtype_code
        self._native = v
        # everything of a step's call but the actions and the stream: fixed until the next reset()
        self._step_head = (C.byref(self.params), N.ptr(self.env_params), self.substeps, N.ptr(self._motor), C.byref(v))
        self._step_tail = (self._obs.data_ptr(), self._reward.data_ptr(), self._terminated.data_ptr(), self._truncated.data_ptr(),
                           self._final_obs.data_ptr(), self._final_return.data_ptr(), self._final_length.data_ptr())

    @property
    def variant(self) -> str:
        """Which instantiation of the step kernel the launches take: "plain" with everything off, else "sub" (substeps != 1) or
        "lag" (an actuator lag, which includes the substep loop), with "+dr" behind it -- or "dr" alone -- under Env.randomize."""
        parts = (["lag"] if self.lag else ["sub"] if self.substeps != 1 else []) + (["dr"] if self.env_params is not None else [])
        return "+".join(parts) or "plain"

    def _info(self):
        info = {"final_obs": self._final_obs, "episode_return": self._final_return, "episode_length": self._final_length}
        if self.env_params is not None:
            info["env_params"] = self.env_params
        return info

    def _require_open(self):
        if self._closed:
            raise RuntimeError("DeviceVecEnv: the env is closed")

    # ---- gymnasium.vector.VectorEnv surface ------------------------------------------------------------------------------------
    def reset(self, seed=None):
        """Every slot starts a new episode; -> (obs [n][S] float32, info).  With a seed: it becomes the object's seed and the episode
        ordinals restart at 0 (two objects reset with the same seed and fed the same actions agree bit for bit).  Without one every
        slot moves on to its next ordinal (the very first reset starts at 0).  The env is read again (parameters, substeps, lag,
        randomisation), and with Env.randomize on the parameter table is drawn HERE -- tg_env_randomize keyed (seed, stream id = reset()
        calls since the seed was set, key_offset = env_offset, key_div = 1) -- and kept until the next reset(): a slot keeps its
        vehicle across the auto-resets inside step().  No host synchronisation."""
        self._require_open()
        restart = seed is not None or not self._started
        if seed is not None:
            self.seed, self._resets = self._checked_seed(seed), 0
        self._read_env()
        with torch.cuda.device(self.device):
            st = N.stream_ptr(self.device)
            N.check(self.lib.tg_vec_env_reset_all(C.byref(self.params), N.ptr(self._motor), C.byref(self._native), int(restart),
                                                  self._obs.data_ptr(), st), "tg_vec_env_reset_all")
            if self._rand_spec is not None:
                N.check(self.lib.tg_env_randomize(C.byref(self.params), C.byref(self._rand_spec), self.env_params.data_ptr(),
                                                  self.num_envs, self.seed, self._resets, self.env_offset, 1, st), "tg_env_randomize")
        self._resets += 1
        self._started = True
        info = {} if self.env_params is None else {"env_params": self.env_params}
        return self._obs, info

    def step(self, actions):
        """One control step of every slot in one launch; -> (obs, reward, terminated, truncated, info).
        actions     float32 device tensor [n][A] (made contiguous if it is not)
        obs         float32 [n][S]: the next observation -- the fresh initial state where the slot's episode ended
        reward      float32 [n]
        terminated  bool [n]: the episode ended in a failure (or Pendulum's balance terminal): do not bootstrap
        truncated   bool [n]: the clock ended it: bootstrap from info["final_obs"]
        info        "final_obs" float32 [n][S] (the state the step produced, before the reset), "episode_return" float32 [n],
                    "episode_length" int32 [n]: rows / entries are defined where terminated | truncated; "env_params" f64 [12][n]
                    with Env.randomize on.
        All of them are this object's buffers: the next step() overwrites them."""
        self._require_open()
        if not self._started:
            raise RuntimeError("DeviceVecEnv: step() before reset()")
        N.require_cuda(actions)
        if actions.dtype != torch.float32 or tuple(actions.shape) != (self.num_envs, self.A):
            raise ValueError(f"DeviceVecEnv: actions must be float32 [{self.num_envs}][{self.A}], got {actions.dtype} "
                             f"{tuple(actions.shape)}")
        if not actions.is_contiguous():
            actions = actions.contiguous()
        if actions.data_ptr() % (4 * self.A):
            actions = actions.clone()                      # (a view that starts inside a row of its parent)
        with torch.cuda.device(self.device):
            N.check(self.lib.tg_vec_env_step(*self._step_head, actions.data_ptr(), *self._step_tail, N.stream_ptr(self.device)),
                    "tg_vec_env_step")
        return self._obs, self._reward, self._term_b, self._trunc_b, self._info()

    def set_state(self, states):
        """Every slot's CURRENT episode starts over from `states` [n][S] with steps = 0 (its ordinal, and so its next reset draw,
        stay): evaluation from chosen states.  -> the observation buffer, now these states rounded to float32."""
        self._require_open()
        if not self._started:
            raise RuntimeError("DeviceVecEnv: set_state() before reset()")
        states = torch.as_tensor(states, device=self.device)
        if tuple(states.shape) != (self.num_envs, self.S):
            raise ValueError(f"DeviceVecEnv: states must be [{self.num_envs}][{self.S}], got {tuple(states.shape)}")
        self._state.copy_(states.t())
        self._obs.copy_(states)
        for buf in (self._steps, self._balanced, self._ep_return, self._motor):
            if buf is not None:
                buf.zero_()
        return self._obs

    @property
    def state(self) -> torch.Tensor:
        """A copy of the current states, [n][S] in the arithmetic dtype."""
        return self._state.t().contiguous()

    @property
    def episode_ordinals(self) -> torch.Tensor:
        """A copy of every slot's current episode ordinal, int64 [n]."""
        return self._episode.long() & 0xFFFFFFFF

    @property
    def episode_steps(self) -> torch.Tensor:
        """A copy of the control steps every slot has taken in its current episode, int32 [n]."""
        return self._steps.clone()

    def close(self):
        """Drop the device buffers; step() / reset() raise afterwards."""
        self._closed = True
        for name in ("_state", "_steps", "_balanced", "_ep_return", "_episode", "_motor", "env_params", "_obs", "_reward", "_terminated",
                     "_truncated", "_final_obs", "_final_return", "_final_length", "_term_b", "_trunc_b"):
            setattr(self, name, None)
