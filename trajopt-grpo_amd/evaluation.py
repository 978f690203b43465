"""Policy evaluation on the device: mean-action rollouts and sweeps over an env's physical parameters.

The reference has no evaluation (its `Pipeline.test()` samples one more training rollout); this is the `deterministic=True`
evaluation of every RL library, plus the sweep a trainer that randomises vehicle parameters needs.  An evaluation is
`cells x episodes x horizon` env-steps on the rollout kernels the training uses:

    ev = Evaluator(env, policy, episodes=256, sweep={"mass": [0.8, 1.0, 1.25], "tether_length": [0.5, 2.0]})
    res = ev.evaluate()          # enqueues everything; nothing is read until a field of `res` is asked for
    res.table                    # one dict per cell: factors, episodes, return_mean/std/min/max, length_mean, timeout_frac, early_frac
    res.returns                  # [cells][episodes] f64, per-episode returns (0 for an episode that did not end)
    res.summary                  # the same statistics over all cells

Every cell starts from the same `episodes` initial states (drawn once from the evaluator's own seed), steps the vehicle of its
factor tuple (parameters that are not swept keep their nominal value) and, with `deterministic=True`, acts with the actor's mean.
Cells are numbered row-major over the swept parameters taken in p[] order (`Evaluator.sweep_names`), the last one fastest.
The evaluator owns its DeviceRollout and RNG stream: it never advances a training rollout's stream and never touches the policy's
running statistics or an optimizer.  Every evaluate() replays the same experiment (same initial states, same draws), so two
evaluations differ only by what the policy has learned in between.
"""
from __future__ import annotations

import copy
import math
from typing import Optional

import numpy as np
import torch

from . import _native as N
from . import hip_ops as K

CELL_COLUMNS = ("episodes", "return_sum", "return_sumsq", "return_min", "return_max", "length_sum", "timeouts", "early")
MAX_ENVS = 2 ** 31 - 1           # env slots of one engine: `len` and the flat row index t * n + e of a time step are 32 / 64-bit


def check_sweep(env, sweep):
    """Evaluator's `sweep`, validated as Env.randomize() validates its ranges: -> [(name, p[] index, [factor, ...]), ...] in p[]
    order.  ValueError names the offending key."""
    if sweep is None:
        return []
    if not hasattr(sweep, "items"):
        raise ValueError("Evaluator: sweep must map parameter names to lists of factors")
    if len(sweep) > 12:
        raise ValueError(f"Evaluator: sweep over {len(sweep)} parameters, an env has at most 12")
    out = []
    slots = env.parameter_slots()                      # (RANDOMIZABLE, plus the motor time constant while the lag is on)
    for name, factors in sweep.items():
        if name not in slots:
            raise ValueError(f"Evaluator: {name!r} is not a sweepable parameter of {type(env).__name__} "
                             f"(sweepable: {', '.join(slots)})")
        try:
            if isinstance(factors, (str, bytes)):
                raise TypeError
            vals = [float(v) for v in factors]
        except (TypeError, ValueError):
            raise ValueError(f"Evaluator: the factors of {name!r} must be a list of numbers, got {factors!r}") from None
        if not vals:
            raise ValueError(f"Evaluator: the factor list of {name!r} is empty")
        if not all(math.isfinite(v) and v > 0.0 for v in vals):
            raise ValueError(f"Evaluator: the factors of {name!r} must be finite and > 0, got {vals}")
        out.append((name, slots[name], vals))
    out.sort(key=lambda item: item[1])
    return out


class EvalResult:
    """What evaluate() returns.  The device tensors are read when a field is first asked for (one copy each, then cached)."""

    def __init__(self, cells_dev, returns_dev, sweep, episodes, early_name):
        self._cells_dev, self._returns_dev = cells_dev, returns_dev
        self.sweep_names = tuple(name for name, _, _ in sweep)
        self._levels = [vals for _, _, vals in sweep]
        self.episodes_per_cell = int(episodes)
        self.early_name = early_name             # what "ended early" means for this env: "failure" / "balanced"
        self._cells = self._returns = self._table = self._summary = None

    @property
    def cells(self) -> np.ndarray:
        """f64 [cells][8], tg_eval_cells' rows (CELL_COLUMNS)."""
        if self._cells is None:
            self._cells = self._cells_dev.cpu().numpy()
            self._cells_dev = None
        return self._cells

    @property
    def returns(self) -> np.ndarray:
        """f64 [cells][episodes]: the return of every episode (0 for one that did not end)."""
        if self._returns is None:
            self._returns = self._returns_dev.cpu().numpy().reshape(-1, self.episodes_per_cell)
            self._returns_dev = None
        return self._returns

    def factors(self, cell: int) -> tuple:
        """The factor tuple of a cell, in `sweep_names` order (row-major decode, the last swept parameter fastest)."""
        out, rem = [], int(cell)
        for vals in reversed(self._levels):
            out.append(vals[rem % len(vals)])
            rem //= len(vals)
        return tuple(reversed(out))

    @staticmethod
    def _stats(row) -> dict:
        n = float(row[0])
        if n <= 0:
            nan = float("nan")
            return {"episodes": 0, "return_mean": nan, "return_std": nan, "return_min": nan, "return_max": nan, "length_mean": nan,
                    "timeout_frac": nan, "early_frac": nan}
        mean = float(row[1]) / n
        return {"episodes": int(n), "return_mean": mean, "return_std": math.sqrt(max(float(row[2]) / n - mean * mean, 0.0)),
                "return_min": float(row[3]), "return_max": float(row[4]), "length_mean": float(row[5]) / n,
                "timeout_frac": float(row[6]) / n, "early_frac": float(row[7]) / n}

    @property
    def table(self) -> list:
        """One dict per cell: `cell`, `factors` (tuple in sweep_names order), episodes, return_mean, return_std (population),
        return_min, return_max, length_mean, timeout_frac, early_frac.  A cell without an ended episode reports episodes 0 and NaN."""
        if self._table is None:
            self._table = [{"cell": c, "factors": self.factors(c), **self._stats(row)} for c, row in enumerate(self.cells)]
        return self._table

    @property
    def summary(self) -> dict:
        """The same statistics over every cell together."""
        if self._summary is None:
            c = self.cells
            row = [c[:, 0].sum(), c[:, 1].sum(), c[:, 2].sum(), c[:, 3].min(), c[:, 4].max(), c[:, 5].sum(), c[:, 6].sum(), c[:, 7].sum()]
            self._summary = {"cells": int(c.shape[0]), "early_name": self.early_name, **self._stats(row)}
        return self._summary


class Evaluator:
    """Deterministic (or sampled) evaluation of `policy` on `env`, optionally over a grid of parameter factors.

    episodes: episodes per cell.  sweep: {name: [factor, ...]} with names of `env.RANDOMIZABLE`; None: one cell -- of randomly drawn
    vehicles (from this evaluator's seed) when `env.randomize` is on, else of nominal ones.  Validated here: ValueError names the key.
    Swarm envs are refused (tg_rollout_final_state does not take them)."""

    def __init__(self, env, policy, episodes: int = 256, sweep=None, seed: int = 0, deterministic: bool = True,
                 compute_dtype: Optional[torch.dtype] = None):
        if int(getattr(env, "n_agents", 1)) > 1:
            raise ValueError(f"Evaluator: swarm envs are not supported ({type(env).__name__} with n_agents={env.n_agents}): the clock / "
                             "failure split of an episode's end needs tg_rollout_final_state, which refuses them")
        if isinstance(episodes, bool) or not isinstance(episodes, (int, np.integer)) or episodes < 1:
            raise ValueError(f"Evaluator: episodes must be a positive integer, got {episodes!r}")
        if not isinstance(deterministic, bool):
            raise ValueError(f"Evaluator: deterministic must be True or False, got {deterministic!r}")
        if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= seed < 2 ** 63:
            raise ValueError(f"Evaluator: seed must be an integer in [0, 2^63), got {seed!r}")
        self.env, self.policy = env, policy
        self.episodes, self.seed, self.deterministic = int(episodes), int(seed), deterministic
        self.compute_dtype = compute_dtype
        self._sweep = check_sweep(env, sweep)
        self.sweep_names = tuple(name for name, _, _ in self._sweep)
        self.cells = 1
        for _, _, vals in self._sweep:
            self.cells *= len(vals)
        if self.cells * self.episodes > MAX_ENVS:
            raise ValueError(f"Evaluator: {self.cells} cells x {self.episodes} episodes = {self.cells * self.episodes} env slots do not fit "
                             f"one engine (at most {MAX_ENVS})")
        self.early_name = "balanced" if env.ENV_ID == N.TG_ENV_PENDULUM else "failure"
        self.engine = None
        self._grid = self._values = self._s_final = self._timeout = None

    def _eval_env(self):
        """The env the engine steps: the caller's, as it is now -- with randomisation switched off on the copy when a sweep supplies
        the vehicles (parameters that are not swept are nominal)."""
        env = copy.copy(self.env)
        if self._sweep:
            env._randomize, env._randomize_seed = None, 0
        return env

    def _fill_cells(self, tr, st):
        """DeviceRollout's prologue hook of a sweep: the parameter grid into the per-env table, cell 0's initial states to every cell."""
        eng = self.engine
        if eng.env_params is None:
            eng.env_params = torch.empty(12, eng.n, dtype=torch.float64, device=eng.device)
        K.env_param_grid(eng.params, self._grid, eng.env_params, 0)
        K.eval_tile_states(eng.traj, self.episodes)

    @torch.no_grad()
    def evaluate(self) -> EvalResult:
        from .rollout import DeviceRollout
        if self.engine is None:
            self.engine = DeviceRollout(self._eval_env(), self.policy, self.cells, self.episodes, restart=False, dtype=torch.float32,
                                        seed=self.seed, compute_dtype=self.compute_dtype, use_graph=False)
            if self._sweep:
                dev = self.engine.device
                self._values = torch.tensor([v for _, _, vals in self._sweep for v in vals], dtype=torch.float64, device=dev)
                self._grid = K.param_grid([i for _, i, _ in self._sweep], [len(v) for _, _, v in self._sweep], self._values, self.episodes)
                self.engine._param_source = self._fill_cells
        eng = self.engine
        eng.env = self._eval_env()
        with torch.cuda.device(eng.device):
            # the same experiment every time: stream 0 of this evaluator's seed, on the host (reset, parameter draw) and on the device
            eng._seed_host, eng._stream_host = self.seed, 0
            eng.rng[1].zero_()
            traj = eng.run(deterministic=self.deterministic)
            self._s_final, self._timeout = K.rollout_final_state(eng.params, traj, self._s_final, self._timeout, env_params=eng.env_params,
                                                                 **({"substeps": eng.substeps} if eng.substeps != 1 else {}),
                                                                 **({"motor": traj.motor} if traj.motor is not None else {}))
            returns, cells = K.eval_cells(traj, self._timeout, self.episodes)
        return EvalResult(cells, returns, self._sweep, self.episodes, self.early_name)
