"""Gaussian actor / actor-critic policies with the reference's surface, resident on the GPU.

Mirrors models/neural_network.py:4-77 and policies/actor_critic.py:73-215, :220-378:
same constructor arguments, `forward / log_prob / value / parameters / state_dict /
load_state_dict / save / load / metadata`, attributes `actor`, `critic`, `cov`, and the
same checkpoint formats (`policy.pt`: bare actor state_dict for the actor-only policy,
`{'actor','critic'}` for the actor-critic).  The MLP GEMMs stay on PyTorch-ROCm
(hipBLASLt -> MFMA); sampling, log-prob and the loss head are HIP kernels (rollout.py,
algorithms.py).  The covariance is a diagonal matrix (actor_critic.py:100-103, :247-250): fixed by default, or -- with
`learn_std=True` -- diag(exp(2 log_std)) of a learned per-dimension `log_std` parameter that the learners train on the device.
With `normalize_obs=True` every path reads states through running per-feature statistics (`policy.obs_norm`, class ObsNorm).
With `normalize_value=True` (actor-critic only) the critic predicts returns standardised with running statistics
(`policy.value_norm`, class ValueNorm); `policy.value()` keeps returning returns.  With `popart=True` as well, PPO rescales the
critic's last layer whenever those statistics move, so that the denormalised predictions stay where they were.
"""
from __future__ import annotations

import math
import os
from typing import Union

import numpy as np
import torch


def default_device():
    return torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")


class ObsNorm:
    """Running observation statistics of a policy built with normalize_obs=True, on the policy's device:
        count f64 [1], mean f64 [S], m2 f64 [S] (sum of squared deviations; var = m2 / count is the population variance),
        table f32 [2][S] = {(float)mean, (float)(1 / sqrt(var + eps))} -- ONE allocation for the life of the policy, rewritten in
        place (count == 0: mean 0, rstd 1), so captured graphs and cached kernel arguments stay valid.
    The normalised observation is one fp32 expression on every path (rollout kernels, learner rows, this class's normalize()):
        xn[k] = clamp((x[k] - table[0][k]) * table[1][k], -clip, +clip)
    subtract, multiply and clamp each rounded on its own; an f64 observation is rounded to f32 first; bf16 paths round xn once.
    The learners call update(traj) at the entry of learn() unless frozen; trajectories keep the RAW observations.  `clip` and `eps`
    are fixed at construction (a captured rollout graph holds the clamp by value).  A deepcopy of a policy owns its own statistics;
    the learners make their old_policy share the policy's object."""

    def __init__(self, dim: int, clip, eps: float, device):
        self.dim, self._clip, self._eps = int(dim), clip, float(eps)
        self.frozen = False
        dev = torch.device(device)
        self.count = torch.zeros(1, dtype=torch.float64, device=dev)
        self.mean = torch.zeros(self.dim, dtype=torch.float64, device=dev)
        self.m2 = torch.zeros(self.dim, dtype=torch.float64, device=dev)
        self.table = torch.stack([torch.zeros(self.dim), torch.ones(self.dim)]).to(dev, torch.float32).contiguous()
        self._work = self._batch = None

    @property
    def clip(self):
        return self._clip

    @property
    def eps(self) -> float:
        return self._eps

    @property
    def clip_value(self) -> float:
        """The clamp as the kernels take it: +inf for obs_clip=None."""
        return math.inf if self.clip is None else float(self.clip)

    @property
    def var(self) -> torch.Tensor:
        return self.m2 / self.count.clamp_min(1.0)

    def freeze(self):
        self.frozen = True
        return self

    def unfreeze(self):
        self.frozen = False
        return self

    def to(self, device):
        """Moves the statistics (policy.to): a move is a new allocation on the new device -- engines are built after it."""
        dev = torch.device(device)
        if dev != self.count.device:
            self.count, self.mean, self.m2, self.table = (t.to(dev) for t in (self.count, self.mean, self.m2, self.table))
            self._work = self._batch = None
        return self

    @torch.no_grad()
    def _merge(self, batch=None) -> None:
        """Chan's merge of batch f64 [S][3] = {n_b, sum (x - mean), sum (x - mean)^2} into the statistics, then the table in place:
        tg_obs_norm_merge on the device; the same operations in torch for a CPU policy (the host path)."""
        if self.count.is_cuda:
            from . import hip_ops as K
            with torch.cuda.device(self.count.device):
                K.obs_norm_merge(batch, self.eps, self.count, self.mean, self.m2, self.table)
            return
        if batch is not None and float(batch[0, 0]) > 0:
            na, nb, sd, sq = self.count[0].clone(), batch[0, 0], batch[:, 1], batch[:, 2]
            n = na + nb
            db = sd / nb
            m2b = (sq - sd * db).clamp_min(0.0)
            self.mean.add_(db * (nb / n))
            self.m2.copy_((self.m2 + m2b) + (db * db) * (na * (nb / n)))
            self.count.fill_(float(n))
        if float(self.count[0]) > 0:
            self.table[0].copy_(self.mean.float())
            self.table[1].copy_((1.0 / torch.sqrt(self.m2 / self.count + self.eps)).float())
        else:
            self.table[0].zero_()
            self.table[1].fill_(1.0)

    @torch.no_grad()
    def update(self, traj, process_group=None) -> None:
        """Merge the valid (t, e) observations of a device trajectory into the statistics and rewrite the table: tg_obs_moments about
        the current mean (identical on every rank, so one pass is safe), ONE all-reduce of the f64 [S][3], tg_obs_norm_merge.  No
        host round trip.  Runs whether or not the policy is frozen: the learners ask `frozen` before they call."""
        from . import distributed as D
        from . import hip_ops as K
        if traj.S != self.dim or traj.obs.device != self.count.device:
            raise ValueError(f"obs_norm.update: a trajectory of {traj.S} features on {traj.obs.device}, statistics of {self.dim} on {self.count.device}")
        with torch.cuda.device(self.count.device):
            need = K.obs_moments_workspace(traj.T * traj.n, self.dim) // 8
            if self._work is None or self._work.numel() < need:
                self._work = torch.empty(need, dtype=torch.float64, device=self.count.device)
            if self._batch is None:
                self._batch = torch.empty(self.dim, 3, dtype=torch.float64, device=self.count.device)
            K.obs_moments(traj, self.mean, self._batch, self._work)
            D.allreduce_sum_(self._batch, process_group, "obs_moments")
            K.obs_norm_merge(self._batch, self.eps, self.count, self.mean, self.m2, self.table)

    @torch.no_grad()
    def set(self, mean, var, count) -> None:
        """Statistics from outside (tests, imported normalisers): per-feature mean and population variance of `count` samples."""
        mean = torch.as_tensor(mean, dtype=torch.float64).reshape(-1)
        var = torch.as_tensor(var, dtype=torch.float64).reshape(-1)
        count = float(count)
        if mean.numel() != self.dim or var.numel() != self.dim or not (count >= 0 and math.isfinite(count)) or bool((var < 0).any()):
            raise ValueError(f"obs_norm.set: mean and var of {self.dim} features (var >= 0) and a finite count >= 0, got "
                             f"{tuple(mean.shape)}, {tuple(var.shape)}, {count!r}")
        self.count.fill_(count)
        self.mean.copy_(mean)
        self.m2.copy_(var * count)
        self._merge(None)

    def normalize(self, x: torch.Tensor) -> torch.Tensor:
        """The normalised observation of x [..., S] in torch (the host path): float32, the kernels' three operations."""
        tab = self.table.to(x.device)
        xn = (x.to(torch.float32) - tab[0]) * tab[1]
        return xn if self.clip is None else torch.clamp(xn, -float(self.clip), float(self.clip))

    def state(self) -> dict:
        return {"obs_norm.count": self.count, "obs_norm.mean": self.mean, "obs_norm.m2": self.m2}

    @torch.no_grad()
    def load_state(self, count, mean, m2) -> None:
        count, mean, m2 = (torch.as_tensor(t, dtype=torch.float64).reshape(-1) for t in (count, mean, m2))
        if count.numel() != 1 or mean.numel() != self.dim or m2.numel() != self.dim:
            raise ValueError(f"obs_norm statistics of shapes {tuple(count.shape)}, {tuple(mean.shape)}, {tuple(m2.shape)} do not fit "
                             f"{self.dim} features")
        self.count.copy_(count)
        self.mean.copy_(mean)
        self.m2.copy_(m2)
        self._merge(None)


OBS_NORM_KEYS = ("obs_norm.count", "obs_norm.mean", "obs_norm.m2")


class ValueNorm:
    """Running statistics of the returns a critic is trained on (normalize_value=True; MAPPO's ValueNorm), on the policy's device:
        count, mean, m2 f64 [1] each (m2: sum of squared deviations; var = m2 / count is the population variance),
        table f32 [4] = {(float)mean, (float)sigma, (float)(1 / sigma), 0}, sigma = sqrt(m2 / count + eps) in f64 -- ONE allocation for
        the life of the policy, rewritten in place (count == 0: {0, 1, 1, 0}, the identity).
    The critic predicts (R - mean) / sigma.  denormalize(v) = v * table[1] + table[0] and normalize(r) = (r - table[0]) * table[2] are
    fp32 expressions of two separately rounded operations, on the device kernels and here alike.  PPO.learn() denormalises every
    critic value that enters a return with the table as it stands at its entry, then merges the batch's returns (unless frozen) and
    regresses the critic onto normalize(R) of the merged statistics.  `eps` is fixed at construction.  A deepcopy of a policy owns
    its own statistics; the learners make their old_policy share the policy's object.

    popart=False (the default): the critic head is NOT rescaled when the statistics move -- the function the critic represents, read
    in return units, jumps by (sigma' - sigma) v + (mean' - mean) at every merge.  popart=True (PopArt, "preserve outputs
    precisely"): a merge that is handed the critic's last Linear rewrites it in the same step, w' = w sigma / sigma',
    b' = (b sigma + mean - mean') / sigma', so that every denormalised prediction stays where it was ("PopArt").
    Only _merge() with a head rescales; set() and load_state() never do (a checkpoint's weights and statistics already agree)."""

    def __init__(self, eps: float, device, popart: bool = False):
        self._eps = float(eps)
        self.frozen = False
        self.popart = bool(popart)
        dev = torch.device(device)
        self.count = torch.zeros(1, dtype=torch.float64, device=dev)
        self.mean = torch.zeros(1, dtype=torch.float64, device=dev)
        self.m2 = torch.zeros(1, dtype=torch.float64, device=dev)
        self.table = torch.tensor([0.0, 1.0, 1.0, 0.0], dtype=torch.float32).to(dev)

    @property
    def eps(self) -> float:
        return self._eps

    @property
    def var(self) -> torch.Tensor:
        return self.m2 / self.count.clamp_min(1.0)

    def freeze(self):
        self.frozen = True
        return self

    def unfreeze(self):
        self.frozen = False
        return self

    def to(self, device):
        """Moves the statistics (policy.to): a move is a new allocation on the new device."""
        dev = torch.device(device)
        if dev != self.count.device:
            self.count, self.mean, self.m2, self.table = (t.to(dev) for t in (self.count, self.mean, self.m2, self.table))
        return self

    @torch.no_grad()
    def _merge(self, moments=None, norm8=None, head=None) -> None:
        """Chan's merge of moments f64 [3] = {n_b, sum, sum of squares} of a batch of returns into the statistics, then the table in
        place and -- norm8 given (tg_ppo_norm's f32 [8]) -- its entries 2 and 3 <- table[0], table[2]: tg_value_norm_merge on the
        device; the same operations in torch for a CPU policy (the host path).
        head (the critic's last Linear, [1][H] weight and [1] bias in fp32; None: the plain merge): PopArt's rescale with the merge --
        tg_value_norm_merge_popart on the device, which writes the masters by raw pointer (the caller sees to the derived layouts);
        the same f64 operations in torch on the host.  The head keeps its bits when nothing was merged, when the statistics were
        empty before the merge, or when either sigma is not a positive finite number."""
        if head is not None:
            w, b = head.weight, head.bias
            if not (w.dtype == b.dtype == torch.float32 and w.is_contiguous() and b.is_contiguous() and w.dim() == 2 and w.shape[0] == 1
                    and tuple(b.shape) == (1,) and w.device == b.device == self.count.device):
                raise ValueError(f"PopArt rescales a contiguous fp32 head of weight [1][H] and bias [1] on {self.count.device}, got weight "
                                 f"{w.dtype} {tuple(w.shape)} on {w.device}, bias {b.dtype} {tuple(b.shape)} on {b.device}")
        if self.count.is_cuda:
            from . import hip_ops as K
            with torch.cuda.device(self.count.device):
                if head is None:
                    K.value_norm_merge(moments, self.eps, self.count, self.mean, self.m2, self.table, norm8)
                else:
                    K.value_norm_merge_popart(moments, self.eps, self.count, self.mean, self.m2, self.table, norm8, head.weight, head.bias)
            return
        merged = moments is not None and float(moments[0]) > 0
        if head is not None and merged and float(self.count[0]) > 0:
            mean_a, sigma_a = self.mean.clone(), torch.sqrt(self.m2 / self.count + self.eps)
        else:
            head = None
        if merged:
            na, nb, s1, s2 = self.count[0].clone(), moments[0], moments[1], moments[2]
            mb = s1 / nb
            m2b = (s2 - s1 * mb).clamp_min(0.0)
            n = na + nb
            w = nb / n
            db = mb - self.mean[0]
            self.mean.add_(db * w)
            self.m2.copy_((self.m2 + m2b) + (db * db) * (na * w))
            self.count.fill_(float(n))
        if float(self.count[0]) > 0:
            sigma = torch.sqrt(self.m2 / self.count + self.eps)
            self.table[0:1].copy_(self.mean.float())
            self.table[1:2].copy_(sigma.float())
            self.table[2:3].copy_((1.0 / sigma).float())
        else:
            self.table.copy_(torch.tensor([0.0, 1.0, 1.0, 0.0]))
        self.table[3] = 0.0
        if norm8 is not None:
            norm8[2], norm8[3] = self.table[0], self.table[2]
        if head is not None:
            sigma_n = torch.sqrt(self.m2 / self.count + self.eps)
            if all(math.isfinite(float(s)) and float(s) > 0 for s in (sigma_a, sigma_n)):
                # (every f64 operation a torch op of its own: rounded one by one, as the kernel's)
                head.weight.copy_((head.weight.double() * (sigma_a / sigma_n)).float())
                head.bias.copy_(((head.bias.double() * sigma_a + (mean_a - self.mean)) / sigma_n).float())

    @torch.no_grad()
    def set(self, mean, var, count) -> None:
        """Statistics from outside (tests, imported normalisers): mean and population variance of `count` returns."""
        mean, var, count = float(mean), float(var), float(count)
        if not (math.isfinite(mean) and math.isfinite(var) and var >= 0 and math.isfinite(count) and count >= 0):
            raise ValueError(f"value_norm.set: a finite mean, a finite var >= 0 and a finite count >= 0, got {mean!r}, {var!r}, {count!r}")
        self.count.fill_(count)
        self.mean.fill_(mean)
        self.m2.copy_(torch.tensor([var], dtype=torch.float64) * count)
        self._merge(None)

    def denormalize(self, v: torch.Tensor) -> torch.Tensor:
        """The return a critic output stands for: v * sigma + mean in float32, multiply and add each rounded on its own."""
        tab = self.table.to(v.device)
        return v.to(torch.float32) * tab[1] + tab[0]

    def normalize(self, r: torch.Tensor) -> torch.Tensor:
        """The critic's target for a return: (r - mean) * (1 / sigma) in float32, the loss heads' two operations."""
        tab = self.table.to(r.device)
        return (r.to(torch.float32) - tab[0]) * tab[2]

    def state(self) -> dict:
        return {"value_norm.count": self.count, "value_norm.mean": self.mean, "value_norm.m2": self.m2}

    @torch.no_grad()
    def load_state(self, count, mean, m2) -> None:
        count, mean, m2 = (torch.as_tensor(t, dtype=torch.float64).reshape(-1) for t in (count, mean, m2))
        if count.numel() != 1 or mean.numel() != 1 or m2.numel() != 1:
            raise ValueError(f"value_norm statistics of shapes {tuple(count.shape)}, {tuple(mean.shape)}, {tuple(m2.shape)}: one number each")
        self.count.copy_(count)
        self.mean.copy_(mean)
        self.m2.copy_(m2)
        self._merge(None)


VALUE_NORM_KEYS = ("value_norm.count", "value_norm.mean", "value_norm.m2")


class NeuralNetwork(torch.nn.Module):
    """Sequential(Linear, act, ..., Linear).  models/neural_network.py:4-77
    (parameter names `network.{0,2,...}.{weight,bias}` match the reference checkpoints)."""

    def __init__(self, input_dim: int, output_dim: int, hidden_dims: list, activation: Union[str, list] = "ReLU"):
        super().__init__()
        self.input_dim, self.output_dim, self.hidden_dims = input_dim, output_dim, hidden_dims
        if hidden_dims:
            if isinstance(activation, str):
                activations = [activation] * len(hidden_dims)
            elif isinstance(activation, list):
                assert len(activation) == len(hidden_dims), \
                    "Number of activation functions must equal the number of hidden layers."
                activations = activation
            else:
                raise TypeError("activation must be either a string or a list of strings.")
            dims = [input_dim] + list(hidden_dims)
            layers = []
            for i in range(len(hidden_dims)):
                layers.append(torch.nn.Linear(dims[i], dims[i + 1]))
                layers.append(getattr(torch.nn, activations[i])())
            layers.append(torch.nn.Linear(dims[-1], output_dim))
            self.network = torch.nn.Sequential(*layers)
        else:
            self.network = torch.nn.Sequential(torch.nn.Linear(input_dim, output_dim))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.network(x)


class ActorCritic:
    """policies/actor_critic.py:9-26."""

    def __call__(self, state):
        return self.forward(state)


class _GaussianBase(ActorCritic):
    has_critic = False

    def __init__(self, input_dim, output_dim, hidden_dims, activation="ReLU", cov=0.1, device=None, learn_std=False, *,
                 normalize_obs=False, obs_clip=10.0, obs_eps=1e-8):
        if not isinstance(learn_std, bool):
            raise ValueError(f"learn_std must be True or False, got {learn_std!r}")
        if not isinstance(normalize_obs, bool):
            raise ValueError(f"normalize_obs must be True or False, got {normalize_obs!r}")
        if obs_clip is not None and (isinstance(obs_clip, bool) or not isinstance(obs_clip, (int, float))
                                     or not (math.isfinite(obs_clip) and obs_clip > 0)):
            raise ValueError(f"obs_clip must be None or a finite number > 0, got {obs_clip!r}")
        if isinstance(obs_eps, bool) or not isinstance(obs_eps, (int, float)) or not (math.isfinite(obs_eps) and obs_eps >= 0):
            raise ValueError(f"obs_eps must be a finite number >= 0, got {obs_eps!r}")
        self.input_dim, self.output_dim = input_dim, output_dim
        self.hidden_dims, self.activation = hidden_dims, activation
        self.device = torch.device(device) if device is not None else default_device()
        self.learn_std = learn_std
        self.log_std = None
        if isinstance(cov, list):
            self.cov = torch.diag(torch.tensor(cov, dtype=torch.float32))        # actor_critic.py:100-103
        else:
            self.cov = torch.diag(torch.tensor([cov] * output_dim, dtype=torch.float32))
        if learn_std:
            # one parameter per action dimension, state-independent: cov = diag(exp(2 log_std)) from here on
            self.log_std = torch.nn.Parameter((0.5 * torch.log(self._diag_of(self._cov))).to(self.device, torch.float32))
            del self._cov                                 # (the constructor's matrix is not the covariance any more)
        self.actor = NeuralNetwork(input_dim, output_dim, hidden_dims, activation).to(self.device)
        self.critic = None
        # running observation normalisation: None when off (no path then touches a table).  The row kernel takes up to 64 features.
        if normalize_obs and input_dim > 64:
            raise ValueError(f"normalize_obs=True supports up to 64 observation features (tg_obs_normalize_rows), got input_dim={input_dim}")
        self.obs_norm = ObsNorm(input_dim, None if obs_clip is None else float(obs_clip), obs_eps, self.device) if normalize_obs else None
        self.value_norm = None                              # (running value normalisation: the actor-critic's keyword)

    # ---- helpers ----------------------------------------------------------
    @staticmethod
    def _diag_of(cov) -> torch.Tensor:
        cov = torch.as_tensor(cov)
        if cov.dim() != 2 or cov.shape[0] != cov.shape[1] or bool((cov - torch.diag(torch.diagonal(cov))).any()):
            raise ValueError(f"policy covariance must be a diagonal square matrix (the rollout and learner kernels sample and "
                             f"score each action dimension on its own); got shape {tuple(cov.shape)}:\n{cov}")
        return torch.diagonal(cov).clone()

    @property
    def cov(self):
        """The covariance matrix.  Fixed policies: the matrix last assigned.  learn_std=True: diag(exp(2 log_std)) as a detached CPU
        tensor (one small device read); assigning a diagonal matrix writes log_std in place."""
        if self.log_std is None:
            return self._cov
        return torch.diag(torch.exp(2.0 * self.log_std.detach()).cpu())

    @cov.setter
    def cov(self, value):
        if self.log_std is None:
            self._cov = value
            return
        d = self._diag_of(value).to(torch.float32)
        if d.numel() != self.output_dim or not bool((d > 0).all()):
            raise ValueError(f"a learned-std policy's covariance must be a positive diagonal {self.output_dim} x {self.output_dim} matrix, got\n{value}")
        with torch.no_grad():
            self.log_std.copy_(0.5 * torch.log(d))

    @property
    def var(self) -> torch.Tensor:
        """diag(cov) as a CPU float32 vector.  The sampling kernels, log_prob and the loss heads all take the covariance as this
        vector, so a covariance with off-diagonal terms (which the reference's MultivariateNormal would honour) is refused."""
        return self._diag_of(self.cov)

    def to(self, device):
        self.device = torch.device(device)
        self.actor.to(self.device)
        if self.critic is not None:
            self.critic.to(self.device)
        if self.log_std is not None:
            self.log_std.data = self.log_std.data.to(self.device)
        if self.obs_norm is not None:
            self.obs_norm.to(self.device)
        if self.value_norm is not None:
            self.value_norm.to(self.device)
        return self

    def _with_log_std(self, params):
        """`params` (the nets' parameters in their existing order), then log_std LAST when it is learned."""
        return list(params) + [self.log_std] if self.log_std is not None else params

    def _load_log_std(self, value):
        """load_state_dict's `log_std` entry: absent -> the current value stays; present on a fixed policy -> refused."""
        if value is None:
            return
        if self.log_std is None:
            raise ValueError("the state dict holds a learned 'log_std', this policy's covariance is fixed: construct it with "
                             "learn_std=True (or drop the key)")
        value = torch.as_tensor(value, dtype=torch.float32)
        if value.shape != self.log_std.shape:
            raise ValueError(f"log_std of shape {tuple(value.shape)} does not fit {tuple(self.log_std.shape)}")
        with torch.no_grad():
            self.log_std.copy_(value)

    def _obs_norm_state(self) -> dict:
        return self.obs_norm.state() if self.obs_norm is not None else {}

    def _load_obs_norm(self, state_dict) -> None:
        """load_state_dict's `obs_norm.*` entries: they and normalize_obs go together, either way round."""
        have = [k for k in OBS_NORM_KEYS if k in state_dict]
        if have and self.obs_norm is None:
            raise ValueError("the state dict holds observation statistics ('obs_norm.*'), this policy reads raw observations: construct "
                             "it with normalize_obs=True (or drop the keys)")
        if self.obs_norm is not None:
            if len(have) != len(OBS_NORM_KEYS):
                raise ValueError("this policy normalises its observations, the state dict holds no 'obs_norm.count' / 'obs_norm.mean' / "
                                 "'obs_norm.m2': it was saved by a policy without normalize_obs=True")
            self.obs_norm.load_state(*(state_dict[k] for k in OBS_NORM_KEYS))

    def _prep(self, x):
        if isinstance(x, np.ndarray):
            x = torch.from_numpy(x).float()
        return x.to(self.device, torch.float32)

    def _prep_obs(self, x):
        """_prep of an observation: what the nets read -- the normalised observation when normalize_obs is on."""
        x = self._prep(x)
        return self.obs_norm.normalize(x) if self.obs_norm is not None else x

    def _logp(self, mean, action):
        k = self.output_dim
        if self.log_std is not None:                   # differentiable in log_std
            ls = self.log_std.to(mean.device)
            quad = (((action - mean) ** 2) * torch.exp(-2.0 * ls)).sum(-1)
            return -0.5 * quad - 0.5 * k * math.log(2 * math.pi) - ls.sum()
        var = self.var.to(mean.device)
        quad = (((action - mean) ** 2) / var).sum(-1)
        return -0.5 * quad - 0.5 * k * math.log(2 * math.pi) - 0.5 * torch.log(var).sum()

    def _entropy(self, shape, device):
        if self.log_std is not None:
            h = 0.5 * self.output_dim * (1.0 + math.log(2 * math.pi)) + self.log_std.to(device).sum()
            return h.expand(shape)
        var = self.var
        h = 0.5 * self.output_dim * (1.0 + math.log(2 * math.pi)) + 0.5 * float(torch.log(var).sum())
        return torch.full(shape, h, dtype=torch.float32, device=device)

    # ---- reference surface ---------------------------------------------------
    def forward(self, state):
        """actor_critic.py:107-138 / :255-289: sample a ~ N(actor(state), cov).
        Returns (action ndarray float32, log_prob Tensor, value Tensor|None)."""
        state = self._prep_obs(state)
        mean = self.actor(state)
        with torch.no_grad():
            std = torch.exp(self.log_std).to(mean.device) if self.log_std is not None else torch.sqrt(self.var).to(mean.device)
            action = mean + std * torch.randn(mean.shape, device=mean.device)
        log_prob = self._logp(mean, action)
        value = self.critic(state) if self.critic is not None else None
        return action.detach().cpu().numpy(), log_prob, value

    def log_prob(self, observation, action):
        """actor_critic.py:140-160 / :291-311 -> (log_prob, entropy)."""
        observation, action = self._prep_obs(observation), self._prep(action)
        mean = self.actor(observation)
        return self._logp(mean, action), self._entropy(mean.shape[:-1], mean.device)

    def metadata(self):
        return {
            "input_dim": self.input_dim,
            "output_dim": self.output_dim,
            "hidden_dims": self.hidden_dims,
            "activation": self.activation,
            "cov": self.cov.tolist() if isinstance(self.cov, torch.Tensor) else self.cov,
            "num_parameters": sum(p.numel() for p in self.parameters()),
            **({"learn_std": True} if self.log_std is not None else {}),
            **({"normalize_obs": True, "obs_clip": self.obs_norm.clip} if self.obs_norm is not None else {}),
            **({"normalize_value": True, "value_eps": self.value_norm.eps} if self.value_norm is not None else {}),
        }


class GaussianActor_NeuralNetwork(_GaussianBase):
    """policies/actor_critic.py:73-215."""

    def value(self, state):
        return [None] * state.shape[0]                                    # :162-173

    def parameters(self):
        return self._with_log_std(self.actor.parameters())

    def state_dict(self):
        sd = self.actor.state_dict()
        if self.log_std is not None:
            sd["log_std"] = self.log_std.data                 # (next to the `network.*` keys)
        sd.update(self._obs_norm_state())
        return sd

    def load_state_dict(self, state_dict):
        state_dict = dict(state_dict)
        self._load_log_std(state_dict.pop("log_std", None))
        self._load_obs_norm(state_dict)
        for k in OBS_NORM_KEYS:
            state_dict.pop(k, None)
        self.actor.load_state_dict(state_dict)

    def save(self, path):
        torch.save({k: v.cpu() for k, v in self.state_dict().items()}, os.path.join(path, "policy.pt"))

    def load(self, path):
        """The reference has no `load` here, so GRPO resume raises; added."""
        self.load_state_dict(torch.load(os.path.join(path, "policy.pt"), weights_only=True, map_location=self.device))


def _check_privileged(ranges):
    """privileged_critic's argument, validated as Env.randomize() validates its ranges: {name: (lo, hi)} in the caller's order, or None
    for None / {} (off).  The names are the env's business: the learner checks them against the env that rolled the buffer out."""
    if ranges is None or (hasattr(ranges, "items") and len(ranges) == 0):
        return None
    if not hasattr(ranges, "items"):
        raise ValueError(f"privileged_critic must map parameter names to (lo, hi), as Env.randomize() takes them, got {ranges!r}")
    if len(ranges) > 12:
        raise ValueError(f"privileged_critic: {len(ranges)} parameters, an env has at most 12")
    checked = {}
    for name, rng in ranges.items():
        if not isinstance(name, str):
            raise ValueError(f"privileged_critic: parameter names are strings, got {name!r}")
        try:
            lo, hi = (float(v) for v in rng)
        except (TypeError, ValueError):
            raise ValueError(f"privileged_critic: the range of {name!r} must be a (lo, hi) pair of numbers, got {rng!r}") from None
        if not (math.isfinite(lo) and math.isfinite(hi) and 0.0 < lo <= hi):
            raise ValueError(f"privileged_critic: the factor range of {name!r} must be finite with 0 < lo <= hi, got ({lo}, {hi})")
        checked[name] = (lo, hi)
    return checked


class GaussianActorCritic_NeuralNetwork(_GaussianBase):
    """policies/actor_critic.py:220-378.

    privileged_critic={name: (lo, hi)} (the mapping one passes to Env.randomize; None / {}: off): an asymmetric actor-critic.  The
    actor reads the observation; the critic, which only training uses, reads P = len(mapping) more columns behind it, one per
    randomised physical parameter in the mapping's order.  For a multiplicative factor f on the nominal value the column holds
    x = (f - c) * s with c = 0.5 * (lo + hi), s = 2 / (hi - lo) (0 when hi == lo): the drawn range on [-1, 1], formed in f64 with
    every operation rounded on its own and rounded once to f32.  These columns pass neither obs_norm nor its clamp."""
    has_critic = True

    def __init__(self, input_dim, output_dim, hidden_dims, activation="ReLU", cov=0.1, device=None, learn_std=False, *,
                 normalize_obs=False, obs_clip=10.0, obs_eps=1e-8, normalize_value=False, value_eps=1e-8, privileged_critic=None,
                 popart=False):
        if not isinstance(normalize_value, bool):
            raise ValueError(f"normalize_value must be True or False, got {normalize_value!r}")
        if not isinstance(popart, bool):
            raise ValueError(f"popart must be True or False, got {popart!r}")
        if popart and not normalize_value:
            raise ValueError("popart=True rescales the critic head when the return statistics move: it needs normalize_value=True")
        if isinstance(value_eps, bool) or not isinstance(value_eps, (int, float)) or not (math.isfinite(value_eps) and value_eps >= 0):
            raise ValueError(f"value_eps must be a finite number >= 0, got {value_eps!r}")
        privileged_critic = _check_privileged(privileged_critic)
        super().__init__(input_dim, output_dim, hidden_dims, activation, cov, device, learn_std, normalize_obs=normalize_obs,
                         obs_clip=obs_clip, obs_eps=obs_eps)
        # None when off: the critic then reads what the actor reads, and nothing below is touched
        self.privileged_critic = privileged_critic
        self.privileged_center = [0.5 * (lo + hi) for lo, hi in (privileged_critic or {}).values()]          # (Python floats, once)
        self.privileged_scale = [2.0 / (hi - lo) if hi > lo else 0.0 for lo, hi in (privileged_critic or {}).values()]
        self.critic = NeuralNetwork(input_dim + len(self.privileged_center), 1, hidden_dims, activation).to(self.device)
        # running value normalisation: None when off (the critic then predicts whatever its learner regresses it onto)
        # (popart=True: PPO hands the merge the critic's last layer, which is then rescaled with the statistics)
        self.value_norm = ValueNorm(value_eps, self.device, popart) if normalize_value else None

    def privileged_features(self, factors, shape=()) -> torch.Tensor:
        """The critic's privileged columns f32 [..., P] of multiplicative factors [..., P] in column order (None: the nominal vehicle,
        every factor 1, broadcast to `shape`): (f - c) * s in f64, subtract and multiply each rounded on its own, one rounding to f32."""
        P = len(self.privileged_center)
        if factors is None:
            f = torch.ones(tuple(shape) + (P,), dtype=torch.float64, device=self.device)
        else:
            if isinstance(factors, np.ndarray):
                factors = torch.from_numpy(factors)
            f = torch.as_tensor(factors).to(self.device, torch.float64)
            if f.shape[-1:] != (P,):
                raise ValueError(f"factors must hold {P} columns (privileged_critic: {', '.join(self.privileged_critic)}), got shape {tuple(f.shape)}")
        c = torch.tensor(self.privileged_center, dtype=torch.float64, device=self.device)
        s = torch.tensor(self.privileged_scale, dtype=torch.float64, device=self.device)
        return ((f - c) * s).to(torch.float32)

    def _critic_input(self, obs, factors):
        """What the critic reads: the prepared observation, and the privileged columns behind it when there are any."""
        if self.privileged_critic is None:
            if factors is not None:
                raise ValueError("factors were given, this policy's critic is not privileged: construct it with privileged_critic={...}")
            return obs
        x = self.privileged_features(factors, obs.shape[:-1])
        return torch.cat([obs, x.expand(obs.shape[:-1] + x.shape[-1:])], dim=-1)

    def forward(self, state, factors=None):
        """_GaussianBase.forward with the critic's value taken of (state, factors): factors [..., P] in column order, None = nominal."""
        if self.privileged_critic is None and factors is None:
            return super().forward(state)
        state = self._prep_obs(state)
        mean = self.actor(state)
        with torch.no_grad():
            std = torch.exp(self.log_std).to(mean.device) if self.log_std is not None else torch.sqrt(self.var).to(mean.device)
            action = mean + std * torch.randn(mean.shape, device=mean.device)
        return action.detach().cpu().numpy(), self._logp(mean, action), self.critic(self._critic_input(state, factors))

    def value(self, state, factors=None):
        v = self.critic(self._critic_input(self._prep_obs(state), factors)).squeeze()                  # :313-323
        return v if self.value_norm is None else self.value_norm.denormalize(v)

    def metadata(self):
        md = super().metadata()
        if self.value_norm is not None and self.value_norm.popart:
            md["popart"] = True
        if self.privileged_critic is not None:
            md["privileged_critic"] = {k: [lo, hi] for k, (lo, hi) in self.privileged_critic.items()}
        return md

    def _check_critic_width(self, state_dict) -> None:
        """load_state_dict's guard: the checkpoint's critic reads input_dim + P columns, or the error names privileged_critic."""
        w = state_dict.get("critic", {}).get("network.0.weight") if hasattr(state_dict.get("critic", None), "get") else None
        if w is None:
            return
        have, want, P = int(w.shape[1]), self.critic.network[0].in_features, len(self.privileged_center)
        if have == want:
            return
        if P == 0:
            raise ValueError(f"the checkpoint's critic reads {have} columns, this policy's {want}: it was saved by a policy with "
                             f"privileged_critic of {have - self.input_dim} parameter(s) -- construct this one with the same privileged_critic mapping")
        raise ValueError(f"the checkpoint's critic reads {have} columns, this policy's critic {self.input_dim} + {P} = {want} "
                         f"(privileged_critic: {', '.join(self.privileged_critic)}): the privileged_critic mappings differ")

    def parameters(self):
        return self._with_log_std(list(self.actor.parameters()) + list(self.critic.parameters()))

    def _load_value_norm(self, state_dict) -> None:
        """load_state_dict's `value_norm.*` entries: they and normalize_value go together, either way round."""
        have = [k for k in VALUE_NORM_KEYS if k in state_dict]
        if have and self.value_norm is None:
            raise ValueError("the state dict holds return statistics ('value_norm.*'), this policy's critic predicts unnormalised "
                             "targets: construct it with normalize_value=True (or drop the keys)")
        if self.value_norm is not None:
            if len(have) != len(VALUE_NORM_KEYS):
                raise ValueError("this policy normalises its value targets, the state dict holds no 'value_norm.count' / "
                                 "'value_norm.mean' / 'value_norm.m2': it was saved by a policy without normalize_value=True")
            self.value_norm.load_state(*(state_dict[k] for k in VALUE_NORM_KEYS))

    def state_dict(self):
        sd = {"actor": self.actor.state_dict(), "critic": self.critic.state_dict()}
        if self.log_std is not None:
            sd["log_std"] = self.log_std.data                 # (top level, next to "actor" / "critic")
        sd.update(self._obs_norm_state())
        if self.value_norm is not None:
            sd.update(self.value_norm.state())
        return sd

    def load_state_dict(self, state_dict):
        self._check_critic_width(state_dict)
        self._load_log_std(state_dict.get("log_std"))
        self._load_obs_norm(state_dict)
        self._load_value_norm(state_dict)
        self.actor.load_state_dict(state_dict["actor"])
        self.critic.load_state_dict(state_dict["critic"])

    def load(self, path):
        sd = torch.load(os.path.join(path, "policy.pt"), weights_only=True, map_location=self.device)
        self.load_state_dict(sd)

    def save(self, save_path):
        sd = {k: ({n: v.cpu() for n, v in d.items()} if isinstance(d, dict) else d.cpu()) for k, d in self.state_dict().items()}
        torch.save(sd, os.path.join(save_path, "policy.pt"))
