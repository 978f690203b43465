"""Gaussian actor / actor-critic policies with the reference's surface, resident on the GPU.

Mirrors models/neural_network.py:4-77 and policies/actor_critic.py:73-215, :220-378:
same constructor arguments, `forward / log_prob / value / parameters / state_dict /
load_state_dict / save / load / metadata`, attributes `actor`, `critic`, `cov`, and the
same checkpoint formats (`policy.pt`: bare actor state_dict for the actor-only policy,
`{'actor','critic'}` for the actor-critic).  The MLP GEMMs stay on PyTorch-ROCm
(hipBLASLt -> MFMA); sampling, log-prob and the loss head are HIP kernels (rollout.py,
algorithms.py).  The covariance is a diagonal matrix (actor_critic.py:100-103, :247-250): fixed by default, or -- with
`learn_std=True` -- diag(exp(2 log_std)) of a learned per-dimension `log_std` parameter that the learners train on the device.
"""
from __future__ import annotations

import math
import os
from typing import Union

import numpy as np
import torch


def default_device():
    return torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")


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

    def __init__(self, input_dim, output_dim, hidden_dims, activation="ReLU", cov=0.1, device=None, learn_std=False):
        if not isinstance(learn_std, bool):
            raise ValueError(f"learn_std must be True or False, got {learn_std!r}")
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

    def _prep(self, x):
        if isinstance(x, np.ndarray):
            x = torch.from_numpy(x).float()
        return x.to(self.device, torch.float32)

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
        state = self._prep(state)
        mean = self.actor(state)
        with torch.no_grad():
            std = torch.exp(self.log_std).to(mean.device) if self.log_std is not None else torch.sqrt(self.var).to(mean.device)
            action = mean + std * torch.randn(mean.shape, device=mean.device)
        log_prob = self._logp(mean, action)
        value = self.critic(state) if self.critic is not None else None
        return action.detach().cpu().numpy(), log_prob, value

    def log_prob(self, observation, action):
        """actor_critic.py:140-160 / :291-311 -> (log_prob, entropy)."""
        observation, action = self._prep(observation), self._prep(action)
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
        return sd

    def load_state_dict(self, state_dict):
        state_dict = dict(state_dict)
        self._load_log_std(state_dict.pop("log_std", None))
        self.actor.load_state_dict(state_dict)

    def save(self, path):
        torch.save({k: v.cpu() for k, v in self.state_dict().items()}, os.path.join(path, "policy.pt"))

    def load(self, path):
        """The reference has no `load` here, so GRPO resume raises; added."""
        self.load_state_dict(torch.load(os.path.join(path, "policy.pt"), weights_only=True, map_location=self.device))


class GaussianActorCritic_NeuralNetwork(_GaussianBase):
    """policies/actor_critic.py:220-378."""
    has_critic = True

    def __init__(self, input_dim, output_dim, hidden_dims, activation="ReLU", cov=0.1, device=None, learn_std=False):
        super().__init__(input_dim, output_dim, hidden_dims, activation, cov, device, learn_std)
        self.critic = NeuralNetwork(input_dim, 1, hidden_dims, activation).to(self.device)

    def value(self, state):
        return self.critic(self._prep(state)).squeeze()                   # :313-323

    def parameters(self):
        return self._with_log_std(list(self.actor.parameters()) + list(self.critic.parameters()))

    def state_dict(self):
        sd = {"actor": self.actor.state_dict(), "critic": self.critic.state_dict()}
        if self.log_std is not None:
            sd["log_std"] = self.log_std.data                 # (top level, next to "actor" / "critic")
        return sd

    def load_state_dict(self, state_dict):
        self._load_log_std(state_dict.get("log_std"))
        self.actor.load_state_dict(state_dict["actor"])
        self.critic.load_state_dict(state_dict["critic"])

    def load(self, path):
        sd = torch.load(os.path.join(path, "policy.pt"), weights_only=True, map_location=self.device)
        self.load_state_dict(sd)

    def save(self, save_path):
        sd = {k: ({n: v.cpu() for n, v in d.items()} if isinstance(d, dict) else d.cpu()) for k, d in self.state_dict().items()}
        torch.save(sd, os.path.join(save_path, "policy.pt"))
