"""Plain float64 restatement of DeviceActor's policy step (csrc/policy_step.hip), for the tests: the MLP in float64 from the float32
parameters, eps from philox_fp64 keyed (seed, env_offset + i, calls[i], STREAM), and both heads as include/trajopt_grpo_hip.h states
them.  Nothing here calls the library."""
import math

import numpy as np
import torch

import philox_fp64 as P

STREAM = 0x70737465                     # TG_POLICY_STEP_STREAM
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


def make_net(S, H, hidden_layers, O, act, seed, scale=1.0):
    """nn.Sequential Linear(S, H) act [Linear(H, H) act]* Linear(H, O) with torch's default init under its own generator; `scale`
    multiplies the head's weights and bias."""
    torch.manual_seed(seed)
    widths = [S] + [H] * hidden_layers
    mods = []
    for a, b in zip(widths[:-1], widths[1:]):
        mods += [torch.nn.Linear(a, b), getattr(torch.nn, act)()]
    net = torch.nn.Sequential(*mods, torch.nn.Linear(H, O))
    with torch.no_grad():
        net[-1].weight.mul_(scale)
        net[-1].bias.mul_(scale)
    return net


def mlp(net, x):
    """Float64 forward of an nn.Sequential of Linear / ReLU / Tanh from its float32 parameters; x [n][S] -> [n][O]."""
    h = np.asarray(x, dtype=np.float64)
    for m in net:
        if isinstance(m, torch.nn.Linear):
            h = h @ m.weight.detach().cpu().numpy().astype(np.float64).T + m.bias.detach().cpu().numpy().astype(np.float64)
        else:
            h = np.tanh(h) if isinstance(m, torch.nn.Tanh) else np.maximum(h, 0.0)
    return h


def eps(seed, env_offset, calls, A):
    """-> eps [n][A] float64 of slots env_offset + 0..n-1 at call counts `calls` [n], and (u_radius, u_angle, is_sin) [n][A]."""
    calls = np.asarray(calls, dtype=np.uint64)
    words = P.draw_np(seed, np.uint64(env_offset) + np.arange(calls.size, dtype=np.uint64), calls, STREAM)
    e, us = P.box_muller(words, A)
    return (np.stack(e, 1), np.stack([u[0] for u in us], 1), np.stack([u[1] for u in us], 1),
            np.stack([np.full_like(u[0], u[2]) for u in us], 1))


def head(out, e, head, log_std=None, bounds=(-5.0, 2.0)):
    """out [n][O], e [n][A] -> dict(action, logp, mean, ls, u), float64."""
    if head == "gaussian":
        mu, ls = out, np.broadcast_to(np.asarray(log_std, dtype=np.float64), out.shape)
    else:
        A = out.shape[1] // 2
        mu, ls = out[:, :A], np.clip(out[:, A:], *bounds)
    u = mu + np.exp(ls) * e
    logp = (-0.5 * e * e - ls - HALF_LOG_2PI).sum(1)
    if head == "gaussian":
        return dict(action=u, logp=logp, mean=mu, ls=ls, u=u)
    a = np.tanh(u)
    return dict(action=a, logp=logp - np.log(1.0 - a * a + 1e-6).sum(1), mean=np.tanh(mu), ls=out[:, A:], u=u)


def refused_nets():
    """(label, builder, head, a word of the reason) of every shape DeviceActor refuses."""
    nn = torch.nn
    return [("H96", lambda: make_net(5, 96, 2, 1, "Tanh", 0), "gaussian", "width 96"),
            ("Sigmoid", lambda: make_net(5, 64, 2, 1, "Sigmoid", 0), "gaussian", "Sigmoid"),
            ("mixed", lambda: nn.Sequential(nn.Linear(5, 64), nn.ReLU(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 1)), "gaussian", "mixed"),
            ("deep", lambda: make_net(5, 64, 6, 1, "Tanh", 0), "gaussian", "6 hidden layers"),
            ("S33", lambda: make_net(33, 64, 2, 1, "Tanh", 0), "gaussian", "input width 33"),
            ("O5", lambda: make_net(5, 64, 2, 5, "Tanh", 0), "gaussian", "5 outputs"),
            ("odd", lambda: make_net(5, 64, 2, 3, "Tanh", 0), "squashed", "3 outputs")]
