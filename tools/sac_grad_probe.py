#!/usr/bin/env python3
"""Times SAC's two gradient steps on DeviceActor against torch autograd of the same nets on the same rows, from Python: the critic
update's forward + backward (q_evaluate(obs, act), an MSE loss, backward) and the actor update's (rsample(obs),
q_evaluate(obs, a, detach_params=True), alpha logp - min q, backward).  Neither arm includes an optimizer step.  Medians of 7 single
calls between two events after 3 warm-up calls, with the spread.

Measured on one MI355X (profiles/r27_sac_grad_probe.md): at 256 and 1,024 rows the native critic update takes 0.56 to 0.61 of torch's
time and the actor update 0.33 to 0.36; at 65,536 rows the actor update takes 0.68 / 0.87 of it, and the CRITIC UPDATE IS SLOWER THAN
TORCH: 1.77 against 1.49 ms on 5-128-128 nets, 2.25 against 2.04 ms on 20-256-256.

    python tools/sac_grad_probe.py --out profiles/sac_grad_probe.json
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import trajopt_grpo_amd as tg  # noqa: E402
from trajopt_grpo_amd import _native as N  # noqa: E402

# (S, A, H): two hidden ReLU layers each, twin critics on [obs, act]
NETS = [(5, 1, 128), (20, 4, 256)]
BATCHES = [256, 1024, 65536]


def net(n_in, H, n_out):
    return nn.Sequential(nn.Linear(n_in, H), nn.ReLU(), nn.Linear(H, H), nn.ReLU(), nn.Linear(H, n_out))


def timed(fn, reps=7, warmup=3):
    """-> (median ms, min ms, max ms) of `reps` single calls between two events."""
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        e0, e1 = N.event_pair()
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


def probe(S, A, H, B, dev):
    torch.manual_seed(0)
    actor, q1, q2 = net(S, H, 2 * A).to(dev), net(S + A, H, 1).to(dev), net(S + A, H, 1).to(dev)
    q_params, pi_params = [*q1.parameters(), *q2.parameters()], list(actor.parameters())
    obs, act, y = torch.randn(B, S, device=dev), torch.rand(B, A, device=dev) * 2 - 1, torch.randn(B, device=dev)
    alpha = 0.2
    da = tg.DeviceActor(actor, q_nets=(q1, q2), num_envs=B, head="squashed", device=dev)

    def clear():
        for p in q_params + pi_params:
            p.grad = None

    def torch_q(o, a):
        x = torch.cat([o, a], dim=-1)
        return q1(x).squeeze(-1), q2(x).squeeze(-1)

    def critic_native():
        clear()
        v1, v2 = da.q_evaluate(obs, act)
        ((v1 - y).pow(2).mean() + (v2 - y).pow(2).mean()).backward()

    def critic_torch():
        clear()
        v1, v2 = torch_q(obs, act)
        ((v1 - y).pow(2).mean() + (v2 - y).pow(2).mean()).backward()

    def actor_native():
        clear()
        a, logp = da.rsample(obs)
        (alpha * logp - torch.min(*da.q_evaluate(obs, a, detach_params=True))).mean().backward()

    def actor_torch():                                                 # tools/vec_env_sac.py's Actor.forward and actor loss
        clear()
        mu, ls = actor(obs).split(A, dim=-1)
        ls = ls.clamp(-5.0, 2.0)
        u = mu + ls.exp() * torch.randn_like(mu)
        a = torch.tanh(u)
        logp = (-0.5 * ((u - mu) / ls.exp()).pow(2) - ls - 0.5 * math.log(2 * math.pi)).sum(-1) - torch.log(1.0 - a.pow(2) + 1e-6).sum(-1)
        (alpha * logp - torch.min(*torch_q(obs, a))).mean().backward()

    res = {"shape": dict(rows=B, S=S, A=A, H=H, hidden_layers=2, activation="ReLU")}
    for name, fn in (("critic_native", critic_native), ("critic_torch", critic_torch), ("actor_native", actor_native),
                     ("actor_torch", actor_torch)):
        med, lo, hi = timed(fn)
        res[name] = {"median_ms": round(med, 4), "min_ms": round(lo, 4), "max_ms": round(hi, 4)}
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sac_grad_probe.py needs an MI355X")
    dev = torch.device("cuda", 0)
    results = [probe(S, A, H, B, dev) for S, A, H in NETS for B in BATCHES]
    for r in results:
        print(json.dumps(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
