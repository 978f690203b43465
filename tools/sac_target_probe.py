#!/usr/bin/env python3
"""Times the SAC target y = rew + disc * (min(Q1', Q2')(s', a') - alpha logp(a'|s')) of a batch three ways, each eagerly and as a
replayed hipGraph: (1) one DeviceActor.sac_target launch; (2) DeviceActor.act plus the torch composition (cat, two critics, min,
arithmetic); (3) the all-torch lines of tools/vec_env_sac.py.  Shapes: B = 256 with 5-64-64 nets (launch latency) and B = 65,536
with 20-256-256 nets.  Per arm: the median of 7 windows of device-event time per call, with the windows' min and max; the arms
alternate inside every window round.

    python tools/sac_target_probe.py [--out profiles/sac_target_probe.json]
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


def mlp(n_in, n_out, hidden):
    return nn.Sequential(nn.Linear(n_in, hidden), nn.ReLU(), nn.Linear(hidden, hidden), nn.ReLU(), nn.Linear(hidden, n_out))


def arms_for(B, S, A, H, dev):
    torch.manual_seed(0)
    actor, q1, q2 = mlp(S, 2 * A, H).to(dev), mlp(S + A, 1, H).to(dev), mlp(S + A, 1, H).to(dev)
    obs, rew, disc = torch.randn(B, S, device=dev), torch.randn(B, device=dev), torch.full((B,), 0.97, device=dev)
    alpha = torch.tensor(0.2, device=dev)
    fused = tg.DeviceActor(actor, q_nets=(q1, q2), num_envs=B, head="squashed", device=dev)
    plain = tg.DeviceActor(actor, num_envs=B, head="squashed", device=dev)

    def torch_rest(a2, logp2):
        x = torch.cat([obs, a2], dim=-1)
        return rew + disc * (torch.min(q1(x).squeeze(-1), q2(x).squeeze(-1)) - alpha * logp2)

    def all_torch():
        mu, ls = actor(obs).split(A, dim=-1)
        ls = ls.clamp(-5.0, 2.0)
        u = mu + ls.exp() * torch.randn_like(mu)
        a2 = torch.tanh(u)
        logp = (-0.5 * ((u - mu) / ls.exp()).pow(2) - ls - 0.5 * math.log(2 * math.pi)).sum(-1)
        return torch_rest(a2, logp - torch.log(1.0 - a2.pow(2) + 1e-6).sum(-1))

    return {"sac_target": lambda: fused.sac_target(obs, rew, disc, alpha),
            "act+torch": lambda: torch_rest(*plain.act(obs)[:2]),
            "all-torch": all_torch}


def graphed(fn, dev):
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream(dev).wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g.replay


def window_us(fn, calls):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / calls


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--windows", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sac_target_probe.py needs an MI355X: there is nothing to time without one")
    dev = torch.device("cuda", 0)
    results = []
    with torch.no_grad():
        for B, S, A, H, calls in ((256, 5, 1, 64, 2000), (65536, 20, 4, 256, 200)):
            eager = arms_for(B, S, A, H, dev)
            runs = {(name, "eager"): fn for name, fn in eager.items()}
            runs.update({(name, "graph"): graphed(fn, dev) for name, fn in eager.items()})
            for fn in runs.values():                                   # warm every arm at this shape
                window_us(fn, calls // 4)
            times = {k: [] for k in runs}
            for _ in range(args.windows):                              # the arms alternate inside a round of windows
                for k, fn in runs.items():
                    times[k].append(window_us(fn, calls))
            for (name, mode), t in times.items():
                r = dict(B=B, S=S, A=A, H=H, arm=name, mode=mode, calls_per_window=calls, median_us=statistics.median(t), min_us=min(t),
                         max_us=max(t))
                results.append(r)
                print(json.dumps(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
