#!/usr/bin/env python3
"""Times DeviceActor.act() against the torch composition it replaces (the lines of tools/vec_env_ppo.py), issued eagerly and replayed
from a hipGraph, and the whole collection step (policy + venv.step + DeviceRolloutStorage.add) from a graph with either policy.
One process, device events around `--inner` calls per sample, `--samples` samples per arm, arms alternating; prints one JSON line per
shape with each arm's median and spread, and the launch's fp32 matrix rate (2 x rows x weights flops over the graph-replayed time).

    python tools/policy_step_probe.py --out profiles/policy_step_probe.jsonl
"""
import argparse
import json
import os
import statistics
import sys

import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import trajopt_grpo_amd as tg  # noqa: E402

SHAPES = [("CartPole", 4096, 64, 2, "Tanh"), ("QuadPole", 65536, 256, 2, "ReLU"), ("QuadPole", 65536, 256, 5, "ReLU")]
PEAK_TFLOPS = 157.3


def mlp(n_in, n_out, hidden, layers, act):
    widths = [n_in] + [hidden] * layers
    mods = []
    for a, b in zip(widths[:-1], widths[1:]):
        mods += [nn.Linear(a, b), getattr(nn, act)()]
    return nn.Sequential(*mods, nn.Linear(hidden, n_out))


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


def sample_us(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0 / inner


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--inner", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("policy_step_probe.py needs an MI355X")
    dev = torch.device("cuda", 0)
    lines = []
    for env_name, n, H, layers, act in SHAPES:
        torch.manual_seed(0)
        venv = tg.DeviceVecEnv(tg.environments.ENV_CLASSES[env_name](max_steps=200), n, seed=0, device=dev)
        S, A = venv.S, venv.A
        actor, critic = mlp(S, A, H, layers, act).to(dev), mlp(S, 1, H, layers, act).to(dev)
        log_std = torch.full((A,), -0.5, device=dev)
        st = tg.DeviceRolloutStorage.for_env(venv, 16, seed=0)
        st.start(venv.reset(seed=0)[0])
        da = tg.DeviceActor.for_env(venv, actor, critic, log_std=log_std)
        obs = venv._obs.clone()

        def torch_policy(x, capturable=False):
            dist = torch.distributions.Normal(actor(x), log_std.exp(), validate_args=False)
            # (dist.sample() is torch.normal(mean, std), which reads std on the host and cannot be captured: the graph arms draw
            # mean + std * randn instead -- one launch more, no host read)
            a = dist.mean + dist.stddev * torch.randn_like(dist.mean) if capturable else dist.sample()
            return a, dist.log_prob(a).sum(-1), critic(x).squeeze(-1)

        def torch_policy_g(x):
            return torch_policy(x, capturable=True)

        def step_with(policy, value_of):
            a, logp, value = policy(st.obs[0])
            o, rew, term, trunc, info = venv.step(a)
            st.add(a, logp, value, o, rew, term, trunc, value_of(info["final_obs"]))

        with torch.no_grad():
            arms = {"act_eager": lambda: da.act(obs), "torch_eager": lambda: torch_policy(obs),
                    "act_graph": graphed(lambda: da.act(obs), dev), "torch_graph": graphed(lambda: torch_policy_g(obs), dev),
                    "step_act_graph": graphed(lambda: step_with(da.act, da.values), dev),
                    "step_torch_graph": graphed(lambda: step_with(torch_policy_g, lambda x: critic(x).squeeze(-1)), dev)}
            for fn in arms.values():
                sample_us(fn, args.inner)
            times = {k: [] for k in arms}
            for _ in range(args.samples):
                for k, fn in arms.items():
                    times[k].append(sample_us(fn, args.inner))
        flops = 2.0 * n * sum(p.numel() for net in (actor, critic) for p in net.parameters() if p.dim() == 2)
        rec = {"env": env_name, "slots": n, "net": f"{S}-{H}x{layers}-{A} {act}", "samples": args.samples, "inner": args.inner,
               "us": {k: {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)} for k, v in times.items()}}
        rec["act_graph_tflops"] = round(flops / statistics.median(times["act_graph"]) * 1e-6, 2)
        rec["act_graph_share_of_fp32_matrix_peak"] = round(rec["act_graph_tflops"] / PEAK_TFLOPS, 4)
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
        venv.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
