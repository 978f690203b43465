#!/usr/bin/env python3
"""One training step of C2's setup (CartPole GRPO, 64 groups x 64 episodes = 4,096 envs, 500-step horizon, fp32, 10 updates per
learn()) with a Tanh actor, timed two ways in one process:
  native    the fp32 fused rollout (tg_fused_rollout_f32_act) + the fp32 chain learner (tg_mlp_f32_forward_backward_act, ...);
  fallback  what a Tanh actor ran on before: the per-step rollout (fused=False, its T steps replayed as a hipGraph) + torch autograd
            (fused_mlp=False).
A step is rollout + learn(); each timed step is bracketed by HIP events after a device synchronisation, after `--warmup` steps.
Prints one JSON line per (actor, path): mean / min / max ms per step and env-steps per second of the rollout."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import trajopt_grpo_amd as tg  # noqa: E402


def run(hidden, native, steps, warmup, T, dev):
    torch.manual_seed(0)
    pol = tg.GaussianActor_NeuralNetwork(5, 1, hidden, activation="Tanh", cov=0.5, device=dev)
    mgr = tg.RolloutManager(lambda: tg.CartPole(max_steps=T), pol, num_workers=64, num_episodes_per_worker=64, seed=3,
                            **({} if native else {"fused": False}))
    buf = tg.Rollout_Buffer(mgr)
    algo = tg.GRPO(epsilon=0.2, beta=0.0, gamma=0.99, policy=pol, optimizer=torch.optim.Adam(pol.parameters(), lr=3e-4),
                   updates_per_iter=10, fused_mlp=native)
    times, env_steps = [], []
    for it in range(warmup + steps):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        buf.sample()
        algo.learn(buf)
        e1.record()
        torch.cuda.synchronize()
        if it == 0:
            m = algo._mlp(pol.actor)
            took = (m is not None and m._f32 is not None and mgr.engine.fused and mgr.engine._fused_f32)
            assert took == native, "the path this run is labelled with was not taken"
        if it >= warmup:
            times.append(e0.elapsed_time(e1))
            env_steps.append(int(mgr.engine.traj.env_steps()))
    ms = sum(times) / len(times)
    return {"actor": "5-" + "-".join(map(str, hidden)) + "-1 Tanh", "path": "native" if native else "fallback", "steps": steps,
            "warmup": warmup, "ms_per_step": round(ms, 3), "ms_min": round(min(times), 3), "ms_max": round(max(times), 3),
            "env_steps_per_s": round(sum(env_steps) / (sum(times) / 1e3), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--horizon", type=int, default=500)
    ap.add_argument("--paths", default="native,fallback")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    with torch.cuda.device(dev):
        for hidden in ((128, 128), (128,) * 4):
            for path in args.paths.split(","):
                print(json.dumps(run(hidden, path == "native", args.steps, args.warmup, args.horizon, dev)), flush=True)


if __name__ == "__main__":
    main()
