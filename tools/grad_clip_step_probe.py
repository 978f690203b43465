#!/usr/bin/env python3
"""What `max_grad_norm` costs, timed in one process on two shapes:
  grpo  one training step of C2's setup (CartPole GRPO, 64 groups x 64 episodes = 4,096 envs, 500-step horizon, fp32 5-128-128-1,
        10 updates per learn()): without a clip the optimizer step rides on the gradient reduction; with one the learner takes the
        norm (two launches) and a separate clipped step;
  ppo   one epoch at the reference factory's size (tools/ppo_factory_epoch.py: 10 x 8 envs, 500 steps, 128x3 actor-critic fp32,
        24 full-batch updates, Adam 2e-4).
Each with max_grad_norm None, 1e30 (never bites) and a biting value (a quarter of the smallest norm a 1e30 run reports).  A step is
rollout + learn(), bracketed by HIP events after a device synchronisation, after `--warmup` steps.  The probe also counts the host
synchronisations issued inside learn() (torch.cuda.synchronize, Event / Stream.synchronize, Tensor.item / .cpu / .tolist / .numpy):
a clip must not add one.  Prints one JSON line per (shape, max_grad_norm)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import trajopt_grpo_amd as tg  # noqa: E402

SYNCS = [(torch.cuda, "synchronize"), (torch.cuda.Event, "synchronize"), (torch.cuda.Stream, "synchronize"), (torch.Tensor, "item"),
         (torch.Tensor, "cpu"), (torch.Tensor, "tolist"), (torch.Tensor, "numpy")]


class count_host_syncs:
    """Counts calls of the host-synchronising entry points while active."""

    def __enter__(self):
        self.n, self._saved = 0, []
        for owner, name in SYNCS:
            orig = getattr(owner, name)
            self._saved.append((owner, name, orig))

            def counted(*a, _orig=orig, **k):
                self.n += 1
                return _orig(*a, **k)
            setattr(owner, name, counted)
        return self

    def __exit__(self, *exc):
        for owner, name, orig in self._saved:
            setattr(owner, name, orig)


def build(shape, max_grad_norm, dev):
    torch.manual_seed(0)
    if shape == "grpo":
        pol = tg.GaussianActor_NeuralNetwork(5, 1, (128, 128), cov=0.5, device=dev)
        mgr = tg.RolloutManager(lambda: tg.CartPole(max_steps=500), pol, num_workers=64, num_episodes_per_worker=64, seed=3)
        algo = tg.GRPO(epsilon=0.2, beta=0.0, gamma=0.99, policy=pol, optimizer=torch.optim.Adam(pol.parameters(), lr=3e-4),
                       updates_per_iter=10, max_grad_norm=max_grad_norm)
    else:
        pol = tg.GaussianActorCritic_NeuralNetwork(5, 1, (128, 128, 128), cov=0.5, device=dev)
        mgr = tg.RolloutManager(lambda: tg.CartPole(), pol, num_workers=10, num_episodes_per_worker=8, seed=0)
        algo = tg.PPO(epsilon=0.2, policy=pol, optimizer=torch.optim.Adam(pol.parameters(), lr=2e-4), ref_model=None,
                      updates_per_iter=24, c1=0.5, kl_coeff=0.5, gamma=0.99, lam=0.95, entropy=0.01, batch_size=None,
                      max_grad_norm=max_grad_norm)
    return pol, mgr, tg.Rollout_Buffer(mgr), algo


def run(shape, label, max_grad_norm, steps, warmup, dev):
    pol, mgr, buf, algo = build(shape, max_grad_norm, dev)
    times, syncs, norms = [], [], []
    for it in range(warmup + steps):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        buf.sample()
        with count_host_syncs() as c:
            algo.learn(buf)
        e1.record()
        torch.cuda.synchronize()
        if it >= warmup:
            times.append(e0.elapsed_time(e1))
            syncs.append(c.n)
            norms += algo.last_stats.get("grad_norm", [])
    m = algo._mlp(pol.actor)
    assert m is not None and m._f32 is not None and bool(algo._fused_adam), "the fp32 chain learner / fused step was not taken"
    ms = sum(times) / len(times)
    out = {"shape": shape, "max_grad_norm": label, "value": max_grad_norm, "steps": steps, "warmup": warmup, "ms_per_step": round(ms, 3),
           "ms_min": round(min(times), 3), "ms_max": round(max(times), 3), "host_syncs_in_learn": sorted(set(syncs))}
    if norms:
        out["grad_norm_min"], out["grad_norm_max"] = min(norms), max(norms)
        out["updates_clipped"] = sum(n + 1e-6 > max_grad_norm for n in norms) / len(norms)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shapes", default="grpo,ppo")
    ap.add_argument("--repeats", type=int, default=2, help="the three settings are run alternately this many times")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    with torch.cuda.device(dev):
        for shape in args.shapes.split(","):
            # (the biting value: a quarter of the smallest pre-clip norm a short run with a clip that never bites reports)
            biting = run(shape, "1e30", 1e30, 2, 1, dev)["grad_norm_min"] / 4.0
            for rep in range(args.repeats):
                for label, value in (("none", None), ("1e30", 1e30), ("biting", biting)):
                    print(json.dumps(run(shape, label, value, args.steps, args.warmup, dev)), flush=True)


if __name__ == "__main__":
    main()
