#!/usr/bin/env python3
"""A compact PPO in plain torch that trains CartPole through DeviceVecEnv only: the usage example of the vector env, and the evidence
that a loop from outside this package learns on these envs.  Nothing of the package's own policies, buffers or learners is used:
torch.nn nets, autograd, Adam, GAE with the terminated / truncated split -- a truncated episode bootstraps from the critic's value of
info["final_obs"], a terminated one from nothing.  It is not a benchmark.

    python tools/vec_env_ppo.py --seeds 0 1 2 --out profiles/curve.txt
"""
import argparse
import os
import sys

import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import trajopt_grpo_amd as tg  # noqa: E402


def mlp(n_in, n_out, hidden=64):
    return nn.Sequential(nn.Linear(n_in, hidden), nn.Tanh(), nn.Linear(hidden, hidden), nn.Tanh(), nn.Linear(hidden, n_out))


def train(seed, args, dev):
    torch.manual_seed(seed)
    venv = tg.DeviceVecEnv(tg.CartPole(max_steps=args.max_steps), args.envs, seed=seed, device=dev)
    n, S, A, L = venv.num_envs, venv.S, venv.A, args.rollout
    actor, critic = mlp(S, A).to(dev), mlp(S, 1).to(dev)
    log_std = nn.Parameter(torch.full((A,), -0.5, device=dev))
    params = list(actor.parameters()) + list(critic.parameters()) + [log_std]
    opt = torch.optim.Adam(params, lr=args.lr)
    buf = {"obs": torch.empty(L, n, S, device=dev), "act": torch.empty(L, n, A, device=dev), "logp": torch.empty(L, n, device=dev),
           "val": torch.empty(L, n, device=dev), "rew": torch.empty(L, n, device=dev), "done": torch.empty(L, n, device=dev)}
    obs, _ = venv.reset(seed=seed)
    curve = []
    for it in range(args.iters):
        ret_sum = torch.zeros((), device=dev)
        ret_cnt = torch.zeros((), device=dev)
        with torch.no_grad():
            for t in range(L):
                buf["obs"][t].copy_(obs)                              # (obs is the env's own buffer: the next step overwrites it)
                dist = torch.distributions.Normal(actor(buf["obs"][t]), log_std.exp())
                act = dist.sample()
                buf["act"][t], buf["logp"][t], buf["val"][t] = act, dist.log_prob(act).sum(-1), critic(buf["obs"][t]).squeeze(-1)
                obs, rew, terminated, truncated, info = venv.step(act)
                # the clock is no part of the task: where it ended the episode, the value of the state it cut off stands in for the rest
                boot = torch.where(truncated, critic(info["final_obs"]).squeeze(-1), 0.0)   # (rows are defined where the slot ended)
                buf["rew"][t] = rew + args.gamma * boot
                done = terminated | truncated
                buf["done"][t] = done
                ret_sum += torch.where(done, info["episode_return"], 0.0).sum()
                ret_cnt += done.sum()
            adv = torch.empty(L, n, device=dev)
            last, nxt = torch.zeros(n, device=dev), critic(obs).squeeze(-1)
            for t in reversed(range(L)):
                live = 1.0 - buf["done"][t]
                delta = buf["rew"][t] + args.gamma * nxt * live - buf["val"][t]
                last = delta + args.gamma * args.lam * live * last
                adv[t], nxt = last, buf["val"][t]
            ret = adv + buf["val"]
        flat = {k: v.reshape(L * n, *v.shape[2:]) for k, v in buf.items()}
        f_adv, f_ret = adv.reshape(-1), ret.reshape(-1)
        for _ in range(args.epochs):
            for idx in torch.randperm(L * n, device=dev).chunk(args.minibatches):
                dist = torch.distributions.Normal(actor(flat["obs"][idx]), log_std.exp())
                ratio = (dist.log_prob(flat["act"][idx]).sum(-1) - flat["logp"][idx]).exp()
                a = f_adv[idx]
                a = (a - a.mean()) / (a.std() + 1e-8)
                pi_loss = -torch.min(ratio * a, ratio.clamp(1 - args.clip, 1 + args.clip) * a).mean()
                v_loss = 0.5 * (critic(flat["obs"][idx]).squeeze(-1) - f_ret[idx]).pow(2).mean()
                opt.zero_grad(set_to_none=True)
                (pi_loss + args.vf_coef * v_loss).backward()
                nn.utils.clip_grad_norm_(params, 0.5)
                opt.step()
        episodes = int(ret_cnt.item())                                # (the one host read of an iteration)
        mean_ret = float(ret_sum.item()) / max(episodes, 1)
        curve.append(((it + 1) * L * n, episodes, mean_ret))
        if it % args.log_every == 0 or it == args.iters - 1:
            print(f"seed {seed} iter {it + 1:3d} env-steps {curve[-1][0]:8d} episodes {episodes:5d} mean episode return {mean_ret:9.3f}", flush=True)
    venv.close()
    return curve


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--seeds", type=int, nargs="+", default=[0])
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--rollout", type=int, default=64, help="steps of every env between two updates")
    ap.add_argument("--iters", type=int, default=80)
    ap.add_argument("--max-steps", type=int, default=200)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--minibatches", type=int, default=4)
    ap.add_argument("--lr", type=float, default=3e-4)
    ap.add_argument("--gamma", type=float, default=0.99)
    ap.add_argument("--lam", type=float, default=0.95)
    ap.add_argument("--clip", type=float, default=0.2)
    ap.add_argument("--vf-coef", type=float, default=0.5)
    ap.add_argument("--log-every", type=int, default=10)
    ap.add_argument("--out", default=None, help="write the curves here: one line per seed and iteration")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("vec_env_ppo.py needs an MI355X: DeviceVecEnv has no CPU fallback")
    dev = torch.device("cuda", 0)
    lines = ["# seed env_steps episodes mean_episode_return"]
    for seed in args.seeds:
        for steps, episodes, mean_ret in train(seed, args, dev):
            lines.append(f"{seed} {steps} {episodes} {mean_ret:.4f}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
