#!/usr/bin/env python3
"""A compact SAC in plain torch that trains CartPole or Pendulum through DeviceVecEnv + DeviceReplayBuffer only: the usage example of
the replay buffer, and the evidence that an off-policy loop from outside this package learns on these envs.  Nothing of the package's
own policies or learners is used: torch.nn nets, autograd, Adam, a tanh-squashed Gaussian actor, twin critics with Polyak targets, a
learned temperature.  The buffer hands over consistent n-step rows, so the target is one line for every --n-step:

    y = rew + disc * (min Q'(next_obs, a') - alpha log pi(a' | next_obs))

with disc = gamma^k where the window was closed by the clock or is still open, and 0 behind a termination.  It is not a benchmark.

    python tools/vec_env_sac.py --env CartPole --seeds 0 1 2 --n-step 3 --out profiles/curve.txt
"""
import argparse
import math
import os
import sys

import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import trajopt_grpo_amd as tg  # noqa: E402


def mlp(n_in, n_out, hidden):
    return nn.Sequential(nn.Linear(n_in, hidden), nn.ReLU(), nn.Linear(hidden, hidden), nn.ReLU(), nn.Linear(hidden, n_out))


class Actor(nn.Module):
    def __init__(self, S, A, hidden):
        super().__init__()
        self.net, self.A = mlp(S, 2 * A, hidden), A

    def forward(self, obs):
        """-> action in (-1, 1)^A and its log-density."""
        mu, log_std = self.net(obs).split(self.A, dim=-1)
        log_std = log_std.clamp(-5.0, 2.0)
        u = mu + log_std.exp() * torch.randn_like(mu)
        a = torch.tanh(u)
        logp = (-0.5 * ((u - mu) / log_std.exp()).pow(2) - log_std - 0.5 * math.log(2 * math.pi)).sum(-1)
        return a, logp - torch.log(1.0 - a.pow(2) + 1e-6).sum(-1)


class TwinQ(nn.Module):
    def __init__(self, S, A, hidden):
        super().__init__()
        self.q1, self.q2 = mlp(S + A, 1, hidden), mlp(S + A, 1, hidden)

    def forward(self, obs, act):
        x = torch.cat([obs, act], dim=-1)
        return self.q1(x).squeeze(-1), self.q2(x).squeeze(-1)


def train(seed, args, dev):
    torch.manual_seed(seed)
    env = tg.environments.ENV_CLASSES[args.env](max_steps=args.max_steps)
    venv = tg.DeviceVecEnv(env, args.envs, seed=seed, device=dev)
    buf = tg.DeviceReplayBuffer.for_env(venv, args.capacity_steps, n_step=args.n_step, gamma=args.gamma, seed=seed)
    S, A = venv.S, venv.A
    actor, critic, target = Actor(S, A, args.hidden).to(dev), TwinQ(S, A, args.hidden).to(dev), TwinQ(S, A, args.hidden).to(dev)
    target.load_state_dict(critic.state_dict())
    log_alpha = nn.Parameter(torch.zeros((), device=dev))
    opt_pi, opt_q = torch.optim.Adam(actor.parameters(), lr=args.lr), torch.optim.Adam(critic.parameters(), lr=args.lr)
    opt_alpha = torch.optim.Adam([log_alpha], lr=args.lr)
    obs, _ = venv.reset(seed=seed)
    buf.start(obs)
    ret_sum, ret_cnt = torch.zeros((), device=dev), torch.zeros((), device=dev)
    curve = []
    for it in range(args.iters):
        with torch.no_grad():
            act = torch.rand(args.envs, A, device=dev) * 2 - 1 if it < args.random_iters else actor(obs)[0]
        obs, rew, terminated, truncated, info = venv.step(act)
        buf.add(act, obs, rew, terminated, truncated, info)              # the env's own buffers as they are: one launch, no clone
        done = terminated | truncated
        ret_sum += torch.where(done, info["episode_return"], 0.0).sum()
        ret_cnt += done.sum()
        if it >= args.random_iters:
            for _ in range(args.updates):
                b_obs, b_act, b_rew, b_next, b_disc, _ = buf.sample(args.batch)
                with torch.no_grad():
                    alpha = log_alpha.exp()
                    a2, logp2 = actor(b_next)
                    y = b_rew + b_disc * (torch.min(*target(b_next, a2)) - alpha * logp2)
                q1, q2 = critic(b_obs, b_act)
                q_loss = (q1 - y).pow(2).mean() + (q2 - y).pow(2).mean()
                opt_q.zero_grad(set_to_none=True)
                q_loss.backward()
                opt_q.step()
                a_new, logp = actor(b_obs)
                pi_loss = (alpha * logp - torch.min(*critic(b_obs, a_new))).mean()
                opt_pi.zero_grad(set_to_none=True)
                pi_loss.backward()
                opt_pi.step()
                alpha_loss = -(log_alpha * (logp.detach().mean() - A))   # (target entropy -A)
                opt_alpha.zero_grad(set_to_none=True)
                alpha_loss.backward()
                opt_alpha.step()
                with torch.no_grad():
                    for p, pt in zip(critic.parameters(), target.parameters()):
                        pt.lerp_(p, args.tau)
        if (it + 1) % args.eval_every == 0:                               # an evaluation point: the episodes that ended since the last
            episodes = int(ret_cnt.item())                                # (the one host read of a block)
            mean_ret = float(ret_sum.item()) / max(episodes, 1)
            curve.append(((it + 1) * args.envs, episodes, mean_ret))
            ret_sum.zero_()
            ret_cnt.zero_()
            if len(curve) % args.log_every == 0 or it + 1 == args.iters:
                print(f"{args.env} seed {seed} env-steps {curve[-1][0]:8d} episodes {episodes:5d} mean episode return {mean_ret:9.3f} "
                      f"alpha {float(log_alpha.detach().exp()):.4f} stored {len(buf)}", flush=True)
    venv.close()
    return curve


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--env", choices=["CartPole", "Pendulum"], default="CartPole")
    ap.add_argument("--seeds", "--seed", type=int, nargs="+", default=[0], dest="seeds")
    ap.add_argument("--n-step", type=int, default=3)
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--iters", type=int, default=3000, help="env steps of every slot")
    ap.add_argument("--random-iters", type=int, default=20, help="steps of uniform random actions before the first update")
    ap.add_argument("--updates", type=int, default=1, help="gradient steps per env step")
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--capacity-steps", type=int, default=2000)
    ap.add_argument("--max-steps", type=int, default=200)
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--lr", type=float, default=3e-4)
    ap.add_argument("--gamma", type=float, default=0.99)
    ap.add_argument("--tau", type=float, default=0.005)
    ap.add_argument("--eval-every", type=int, default=50, help="env steps of every slot per evaluation point")
    ap.add_argument("--log-every", type=int, default=10, help="print every this many evaluation points")
    ap.add_argument("--out", default=None, help="write the curves here: one line per seed and evaluation point")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("vec_env_sac.py needs an MI355X: DeviceVecEnv and DeviceReplayBuffer have no CPU fallback")
    dev = torch.device("cuda", 0)
    lines = ["# env n_step seed env_steps episodes mean_episode_return"]
    for seed in args.seeds:
        curve = train(seed, args, dev)
        lines += [f"{args.env} {args.n_step} {seed} {steps} {episodes} {mean_ret:.4f}" for steps, episodes, mean_ret in curve]
        first, last = curve[:10], curve[-10:]
        for label, part in (("first", first), ("last", last)):
            eps = sum(e for _, e, _ in part)
            print(f"{args.env} seed {seed} n_step {args.n_step}: {label} ten evaluation points, episode-weighted mean return "
                  f"{sum(e * r for _, e, r in part) / max(eps, 1):.3f} over {eps} episodes", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
