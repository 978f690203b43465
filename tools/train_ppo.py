#!/usr/bin/env python3
"""End-to-end learning check: PPO with the reference factories' hyper-parameters but 4,096 parallel episodes per
epoch instead of 50-80.

    python3 tools/train_ppo.py [epochs] [CartPole|Pendulum|QuadPole2D|QuadPole] [bf16|fp32] [--randomize name=lo:hi ...]
                               [--learn-std] [--normalize-obs] [--normalize-value] [--popart] [--gae] [--privileged-critic]
                               [--eval-every N] [--eval-episodes E] [--eval-sweep name=f1,f2,... ...] [--desired-kl KL]
                               [--target-kl KL] [--kl-every N] [--substeps K] [--motor-tau SECONDS]

--substeps K: control decimation (Env.substeps = K, 1..64): K physics steps of timestep / K per policy step, so the control period,
the horizon in policy steps and the learner's cost stay what they are and only the integration gets finer.  Not for Pendulum.

--motor-tau SECONDS: a first-order rotor lag (Env.motor_time_constant, e.g. 0.05) in front of every physics step; QuadPole2D and
QuadPole only.  `--randomize motor_time_constant=0.5:2` then draws every env slot's own time constant.

--desired-kl KL: the KL-adaptive learning rate (PPO(desired_kl=KL), e.g. 0.01): once per learn() the rate is divided by 1.5 when the
measured KL between the policy before and after the updates exceeds 2 KL and multiplied by 1.5 when it is below KL / 2.

--target-kl KL: early stopping of a learn()'s updates (PPO(target_kl=KL), e.g. 0.02): after every --kl-every N-th update (default 1) the
KL is measured on the device, and once it exceeds 1.5 KL the remaining updates of that learn() change nothing.  --kl-every with
--desired-kl makes the rate follow the rule at every such check instead of once per learn().

--eval-every N: every N epochs a deterministic evaluation (trajopt_grpo_amd.Evaluator: mean actions, its own seed and RNG stream) of
--eval-episodes E episodes per cell (default 256) is printed beside the sampled training return.  --eval-sweep (repeatable): the
evaluation runs one cell per combination of the listed factors on those physical parameters, e.g. `--eval-sweep mass=0.8,1,1.25`.

--normalize-value: running value normalisation (policy.value_norm): the critic regresses onto returns standardised with running
statistics and is denormalised wherever it enters a return.  --popart (with --normalize-value): the critic head is rescaled when
those statistics move (policy.value_norm.popart).  --gae: monte_carlo=False (GAE(gamma, 0.95) advantages).

--randomize (repeatable): per-env domain randomisation, e.g. `--randomize mass=0.8:1.25 --randomize tether_length=0.5:2` -- every
env slot draws its own factor on that physical parameter in every rollout (Env.randomize).
--privileged-critic: the critic also reads each env slot's drawn parameters (the policy's privileged_critic takes the --randomize
ranges); an error without --randomize.

CartPole / QuadPole2D (pipelines/cartpole_pipeline_ppo.py, quadpole2d_pipeline_ppo.py; Pendulum takes the same): 128x3 actor-critic, cov 0.5,
eps 0.2, gamma 0.99, 24 full-batch updates, Adam 2e-4 (published curves: -37 -> ~800 and -70 -> ~1047).
QuadPole (quadpole_pipeline_ppo.py): 256x5, cov 0.3, gamma 0.999, 32 updates, Adam 3e-4, bf16 policy compute."""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import trajopt_grpo_amd as tg  # noqa: E402


def pop_randomize(argv):
    """Removes every `--randomize name=lo:hi` from argv; -> {name: (lo, hi)}."""
    ranges, rest, k = {}, [], 0
    while k < len(argv):
        if argv[k] == "--randomize" or argv[k].startswith("--randomize="):
            item = argv[k].split("=", 1)[1] if argv[k].startswith("--randomize=") else (argv[k + 1] if k + 1 < len(argv) else "")
            k += 1 if argv[k].startswith("--randomize=") else 2
            try:
                name, rng = item.split("=", 1)
                lo, hi = rng.split(":", 1)
                ranges[name] = (float(lo), float(hi))
            except ValueError:
                raise SystemExit(f"--randomize expects name=lo:hi, got {item!r}")
        else:
            rest.append(argv[k])
            k += 1
    return ranges, rest


def pop_valued(argv, flag):
    """Removes every `flag value` / `flag=value` from argv; -> ([value, ...], the rest)."""
    values, rest, k = [], [], 0
    while k < len(argv):
        if argv[k] == flag:
            if k + 1 >= len(argv):
                raise SystemExit(f"{flag} expects a value")
            values.append(argv[k + 1])
            k += 2
        elif argv[k].startswith(flag + "="):
            values.append(argv[k].split("=", 1)[1])
            k += 1
        else:
            rest.append(argv[k])
            k += 1
    return values, rest


def pop_eval(argv):
    """-> (eval_every or None, eval_episodes, sweep {name: [factor, ...]} or None, the rest of argv)."""
    every, argv = pop_valued(argv, "--eval-every")
    episodes, argv = pop_valued(argv, "--eval-episodes")
    items, argv = pop_valued(argv, "--eval-sweep")
    sweep = {}
    for item in items:
        try:
            name, vals = item.split("=", 1)
            sweep[name] = [float(v) for v in vals.split(",")]
        except ValueError:
            raise SystemExit(f"--eval-sweep expects name=f1,f2,..., got {item!r}")
    try:
        every = int(every[-1]) if every else None
        episodes = int(episodes[-1]) if episodes else 256
    except ValueError:
        raise SystemExit("--eval-every and --eval-episodes expect integers")
    if every is not None and every < 1:
        raise SystemExit("--eval-every expects a positive integer")
    if every is None and (sweep or items):
        raise SystemExit("--eval-sweep needs --eval-every N")
    return every, episodes, sweep or None, argv


def pop_motor_tau(argv):
    """(--motor-tau SECONDS or 0.0, the remaining arguments); SystemExit on a value that is not a number."""
    vals, argv = pop_valued(argv, "--motor-tau")
    try:
        return (float(vals[-1]) if vals else 0.0), argv
    except ValueError:
        raise SystemExit("--motor-tau expects a number of seconds")


def build_env(name, ranges, substeps=1, motor_tau=0.0):
    """The env a run trains on.  The lag is set before the ranges are: "motor_time_constant" is a randomisable name only while it is on."""
    env = tg.environments.ENV_CLASSES[name]()
    if motor_tau != 0.0:
        env.motor_time_constant = motor_tau                       # (ValueError: an env without rotors, a negative or non-finite value)
    env.randomize(ranges)
    if substeps != 1:
        env.substeps = substeps                                   # (ValueError: Pendulum, or K outside 1..64)
        env.timestep = env.timestep / substeps                    # the control period stays the reference's
    return env


def main():
    ranges, sys.argv[1:] = pop_randomize(sys.argv[1:])
    eval_every, eval_episodes, eval_sweep, sys.argv[1:] = pop_eval(sys.argv[1:])
    desired_kl, sys.argv[1:] = pop_valued(sys.argv[1:], "--desired-kl")
    try:
        desired_kl = float(desired_kl[-1]) if desired_kl else None    # the KL-adaptive learning rate (PPO(desired_kl=...))
    except ValueError:
        raise SystemExit("--desired-kl expects a number")
    target_kl, sys.argv[1:] = pop_valued(sys.argv[1:], "--target-kl")
    kl_every, sys.argv[1:] = pop_valued(sys.argv[1:], "--kl-every")
    try:
        target_kl = float(target_kl[-1]) if target_kl else None       # early stopping (PPO(target_kl=...))
        kl_every = int(kl_every[-1]) if kl_every else None            # a check behind every kl_every-th update
    except ValueError:
        raise SystemExit("--target-kl expects a number, --kl-every an integer")
    substeps, sys.argv[1:] = pop_valued(sys.argv[1:], "--substeps")
    try:
        substeps = int(substeps[-1]) if substeps else 1
    except ValueError:
        raise SystemExit("--substeps expects an integer")
    motor_tau, sys.argv[1:] = pop_motor_tau(sys.argv[1:])
    learn_std = "--learn-std" in sys.argv                         # a learned per-dimension log-std instead of the fixed covariance
    sys.argv = [a for a in sys.argv if a != "--learn-std"]
    normalize_obs = "--normalize-obs" in sys.argv                 # running observation normalisation (policy.obs_norm)
    sys.argv = [a for a in sys.argv if a != "--normalize-obs"]
    normalize_value = "--normalize-value" in sys.argv             # running value normalisation (policy.value_norm)
    popart = "--popart" in sys.argv                               # PopArt's rescale of the critic head (needs --normalize-value)
    gae = "--gae" in sys.argv                                     # monte_carlo=False
    privileged = "--privileged-critic" in sys.argv                # an asymmetric actor-critic: the critic reads the drawn parameters
    sys.argv = [a for a in sys.argv if a not in ("--normalize-value", "--popart", "--gae", "--privileged-critic")]
    if privileged and not ranges:
        raise SystemExit("--privileged-critic needs at least one --randomize name=lo:hi: the critic reads the randomised parameters")
    epochs = int(sys.argv[1]) if len(sys.argv) > 1 else 120
    name = sys.argv[2] if len(sys.argv) > 2 else "CartPole"
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    if name == "QuadPole":
        S, A, hidden, cov, lr, upd, gamma, cdt = 20, 4, (256,) * 5, 0.3, 3e-4, 32, 0.999, torch.bfloat16
        if len(sys.argv) > 3 and sys.argv[3] == "fp32":          # the reference's own precision: the H = 256 fp32 chain learner
            cdt = None
    else:
        S, A = {"CartPole": (5, 1), "Pendulum": (3, 1)}.get(name, (10, 2))
        hidden, cov, lr, upd, gamma, cdt = (128, 128, 128), 0.5, 2e-4, 24, 0.99, None
        if len(sys.argv) > 3 and sys.argv[3] == "bf16":          # bf16 policy compute: fused bf16 rollout + chain kernels at H = 128
            cdt = torch.bfloat16
    pol = tg.GaussianActorCritic_NeuralNetwork(S, A, hidden, cov=cov, device=dev, **({"learn_std": True} if learn_std else {}),
                                               **({"normalize_obs": True} if normalize_obs else {}),
                                               **({"normalize_value": True} if normalize_value else {}),
                                               **({"popart": True} if popart else {}),
                                               **({"privileged_critic": ranges} if privileged else {}))

    def make_env():
        return build_env(name, ranges, substeps, motor_tau)

    make_env()                                                    # (refuses a bad name, range or K before anything is allocated)
    mgr = tg.RolloutManager(make_env, pol, num_workers=64, num_episodes_per_worker=64,
                            seed=0, compute_dtype=cdt)
    buf = tg.Rollout_Buffer(mgr)
    algo = tg.PPO(epsilon=0.2, policy=pol, optimizer=torch.optim.Adam(pol.parameters(), lr=lr), ref_model=None,
                  updates_per_iter=upd, c1=0.5, kl_coeff=0.5, gamma=gamma, lam=0.95, entropy=0.01, batch_size=None,
                  autocast_dtype=cdt, **({"monte_carlo": False} if gae else {}), desired_kl=desired_kl,
                  **({"target_kl": target_kl} if target_kl is not None else {}), **({"kl_every": kl_every} if kl_every is not None else {}))
    evaluator = None
    if eval_every is not None:                                    # (refuses a bad sweep before the first epoch)
        evaluator = tg.Evaluator(make_env(), pol, episodes=eval_episodes, sweep=eval_sweep,
                                 seed=1, compute_dtype=cdt)
    t0 = time.time()
    for ep in range(epochs):
        buf.sample()
        algo.learn(buf)
        if evaluator is not None and (ep + 1) % eval_every == 0:
            res = evaluator.evaluate()
            s = res.summary
            print(f"epoch {ep:4d}  eval return {s['return_mean']:9.2f} +- {s['return_std']:.2f}  len {s['length_mean']:6.1f}  "
                  f"timeout {s['timeout_frac']:.3f}  {res.early_name} {s['early_frac']:.3f}", flush=True)
            if eval_sweep:
                for row in res.table:
                    print("      " + "  ".join(f"{n} x{f:g}" for n, f in zip(res.sweep_names, row["factors"]))
                          + f"  return {row['return_mean']:9.2f}  len {row['length_mean']:6.1f}  timeout {row['timeout_frac']:.3f}", flush=True)
        if ep % 10 == 0 or ep == epochs - 1:
            print(f"epoch {ep:4d}  avg return {float(buf.avg_reward[-1]):9.2f}  mean len {float(buf.device_traj.len.float().mean()):6.1f}  "
                  f"elapsed {time.time() - t0:6.1f}s"
                  + (f"  log_std {[round(v, 4) for v in algo.last_stats['log_std']]}" if learn_std else "")
                  + (f"  obs_count {algo.last_stats['obs_count']:.0f}" if normalize_obs else "")
                  + (f"  kl {algo.last_stats['approx_kl']:.4f} clip {algo.last_stats['clip_fraction']:.3f} lr {algo.last_stats['lr']:.2e}"
                     if desired_kl is not None else "")
                  + (f"  updates {algo.last_stats['n_updates']}/{upd}" if target_kl is not None else "")
                  + (f"  value mean {algo.last_stats['value_mean']:.2f} std {algo.last_stats['value_std']:.2f}"
                     f" ev {algo.last_stats['explained_variance']:.3f}" if normalize_value else ""), flush=True)
    print("first -> last:", float(buf.avg_reward[0]), "->", float(buf.avg_reward[-1]), " max", float(max(buf.avg_reward)))


if __name__ == "__main__":
    main()
