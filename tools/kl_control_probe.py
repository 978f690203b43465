#!/usr/bin/env python3
"""Step time of PPO with the policy-shift measurement (kl_stats=True) against the plain learner: same commit, same process, same
seeds.

    python3 tools/kl_control_probe.py [--shape c3|c2|both] [--reps 7] [--warmup 2]

c3: 65,536 QuadPole envs x 256 steps, PPO, actor-critic 20-256x5-{4,1} in bf16, 32 full-batch updates (bench.py's headline shape)
c2:  4,096 CartPole envs x 500 steps, PPO, actor-critic 5-128-128-{1,1} in fp32, 10 full-batch updates
The on arm adds, once per learn() and behind its last optimizer step: one no-grad actor pass over the valid rows, tg_policy_shift on
each chunk's means, tg_policy_shift_finish, tg_lr_adapt and a 64-byte copy to pinned memory.  It measures only (kl_stats=True, no
desired_kl): the learning rate stays, so both arms hold the same weights and the same rows in every repetition and the difference
is the measurement alone.  Each repetition is one Rollout_Buffer.sample() and one learn() between HIP events on the launch stream;
the two arms alternate within a repetition so that clock and thermal drift hit both alike.  Prints one JSON line per shape: median
and spread of each arm (milliseconds, and nanoseconds per env-step), the on / off ratios, the off arm's env-steps per second (to
hold against bench.py's headline on the same machine) and the on arm's last statistics."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import trajopt_grpo_amd as tg  # noqa: E402

SHAPES = {
    "c3": dict(env="QuadPole", S=20, A=4, hidden=(256,) * 5, cov=0.3, G=256, E=256, T=256, cdt=torch.bfloat16, updates=32, gamma=0.999),
    "c2": dict(env="CartPole", S=5, A=1, hidden=(128, 128), cov=0.5, G=64, E=64, T=500, cdt=None, updates=10, gamma=0.99),
}


def make_arm(c, kl_stats, dev):
    torch.manual_seed(0)
    pol = tg.GaussianActorCritic_NeuralNetwork(c["S"], c["A"], c["hidden"], cov=c["cov"], device=dev)
    env_cls = tg.environments.ENV_CLASSES[c["env"]]
    mgr = tg.RolloutManager(lambda: env_cls(max_steps=c["T"]), pol, num_workers=c["G"], num_episodes_per_worker=c["E"], seed=1234,
                            compute_dtype=c["cdt"], use_graph=False)
    buf = tg.Rollout_Buffer(mgr)
    opt = torch.optim.Adam(pol.parameters(), lr=3e-4)
    algo = tg.PPO(epsilon=0.2, policy=pol, optimizer=opt, ref_model=None, updates_per_iter=c["updates"], c1=0.5, kl_coeff=0.5,
                  gamma=c["gamma"], lam=0.95, entropy=0.01, batch_size=None, autocast_dtype=c["cdt"], **({"kl_stats": True} if kl_stats else {}))
    return buf, algo


def measure(shape, reps, warmup):
    c = SHAPES[shape]
    dev = torch.device("cuda", 0)
    arms = {"off": make_arm(c, False, dev), "on": make_arm(c, True, dev)}
    step, learn, env_steps = ({k: [] for k in arms} for _ in range(3))
    for rep in range(warmup + reps):
        for k, (buf, algo) in arms.items():
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            ev[0].record()
            buf.sample()
            ev[1].record()
            algo.learn(buf)
            ev[2].record()
            ev[2].synchronize()
            if rep >= warmup:
                step[k].append(ev[0].elapsed_time(ev[2]))
                learn[k].append(ev[1].elapsed_time(ev[2]))
                env_steps[k].append(float(buf.device_traj.env_steps()))
    out = {"shape": shape, "envs": c["G"] * c["E"], "horizon": c["T"], "updates": c["updates"], "reps": reps, "warmup": warmup}
    for k in arms:
        for name, xs in (("step_ms", step[k]), ("learn_ms", learn[k])):
            out[f"{k}_{name}_median"], out[f"{k}_{name}_min"], out[f"{k}_{name}_max"] = statistics.median(xs), min(xs), max(xs)
        out[f"{k}_env_steps_per_s"] = statistics.median(e / (t * 1e-3) for e, t in zip(env_steps[k], step[k]))
        ns = [t * 1e6 / e for t, e in zip(step[k], env_steps[k])]
        out[f"{k}_ns_per_env_step_median"], out[f"{k}_ns_per_env_step_min"], out[f"{k}_ns_per_env_step_max"] = statistics.median(ns), min(ns), max(ns)
    out["same_rows_in_both_arms"] = env_steps["off"] == env_steps["on"]
    out["off_spread"] = (out["off_ns_per_env_step_max"] - out["off_ns_per_env_step_min"]) / out["off_ns_per_env_step_median"]
    out["on_over_off"] = out["on_ns_per_env_step_median"] / out["off_ns_per_env_step_median"]
    out["on_minus_off_learn_ms"] = out["on_learn_ms_median"] - out["off_learn_ms_median"]
    stats = arms["on"][1].last_stats
    out["on_stats"] = {k: stats.get(k) for k in ("approx_kl", "clip_fraction", "log_ratio_mean", "lr")}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="both", choices=["c3", "c2", "both"])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    for shape in (("c3", "c2") if a.shape == "both" else (a.shape,)):
        print(json.dumps(measure(shape, a.reps, a.warmup)), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
