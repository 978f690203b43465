#!/usr/bin/env python3
"""Step time of PPO with running value normalisation (normalize_value=True) against the plain learner: same commit, same process,
same seeds.

    python3 tools/value_norm_probe.py [--shape c3|c2|both] [--reps 7] [--warmup 2]

c3: 65,536 QuadPole envs x 256 steps, PPO, actor-critic 20-256x5-{4,1} in bf16, 32 full-batch updates (bench.py's headline shape)
c2:  4,096 CartPole envs x 500 steps, PPO, actor-critic 5-128-128-{1,1} in fp32, 10 full-batch updates
The on arm runs tg_scatter_rows_affine in place of tg_scatter_rows and one tg_value_norm_merge launch after tg_ppo_norm --
unfrozen, as in training.
Each repetition is one Rollout_Buffer.sample(), one prologue-only learn() (a second PPO on the same policy with
updates_per_iter=0: everything learn() does before its first update; the on arm's statistics are frozen for this call, so that a
batch is merged once -- the merge launch runs all the same) and one full learn(), each between HIP events on the launch stream.  The
two arms alternate within a repetition so that clock and thermal drift hit both alike; both start from the same weights.  Prints one
JSON line per shape: median and spread of each arm (milliseconds, and nanoseconds per env-step: the row count of a step changes as
the policy learns), the on / off ratios, and the off arm's env-steps per second (to hold against bench.py's headline on the same
machine)."""
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


def make_arm(c, normalize_value, dev):
    torch.manual_seed(0)
    pol = tg.GaussianActorCritic_NeuralNetwork(c["S"], c["A"], c["hidden"], cov=c["cov"], device=dev,
                                               **({"normalize_value": True} if normalize_value else {}))
    env_cls = tg.environments.ENV_CLASSES[c["env"]]
    mgr = tg.RolloutManager(lambda: env_cls(max_steps=c["T"]), pol, num_workers=c["G"], num_episodes_per_worker=c["E"], seed=1234,
                            compute_dtype=c["cdt"], use_graph=False)
    buf = tg.Rollout_Buffer(mgr)
    opt = torch.optim.Adam(pol.parameters(), lr=3e-4)
    kw = dict(epsilon=0.2, policy=pol, optimizer=opt, ref_model=None, c1=0.5, kl_coeff=0.5, gamma=c["gamma"], lam=0.95, entropy=0.01,
              batch_size=None, autocast_dtype=c["cdt"])
    return buf, tg.PPO(updates_per_iter=c["updates"], **kw), tg.PPO(updates_per_iter=0, **kw)


def measure(shape, reps, warmup):
    c = SHAPES[shape]
    dev = torch.device("cuda", 0)
    arms = {"off": make_arm(c, False, dev), "on": make_arm(c, True, dev)}
    step, learn, prologue, env_steps = ({k: [] for k in arms} for _ in range(4))
    for rep in range(warmup + reps):
        for k, (buf, algo, algo0) in arms.items():
            vn = algo.policy.value_norm
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            ev[0].record()
            buf.sample()
            ev[1].record()
            if vn is not None:
                vn.freeze()
            algo0.learn(buf)
            if vn is not None:
                vn.unfreeze()
            ev[2].record()
            algo.learn(buf)
            ev[3].record()
            ev[3].synchronize()
            if rep >= warmup:
                step[k].append(ev[0].elapsed_time(ev[1]) + ev[2].elapsed_time(ev[3]))
                learn[k].append(ev[2].elapsed_time(ev[3]))
                prologue[k].append(ev[1].elapsed_time(ev[2]))
                env_steps[k].append(float(buf.device_traj.env_steps()))
    out = {"shape": shape, "envs": c["G"] * c["E"], "horizon": c["T"], "updates": c["updates"], "reps": reps, "warmup": warmup}
    for k in arms:
        for name, xs in (("step_ms", step[k]), ("learn_ms", learn[k]), ("prologue_ms", prologue[k])):
            out[f"{k}_{name}_median"], out[f"{k}_{name}_min"], out[f"{k}_{name}_max"] = statistics.median(xs), min(xs), max(xs)
        out[f"{k}_env_steps_per_s"] = statistics.median(e / (t * 1e-3) for e, t in zip(env_steps[k], step[k]))
        # the number of valid rows changes from one iteration to the next (and between the arms, whose policies drift apart), so the
        # comparison is on time per env-step
        ns = [t * 1e6 / e for t, e in zip(step[k], env_steps[k])]
        out[f"{k}_ns_per_env_step_median"], out[f"{k}_ns_per_env_step_min"], out[f"{k}_ns_per_env_step_max"] = statistics.median(ns), min(ns), max(ns)
    out["off_spread"] = (out["off_ns_per_env_step_max"] - out["off_ns_per_env_step_min"]) / out["off_ns_per_env_step_median"]
    out["off_prologue_spread"] = (out["off_prologue_ms_max"] - out["off_prologue_ms_min"]) / out["off_prologue_ms_median"]
    out["on_over_off"] = out["on_ns_per_env_step_median"] / out["off_ns_per_env_step_median"]
    out["on_over_off_prologue_ms"] = out["on_prologue_ms_median"] / out["off_prologue_ms_median"]
    stats = arms["on"][1].last_stats
    out["on_value_stats"] = {k: stats.get(k) for k in ("value_mean", "value_std", "value_count", "explained_variance")}
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
