#!/usr/bin/env python3
"""PPO with PopArt (normalize_value=True, popart=True) against PPO with running value normalisation alone: same commit, same process,
same seeds.

    python3 tools/popart_probe.py [--what time|learning|both] [--shape c3|c2|both] [--reps 7] [--warmup 2] [--seeds 3] [--iters 12]

(a) time.  c3: 65,536 QuadPole envs x 256 steps, actor-critic 20-256x5-{4,1} in bf16, 32 full-batch updates (bench.py's headline
    shape); c2: 4,096 CartPole envs x 500 steps, actor-critic 5-128-128-{1,1} in fp32, 10 full-batch updates.  Both arms normalise
    their value targets; the on arm's merge launch is tg_value_norm_merge_popart in place of tg_value_norm_merge, followed by the
    rebuild of the critic's derived weight layouts.  Each repetition is one Rollout_Buffer.sample(), one prologue-only learn() (a
    second PPO on the same policy with updates_per_iter=0: everything learn() does before its first update, the merge, the rescale
    and the rebuild included) and one full learn(), each between HIP events on the launch stream.  The statistics and the critic
    head are put back between the two (outside the timed spans, in both arms), so that a batch is merged once.  The arms alternate
    within a repetition; both start from the same weights.  One JSON line per shape: median and spread of each arm (milliseconds,
    and nanoseconds per env-step), the on / off ratios beside the off arm's own spread.
(b) learning.  A reduced QuadPole PPO run (1,024 envs x 128 steps, 20-128x3 in bf16, 8 full-batch updates per iteration), `--seeds`
    seeds, `--iters` iterations per arm: the FIRST update's critic_loss of every learn() -- the squared error, in normalised units,
    of the critic the previous learn() left against this learn()'s targets, which is what the rescale is meant to lower -- and the
    last update's, per iteration, averaged over the seeds, with popart_scale / popart_shift of the on arm.  One JSON line."""
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
    "small": dict(env="QuadPole", S=20, A=4, hidden=(128,) * 3, cov=0.3, G=32, E=32, T=128, cdt=torch.bfloat16, updates=8, gamma=0.99),
}


def make_arm(c, popart, dev, seed=0, prologue=True):
    torch.manual_seed(seed)
    pol = tg.GaussianActorCritic_NeuralNetwork(c["S"], c["A"], c["hidden"], cov=c["cov"], device=dev, normalize_value=True,
                                               **({"popart": True} if popart else {}))
    env_cls = tg.environments.ENV_CLASSES[c["env"]]
    mgr = tg.RolloutManager(lambda: env_cls(max_steps=c["T"]), pol, num_workers=c["G"], num_episodes_per_worker=c["E"], seed=1234 + seed,
                            compute_dtype=c["cdt"], use_graph=False)
    buf = tg.Rollout_Buffer(mgr)
    opt = torch.optim.Adam(pol.parameters(), lr=3e-4)
    kw = dict(epsilon=0.2, policy=pol, optimizer=opt, ref_model=None, c1=0.5, kl_coeff=0.5, gamma=c["gamma"], lam=0.95, entropy=0.01,
              batch_size=None, autocast_dtype=c["cdt"])
    return buf, tg.PPO(updates_per_iter=c["updates"], **kw), (tg.PPO(updates_per_iter=0, **kw) if prologue else None)


def measure(shape, reps, warmup):
    c = SHAPES[shape]
    dev = torch.device("cuda", 0)
    arms = {"off": make_arm(c, False, dev), "on": make_arm(c, True, dev)}
    step, learn, prologue, env_steps = ({k: [] for k in arms} for _ in range(4))
    for rep in range(warmup + reps):
        for k, (buf, algo, algo0) in arms.items():
            vn, head = algo.policy.value_norm, algo.policy.critic.network[-1]
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
            ev[0].record()
            buf.sample()
            kept =[t.clone() for t in (vn.count, vn.mean, vn.m2, head.weight.detach(), head.bias.detach())]
            ev[1].record()
            algo0.learn(buf)
            ev[2].record()
            with torch.no_grad():                       # (untimed: the batch is merged once, by the full learn() below)
                head.weight.copy_(kept[3])
                head.bias.copy_(kept[4])
            vn.load_state(*kept[:3])
            ev[3].record()
            algo.learn(buf)
            ev[4].record()
            ev[4].synchronize()
            if rep >= warmup:
                step[k].append(ev[0].elapsed_time(ev[1]) + ev[3].elapsed_time(ev[4]))
                learn[k].append(ev[3].elapsed_time(ev[4]))
                prologue[k].append(ev[1].elapsed_time(ev[2]))
                env_steps[k].append(float(buf.device_traj.env_steps()))
    out = {"what": "time", "shape": shape, "envs": c["G"] * c["E"], "horizon": c["T"], "updates": c["updates"], "reps": reps,
           "warmup": warmup}
    for k in arms:
        for name, xs in (("step_ms", step[k]), ("learn_ms", learn[k]), ("prologue_ms", prologue[k])):
            out[f"{k}_{name}_median"], out[f"{k}_{name}_min"], out[f"{k}_{name}_max"] = statistics.median(xs), min(xs), max(xs)
        out[f"{k}_env_steps_per_s"] = statistics.median(e / (t * 1e-3) for e, t in zip(env_steps[k], step[k]))
        # (the number of valid rows changes from one iteration to the next, and between the arms: the comparison is per env-step)
        ns = [t * 1e6 / e for t, e in zip(step[k], env_steps[k])]
        out[f"{k}_ns_per_env_step_median"], out[f"{k}_ns_per_env_step_min"], out[f"{k}_ns_per_env_step_max"] = statistics.median(ns), min(ns), max(ns)
    out["off_spread"] = (out["off_ns_per_env_step_max"] - out["off_ns_per_env_step_min"]) / out["off_ns_per_env_step_median"]
    out["off_prologue_spread"] = (out["off_prologue_ms_max"] - out["off_prologue_ms_min"]) / out["off_prologue_ms_median"]
    out["on_over_off"] = out["on_ns_per_env_step_median"] / out["off_ns_per_env_step_median"]
    out["on_over_off_prologue_ms"] = out["on_prologue_ms_median"] / out["off_prologue_ms_median"]
    stats = arms["on"][1].last_stats
    out["on_value_stats"] = {k: stats.get(k) for k in ("value_mean", "value_std", "value_count", "popart_scale", "popart_shift")}
    return out


def learning(seeds, iters):
    c = SHAPES["small"]
    dev = torch.device("cuda", 0)
    runs = {"off": [], "on": []}
    for seed in range(seeds):
        for k in ("off", "on"):                          # (alternating, in one process)
            buf, algo, _ = make_arm(c, k == "on", dev, seed=seed, prologue=False)
            rows = []
            for _ in range(iters):
                buf.sample()
                algo.learn(buf)
                s = algo.last_stats
                rows.append({"first": s["critic_loss"][0], "last": s["critic_loss"][-1], "value_mean": s["value_mean"],
                             "value_std": s["value_std"], "scale": s.get("popart_scale"), "shift": s.get("popart_shift")})
            runs[k].append(rows)
    out = {"what": "learning", "envs": c["G"] * c["E"], "horizon": c["T"], "updates": c["updates"], "seeds": seeds, "iters": iters}
    for k, per_seed in runs.items():
        for name in ("first", "last"):
            out[f"{k}_critic_loss_{name}_update"] = [statistics.mean(r[i][name] for r in per_seed) for i in range(iters)]
            out[f"{k}_critic_loss_{name}_update_by_seed"] = [[r[i][name] for i in range(iters)] for r in per_seed]
        out[f"{k}_value_mean"] = [statistics.mean(r[i]["value_mean"] for r in per_seed) for i in range(iters)]
        out[f"{k}_value_std"] = [statistics.mean(r[i]["value_std"] for r in per_seed) for i in range(iters)]
    out["on_popart_scale_by_seed"] = [[r[i]["scale"] for i in range(iters)] for r in runs["on"]]
    out["on_popart_shift_by_seed"] = [[r[i]["shift"] for i in range(iters)] for r in runs["on"]]
    # iteration 0 fills the statistics (nothing to rescale): the comparison starts at iteration 1
    on, off = out["on_critic_loss_first_update"][1:], out["off_critic_loss_first_update"][1:]
    out["first_update_on_over_off_by_iteration"] = [a / b for a, b in zip(on, off)]
    out["first_update_on_over_off_mean"] = sum(on) / sum(off)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="both", choices=["time", "learning", "both"])
    ap.add_argument("--shape", default="both", choices=["c3", "c2", "both"])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seeds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=12)
    a = ap.parse_args()
    if a.what in ("time", "both"):
        for shape in (("c3", "c2") if a.shape == "both" else (a.shape,)):
            print(json.dumps(measure(shape, a.reps, a.warmup)), flush=True)
            torch.cuda.empty_cache()
    if a.what in ("learning", "both"):
        print(json.dumps(learning(a.seeds, a.iters)), flush=True)


if __name__ == "__main__":
    main()
