#!/usr/bin/env python3
"""What GRPO(baseline="step") costs and what it does to learning: same commit, same process, same seeds.

    python3 tools/grpo_baseline_probe.py [--parts kernel,step,curves] [--reps 7] [--warmup 2] [--seeds 3] [--iters 30]

kernel: tg_grpo_step_advantage (both modes) at the C2 (64 x 64 CartPole envs x 500 steps) and C4 per-GPU (128 x 256 QuadPole envs x
        256 steps) shapes, on returns-to-go with episode-length masks, against what it replaces on the same arrays
        (tg_masked_moments + tg_group_normalize) and against a plain device copy of the same bytes (R -> A, 4 B read + 4 B written per
        entry).  Each sample is `--batch` back-to-back calls between two HIP events; medians of --reps samples, the spread
        (max - min) / median of each arm, and the achieved TB/s on the algorithmic bytes (4 B of R and 1 B of mask read, 4 B of A
        written, per entry and ONCE -- the kernels read R and the mask twice, so their own traffic is higher).
step:   one Rollout_Buffer.sample() + GRPO.learn() at the C2 and C4 per-GPU shapes with baseline="step" against "group"; the arms
        alternate within a repetition; milliseconds per step, the off arm's own spread, the on / off ratio.
curves: mean episode length per iteration, both baselines, --seeds seeds x --iters iterations: CartPole (64 x 64 envs, fp32
        5-128-128-1, the C2 hyper-parameters) and QuadPole restart groups at a reduced size (32 x 32 envs x 128 steps, bf16 256 x 5),
        with maximize=True (ascent on J; --descend: the reference's sign, GRPO's default, under which episodes get shorter).
Prints one JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import trajopt_grpo_amd as tg  # noqa: E402

K = tg.hip_ops
SHAPES = {
    "c2": dict(env="CartPole", S=5, A=1, hidden=(128, 128), cov=0.5, G=64, E=64, T=500, cdt=None, gamma=0.5, restart=False),
    "c4": dict(env="QuadPole", S=20, A=4, hidden=(256,) * 5, cov=0.3, G=128, E=256, T=256, cdt=torch.bfloat16, gamma=0.99, restart=True),
    "c4_small": dict(env="QuadPole", S=20, A=4, hidden=(256,) * 5, cov=0.3, G=32, E=32, T=128, cdt=torch.bfloat16, gamma=0.99, restart=True),
}


def spread(xs):
    return (max(xs) - min(xs)) / statistics.median(xs)


def kernel_part(args, dev):
    for shape in ("c2", "c4"):
        c = SHAPES[shape]
        T, n, E = c["T"], c["G"] * c["E"], c["E"]
        gen = torch.Generator().manual_seed(0)
        ln = torch.randint(T // 8, T + 1, (n,), generator=gen)
        mask = (torch.arange(T)[:, None] < ln[None, :]).to(torch.uint8).to(dev)
        rtg = K.rtg_scan(torch.ones(T, n, device=dev) * mask, mask, c["gamma"])
        out, out2 = torch.empty_like(rtg), torch.empty_like(rtg)
        work = torch.empty(3 * (n // E) * T, dtype=torch.float64, device=dev)
        group = torch.empty(n // E, 3, dtype=torch.float64, device=dev)
        arms = {
            "step_std": lambda: K.grpo_step_advantage(rtg, mask, E, True, out=out, work=work, group=group),
            "step_none": lambda: K.grpo_step_advantage(rtg, mask, E, False, out=out, work=work, group=group),
            "moments_normalize": lambda: K.group_normalize(rtg, mask, K.masked_moments(rtg, mask, E), 0, E),
            "copy": lambda: out2.copy_(rtg),
        }
        times = {k: [] for k in arms}
        for rep in range(args.warmup + args.reps):
            for k, fn in arms.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.batch):
                    fn()
                b.record()
                b.synchronize()
                if rep >= args.warmup:
                    times[k].append(a.elapsed_time(b) * 1e3 / args.batch)
        line = {"part": "kernel", "shape": shape, "T": T, "n": n, "E": E, "valid_share": float(mask.float().mean()), "reps": args.reps, "batch": args.batch}
        for k, xs in times.items():
            us = statistics.median(xs)
            byts = (8 if k == "copy" else 9) * T * n
            line[k] = {"us_median": round(us, 2), "us_min": round(min(xs), 2), "us_max": round(max(xs), 2), "spread": round(spread(xs), 3),
                       "algorithmic_TB_per_s": round(byts / us * 1e-6, 3)}
        line["step_std_over_moments_normalize"] = round(line["step_std"]["us_median"] / line["moments_normalize"]["us_median"], 3)
        line["step_std_over_copy"] = round(line["step_std"]["us_median"] / line["copy"]["us_median"], 3)
        print(json.dumps(line), flush=True)


def make_arm(c, dev, baseline, seed=0, updates=10, maximize=False):
    torch.manual_seed(seed)
    pol = tg.GaussianActor_NeuralNetwork(c["S"], c["A"], c["hidden"], cov=c["cov"], device=dev)
    env_cls = tg.environments.ENV_CLASSES[c["env"]]
    mgr = tg.RolloutManager(lambda: env_cls(max_steps=c["T"]), pol, restart=c["restart"], num_workers=c["G"], num_episodes_per_worker=c["E"],
                            seed=1234 + seed, compute_dtype=c["cdt"], use_graph=False)
    algo = tg.GRPO(epsilon=0.15, beta=0.5, gamma=c["gamma"], policy=pol, optimizer=torch.optim.Adam(pol.parameters(), lr=3e-4),
                   updates_per_iter=updates, autocast_dtype=c["cdt"], baseline=baseline, maximize=maximize)
    return tg.Rollout_Buffer(mgr), algo


def step_part(args, dev):
    for shape in ("c2", "c4"):
        c = SHAPES[shape]
        arms = {"group": make_arm(c, dev, "group"), "step": make_arm(c, dev, "step")}
        step, learn = ({k: [] for k in arms} for _ in range(2))
        for rep in range(args.warmup + args.reps):
            for k, (buf, algo) in arms.items():
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                ev[0].record()
                buf.sample()
                ev[1].record()
                algo.learn(buf)
                ev[2].record()
                ev[2].synchronize()
                if rep >= args.warmup:
                    step[k].append(ev[0].elapsed_time(ev[2]))
                    learn[k].append(ev[1].elapsed_time(ev[2]))
        line = {"part": "step", "shape": shape, "envs": c["G"] * c["E"], "horizon": c["T"], "reps": args.reps}
        for k in arms:
            line[k] = {"step_ms_median": round(statistics.median(step[k]), 4), "step_ms_min": round(min(step[k]), 4), "step_ms_max": round(max(step[k]), 4),
                       "learn_ms_median": round(statistics.median(learn[k]), 4), "learn_spread": round(spread(learn[k]), 3)}
        line["off_spread"] = round(spread(step["group"]), 3)
        line["learn_step_over_group"] = round(line["step"]["learn_ms_median"] / line["group"]["learn_ms_median"], 4)
        line["note"] = "the arms' policies diverge after the first update, so their row counts differ: compare the learn() times with that in mind"
        line["baseline_explained"] = arms["step"][1].last_stats.get("baseline_explained")
        print(json.dumps(line), flush=True)
        del arms
        torch.cuda.empty_cache()


def curves_part(args, dev):
    for shape in ("c2", "c4_small"):
        c = SHAPES[shape]
        for baseline in ("group", "step"):
            runs = []
            for seed in range(args.seeds):
                buf, algo = make_arm(c, dev, baseline, seed=seed, maximize=not args.descend)
                lengths = []
                for _ in range(args.iters):
                    buf.sample()
                    traj = buf.device_traj
                    lengths.append(round(float(traj.mask.sum()) / traj.n, 2))
                    algo.learn(buf)
                runs.append(lengths)
                del buf, algo
            mean = [round(statistics.mean(r[i] for r in runs), 2) for i in range(args.iters)]
            print(json.dumps({"part": "curves", "shape": shape, "baseline": baseline, "maximize": not args.descend, "seeds": args.seeds, "mean_episode_length": mean,
                              "per_seed_last": [r[-1] for r in runs]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="kernel,step,curves")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--seeds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--descend", action="store_true", help="curves: maximize=False, the reference's sign (descent on J: episodes get shorter)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("this probe measures on the GPU: no device found")
    dev = torch.device("cuda", 0)
    with torch.cuda.device(dev):
        for part in args.parts.split(","):
            {"kernel": kernel_part, "step": step_part, "curves": curves_part}[part](args, dev)


if __name__ == "__main__":
    main()
