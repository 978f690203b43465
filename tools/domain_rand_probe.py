#!/usr/bin/env python3
"""Rollout time with per-env domain randomisation on against off: same commit, same process, same seeds.

    python3 tools/domain_rand_probe.py [--shape c3|c2|both] [--reps 7] [--warmup 2]

c3: 65,536 QuadPole envs x 256 steps, 256x5 actor, bf16 fused rollout (tg_fused_rollout / tg_fused_rollout_dr)
c2:  4,096 CartPole envs x 500 steps, 128x2 actor, fp32 fused rollout (tg_fused_rollout_f32 / tg_fused_rollout_f32_act_dr)
Each repetition is one DeviceRollout.run() (begin, reset, [tg_env_randomize], the fused launch, finish) between two HIP events on
the launch stream; the two arms alternate within a repetition so that clock and thermal drift hit both alike.  Prints one JSON
line per shape: the median and the spread of each arm and the ratio of the medians."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import trajopt_grpo_amd as tg  # noqa: E402

SHAPES = {
    "c3": dict(env="QuadPole", S=20, A=4, hidden=(256,) * 5, G=256, E=256, T=256, cdt=torch.bfloat16,
               ranges={"mass": (0.8, 1.25), "load_mass": (0.5, 2.0), "tether_length": (0.5, 2.0), "Ixx": (0.5, 2.0), "Iyy": (0.5, 2.0),
                       "Izz": (0.5, 2.0), "arm_length": (0.8, 1.25)}),
    "c2": dict(env="CartPole", S=5, A=1, hidden=(128, 128), G=64, E=64, T=500, cdt=None,
               ranges={"masscart": (0.5, 2.0), "masspole": (0.5, 2.0), "length": (0.5, 2.0)}),
}


def measure(shape, reps, warmup):
    c = SHAPES[shape]
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    pol = tg.GaussianActor_NeuralNetwork(c["S"], c["A"], c["hidden"], cov=0.3, device=dev)
    cls = tg.environments.ENV_CLASSES[c["env"]]
    arms = {"off": tg.DeviceRollout(cls(max_steps=c["T"]), pol, c["G"], c["E"], seed=1, compute_dtype=c["cdt"]),
            "on": tg.DeviceRollout(cls(max_steps=c["T"]).randomize(c["ranges"]), pol, c["G"], c["E"], seed=1, compute_dtype=c["cdt"])}
    assert all(e.fused for e in arms.values())
    times = {k: [] for k in arms}
    steps = {}
    for rep in range(warmup + reps):
        for k, eng in arms.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            tr = eng.run()
            b.record()
            b.synchronize()
            if rep >= warmup:
                times[k].append(a.elapsed_time(b))
                steps[k] = tr.env_steps()
    out = {"shape": shape, "envs": c["G"] * c["E"], "horizon": c["T"], "reps": reps, "warmup": warmup}
    for k in arms:
        out[f"{k}_ms_median"] = statistics.median(times[k])
        out[f"{k}_ms_min"], out[f"{k}_ms_max"] = min(times[k]), max(times[k])
        out[f"{k}_env_steps_last"] = steps[k]
    out["on_over_off"] = out["on_ms_median"] / out["off_ms_median"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="both", choices=["c3", "c2", "both"])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    for shape in (("c3", "c2") if a.shape == "both" else (a.shape,)):
        print(json.dumps(measure(shape, a.reps, a.warmup)), flush=True)


if __name__ == "__main__":
    main()
