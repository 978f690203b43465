#!/usr/bin/env python3
"""What the actuator lag (Env.motor_time_constant) costs on the device rollout paths.

    python3 tools/motor_lag_probe.py [--reps 7] [--warmup 2] [--only fused_bf16,fused_f32,per_step,forced]

Four paths, each with the lag off and on in one process; every figure is the median (min, max) of `reps` repetitions between HIP
events on the launch stream:
  fused_bf16   tg_fused_rollout at bench.py's C3 shape: 65,536 QuadPole envs x 256 steps, actor 20-256x5-4 in bf16
  fused_f32    tg_fused_rollout_f32: 4,096 QuadPole2D envs x 500 steps, actor 10-128-128-2 in fp32
  per_step     65,536 QuadPole envs x 256 steps, one actor forward and one tg_rollout_step launch per step (fp32 GEMM chain)
  forced       the same trajectory replayed by ONE tg_rollout_forced launch (timed: that launch and the finish statistics)
Arms:
  off          motor_time_constant = 0: the parent's entry points and kernels (the comparison base, with its own spread)
  on           motor_time_constant = 0.05 s: the `_lag` entries (substeps = 1), which also write the motor record
The `on` arm includes the zero-fill of the motor record in the prologue where the timed region includes the prologue (every path but
`forced`).  Each arm also reports the valid steps of its last trajectory (the lag changes the dynamics: the episodes end elsewhere)
and its time per valid step; `per_valid_step_over_off` is the ratio of those, beside `over_off`, the ratio of the launches' times.
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import trajopt_grpo_amd as tg  # noqa: E402

N = tg._native
TAU = 0.05


def timed(fn, reps, warmup, prep=None):
    out = []
    for rep in range(warmup + reps):
        if prep is not None:
            prep()
        a, b = N.event_pair()
        a.record()
        fn()
        b.record()
        b.synchronize()
        if rep >= warmup:
            out.append(a.elapsed_time(b) * 1e3)                          # microseconds
    return {"median_us": round(statistics.median(out), 1), "min_us": round(min(out), 1), "max_us": round(max(out), 1)}


def make_env(name, T, tau):
    env = tg.environments.ENV_CLASSES[name](max_steps=T)
    env.motor_time_constant = tau
    return env


def arms(name, T, G, E, pol, reps, warmup, path, **engine_kw):
    out = {}
    for arm, tau in (("off", 0.0), ("on", TAU)):
        eng = tg.DeviceRollout(make_env(name, T, tau), pol, G, E, seed=1234, **engine_kw)
        if path == "forced":
            traj = eng.run()                                             # a sampled trajectory whose actions the replay is handed
            s0, act = traj.obs[:, 0, :].clone(), traj.act.clone()

            def prep():
                eng._enqueue_prepare(None)
                eng.traj.obs[:, 0, :].copy_(s0)
                eng.traj.act.copy_(act)

            with torch.cuda.device(eng.device):
                res = timed(lambda: eng._enqueue_steps(sample=False), reps, warmup, prep)
        else:
            res = timed(eng.run, reps, warmup)
        torch.cuda.synchronize()
        assert eng.lag == (tau > 0.0) and (eng.traj.motor is not None) == eng.lag
        res["valid_steps"] = int(eng.traj.len.clamp_min(0).sum())
        res["ns_per_valid_step"] = round(res["median_us"] * 1e3 / max(res["valid_steps"], 1), 4)
        out[arm] = res
        del eng
    base = out["off"]
    out["on"]["over_off"] = round(out["on"]["median_us"] / base["median_us"], 4)
    out["on"]["per_valid_step_over_off"] = round(out["on"]["ns_per_valid_step"] / base["ns_per_valid_step"], 4)
    out["off_spread"] = round((base["max_us"] - base["min_us"]) / base["median_us"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="fused_bf16,fused_f32,per_step,forced")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    want = set(args.only.split(","))
    result = {}
    torch.manual_seed(0)
    if "fused_bf16" in want:
        pol = tg.GaussianActor_NeuralNetwork(20, 4, (256,) * 5, cov=0.3, device=dev)
        result["fused_bf16"] = {"shape": "QuadPole 65536 x 256, 20-256x5-4 bf16",
                                **arms("QuadPole", 256, 256, 256, pol, args.reps, args.warmup, "run", compute_dtype=torch.bfloat16, fused=True)}
    if "fused_f32" in want:
        pol = tg.GaussianActor_NeuralNetwork(10, 2, (128, 128), cov=0.5, device=dev)
        result["fused_f32"] = {"shape": "QuadPole2D 4096 x 500, 10-128-128-2 fp32",
                               **arms("QuadPole2D", 500, 64, 64, pol, args.reps, args.warmup, "run", fused=True)}
    if want & {"per_step", "forced"}:
        pol = tg.GaussianActor_NeuralNetwork(20, 4, (128, 128), cov=0.3, device=dev)
        for path in ("per_step", "forced"):
            if path in want:
                result[path] = {"shape": "QuadPole 65536 x 256, 20-128-128-4 fp32",
                                **arms("QuadPole", 256, 256, 256, pol, args.reps, args.warmup, "run" if path == "per_step" else "forced",
                                       fused=False, use_graph=False)}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
