#!/usr/bin/env python3
"""What control decimation (Env.substeps) costs on the device rollout paths.

    python3 tools/substeps_probe.py [--reps 7] [--warmup 2] [--only fused_bf16,fused_f32,per_step,forced]

Four paths, each in three arms; every figure is the median (min, max) of `reps` repetitions between HIP events on the launch stream:
  fused_bf16   tg_fused_rollout at bench.py's C3 shape: 65,536 QuadPole envs x 256 steps, actor 20-256x5-4 in bf16
  fused_f32    tg_fused_rollout_f32 at the C2 shape: 4,096 CartPole envs x 500 steps, actor 5-128-128-1 in fp32
  per_step     65,536 QuadPole envs x 256 steps, one actor forward and one tg_rollout_step launch per step (fp32 GEMM chain)
  forced       the same trajectory replayed by ONE tg_rollout_forced launch (timed: that launch and the finish statistics)
Arms:
  plain        the entry point without `_sub` (the comparison base, with its own spread)
  sub_k1       the `_sub` entry with substeps = 1: the Substepped kernel doing the plain kernel's work
  sub_k4       Env.substeps = 4 with timestep / 4: the same control period and horizon, four physics steps per policy step
Each arm also reports the valid control steps of its last trajectory (the arms' episodes differ: finer physics ends them elsewhere).
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
R = tg.rollout
PLAIN_ENTRIES = (R.fused_entry, R.step_entry, R.sub_tail)


def force_sub_entries(on: bool):
    """on: every launch of a substeps == 1 engine goes through the `_sub` entry points with substeps = 1."""
    if not on:
        R.fused_entry, R.step_entry, R.sub_tail = PLAIN_ENTRIES
        return
    fused, step, _ = PLAIN_ENTRIES

    def fused_k1(f32, act, ptab, obs_norm, substeps=1):
        name, table, tail = fused(f32, act, ptab, obs_norm, 2)
        return name, table, tail[:-1] + (1,)

    R.fused_entry = fused_k1
    R.step_entry = lambda forced, ptab, substeps=1: step(forced, ptab, 2)
    R.sub_tail = lambda substeps: (1,)


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


def make_env(name, T, k):
    env = tg.environments.ENV_CLASSES[name](max_steps=T)
    if k != 1:
        env.substeps = k
        env.timestep = env.timestep / k
    return env


def arms(name, T, G, E, pol, reps, warmup, path, **engine_kw):
    out = {}
    for arm, k, forced_sub in (("plain", 1, False), ("sub_k1", 1, True), ("sub_k4", 4, False)):
        force_sub_entries(forced_sub)
        try:
            eng = tg.DeviceRollout(make_env(name, T, k), pol, G, E, seed=1234, **engine_kw)
            if path == "forced":
                traj = eng.run()                                         # a sampled trajectory whose actions the replay is handed
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
            res["control_steps"] = int(eng.traj.len.clamp_min(0).sum())
            res["substeps"] = k
            out[arm] = res
            del eng
        finally:
            force_sub_entries(False)
    base = out["plain"]
    for arm in ("sub_k1", "sub_k4"):
        out[arm]["over_plain"] = round(out[arm]["median_us"] / base["median_us"], 4)
    out["plain_spread"] = round((base["max_us"] - base["min_us"]) / base["median_us"], 4)
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
        pol = tg.GaussianActor_NeuralNetwork(5, 1, (128, 128), cov=0.5, device=dev)
        result["fused_f32"] = {"shape": "CartPole 4096 x 500, 5-128-128-1 fp32",
                               **arms("CartPole", 500, 64, 64, pol, args.reps, args.warmup, "run", fused=True)}
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
