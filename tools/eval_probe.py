#!/usr/bin/env python3
"""What an evaluation costs on the device: the statistics kernels against the training path's own reduction of the same reward
array, and a whole Evaluator.evaluate() of a sweep against one training rollout of the same env count.

    python3 tools/eval_probe.py [--reps 7] [--warmup 2]

One process, 65,536 QuadPole envs x 256 steps (bench.py's headline shape; actor 20-256x5-4 in bf16 on the fused rollout kernel).
Each figure is the median of `reps` repetitions between HIP events on the launch stream:
  finish_stats   tg_rollout_finish_stats of the sampled trajectory (two launches; reads rew [T][n] and len [n]): the yardstick
  eval_cells     tg_eval_cells, 16 cells x 4,096 episodes (two launches; reads rew up to each episode's length, len twice, timeout,
                 writes and re-reads the f64 returns; mask is not read: len says the same)
  final_state    tg_rollout_final_state (one launch; one observation and action column per env, one state row written)
  rollout        one sampled DeviceRollout.run() of 65,536 envs
  evaluate       Evaluator.evaluate() of a 4 x 4 sweep (mass x tether_length) at 4,096 episodes per cell: reset, grid, tile, the
                 mean-action rollout on the `_dr` kernel, final state, cell statistics
Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import trajopt_grpo_amd as tg  # noqa: E402

N = tg._native
K = tg.hip_ops


def timed(fn, reps, warmup):
    out = []
    for rep in range(warmup + reps):
        a, b = N.event_pair()
        a.record()
        fn()
        b.record()
        b.synchronize()
        if rep >= warmup:
            out.append(a.elapsed_time(b) * 1e3)                          # microseconds
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    G, E, T, S, A = 16, 4096, 256, 20, 4
    n = G * E
    torch.manual_seed(0)
    pol = tg.GaussianActor_NeuralNetwork(S, A, (256,) * 5, cov=0.3, device=dev)
    eng = tg.DeviceRollout(tg.QuadPole(max_steps=T), pol, G, E, seed=1234, compute_dtype=torch.bfloat16, fused=True)
    traj = eng.run()
    torch.cuda.synchronize()
    lib, st = N.load(), N.stream_ptr(dev)
    tr = traj.native()
    stats, work = torch.zeros(3, dtype=torch.float64, device=dev), torch.empty(256, dtype=torch.float64, device=dev)
    s_final = torch.empty(n, S, dtype=torch.float32, device=dev)
    timeout = torch.empty(n, dtype=torch.uint8, device=dev)
    returns, cells = torch.empty(n, dtype=torch.float64, device=dev), torch.empty(G, 8, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        t_stats = timed(lambda: N.check(lib.tg_rollout_finish_stats(C.byref(tr), None, stats.data_ptr(), work.data_ptr(), st)), args.reps, args.warmup)
        t_final = timed(lambda: K.rollout_final_state(eng.params, traj, s_final, timeout), args.reps, args.warmup)
        t_cells = timed(lambda: K.eval_cells(traj, timeout, E, returns, cells), args.reps, args.warmup)
        steps = int(traj.len.clamp_min(0).sum())
        ended = int(((traj.len >= 1) & (traj.len <= T)).sum())
        assert abs(float(cells[:, 1].sum()) - float(stats[0])) <= 1e-9 * abs(float(stats[0])) + 1e-6      # the same rewards, summed twice
        t_rollout = timed(lambda: eng.run(), args.reps, args.warmup)
        ev = tg.Evaluator(tg.QuadPole(max_steps=T), pol, episodes=E, sweep={"mass": [0.7, 0.9, 1.1, 1.4], "tether_length": [0.5, 0.8, 1.25, 2.0]},
                          seed=1, compute_dtype=torch.bfloat16)
        t_eval = timed(lambda: ev.evaluate(), args.reps, args.warmup)
        res = ev.evaluate()
        eval_steps = int(ev.engine.traj.len.clamp_min(0).sum())
    bytes_stats = 4 * T * n + 4 * n
    bytes_cells = 4 * steps + 2 * 4 * n + n + 2 * 8 * n                  # rewards of the valid steps, len twice, timeout, returns out + in
    bytes_final = ended * (4 * (S + A) + 4 * S) + 4 * n + n
    fmt = lambda t: {"median_us": round(t[0], 2), "min_us": round(t[1], 2), "max_us": round(t[2], 2)}
    print(json.dumps({
        "shape": {"env": "QuadPole", "n": n, "T": T, "cells": G, "episodes_per_cell": E, "env_steps_of_the_trajectory": steps},
        "finish_stats": {**fmt(t_stats), "bytes": bytes_stats}, "eval_cells": {**fmt(t_cells), "bytes": bytes_cells},
        "final_state": {**fmt(t_final), "bytes": bytes_final},
        "eval_cells_over_finish_stats": round(t_cells[0] / t_stats[0], 3),
        "rollout": {**fmt(t_rollout), "env_steps": steps}, "evaluate_4x4": {**fmt(t_eval), "env_steps": eval_steps},
        "evaluate_over_rollout": round(t_eval[0] / t_rollout[0], 3),
        "evaluate_summary": {k: (round(v, 3) if isinstance(v, float) else v) for k, v in res.summary.items()},
    }))


if __name__ == "__main__":
    main()
