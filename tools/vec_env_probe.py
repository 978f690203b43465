#!/usr/bin/env python3
"""What one DeviceVecEnv.step() costs, against the composition of entry points it replaces.

    python3 tools/vec_env_probe.py [--reps 7] [--warmup 2] [--steps 200]

Two shapes, float32: 4,096 CartPole slots and 65,536 QuadPole slots (max_steps = 200, small random actions: both kinds of ending
occur while the window runs).  Two arms, the same work per step -- n actions [n][A] in, n observations [n][S], rewards and done flags
out, ended slots reset:
  vec_env       DeviceVecEnv.step(): one tg_vec_env_step launch
  composition   what the entry points without it need: the action transpose to [A][n], tg_env_step in place, tg_env_reset into a
                spare state, the done mask, torch.where selects for the state and the step count, the transpose to [n][S]
                (8 launches: the done mask is two; no substeps, lag, per-env parameters, episode statistics or final observations)
Each arm is timed two ways, per step, as the median (min, max) of `reps` windows of `steps` steps between HIP events:
  eager         the calls issued from Python one by one: what a training loop pays (host-bound when the kernels are short)
  graph         the same `steps` steps captured once into a hipGraph and replayed: the device time of the launches alone.  The
                vector env can be captured because nothing its launch takes by value changes from step to step; the composition's
                tg_env_reset takes the stream id by value, so a replay repeats its draws (the work is the same).
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


def window_stats(us):
    med = statistics.median(us)
    return {"median_us": round(med, 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2), "spread": round((max(us) - min(us)) / med, 4)}


def timed(fn, reps, warmup, steps):
    """fn() runs `steps` steps; -> per-step microseconds of `reps` windows."""
    out = []
    for rep in range(warmup + reps):
        a, b = N.event_pair()
        a.record()
        fn()
        b.record()
        b.synchronize()
        if rep >= warmup:
            out.append(a.elapsed_time(b) * 1e3 / steps)
    return window_stats(out)


def both_ways(one_step, reps, warmup, steps):
    def eager():
        for _ in range(steps):
            one_step()

    res = {"eager": timed(eager, reps, warmup, steps)}
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        one_step()                                                       # (every allocation of a step made once before the capture)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eager()
    res["graph"] = timed(graph.replay, reps, warmup, steps)
    return res


def composition(env, n, dev, seed):
    """One step from the entry points that exist without the vector env; -> callable(actions [n][A])."""
    lib, p, S, T = N.load(), env.native_params(), env.obs_dim, int(env.max_steps)
    state, fresh = torch.zeros(S, n, device=dev), torch.zeros(S, n, device=dev)
    steps = torch.zeros(n, dtype=torch.int32, device=dev)
    rew, trunc = torch.zeros(n, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev)
    zero = torch.zeros((), dtype=torch.int32, device=dev)
    counter = [0]
    N.check(lib.tg_env_reset(C.byref(p), N.TG_F32, state.data_ptr(), n, n, seed, 0, 0, 1, N.stream_ptr(dev)), "tg_env_reset")

    def one_step(actions):
        st = N.stream_ptr(dev)
        act = actions.t().contiguous()
        N.check(lib.tg_env_step(C.byref(p), N.TG_F32, state.data_ptr(), n, act.data_ptr(), n, state.data_ptr(), n, steps.data_ptr(), None,
                                rew.data_ptr(), trunc.data_ptr(), n, st), "tg_env_step")
        counter[0] += 1
        N.check(lib.tg_env_reset(C.byref(p), N.TG_F32, fresh.data_ptr(), n, n, seed, counter[0], 0, 1, st), "tg_env_reset")
        done = trunc.view(torch.bool) | (steps >= T)
        torch.where(done, fresh, state, out=state)
        torch.where(done, zero, steps, out=steps)
        return state.t().contiguous(), rew, done

    return one_step


def probe(name, n, reps, warmup, steps, dev):
    env = tg.environments.ENV_CLASSES[name](max_steps=200)
    torch.manual_seed(0)
    actions = (torch.randn(n, env.act_dim, device=dev) * 0.3).contiguous()
    vec = tg.DeviceVecEnv(env, n, seed=1, device=dev)
    vec.reset(seed=1)
    out = {"shape": f"{name} x {n}, float32", "vec_env": both_ways(lambda: vec.step(actions), reps, warmup, steps)}
    comp = composition(env, n, dev, 1)
    out["composition"] = both_ways(lambda: comp(actions), reps, warmup, steps)
    for how in ("eager", "graph"):
        out[f"composition_over_vec_env_{how}"] = round(out["composition"][how]["median_us"] / out["vec_env"][how]["median_us"], 3)
    torch.cuda.synchronize()
    out["episodes_ended_in_vec_env"] = int(vec.episode_ordinals.sum())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=200)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("vec_env_probe.py needs an MI355X")
    dev = torch.device("cuda", 0)
    result = {}
    with torch.cuda.device(dev):
        for key, name, n in (("cartpole_4096", "CartPole", 4096), ("quadpole_65536", "QuadPole", 65536)):
            result[key] = probe(name, n, args.reps, args.warmup, args.steps, dev)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
