#!/usr/bin/env python3
"""What DeviceReplayBuffer.add() and .sample() cost, against the torch compositions they replace.

    python3 tools/replay_probe.py [--reps 7] [--warmup 2] [--steps 200]

add: two shapes -- 4,096 slots of CartPole's widths (S = 5, A = 1) and 65,536 slots of QuadPole's (S = 20, A = 4) -- at n_step 1 and
3, a ring of 64 time slots, synthetic step results with 2 % of the slots ending per step (half terminated, half truncated; the
buffer's work does not depend on where the numbers come from).  Two arms, the same stored rows (checked once before timing):
  replay        DeviceReplayBuffer.add(): one tg_replay_push launch
  torch         the same rule in torch ops with a device-side cursor: a clone of obs, torch.where on final_obs, index_copy_ of the
                five row arrays (obs, act, rew, next_obs, disc), and per open step j an index_select / where / index_copy_ round for
                rew, next_obs and disc (no nstep array)
sample: B = 256 and 65,536 from the full 65,536-slot ring:
  replay        DeviceReplayBuffer.sample(B): one tg_replay_sample launch (draws included)
  torch         torch.randint + five index_select on the same storage
Each arm is timed two ways, per call, as the median (min, max) of `reps` windows of `steps` calls between HIP events: issued eagerly
from Python, and captured once into a hipGraph and replayed (the device time of the launches alone).  Prints one JSON line."""
import argparse
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


def both_ways(one_call, reps, warmup, steps):
    def eager():
        for _ in range(steps):
            one_call()

    res = {"eager": timed(eager, reps, warmup, steps)}
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        one_call()                                                       # (every allocation of a call made once before the capture)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eager()
    res["graph"] = timed(graph.replay, reps, warmup, steps)
    return res


class TorchReplay:
    """DeviceReplayBuffer's push rule as torch ops; the cursor, fill count and open counts live on the device, so it can be captured."""

    def __init__(self, S, A, n, K, n_step, gamma, dev):
        self.n, self.K, self.n_step = n, K, n_step
        self.g = torch.tensor(tg.replay.discount_table(gamma, n_step), device=dev)
        rows = K * n
        self.obs, self.next_obs = torch.zeros(rows, S, device=dev), torch.zeros(rows, S, device=dev)
        self.act, self.rew, self.disc = torch.zeros(rows, A, device=dev), torch.zeros(rows, device=dev), torch.zeros(rows, device=dev)
        self.last_obs = torch.zeros(n, S, device=dev)
        self.cursor = torch.zeros((), dtype=torch.int64, device=dev)
        self.open = torch.zeros(n, dtype=torch.int64, device=dev)
        self.ar = torch.arange(n, device=dev)
        self.zero = torch.zeros((), device=dev)

    def start(self, obs):
        self.last_obs.copy_(obs)
        self.open.zero_()

    def add(self, actions, obs, reward, terminated, truncated, info):
        n, K = self.n, self.K
        kept = obs.clone()                                               # (the env overwrites its buffer: what a torch loop must keep)
        done = terminated | truncated
        nx = torch.where(done[:, None], info["final_obs"], kept)
        rows = self.cursor * n + self.ar
        self.obs.index_copy_(0, rows, self.last_obs)
        self.act.index_copy_(0, rows, actions)
        self.rew.index_copy_(0, rows, reward)
        self.next_obs.index_copy_(0, rows, nx)
        self.disc.index_copy_(0, rows, torch.where(terminated, self.zero, self.g[1]))
        for j in range(1, self.n_step):
            live = self.open >= j
            rows_j = torch.remainder(self.cursor - j, K) * n + self.ar
            grown = self.rew.index_select(0, rows_j) + self.g[j] * reward      # (two roundings, as the kernel's)
            self.rew.index_copy_(0, rows_j, torch.where(live, grown, self.rew.index_select(0, rows_j)))
            self.next_obs.index_copy_(0, rows_j, torch.where(live[:, None], nx, self.next_obs.index_select(0, rows_j)))
            self.disc.index_copy_(0, rows_j, torch.where(live, torch.where(terminated, self.zero, self.g[j + 1]),
                                                         self.disc.index_select(0, rows_j)))
        self.open.copy_(torch.where(done, 0, (self.open + 1).clamp(max=self.n_step - 1)))
        self.cursor.copy_(torch.remainder(self.cursor + 1, K))
        self.last_obs.copy_(kept)


def step_results(S, A, n, dev, variants=8):
    """`variants` synthetic (actions, obs, reward, terminated, truncated, info) tuples, cycled through."""
    gen = torch.Generator(device=dev).manual_seed(0)
    out = []
    for _ in range(variants):
        done = torch.rand(n, device=dev, generator=gen) < 0.02
        term = done & (torch.rand(n, device=dev, generator=gen) < 0.5)
        out.append((torch.randn(n, A, device=dev, generator=gen), torch.randn(n, S, device=dev, generator=gen),
                    torch.randn(n, device=dev, generator=gen), term, done & ~term,
                    {"final_obs": torch.randn(n, S, device=dev, generator=gen)}))
    return out


def probe_add(S, A, n, n_step, reps, warmup, steps, dev, K=64):
    feed = step_results(S, A, n, dev)
    ours = tg.DeviceReplayBuffer(S, A, n, K, n_step=n_step, gamma=0.99, device=dev)
    theirs = TorchReplay(S, A, n, K, n_step, 0.99, dev)
    first = torch.randn(n, S, device=dev)
    ours.start(first)
    theirs.start(first)
    for k in range(2 * K + 3):                                           # the two arms store the same rows
        ours.add(*feed[k % len(feed)])
        theirs.add(*feed[k % len(feed)])
    same = all(torch.equal(getattr(ours, name), getattr(theirs, name)) for name in ("obs", "act", "rew", "next_obs", "disc"))
    turn = [0]

    def call(buf):
        def one():
            buf.add(*feed[turn[0] % len(feed)])
            turn[0] += 1
        return one

    out = {"shape": f"S={S} A={A} n={n} K={K} n_step={n_step}", "arms_store_the_same_rows": bool(same),
           "replay": both_ways(call(ours), reps, warmup, steps), "torch": both_ways(call(theirs), reps, warmup, steps)}
    for how in ("eager", "graph"):
        out[f"torch_over_replay_{how}"] = round(out["torch"][how]["median_us"] / out["replay"][how]["median_us"], 3)
    return out, ours


def probe_sample(buf, B, reps, warmup, steps, dev):
    R = len(buf)

    def torch_sample():
        idx = torch.randint(R, (B,), device=dev)
        return (buf.obs.index_select(0, idx), buf.act.index_select(0, idx), buf.rew.index_select(0, idx),
                buf.next_obs.index_select(0, idx), buf.disc.index_select(0, idx), idx)

    out = {"shape": f"B={B} from {R} rows, S={buf.obs_dim} A={buf.act_dim}",
           "replay": both_ways(lambda: buf.sample(B), reps, warmup, steps), "torch": both_ways(torch_sample, reps, warmup, steps)}
    for how in ("eager", "graph"):
        out[f"torch_over_replay_{how}"] = round(out["torch"][how]["median_us"] / out["replay"][how]["median_us"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=200)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("replay_probe.py needs an MI355X")
    dev = torch.device("cuda", 0)
    result = {}
    with torch.cuda.device(dev):
        big = None
        for key, S, A, n in (("cartpole_4096", 5, 1, 4096), ("quadpole_65536", 20, 4, 65536)):
            for n_step in (1, 3):
                result[f"add_{key}_n{n_step}"], big = probe_add(S, A, n, n_step, args.reps, args.warmup, args.steps, dev)
        for B in (256, 65536):
            result[f"sample_{B}"] = probe_sample(big, B, args.reps, args.warmup, args.steps, dev)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
