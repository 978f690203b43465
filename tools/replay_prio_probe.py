#!/usr/bin/env python3
"""What prioritised sampling costs on DeviceReplayBuffer(prioritized=True), against the torch composition it replaces.

    python3 tools/replay_prio_probe.py [--reps 7] [--warmup 2] [--steps 100]

Two full rings: 4,096 slots x 256 time slots of CartPole's widths (S = 5, A = 1; 1,048,576 rows) and 65,536 x 64 of QuadPole's
(S = 20, A = 4; 4,194,304 rows), every priority set once to |N(0, 1)| ** alpha.  At B = 256 and 65,536:
  sample   replay: DeviceReplayBuffer.sample(B), two launches (descent + gather, normalisation)
           torch:  cumsum over all priorities, stratified targets, searchsorted, five index_select, the weights by pow and a max
  update   replay: update_priorities(idx, td) -- the zero and atomicMax launches, the levels above, the crown
           torch:  index_put_ of (|td| + eps) ** alpha into the flat priority vector (which the next torch sample cumsums again)
and the cost of add() with and without priorities on both shapes.  Every figure is per call, the median (min, max) of `reps` windows
of `steps` calls between HIP events, with the arm's own spread (max - min) / median.  The replay arms are timed two ways: issued
eagerly from Python, and captured once into a hipGraph and replayed (the device time of the launches alone).  The torch arms are
timed eagerly only: torch's multi-block reductions (the max) record a memset node when captured, which this project keeps out of
its graphs.  Prints one JSON line."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import trajopt_grpo_amd as tg  # noqa: E402
from replay_probe import both_ways, step_results, timed  # noqa: E402


def against_torch(shape, ours, theirs, reps, warmup, steps):
    def eager():
        for _ in range(steps):
            theirs()
    out = {"shape": shape, "replay": both_ways(ours, reps, warmup, steps), "torch": {"eager": timed(eager, reps, warmup, steps)}}
    out["torch_over_replay_eager"] = round(out["torch"]["eager"]["median_us"] / out["replay"]["eager"]["median_us"], 3)
    return out


def filled(S, A, n, K, dev, prioritized):
    buf = tg.DeviceReplayBuffer(S, A, n, K, n_step=3, gamma=0.99, device=dev, prioritized=prioritized)
    feed = step_results(S, A, n, dev)
    buf.start(torch.randn(n, S, device=dev))
    for k in range(K + 3):
        buf.add(*feed[k % len(feed)])
    return buf, feed


def probe_add(S, A, n, K, reps, warmup, steps, dev):
    out = {"shape": f"S={S} A={A} n={n} K={K} n_step=3"}
    keep = None
    for key, prioritized in (("plain", False), ("prioritized", True)):
        buf, feed = filled(S, A, n, K, dev, prioritized)
        turn = [0]

        def one():
            buf.add(*feed[turn[0] % len(feed)])
            turn[0] += 1
        out[key] = both_ways(one, reps, warmup, steps)
        keep = buf
    for how in ("eager", "graph"):
        out[f"added_us_{how}"] = round(out["prioritized"][how]["median_us"] - out["plain"][how]["median_us"], 2)
    return out, keep


def probe_batch(buf, B, reps, warmup, steps, dev):
    R, alpha, beta, eps = len(buf), buf.alpha, buf.beta, buf.priority_eps
    flat = buf.priorities.clone()                                        # the torch arm's own priority vector
    ar = torch.arange(B, device=dev, dtype=torch.float64)
    td = torch.randn(B, device=dev)
    idx = torch.randint(R, (B,), device=dev)

    def torch_sample():
        cs = torch.cumsum(flat, 0, dtype=torch.float64)
        t = (ar + torch.rand(B, device=dev, dtype=torch.float64)) / B * cs[-1]
        rows = torch.searchsorted(cs, t, right=True).clamp_(max=R - 1)
        w = (R * flat.index_select(0, rows) / cs[-1]).pow(-beta)
        return (buf.obs.index_select(0, rows), buf.act.index_select(0, rows), buf.rew.index_select(0, rows),
                buf.next_obs.index_select(0, rows), buf.disc.index_select(0, rows), rows, (w / w.max()).float())

    def torch_update():
        flat.index_put_((idx,), (td.abs() + eps).pow(alpha))

    shape = f"B={B} from {R} rows, S={buf.obs_dim} A={buf.act_dim}"
    return (against_torch(shape, lambda: buf.sample(B), torch_sample, reps, warmup, steps),
            against_torch(shape, lambda: buf.update_priorities(idx, td), torch_update, reps, warmup, steps))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=100)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("replay_prio_probe.py needs an MI355X")
    dev = torch.device("cuda", 0)
    result = {}
    with torch.cuda.device(dev):
        for key, S, A, n, K in (("cartpole_4096x256", 5, 1, 4096, 256), ("quadpole_65536x64", 20, 4, 65536, 64)):
            result[f"add_{key}"], buf = probe_add(S, A, n, K, args.reps, args.warmup, args.steps, dev)
            buf.update_priorities(torch.arange(len(buf), device=dev), torch.randn(len(buf), device=dev))   # spread priorities
            for B in (256, 65536):
                result[f"sample_{key}_B{B}"], result[f"update_{key}_B{B}"] = probe_batch(buf, B, args.reps, args.warmup, args.steps, dev)
            del buf
            torch.cuda.empty_cache()
            print(json.dumps(result), file=sys.stderr, flush=True)       # (the results so far)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
