#!/usr/bin/env python3
"""What DeviceRolloutStorage's add(), compute_returns() and shuffle() + minibatch() cost, against the torch compositions of
tools/vec_env_ppo.py that they replace.

    python3 tools/segment_probe.py [--reps 7] [--warmup 2] [--steps 50]

Two shapes -- 4,096 slots of CartPole's widths (S = 5, A = 1) and 65,536 slots of QuadPole's (S = 20, A = 4) -- with L = 128,
synthetic step results with 2 % of the slots ending per step (half terminated, half truncated).  Per shape, three pairs of arms:
  add       storage: one tg_segment_push launch          torch: lines 41-50 of the tool (copy_ of obs, act / logp / val rows, where on the
                                                                 truncation, rew + gamma * boot, the done row), cycling through t
  returns   storage: one tg_segment_gae launch           torch: the reversed loop of lines 53-60 over the same stored segment
  batch     storage: tg_segment_permute + one            torch: randperm(L n) + the six index_selects of one minibatch
            tg_segment_gather of L n / 4 rows
The torch arm is never the code under test.  Each arm is timed two ways, per call, as the median (min, max) of `reps` windows of
`steps` calls between HIP events: issued from Python, and captured once into a hipGraph and replayed (the torch arm of `batch` from
Python only).  Prints one JSON line."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import trajopt_grpo_amd as tg  # noqa: E402
from replay_probe import both_ways, timed  # noqa: E402


def step_results(S, A, n, dev, variants=8):
    gen = torch.Generator(device=dev).manual_seed(0)
    out = []
    for _ in range(variants):
        done = torch.rand(n, device=dev, generator=gen) < 0.02
        term = done & (torch.rand(n, device=dev, generator=gen) < 0.5)
        r = lambda *shape: torch.randn(*shape, device=dev, generator=gen)
        out.append((r(n, A), r(n), r(n), r(n, S), r(n), term, done & ~term, r(n)))      # add()'s eight arguments
    return out


def probe(S, A, n, L, reps, warmup, steps, dev, gamma=0.99, lam=0.95, minibatches=4):
    feed = step_results(S, A, n, dev)
    st = tg.DeviceRolloutStorage(S, A, n, L, gamma=gamma, lam=lam, device=dev)
    st.start(torch.randn(n, S, device=dev))
    buf = {k: torch.empty(L, n, *w, device=dev) for k, w in (("obs", (S,)), ("act", (A,)), ("logp", ()), ("val", ()), ("rew", ()), ("done", ()))}
    turn = [0, 0]

    def storage_add():
        st.add(*feed[turn[0] % len(feed)])
        turn[0] += 1

    def torch_add():
        act, logp, val, obs, rew, terminated, truncated, final_value = feed[turn[1] % len(feed)]
        t = turn[1] % L
        buf["obs"][t].copy_(obs)
        buf["act"][t], buf["logp"][t], buf["val"][t] = act, logp, val
        buf["rew"][t] = rew + gamma * torch.where(truncated, final_value, 0.0)
        buf["done"][t] = terminated | truncated
        turn[1] += 1

    out = {"shape": f"S={S} A={A} n={n} L={L}"}
    out["add"] = {"storage": both_ways(storage_add, reps, warmup, steps), "torch": both_ways(torch_add, reps, warmup, steps)}
    for k in range(2 * L):                                              # both arms hold the same whole segment from here on
        st.add(*feed[k % len(feed)])
    for name, src in (("act", st.act), ("logp", st.logp), ("val", st.val), ("rew", st.rew)):
        buf[name].copy_(src)
    buf["obs"].copy_(torch.cat([st.first_obs[None], st.obs[1:L]]))
    buf["done"].copy_(st.done)
    last_value = torch.randn(n, device=dev)
    adv = torch.empty(L, n, device=dev)

    def torch_returns():
        last, nxt = torch.zeros(n, device=dev), last_value
        for t in reversed(range(L)):
            live = 1.0 - buf["done"][t]
            delta = buf["rew"][t] + gamma * nxt * live - buf["val"][t]
            last = delta + gamma * lam * live * last
            adv[t], nxt = last, buf["val"][t]
        return adv + buf["val"]

    ret = torch_returns()
    got_adv, got_ret = st.compute_returns(last_value)
    out["arms_compute_the_same_returns"] = bool(torch.equal(got_adv, adv) and torch.equal(got_ret, ret))
    out["returns"] = {"storage": both_ways(lambda: st.compute_returns(last_value), reps, warmup, max(steps // 10, 2)),
                      "torch": both_ways(torch_returns, reps, warmup, max(steps // 10, 2))}
    flat = {k: v.reshape(L * n, *v.shape[2:]) for k, v in buf.items()}
    f_adv, f_ret = adv.reshape(-1), ret.reshape(-1)

    def storage_batch():
        st.shuffle()
        return st.minibatch(0, minibatches)

    def torch_batch():
        idx = torch.randperm(L * n, device=dev).chunk(minibatches)[0]
        return flat["obs"][idx], flat["act"][idx], flat["logp"][idx], f_adv[idx], f_ret[idx], flat["val"][idx]

    # (the torch arm of `batch` is issued from Python only: no capture of torch.randperm is attempted)
    out["batch"] = {"storage": both_ways(storage_batch, reps, warmup, steps),
                    "torch": {"eager": timed(lambda: [torch_batch() for _ in range(steps)], reps, warmup, steps)}}
    for what in ("add", "returns", "batch"):
        for how in ("eager", "graph") if "graph" in out[what]["torch"] else ("eager",):
            out[what][f"torch_over_storage_{how}"] = round(out[what]["torch"][how]["median_us"] / out[what]["storage"][how]["median_us"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=50)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("segment_probe.py needs an MI355X")
    dev = torch.device("cuda", 0)
    result = {}
    with torch.cuda.device(dev):
        for key, S, A, n in (("cartpole_4096", 5, 1, 4096), ("quadpole_65536", 20, 4, 65536)):
            result[key] = probe(S, A, n, 128, args.reps, args.warmup, args.steps, dev)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
