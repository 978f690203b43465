#!/usr/bin/env python3
"""What target_kl / kl_every cost and what a stop saves: PPO learn() with checks between the updates against the plain learner, same
commit, same process, same seeds (patterned on tools/kl_control_probe.py).

    python3 tools/kl_stop_probe.py [--shape c3|c2|both] [--reps 7] [--warmup 2]

c3: 65,536 QuadPole envs x 256 steps, PPO, actor-critic 20-256x5-{4,1} in bf16, 32 full-batch updates (bench.py's headline shape)
c2:  4,096 CartPole envs x 500 steps, PPO, actor-critic 5-128-128-{1,1} in fp32, 10 full-batch updates
Arms (each its own policy, buffer and optimizer, all from the same seed):
    off         the plain learner
    every1      target_kl = 1e30 (never fires), kl_every = 1: a check behind every update but the last, the `_ctl` Adam launches, the
                host's wait on the check one back
    every4      the same with kl_every = 4
    stop_third  target_kl = 1e-30 with kl_every = updates // 3: the first check latches, a third of the way in; the host follows one
                check later (_KL_BREAK_LAG = 1), the updates in between are gated on the device
The learning rate is 0 in off, every1 and every4, so that these arms hold the same weights and the same rows in every repetition and
the difference is the checks alone (they measure a kl of zero, or of rounding size where the first update's own forward pass wrote
the old log-probabilities).  stop_third needs a policy that moves:
it runs at lr = 3e-4, so its weights -- and with them the number of valid rows of its rollouts -- drift away from the other arms'.
A learn() costs time per valid row, so every arm also reports nanoseconds of learn() per valid row: that is the figure to hold
stop_third against off with.  Each repetition is one Rollout_Buffer.sample() and one learn() between HIP events on
the launch stream (learn() alone is timed); the arms alternate within a repetition.  Prints one JSON line per shape: median and spread
of learn() per arm in milliseconds, the off arm's own spread, each arm's difference to off, and the cost of one check
((every1 - off) / (updates - 1))."""
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
}


def arms_of(c):
    return {"off": (0.0, {}), "every1": (0.0, {"target_kl": 1e30, "kl_every": 1}), "every4": (0.0, {"target_kl": 1e30, "kl_every": 4}),
            "stop_third": (3e-4, {"target_kl": 1e-30, "kl_every": max(c["updates"] // 3, 1)})}


def make_arm(c, lr, kw, dev):
    torch.manual_seed(0)
    pol = tg.GaussianActorCritic_NeuralNetwork(c["S"], c["A"], c["hidden"], cov=c["cov"], device=dev)
    env_cls = tg.environments.ENV_CLASSES[c["env"]]
    mgr = tg.RolloutManager(lambda: env_cls(max_steps=c["T"]), pol, num_workers=c["G"], num_episodes_per_worker=c["E"], seed=1234,
                            compute_dtype=c["cdt"], use_graph=False)
    buf = tg.Rollout_Buffer(mgr)
    opt = torch.optim.Adam(pol.parameters(), lr=lr)
    algo = tg.PPO(epsilon=0.2, policy=pol, optimizer=opt, ref_model=None, updates_per_iter=c["updates"], c1=0.5, kl_coeff=0.5,
                  gamma=c["gamma"], lam=0.95, entropy=0.01, batch_size=None, autocast_dtype=c["cdt"], **kw)
    return buf, algo


def measure(shape, reps, warmup):
    c = SHAPES[shape]
    dev = torch.device("cuda", 0)
    arms = {k: make_arm(c, lr, kw, dev) for k, (lr, kw) in arms_of(c).items()}
    learn, rows = {k: [] for k in arms}, {k: [] for k in arms}
    for rep in range(warmup + reps):
        for k, (buf, algo) in arms.items():
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            buf.sample()
            ev[0].record()
            algo.learn(buf)
            ev[1].record()
            ev[1].synchronize()
            if rep >= warmup:
                learn[k].append(ev[0].elapsed_time(ev[1]))
                rows[k].append(float(buf.device_traj.env_steps()))
    out = {"shape": shape, "envs": c["G"] * c["E"], "horizon": c["T"], "updates": c["updates"], "reps": reps, "warmup": warmup}
    for k in arms:
        out[f"{k}_learn_ms_median"], out[f"{k}_learn_ms_min"], out[f"{k}_learn_ms_max"] = statistics.median(learn[k]), min(learn[k]), max(learn[k])
        per_row = [t * 1e6 / r for t, r in zip(learn[k], rows[k])]
        out[f"{k}_rows_median"] = statistics.median(rows[k])
        out[f"{k}_ns_per_row_median"], out[f"{k}_ns_per_row_min"], out[f"{k}_ns_per_row_max"] = statistics.median(per_row), min(per_row), max(per_row)
    off = out["off_learn_ms_median"]
    out["off_spread"] = (out["off_learn_ms_max"] - out["off_learn_ms_min"]) / off
    for k in arms:
        if k != "off":
            out[f"{k}_minus_off_ms"] = out[f"{k}_learn_ms_median"] - off
            out[f"{k}_over_off"] = out[f"{k}_learn_ms_median"] / off
    out["same_rows_off_every1_every4"] = rows["off"] == rows["every1"] == rows["every4"]
    out["stop_third_over_off_per_row"] = out["stop_third_ns_per_row_median"] / out["off_ns_per_row_median"]
    out["one_check_ms"] = out["every1_minus_off_ms"] / (c["updates"] - 1)
    for k in ("every1", "stop_third"):
        st = arms[k][1].last_stats
        out[f"{k}_stats"] = {n: st.get(n) for n in ("n_updates", "kl_stopped", "approx_kl")} | {"checks": len(st.get("kl_checks", []))}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="both", choices=["c3", "c2", "both"])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    for shape in (("c3", "c2") if a.shape == "both" else (a.shape,)):
        print(json.dumps(measure(shape, a.reps, a.warmup)), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
