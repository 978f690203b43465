#!/usr/bin/env python3
"""Step time of PPO with a privileged critic (privileged_critic={...}) against the plain learner on the same randomised env, and the
row kernel on its own against a plain copy: same commit, same process, same seeds.

    python3 tools/privileged_probe.py [--shape c3|c2|both|none] [--reps 7] [--warmup 2] [--no-kernel]

c3: 65,536 QuadPole envs x 256 steps, PPO, actor-critic 20-256x5-{4,1} in bf16, 32 full-batch updates (bench.py's headline shape),
    mass and tether_length randomised: the critic reads 22 columns, both nets pad to 32
c2:  4,096 CartPole envs x 500 steps, PPO, actor-critic 5-128-128-{1,1} in fp32, 10 full-batch updates, length and masscart
    randomised: the critic reads 7 columns, both nets pad to 8
The on arm runs one tg_privileged_rows launch per learn() into a workspace of T * n critic rows, and every critic pass reads those
rows; the off arm's critic reads the actor's.  Each repetition is one Rollout_Buffer.sample(), one prologue-only learn() (a second PPO
on the same policy with updates_per_iter=0) and one full learn(), each between HIP events on the launch stream.  The arms alternate
within a repetition so that clock and thermal drift hit both alike; both start from the same actor weights.  One JSON line per shape:
median and spread of each arm (milliseconds, and nanoseconds per env-step: the row count of a step changes as the policy learns), the
on / off ratios, and the off arm's env-steps per second.

The kernel line: tg_privileged_rows at the C3 row count (T * n = 16,777,216 bf16 rows, pads 32 and 32, two parameter columns, a shuffled
index) against `dst.copy_(src)` of the same two buffers, alternating, each between HIP events; achieved bytes/s counts
rows * (src_pad + dst_pad) * elem + 8 * rows for the kernel (the index it reads) and rows * (src_pad + dst_pad) * elem for the copy."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import trajopt_grpo_amd as tg  # noqa: E402

SHAPES = {
    "c3": dict(env="QuadPole", S=20, A=4, hidden=(256,) * 5, cov=0.3, G=256, E=256, T=256, cdt=torch.bfloat16, updates=32, gamma=0.999,
               ranges={"mass": (0.7, 1.4), "tether_length": (0.5, 2.0)}),
    "c2": dict(env="CartPole", S=5, A=1, hidden=(128, 128), cov=0.5, G=64, E=64, T=500, cdt=None, updates=10, gamma=0.99,
               ranges={"length": (0.6, 1.7), "masscart": (0.75, 1.3)}),
}


def make_arm(c, privileged, dev):
    torch.manual_seed(0)
    pol = tg.GaussianActorCritic_NeuralNetwork(c["S"], c["A"], c["hidden"], cov=c["cov"], device=dev,
                                               **({"privileged_critic": c["ranges"]} if privileged else {}))
    env_cls = tg.environments.ENV_CLASSES[c["env"]]
    mgr = tg.RolloutManager(lambda: env_cls(max_steps=c["T"]).randomize(c["ranges"], seed=5), pol, num_workers=c["G"],
                            num_episodes_per_worker=c["E"], seed=1234, compute_dtype=c["cdt"], use_graph=False)
    buf = tg.Rollout_Buffer(mgr)
    opt = torch.optim.Adam(pol.parameters(), lr=3e-4)
    kw = dict(epsilon=0.2, policy=pol, optimizer=opt, ref_model=None, c1=0.5, kl_coeff=0.5, gamma=c["gamma"], lam=0.95, entropy=0.01,
              batch_size=None, autocast_dtype=c["cdt"])
    return buf, tg.PPO(updates_per_iter=c["updates"], **kw), tg.PPO(updates_per_iter=0, **kw)


def measure(shape, reps, warmup):
    c = SHAPES[shape]
    dev = torch.device("cuda", 0)
    arms = {"off": make_arm(c, False, dev), "on": make_arm(c, True, dev)}
    step, learn, prologue, env_steps = ({k: [] for k in arms} for _ in range(4))
    for rep in range(warmup + reps):
        for k, (buf, algo, algo0) in arms.items():
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            ev[0].record()
            buf.sample()
            ev[1].record()
            algo0.learn(buf)
            ev[2].record()
            algo.learn(buf)
            ev[3].record()
            ev[3].synchronize()
            if rep >= warmup:
                step[k].append(ev[0].elapsed_time(ev[1]) + ev[2].elapsed_time(ev[3]))
                learn[k].append(ev[2].elapsed_time(ev[3]))
                prologue[k].append(ev[1].elapsed_time(ev[2]))
                env_steps[k].append(float(buf.device_traj.env_steps()))
    m_a, m_c = (arms["on"][1]._mlp(net) for net in (arms["on"][1].policy.actor, arms["on"][1].policy.critic))
    out = {"shape": shape, "envs": c["G"] * c["E"], "horizon": c["T"], "updates": c["updates"], "reps": reps, "warmup": warmup,
           "privileged_columns": len(c["ranges"]), "actor_in_pad": m_a.in_pad, "critic_in_pad": m_c.in_pad,
           "critic_rows_workspace_bytes": c["T"] * c["G"] * c["E"] * m_c.in_pad * (2 if c["cdt"] == torch.bfloat16 else 4)}
    for k in arms:
        for name, xs in (("step_ms", step[k]), ("learn_ms", learn[k]), ("prologue_ms", prologue[k])):
            out[f"{k}_{name}_median"], out[f"{k}_{name}_min"], out[f"{k}_{name}_max"] = statistics.median(xs), min(xs), max(xs)
        out[f"{k}_env_steps_per_s"] = statistics.median(e / (t * 1e-3) for e, t in zip(env_steps[k], step[k]))
        # the number of valid rows changes from one iteration to the next (and between the arms, whose policies drift apart), so the
        # comparison is on time per env-step
        ns = [t * 1e6 / e for t, e in zip(step[k], env_steps[k])]
        out[f"{k}_ns_per_env_step_median"], out[f"{k}_ns_per_env_step_min"], out[f"{k}_ns_per_env_step_max"] = statistics.median(ns), min(ns), max(ns)
    out["off_spread"] = (out["off_ns_per_env_step_max"] - out["off_ns_per_env_step_min"]) / out["off_ns_per_env_step_median"]
    out["off_prologue_spread"] = (out["off_prologue_ms_max"] - out["off_prologue_ms_min"]) / out["off_prologue_ms_median"]
    out["on_over_off"] = out["on_ns_per_env_step_median"] / out["off_ns_per_env_step_median"]
    out["on_over_off_prologue_ms"] = out["on_prologue_ms_median"] / out["off_prologue_ms_median"]
    return out


def measure_kernel(reps, warmup):
    """tg_privileged_rows at C3's T * n rows against dst.copy_(src) of the same buffers, alternating."""
    c = SHAPES["c3"]
    dev = torch.device("cuda", 0)
    rows, n, pad, S = c["T"] * c["G"] * c["E"], c["G"] * c["E"], 32, c["S"]
    g = torch.Generator(device=dev).manual_seed(0)
    src = torch.randn(rows, pad, device=dev, generator=g, dtype=torch.float32).to(torch.bfloat16)
    dst = torch.empty_like(src)
    idx = torch.randperm(rows, device=dev, generator=g)               # every cell once, in no order: the gathers scatter over the table
    idx_sorted = torch.arange(rows, device=dev)                       # (tg_learn_compact's own order: time-major, env fastest)
    table = torch.rand(12, n, device=dev, generator=g, dtype=torch.float64) + 0.5
    pol = tg.GaussianActorCritic_NeuralNetwork(S, c["A"], (8,), device="cpu", privileged_critic=c["ranges"])
    spec = tg.algorithms.privileged_spec(pol, tg.environments.ENV_CLASSES[c["env"]]())
    elem = src.element_size()
    arms = {"copy": (lambda: dst.copy_(src), rows * 2 * pad * elem),
            "kernel_shuffled_idx": (lambda: tg.hip_ops.privileged_rows(src, S, idx, n, table, spec, dst, 31), rows * 2 * pad * elem + 8 * rows),
            "kernel_sorted_idx": (lambda: tg.hip_ops.privileged_rows(src, S, idx_sorted, n, table, spec, dst, 31), rows * 2 * pad * elem + 8 * rows)}
    ms = {k: [] for k in arms}
    for rep in range(warmup + reps):
        for k, (fn, _) in arms.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if rep >= warmup:
                ms[k].append(a.elapsed_time(b))
    out = {"shape": "kernel_c3_rows", "rows": rows, "src_pad": pad, "dst_pad": pad, "dtype": "bf16", "privileged_columns": spec.count,
           "reps": reps, "warmup": warmup}
    for k, (_, nbytes) in arms.items():
        med = statistics.median(ms[k])
        out[f"{k}_ms_median"], out[f"{k}_ms_min"], out[f"{k}_ms_max"] = med, min(ms[k]), max(ms[k])
        out[f"{k}_bytes"] = nbytes
        out[f"{k}_bytes_per_s"] = nbytes / (med * 1e-3)
    out["copy_spread"] = (out["copy_ms_max"] - out["copy_ms_min"]) / out["copy_ms_median"]
    for k in ("kernel_shuffled_idx", "kernel_sorted_idx"):
        out[f"{k}_over_copy_per_byte"] = (out[f"{k}_ms_median"] / out[f"{k}_bytes"]) / (out["copy_ms_median"] / out["copy_bytes"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="both", choices=["c3", "c2", "both", "none"])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-kernel", action="store_true")
    a = ap.parse_args()
    if not a.no_kernel:
        print(json.dumps(measure_kernel(a.reps, a.warmup)), flush=True)
        torch.cuda.empty_cache()
    for shape in {"both": ("c3", "c2"), "none": ()}.get(a.shape, (a.shape,)):
        print(json.dumps(measure(shape, a.reps, a.warmup)), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
