#!/usr/bin/env python3
"""Times DeviceActor.evaluate() + backward() against the torch composition it replaces (actor(obs), critic(obs), a Normal log-prob and
.backward()) on the same rows, from Python, and the native path's three stages on their own.  Medians of 7 with the spread.

    python tools/policy_grad_probe.py --out profiles/policy_grad_probe.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import trajopt_grpo_amd as tg  # noqa: E402
from trajopt_grpo_amd import _native as N  # noqa: E402

# (rows, S, H, hidden layers, A, activation), each with a critic of the same trunk
SHAPES = [(4096, 5, 64, 2, 1, "Tanh"), (65536, 20, 256, 2, 4, "ReLU")]
HALF_LOG_2PI = 0.9189385332046727


def net(S, H, nh, O, act):
    mods, w = [], S
    for _ in range(nh):
        mods += [nn.Linear(w, H), getattr(nn, act)()]
        w = H
    return nn.Sequential(*mods, nn.Linear(H, O))


def timed(fn, reps=7, warmup=3):
    """-> (median ms, min ms, max ms) of `reps` single calls between two events."""
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        e0, e1 = N.event_pair()
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


def probe(shape, dev):
    m, S, H, nh, A, act = shape
    torch.manual_seed(0)
    actor, critic = net(S, H, nh, A, act).to(dev), net(S, H, nh, 1, act).to(dev)
    log_std = nn.Parameter(torch.full((A,), -0.5, device=dev))
    params = [*actor.parameters(), *critic.parameters(), log_std]
    obs, action, c, d = torch.randn(m, S, device=dev), torch.randn(m, A, device=dev), torch.randn(m, device=dev), torch.randn(m, device=dev)
    da = tg.DeviceActor(actor, critic, num_envs=1, log_std=log_std, device=dev)

    def loss(logp, ent, value):
        return (c * logp).mean() + 0.01 * ent.mean() + (d * value).mean()

    def native():
        for p in params:
            p.grad = None
        loss(*da.evaluate(obs, action)).backward()

    def torch_arm():
        for p in params:
            p.grad = None
        mu = actor(obs)
        ls = log_std.expand_as(mu)
        logp = (-0.5 * ((action - mu) / ls.exp()).pow(2) - ls - HALF_LOG_2PI).sum(-1)
        loss(logp, (ls + 0.5 + HALF_LOG_2PI).sum(-1), critic(obs).squeeze(-1)).backward()

    # the three stages on their own, on one workspace (what _Evaluate launches)
    ws = da._eval_workspace(m)
    out = [torch.empty(m, device=dev) for _ in range(3)]
    g = [torch.randn(m, device=dev) for _ in range(3)]
    flat = [torch.empty(k, device=dev) for k in ws.grad_floats]
    s = da._eval_args(ws, obs, action, log_std.detach(), *out)
    s.d_g_logp, s.d_g_entropy, s.d_g_value = (t.data_ptr() for t in g)
    s.d_grad_actor, s.d_grad_critic = (t.data_ptr() for t in flat)
    a_tab, c_tab, _keep = da._eval_tables()
    stage = {name: (lambda fn=getattr(da.lib, "tg_policy_eval_" + name): N.check(fn(a_tab, c_tab, C.byref(s), N.stream_ptr(dev)), name))
             for name in ("forward", "backward", "weight_grad")}
    res = {"shape": dict(rows=m, S=S, H=H, hidden_layers=nh, A=A, activation=act)}
    for name, fn in (("native_evaluate_backward", native), ("torch_forward_backward", torch_arm), *stage.items()):
        med, lo, hi = timed(fn)
        res[name] = {"median_ms": round(med, 4), "min_ms": round(lo, 4), "max_ms": round(hi, 4)}
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("policy_grad_probe.py needs an MI355X")
    dev = torch.device("cuda", 0)
    results = [probe(shape, dev) for shape in SHAPES]
    for r in results:
        print(json.dumps(r))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
