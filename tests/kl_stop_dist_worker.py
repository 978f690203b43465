"""One rank of the target_kl rank-count test (tests/test_kl_stop_gpu.py), in the style of kl_control_dist_worker.py.

Started as a fresh child process: `python kl_stop_dist_worker.py RANK WORLD PORT OUT.pt`.  World > 1: gloo process group, all ranks
share cuda:0, each owns a contiguous range of whole groups.  Every case rolls out once, then runs learn() twice from the same weights:
with a target_kl that never fires (the kl behind every update, all-reduced: the same numbers on every rank), and with a target_kl
halfway between two of them.  It records where the second run stopped, its checks as float64 bit patterns, the step counters and
the weights."""
import copy
import os
import struct
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

LR0, UPDATES = 3e-4, 6
# name -> (algorithm, env, horizon, obs, act, hidden, groups G, episodes E)
CASES = {
    "ppo_f32_full": ("ppo", "QuadPole", 8, 20, 4, (64, 64), 4, 8),
    "grpo_f32": ("grpo", "CartPole", 16, 5, 1, (64,), 4, 16),
}


def make(tg, algo_name, pol0, **kw):
    pol = copy.deepcopy(pol0)
    opt = torch.optim.Adam(pol.parameters(), lr=LR0)
    if algo_name == "ppo":
        return tg.PPO(epsilon=0.2, policy=pol, optimizer=opt, ref_model=None, updates_per_iter=UPDATES, gamma=0.99, batch_size=None, **kw)
    return tg.GRPO(epsilon=0.2, beta=0.0, gamma=0.9, policy=pol, optimizer=opt, updates_per_iter=UPDATES, **kw)


def run_cases(rank, world):
    import trajopt_grpo_amd as tg
    dev = torch.device("cuda", 0)
    out = {}
    for name, (algo_name, env_name, T, S, A, hidden, G, E) in CASES.items():
        torch.manual_seed(1234)                                   # identical initial weights on every rank
        cls = tg.GaussianActorCritic_NeuralNetwork if algo_name == "ppo" else tg.GaussianActor_NeuralNetwork
        pol0 = cls(S, A, hidden, cov=0.3, device=dev)
        env_cls = getattr(tg, env_name)
        mgr = tg.RolloutManager(lambda: env_cls(max_steps=T), pol0, num_workers=G, num_episodes_per_worker=E, seed=7)
        buf = tg.Rollout_Buffer(mgr)
        buf.sample()
        probe = make(tg, algo_name, pol0, target_kl=1e30)
        probe.learn(buf)
        kls = probe.last_stats["kl_checks"]
        stop = next(j for j in range(2, len(kls) + 1) if kls[j - 1] > 1.01 * max(kls[:j - 1]))
        target = (max(kls[:stop - 1]) + kls[stop - 1]) / 2.0 / 1.5
        algo = make(tg, algo_name, pol0, target_kl=target)
        algo.learn(buf)
        st = algo.last_stats
        torch.cuda.synchronize()
        steps = sorted({float(algo.optimizer.state[p]["step"]) for g in algo.optimizer.param_groups for p in g["params"]})
        out[name] = {"n_updates": st["n_updates"], "kl_stopped": st["kl_stopped"], "kl_checks": st["kl_checks"], "updates": UPDATES,
                     "probe_kl": kls, "target_kl": target, "steps": steps,
                     "kl_bits": [struct.unpack("<Q", struct.pack("<d", k))[0] for k in st["kl_checks"]],
                     "weights": [p.detach().cpu().clone() for p in algo.policy.parameters()]}
    return out


def main():
    rank, world, port, path = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    if world > 1:
        import torch.distributed as dist
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.save(run_cases(rank, world), path)
    finally:
        if world > 1:
            import torch.distributed as dist
            dist.destroy_process_group()


if __name__ == "__main__":
    main()
