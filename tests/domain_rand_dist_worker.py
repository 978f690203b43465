"""One rank of the domain-randomisation sharding test (tests/test_domain_rand_gpu.py), in the style of bootstrap_dist_worker.py.

Started as a fresh child process: `python domain_rand_dist_worker.py RANK WORLD PORT OUT.pt`.  World > 1: gloo process group, all
ranks share cuda:0, each owns a contiguous range of whole groups.  Every case runs two randomised rollouts and records the rank's
group range, its parameter tables and its trajectories."""
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

# name -> (env, kwargs, ranges, horizon, obs, act, hidden, groups G, episodes E, restart)
CASES = {
    "quadpole_f32_fused": ("QuadPole", {}, {"mass": (0.7, 1.4), "Ixx": (0.5, 2.0), "tether_length": (0.5, 2.0)}, 24, 20, 4, (64, 64), 8, 16, False),
    "cartpole_restart": ("CartPole", {}, {"masspole": (0.5, 2.0), "length": (0.5, 2.0)}, 32, 5, 1, (64, 64), 4, 8, True),
    "swarm": ("QuadPoleSwarm", {"n_agents": 4}, {"load_mass": (0.5, 2.0), "arm_length": (0.8, 1.25)}, 16, 20, 4, (64, 64), 4, 4, False),
}


def run_cases(rank, world):
    import trajopt_grpo_amd as tg
    dev = torch.device("cuda", 0)
    out = {}
    for name, (env_name, kw, ranges, T, S, A, hidden, G, E, restart) in CASES.items():
        torch.manual_seed(99)                                     # identical weights on every rank
        pol = tg.GaussianActor_NeuralNetwork(S, A, hidden, cov=0.3, device=dev)
        env_cls = getattr(tg, env_name)
        mgr = tg.RolloutManager(lambda: env_cls(max_steps=T, **kw).randomize(ranges, seed=5), pol, restart=restart, num_workers=G,
                                num_episodes_per_worker=E, seed=21)
        runs = []
        for _ in range(2):
            tr = mgr.rollout_device()
            torch.cuda.synchronize()
            runs.append({k: getattr(tr, k).cpu().clone() for k in ("obs", "act", "rew", "mask", "len")})
            runs[-1]["env_params"] = mgr.engine.env_params.cpu().clone()
        out[name] = {"groups": (mgr.group_lo, mgr.group_hi), "E": mgr.engine.E, "runs": runs}
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
