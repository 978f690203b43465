"""One rank of the KL-adaptive learning-rate rank-count test (tests/test_kl_control_gpu.py), in the style of grad_clip_dist_worker.py.

Started as a fresh child process: `python kl_control_dist_worker.py RANK WORLD PORT OUT.pt`.  World > 1: gloo process group, all
ranks share cuda:0, each owns a contiguous range of whole groups.  Every case runs rollout -> Rollout_Buffer.sample -> learn() with
`desired_kl` set and records last_stats' approx_kl / clip_fraction / log_ratio_mean / lr after every learn(), as numbers and as
float64 bit patterns."""
import os
import struct
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

LR0 = 3e-4
KEYS = ("approx_kl", "clip_fraction", "log_ratio_mean", "lr")
# name -> (algorithm, env, horizon, obs, act, hidden, groups G, episodes E, updates, desired_kl, learn() calls).
# grpo_stale_old: the policy is moved after the learner took its copy and NO update runs (updates_per_iter = 0): the measurement
# compares the policy with the stale old policy on rows that are the same bits at every world size.  desired_kl = 10 (1e-12): every
# kl lies far below (above) the band, so the decisions cannot depend on rounding.
CASES = {
    "grpo_stale_old": ("grpo", "CartPole", 32, 5, 1, (128, 128), 4, 16, 0, 1e-12, 1),
    "ppo_f32_full": ("ppo", "QuadPole", 8, 20, 4, (64, 64), 4, 8, 2, 10.0, 2),
}


def run_cases(rank, world):
    import trajopt_grpo_amd as tg
    dev = torch.device("cuda", 0)
    out = {}
    for name, (algo_name, env_name, T, S, A, hidden, G, E, updates, desired_kl, learns) in CASES.items():
        torch.manual_seed(1234)                                   # identical initial weights on every rank
        cls = tg.GaussianActorCritic_NeuralNetwork if algo_name == "ppo" else tg.GaussianActor_NeuralNetwork
        pol = cls(S, A, hidden, cov=0.3, device=dev)
        env_cls = getattr(tg, env_name)
        mgr = tg.RolloutManager(lambda: env_cls(max_steps=T), pol, num_workers=G, num_episodes_per_worker=E, seed=7)
        buf = tg.Rollout_Buffer(mgr)
        buf.sample()
        opt = torch.optim.Adam(pol.parameters(), lr=LR0)
        if algo_name == "ppo":
            algo = tg.PPO(epsilon=0.2, policy=pol, optimizer=opt, ref_model=None, updates_per_iter=updates, gamma=0.99, batch_size=None,
                          desired_kl=desired_kl)
        else:
            algo = tg.GRPO(epsilon=0.15, beta=0.5, gamma=0.5, policy=pol, optimizer=opt, updates_per_iter=updates, desired_kl=desired_kl)
            with torch.no_grad():                                 # (the same draw on every rank: the generator was seeded above)
                for p in pol.parameters():
                    p.add_(0.02 * torch.randn_like(p))
        stats = []
        for _ in range(learns):
            algo.learn(buf)
            st = algo.last_stats
            stats.append({k: float(st[k]) for k in KEYS})
        torch.cuda.synchronize()
        n_valid = torch.tensor([float(buf.device_traj.mask.sum())], dtype=torch.float64)
        if world > 1:
            import torch.distributed as dist
            dist.all_reduce(n_valid)
        out[name] = {"stats": stats, "lr0": LR0, "n_valid": float(n_valid[0]), "same_rows": updates == 0,
                     "bits": [struct.unpack("<Q", struct.pack("<d", s[k]))[0] for s in stats for k in KEYS]}
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
