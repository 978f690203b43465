"""One rank of the learned-log-std rank-count test (tests/test_learned_std_gpu.py), in the style of bootstrap_dist_worker.py.

Started as a fresh child process: `python learned_std_dist_worker.py RANK WORLD PORT OUT.pt`.  World > 1: gloo process group, all ranks
share cuda:0, each owns a contiguous range of whole groups.  Every case runs rollout -> Rollout_Buffer.sample -> one learn() of a
learn_std=True policy and records this rank's recorded actions, the post-step weights, log_std and its gradient."""
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

# name -> (algorithm, env, horizon, obs, act, hidden, groups G, episodes E): fp32 learners, full batch
CASES = {
    "ppo_chain": ("ppo", "CartPole", 32, 5, 1, (128,) * 3, 4, 16),
    "grpo_resident": ("grpo", "CartPole", 32, 5, 1, (128, 128), 4, 16),
    "ppo_quadpole2d": ("ppo", "QuadPole2D", 16, 10, 2, (64, 64), 4, 8),
}
ENTROPY = 0.01


def run_cases(rank, world):
    import trajopt_grpo_amd as tg
    dev = torch.device("cuda", 0)
    out = {}
    for name, (algo_name, env_name, T, S, A, hidden, G, E) in CASES.items():
        torch.manual_seed(1234)                                   # identical initial weights on every rank
        cls = tg.GaussianActorCritic_NeuralNetwork if algo_name == "ppo" else tg.GaussianActor_NeuralNetwork
        pol = cls(S, A, hidden, cov=[0.3, 0.5][:A], device=dev, learn_std=True)
        env_cls = getattr(tg, env_name)
        mgr = tg.RolloutManager(lambda: env_cls(max_steps=T), pol, num_workers=G, num_episodes_per_worker=E, seed=7)
        buf = tg.Rollout_Buffer(mgr)
        buf.sample()
        opt = torch.optim.Adam(pol.parameters(), lr=3e-4)
        if algo_name == "ppo":
            algo = tg.PPO(epsilon=0.2, policy=pol, optimizer=opt, ref_model=None, updates_per_iter=1, gamma=0.99, batch_size=None,
                          entropy=ENTROPY)
        else:
            algo = tg.GRPO(epsilon=0.2, beta=0.0, gamma=0.99, policy=pol, optimizer=opt, updates_per_iter=1)
        log_std0 = pol.log_std.detach().cpu().clone()
        algo.learn(buf)
        torch.cuda.synchronize()
        out[name] = {"actions": buf.group_actions.detach().cpu().clone(), "weights": [p.detach().cpu() for p in pol.parameters()],
                     "log_std0": log_std0, "log_std": pol.log_std.detach().cpu().clone(), "grad": pol.log_std.grad.detach().cpu().clone(),
                     "stats_log_std": algo.last_stats["log_std"]}
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
