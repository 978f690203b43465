"""One rank of the step-baseline rank-count test (tests/test_grpo_baseline_gpu.py), in the style of grad_clip_dist_worker.py.

Started as a fresh child process: `python grpo_baseline_dist_worker.py RANK WORLD PORT OUT.pt`.  World > 1: gloo process group, all
ranks share cuda:0, each owns a contiguous range of whole groups.  Every case runs rollout -> Rollout_Buffer.sample -> learn() with
baseline="step" and records the [T][n_local] advantage array the row compaction read, the mask, last_stats and the post-step weights."""
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

# name -> (env, horizon, obs, act, hidden, groups G, episodes E, restart, adv_scale): fp32 learners
CASES = {
    "cartpole_std": ("CartPole", 32, 5, 1, (128, 128), 8, 16, False, "std"),
    "quadpole_restart_none": ("QuadPole", 16, 20, 4, (64, 64), 4, 8, True, "none"),
}


def run_cases(rank, world):
    import trajopt_grpo_amd as tg
    dev = torch.device("cuda", 0)
    out = {}
    for name, (env_name, T, S, A, hidden, G, E, restart, adv_scale) in CASES.items():
        torch.manual_seed(1234)                                   # identical initial weights on every rank
        pol = tg.GaussianActor_NeuralNetwork(S, A, hidden, cov=0.3, device=dev)
        env_cls = getattr(tg, env_name)
        mgr = tg.RolloutManager(lambda: env_cls(max_steps=T), pol, num_workers=G, num_episodes_per_worker=E, seed=7, restart=restart)
        buf = tg.Rollout_Buffer(mgr)
        buf.sample()
        algo = tg.GRPO(epsilon=0.15, beta=0.5, gamma=0.9, policy=pol, optimizer=torch.optim.Adam(pol.parameters(), lr=3e-4),
                       updates_per_iter=2, baseline="step", adv_scale=adv_scale)
        seen = {}
        inner = algo._advantage_source

        def recording(traj, rtg, moments, inner=inner, seen=seen):
            src0, mom, mode = inner(traj, rtg, moments)
            seen["adv"], seen["mask"], seen["E"] = src0.detach().cpu().clone(), traj.mask.cpu().clone(), traj.E
            return src0, mom, mode
        algo._advantage_source = recording
        algo.learn(buf)
        torch.cuda.synchronize()
        st = algo.last_stats
        out[name] = {"weights": [p.detach().cpu() for p in pol.parameters()], "adv": seen["adv"], "mask": seen["mask"], "E": seen["E"],
                     "J": st["J"], "baseline": st["baseline"], "baseline_explained": st["baseline_explained"]}
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
