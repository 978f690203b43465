"""One rank of the gradient-clipping rank-count test (tests/test_grad_clip_gpu.py), in the style of dist_product_worker.py.

Started as a fresh child process: `python grad_clip_dist_worker.py RANK WORLD PORT OUT.pt`.  World > 1: gloo process group, all
ranks share cuda:0, each owns a contiguous range of whole groups.  Every case runs rollout -> Rollout_Buffer.sample -> learn() with
`max_grad_norm` set and records the post-step weights and the pre-clip norms (as numbers and as float32 bit patterns)."""
import os
import struct
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

# name -> (algorithm, env, horizon, obs, act, hidden, groups G, episodes E, max_grad_norm): fp32 learners, full batch.  The clip
# values sit far below the norms these shapes produce (GRPO's objective is a sum over rows, PPO's a mean); the test asserts it.
CASES = {
    "grpo_f32": ("grpo", "CartPole", 32, 5, 1, (128, 128), 4, 16, 0.5),
    "ppo_f32_full": ("ppo", "QuadPole", 8, 20, 4, (64, 64), 4, 8, 0.01),
}


def run_cases(rank, world):
    import trajopt_grpo_amd as tg
    dev = torch.device("cuda", 0)
    out = {}
    for name, (algo_name, env_name, T, S, A, hidden, G, E, max_norm) in CASES.items():
        torch.manual_seed(1234)                                   # identical initial weights on every rank
        cls = tg.GaussianActorCritic_NeuralNetwork if algo_name == "ppo" else tg.GaussianActor_NeuralNetwork
        pol = cls(S, A, hidden, cov=0.3, device=dev)
        env_cls = getattr(tg, env_name)
        mgr = tg.RolloutManager(lambda: env_cls(max_steps=T), pol, num_workers=G, num_episodes_per_worker=E, seed=7)
        buf = tg.Rollout_Buffer(mgr)
        buf.sample()
        opt = torch.optim.Adam(pol.parameters(), lr=3e-4)
        if algo_name == "ppo":
            algo = tg.PPO(epsilon=0.2, policy=pol, optimizer=opt, ref_model=None, updates_per_iter=2, gamma=0.99, batch_size=None,
                          max_grad_norm=max_norm)
        else:
            algo = tg.GRPO(epsilon=0.15, beta=0.5, gamma=0.5, policy=pol, optimizer=opt, updates_per_iter=2, max_grad_norm=max_norm)
        algo.learn(buf)
        torch.cuda.synchronize()
        norms = algo.last_stats["grad_norm"]
        out[name] = {"weights": [p.detach().cpu() for p in pol.parameters()], "grad_norm": norms, "max_grad_norm": max_norm,
                     "grad_norm_bits": [struct.unpack("<I", struct.pack("<f", n))[0] for n in norms]}
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
