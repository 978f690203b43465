"""One rank of the PopArt rank-count test (tests/test_popart_gpu.py), in the style of value_norm_dist_worker.py.

Started as a fresh child process: `python popart_dist_worker.py RANK WORLD PORT OUT.pt`.  World > 1: gloo process group, all ranks share
cuda:0, each owns a contiguous range of whole groups.  Two rollout -> sample -> learn() rounds of a normalize_value=True, popart=True
policy: the first fills the statistics, the second moves them and rescales the critic head -- from the all-reduced moments, the same
launch on the same numbers on every rank, no collective of its own.  Records, per learn(), this rank's returns on its [T][n] grid (0
off the mask) with the mask and last_stats' entries, and at the end the critic head, the statistics and every weight."""
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from value_norm_dist_worker import make_env                      # noqa: E402  (the same ragged 32-step envs)

ENV, T, S, A, HIDDEN, G, E = "CartPole", 32, 5, 1, (128, 128, 128), 4, 40


def run(rank, world):
    import trajopt_grpo_amd as tg
    dev = torch.device("cuda", 0)
    torch.manual_seed(1234)                                       # identical initial weights on every rank
    pol = tg.GaussianActorCritic_NeuralNetwork(S, A, HIDDEN, cov=0.5, device=dev, normalize_value=True, popart=True)
    mgr = tg.RolloutManager(lambda: make_env(tg, ENV, T), pol, num_workers=G, num_episodes_per_worker=E, seed=7)
    buf = tg.Rollout_Buffer(mgr)
    algo = tg.PPO(epsilon=0.2, policy=pol, optimizer=torch.optim.Adam(pol.parameters(), lr=3e-4), ref_model=None, updates_per_iter=2,
                  gamma=0.99, batch_size=None, monte_carlo=True)
    out = {"learns": []}
    for _ in range(2):
        buf.sample()
        algo.learn(buf)
        torch.cuda.synchronize()
        traj = buf.device_traj
        ret = algo._ws._buf["ret_full"][:traj.T * traj.n].view(traj.T, traj.n)
        stats = algo.last_stats
        out["learns"].append({"returns": torch.where(traj.mask.bool(), ret, torch.zeros_like(ret)).cpu().clone(),
                              "mask": traj.mask.bool().cpu().clone(),
                              "stats": {k: stats[k] for k in ("value_mean", "value_std", "value_count", "popart_scale", "popart_shift",
                                                              "n_valid")}})
    vn, head = pol.value_norm, pol.critic.network[-1]
    out.update(count=vn.count.cpu().clone(), mean=vn.mean.cpu().clone(), m2=vn.m2.cpu().clone(), table=vn.table.cpu().clone(), eps=vn.eps,
               head_w=head.weight.detach().cpu().clone(), head_b=head.bias.detach().cpu().clone(),
               weights=[p.detach().cpu().clone() for p in pol.parameters()])
    return out


def main():
    rank, world, port, path = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    if world > 1:
        import torch.distributed as dist
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.save(run(rank, world), path)
    finally:
        if world > 1:
            import torch.distributed as dist
            dist.destroy_process_group()


if __name__ == "__main__":
    main()
