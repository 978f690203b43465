"""One rank of the value-normalisation rank-count test (tests/test_value_norm_gpu.py), in the style of bootstrap_dist_worker.py.

Started as a fresh child process: `python value_norm_dist_worker.py RANK WORLD PORT OUT.pt`.  World > 1: gloo process group, all ranks
share cuda:0, each owns a contiguous range of whole groups.  Every case runs rollout -> Rollout_Buffer.sample -> one learn() of a
normalize_value=True policy (the ranks' moments of the returns are all-reduced once, as "ppo_moments", and merged into the statistics
on every rank) and records this rank's returns on its [T][n] grid (0 off the mask) with the mask, the statistics and the table,
last_stats' entries and the post-step weights."""
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

# name -> (env, horizon, obs, act, hidden, groups G, episodes E, monte_carlo, bootstrap_truncated): fp32 learners, full batch
CASES = {
    "cartpole_mc": ("CartPole", 32, 5, 1, (128, 128, 128), 4, 40, True, False),
    "quadpole2d_gae_boot": ("QuadPole2D", 32, 10, 2, (128, 128, 128), 4, 40, False, True),
}


def make_env(tg, name, T):
    """Envs whose episodes end raggedly within a 32-step horizon under a fresh policy: CartPole on a 0.05 s step (some carts leave
    the track, some episodes run into the clock), QuadPole2D inside a 0.3 m box (about half the episodes leave it before step 32)."""
    if name == "CartPole":
        return tg.CartPole(max_steps=T, timestep=0.05)
    env = tg.QuadPole2D(max_steps=T)
    env.spatial_bounds = ((-0.3, 0.3), (-0.3, 0.3))
    return env


def run_cases(rank, world):
    import trajopt_grpo_amd as tg
    dev = torch.device("cuda", 0)
    out = {}
    for name, (env_name, T, S, A, hidden, G, E, monte_carlo, boot) in CASES.items():
        torch.manual_seed(1234)                                   # identical initial weights on every rank
        pol = tg.GaussianActorCritic_NeuralNetwork(S, A, hidden, cov=0.5, device=dev, normalize_value=True)
        mgr = tg.RolloutManager(lambda: make_env(tg, env_name, T), pol, num_workers=G, num_episodes_per_worker=E, seed=7)
        buf = tg.Rollout_Buffer(mgr)
        buf.sample()
        algo = tg.PPO(epsilon=0.2, policy=pol, optimizer=torch.optim.Adam(pol.parameters(), lr=3e-4), ref_model=None, updates_per_iter=1,
                      gamma=0.99, batch_size=None, monte_carlo=monte_carlo, bootstrap_truncated=boot)
        algo.learn(buf)
        torch.cuda.synchronize()
        traj = buf.device_traj
        ret = algo._ws._buf["ret_full"][:traj.T * traj.n].view(traj.T, traj.n)
        vn = pol.value_norm
        stats = algo.last_stats
        out[name] = {"returns": torch.where(traj.mask.bool(), ret, torch.zeros_like(ret)).cpu().clone(), "mask": traj.mask.bool().cpu().clone(),
                     "count": vn.count.cpu().clone(), "mean": vn.mean.cpu().clone(),
                     "m2": vn.m2.cpu().clone(), "table": vn.table.cpu().clone(), "eps": vn.eps, "norm8": algo.norm8.cpu().clone(),
                     "stats": {k: stats[k] for k in ("value_mean", "value_std", "value_count", "explained_variance", "n_valid")},
                     "weights": [p.detach().cpu().clone() for p in pol.parameters()]}
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
