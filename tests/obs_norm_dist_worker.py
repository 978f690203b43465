"""One rank of the observation-normalisation rank-count test (tests/test_obs_norm_gpu.py), in the style of learned_std_dist_worker.py.

Started as a fresh child process: `python obs_norm_dist_worker.py RANK WORLD PORT OUT.pt`.  World > 1: gloo process group, all ranks
share cuda:0, each owns a contiguous range of whole groups.  Every case runs rollout -> Rollout_Buffer.sample -> one learn() of a
normalize_obs=True policy (its statistics take the rollout in at the entry: one all-reduce of the ranks' moments) -> a second
rollout -- after, first, a rollout -> obs_norm.update() -> rollout without any optimizer step -- and records this rank's valid observation rows, the statistics and the table, the post-step weights and both rollouts'
actions."""
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

# name -> (algorithm, env, horizon, obs, act, hidden, groups G, episodes E, compute dtype)
CASES = {
    "ppo_f32": ("ppo", "QuadPole", 40, 20, 4, (64, 64), 6, 24, None),
    "grpo_bf16": ("grpo", "QuadPole2D", 40, 10, 2, (128, 128), 6, 24, torch.bfloat16),
}


def run_cases(rank, world):
    import trajopt_grpo_amd as tg
    dev = torch.device("cuda", 0)
    out = {}
    for name, (algo_name, env_name, T, S, A, hidden, G, E, cdt) in CASES.items():
        torch.manual_seed(1234)                                   # identical initial weights on every rank
        cls = tg.GaussianActorCritic_NeuralNetwork if algo_name == "ppo" else tg.GaussianActor_NeuralNetwork
        pol = cls(S, A, hidden, cov=0.3, device=dev, normalize_obs=True)
        env_cls = getattr(tg, env_name)
        mgr = tg.RolloutManager(lambda: env_cls(max_steps=T), pol, num_workers=G, num_episodes_per_worker=E, seed=7, compute_dtype=cdt)
        buf = tg.Rollout_Buffer(mgr)
        # update() alone, then a rollout with the merged table and the initial weights (identical on every rank count)
        buf.sample()
        pol.obs_norm.update(mgr.engine.traj, None)
        upd_table = pol.obs_norm.table.cpu().clone()
        buf.sample()
        upd_actions = buf.group_actions.detach().cpu().clone()
        pol.obs_norm.set(torch.zeros(S), torch.ones(S), 0)        # back to identity statistics for the learn() case
        mgr.shutdown()
        mgr = tg.RolloutManager(lambda: env_cls(max_steps=T), pol, num_workers=G, num_episodes_per_worker=E, seed=7, compute_dtype=cdt)
        buf = tg.Rollout_Buffer(mgr)
        buf.sample()
        tr = mgr.engine.traj
        rows = tr.obs[:, :T, :][:, tr.mask.bool()].t().double().cpu().clone()         # this rank's valid rows, time-major
        actions0 = buf.group_actions.detach().cpu().clone()
        opt = torch.optim.Adam(pol.parameters(), lr=3e-4)
        if algo_name == "ppo":
            algo = tg.PPO(epsilon=0.2, policy=pol, optimizer=opt, ref_model=None, updates_per_iter=1, gamma=0.99, batch_size=None,
                          autocast_dtype=cdt)
        else:
            algo = tg.GRPO(epsilon=0.2, beta=0.0, gamma=0.99, policy=pol, optimizer=opt, updates_per_iter=1, autocast_dtype=cdt)
        algo.learn(buf)
        torch.cuda.synchronize()
        on = pol.obs_norm
        rec = {"rows": rows, "actions0": actions0, "weights": [p.detach().cpu().clone() for p in pol.parameters()],
               "count": on.count.cpu().clone(), "mean": on.mean.cpu().clone(), "m2": on.m2.cpu().clone(), "table": on.table.cpu().clone(),
               "eps": on.eps, "obs_count": algo.last_stats["obs_count"], "upd_table": upd_table, "upd_actions": upd_actions}
        on.freeze()
        buf.sample()
        rec["actions1"] = buf.group_actions.detach().cpu().clone()
        out[name] = rec
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
