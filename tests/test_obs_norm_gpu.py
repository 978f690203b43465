"""Running observation normalisation on the MI355X (policies: normalize_obs=True; tg_obs_moments, tg_obs_norm_merge,
tg_obs_normalize_rows, tg_learn_compact_on, tg_fused_rollout_on, tg_fused_rollout_f32_on):

  1. identity is unchanged: count = 0 (mean 0, rstd 1), no clamp, frozen gives the plain rollout bit for bit on every rollout
     path ((x - 0) * 1 is exact: tolerance zero), with and without domain randomisation on one env;
  2. moments and merge: three ragged trajectories (f32 and f64) merged on the device against tests/obs_norm_fp64.py -- count exact,
     mean and m2 within the reordering bound derived there, the f32 table within 1 ulp of the table of the device's own statistics;
  3. learner rows: tg_learn_compact_on and tg_obs_normalize_rows (SoA slot and row-major) against the torch expression, bit for
     bit in f32 and after the bf16 rounding, zero padding, ones column present and marked, the clamp binding on some entries only;
  4. the actor inside the fused kernels: the recorded action against mean_ref(xn) + sigma eps within the rigorous bounds of
     test_fused_rollout_fp64.py / test_tanh_gpu.py, xn the exact fp32 expression of the recorded raw observation;
  5. the learner is otherwise unchanged: a frozen normalised policy on raw observations and a plain policy on a hand-built
     trajectory holding xn end with bit-identical weights (GRPO, PPO, bf16 chain, f32 chain, PPO minibatch mode);
  6. learn() updates, then uses: statistics after one learn() equal the restatement's merge of that rollout's valid rows; frozen
     they keep their bits; a captured per-step graph replays with the rewritten table, no recapture;
  7. two ranks against one: statistics within the bound of 2, the table within 1 ulp, post-step weights at the bar of
     test_distributed_gpu.py's harness, and -- where the tables are equal -- the next rollout bit for bit;
  plus PPO's bootstrap rows (the s_final input rows under this learn()'s table) and GRPO's reference policy reading raw rows through
  its own, frozen statistics."""
import os
import socket
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import obs_norm_fp64 as Y
import test_fused_rollout_fp64 as F
from test_tanh_gpu import f32_tanh_mean_and_bound

pytestmark = pytest.mark.gpu

DIMS = F.DIMS
T0, G0, E0 = 40, 6, 24            # n = 144: a partial wave, a partial 128/256-env workgroup, T > 8 (the bf16 kernel compacts)


@pytest.fixture(scope="module")
def tg():
    import trajopt_grpo_amd as tg
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return tg


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def make_env(tg, name, T, ranges=None, **kw):
    env = tg.environments.ENV_CLASSES[name](max_steps=T, **kw)
    if ranges is not None:
        env.randomize(ranges, seed=3)
    return env


def snapshot(tr):
    torch.cuda.synchronize()
    return {k: getattr(tr, k).clone() for k in ("obs", "act", "rew", "mask", "len")}


def same(a, b):
    return all(torch.equal(a[k], b[k]) for k in ("obs", "act", "rew", "mask", "len"))


def twin(tg, pol, **kw):
    """A policy of pol's class, shape and weights with normalize_obs=True (+ kw)."""
    hidden = pol.hidden_dims
    new = type(pol)(pol.input_dim, pol.output_dim, hidden, activation=pol.activation, cov=pol.var.tolist(), device=pol.device,
                    normalize_obs=True, **kw)
    new.actor.load_state_dict(pol.actor.state_dict())
    if pol.critic is not None:
        new.critic.load_state_dict(pol.critic.state_dict())
    return new


def distinct_stats(S, seed=0):
    """Per-feature statistics that are all different (an index slip shows) and in the range of the envs' states."""
    rng = np.random.default_rng(seed)
    return rng.uniform(-0.5, 0.5, size=S) * (1.0 + np.arange(S)), rng.uniform(0.05, 2.0, size=S) * (1.0 + 0.5 * np.arange(S)), 1000.0


def xn_torch(x, on):
    """The definition, in torch on the device: x (any float dtype) [..., S] -> float32."""
    xn = (x.to(torch.float32) - on.table[0]) * on.table[1]
    return xn if on.clip is None else torch.clamp(xn, -float(on.clip), float(on.clip))


# --------------------------------------------------------------------------------------------------------------------------------
# 1. identity is unchanged
# --------------------------------------------------------------------------------------------------------------------------------
PATHS = ["per_step_f64", "per_step_f32", "forced", "fused_bf16", "f32_relu_16", "f32_relu_32", "f32_tanh_16", "f32_tanh_32"]
CASES = [(n, False) for n in ("CartPole", "Pendulum", "QuadPole2D", "QuadPole", "QuadPoleSwarm")] + [("QuadPole", True)]


@pytest.mark.parametrize("name,randomized", CASES, ids=[n + ("-dr" if r else "") for n, r in CASES])
@pytest.mark.parametrize("path", PATHS)
def test_identity_statistics_give_the_plain_rollout_bit_for_bit(tg, dev, name, randomized, path):
    from oracle import envs as E
    base = "QuadPole" if name == "QuadPoleSwarm" else name
    S, A = DIMS[base]
    kw = {"n_agents": 4} if name == "QuadPoleSwarm" else {}
    torch.manual_seed(5)
    hidden = (128, 128) if path == "fused_bf16" else (64, 64)
    act = "Tanh" if "tanh" in path else "ReLU"
    pol = tg.GaussianActor_NeuralNetwork(S, A, hidden, activation=act, cov=0.3, device=dev)
    pol_on = twin(tg, pol, obs_clip=None)
    pol_on.obs_norm.freeze()
    assert float(pol_on.obs_norm.count) == 0.0
    ekw = dict(seed=13)
    if path == "fused_bf16":
        ekw.update(compute_dtype=torch.bfloat16)
    elif path == "per_step_f64":
        ekw.update(dtype=torch.float64)
    elif path in ("per_step_f32", "forced"):
        ekw.update(fused=False)
    ranges = {k: (0.7, 1.4) for k in tg.environments.ENV_CLASSES[name].RANDOMIZABLE} if randomized else None
    results = []
    for p in (pol, pol_on):
        eng = tg.DeviceRollout(make_env(tg, name, T0, ranges, **kw), p, G0, E0, **ekw)
        if path.startswith("f32_"):
            eng.f32_block_envs = int(path[-2:])
        assert eng.fused == (path == "fused_bf16" or path.startswith("f32_"))
        if path == "forced":
            rng = np.random.default_rng(3)
            tr = eng.run(initial_states=E.sample_initial_states(base, eng.n, rng),
                         forced_actions=rng.normal(size=(eng.n, T0, A)).astype(np.float32) * 0.6)
        else:
            tr = eng.run()
        results.append(snapshot(tr))
        assert (eng.env_params is not None) == randomized
    assert int(results[0]["len"].min()) >= 1 and float(results[0]["obs"].abs().sum()) > 0
    assert same(results[0], results[1])


# --------------------------------------------------------------------------------------------------------------------------------
# 2. moments and merge
# --------------------------------------------------------------------------------------------------------------------------------
def ragged_trajectory(tg, dev, S, A, T, G, Eps, dtype, seed):
    n = G * Eps
    tr = tg.rollout.DeviceTrajectory(S, A, T, n, G, Eps, dtype, dev)
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, T + 1, size=n)
    lens[0], lens[1] = 1, T
    assert lens.min() == 1 and lens.max() == T and len(set(lens.tolist())) > T // 2      # lengths span 1..T
    scale, shift = np.logspace(-2, 2, S), rng.normal(size=S) * np.logspace(1, -1, S) + 0.05 * seed
    obs = shift[:, None, None] + rng.normal(size=(S, T + 1, n)) * scale[:, None, None]
    mask = (np.arange(T)[:, None] < lens[None, :])
    obs[:, :T, :] *= mask[None]                                                          # zero beyond each episode, as a rollout leaves it
    tr.obs.copy_(torch.from_numpy(obs).to(dtype))
    tr.mask.copy_(torch.from_numpy(mask.astype(np.uint8)))
    tr.len.copy_(torch.from_numpy(lens.astype(np.int32)))
    return tr


def valid_rows(tr):
    """f64 [N][S]: the valid (t, e) observations in time-major order, as stored (an f32 observation is exact in f64)."""
    m = tr.mask.bool().cpu().numpy()
    obs = tr.obs[:, :tr.T, :].double().cpu().numpy()
    return np.ascontiguousarray(obs[:, m].T)


def check_statistics(on, batches, means_before):
    """count exact; mean and m2 against the exact statistics of the concatenated rows within Y.merge_bounds; the table within 1 ulp
    of the table of the device's own f64 statistics."""
    torch.cuda.synchronize()
    allx = np.concatenate(batches).astype(np.longdouble)
    mean_ref = allx.mean(0)
    m2_ref = ((allx - mean_ref) ** 2).sum(0)
    e_mean, e_m2 = Y.merge_bounds(batches, means_before)
    count, mean, m2 = float(on.count), on.mean.cpu().numpy(), on.m2.cpu().numpy()
    err_mean, err_m2 = np.abs(mean - mean_ref.astype(np.float64)), np.abs(m2 - m2_ref.astype(np.float64))
    print("obs_norm statistics: max err mean / bound", float((err_mean / (e_mean + Y.U * np.abs(mean))).max()),
          "max err m2 / bound", float((err_m2 / (e_m2 + Y.U * np.abs(m2))).max()))
    assert count == float(allx.shape[0])
    assert np.all(err_mean <= e_mean + Y.U * np.abs(mean)), (err_mean, e_mean)
    assert np.all(err_m2 <= e_m2 + Y.U * np.abs(m2)), (err_m2, e_m2)
    tab, want = on.table.cpu().numpy(), Y.table(count, mean, m2, on.eps)
    assert np.all(np.abs(tab.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_three_merged_rollouts_match_the_fp64_restatement(tg, dev, dtype):
    S, A, T, G, Eps = 20, 4, 37, 6, 25                                                   # n = 150
    pol = tg.GaussianActor_NeuralNetwork(S, A, (64, 64), device=dev, normalize_obs=True)
    on = pol.obs_norm
    tab_ptr = on.table.data_ptr()
    batches, means_before = [], []
    for i in range(3):
        tr = ragged_trajectory(tg, dev, S, A, T, G, Eps, dtype, seed=10 + i)
        means_before.append(on.mean.cpu().numpy().copy())
        on.update(tr)
        batches.append(valid_rows(tr))
    assert on.table.data_ptr() == tab_ptr
    check_statistics(on, batches, means_before)
    # deterministic: the same three trajectories again give the same bits
    pol2 = tg.GaussianActor_NeuralNetwork(S, A, (64, 64), device=dev, normalize_obs=True)
    for i in range(3):
        pol2.obs_norm.update(ragged_trajectory(tg, dev, S, A, T, G, Eps, dtype, seed=10 + i))
    for a, b in ((on.count, pol2.obs_norm.count), (on.mean, pol2.obs_norm.mean), (on.m2, pol2.obs_norm.m2), (on.table, pol2.obs_norm.table)):
        assert torch.equal(a, b)
    # set() / count == 0 on the device
    on.set(np.arange(S), np.ones(S), 0)
    torch.cuda.synchronize()
    assert torch.equal(on.table.cpu(), torch.stack([torch.zeros(S), torch.ones(S)]))


# --------------------------------------------------------------------------------------------------------------------------------
# 3. learner rows
# --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("cd", [torch.float32, torch.bfloat16], ids=["rows_f32", "rows_bf16"])
def test_learner_rows_hold_the_normalised_observation_bit_for_bit(tg, dev, dtype, cd):
    K, M = tg.hip_ops, tg.mlp
    S, A, T, G, Eps = 20, 4, 37, 6, 25
    tr = ragged_trajectory(tg, dev, S, A, T, G, Eps, dtype, seed=21)
    tr.act.copy_(torch.randn_like(tr.act))
    pol = tg.GaussianActor_NeuralNetwork(S, A, (64, 64), device=dev, normalize_obs=True, obs_clip=1.25)
    on = pol.obs_norm
    rows = valid_rows(tr)
    on.set(rows.mean(0) + 0.1 * rows.std(0) * np.arange(S) / S, rows.var(0) * (1.0 + 0.1 * np.arange(S)), rows.shape[0])
    idx_ref = tr.mask.reshape(-1).nonzero().squeeze(1)
    x_valid = tr.obs_rows().index_select(0, idx_ref)                                    # [rows][S], raw
    want = xn_torch(x_valid, on)
    bound = (want.abs() == 1.25).float().mean().item()
    assert 0.0 < bound < 1.0 and 0.0 < 1.0 - bound < 1.0                                 # the clamp binds on some entries, not on others
    want_cd = want.to(cd)
    cap, in_pad = T * tr.n, 32
    # tg_learn_compact_on
    work = torch.empty((K.learn_count_workspace(cap) + 3) // 4, dtype=torch.int32, device=dev)
    total = torch.empty(2, dtype=torch.int64, device=dev)
    K.learn_count(tr.mask, -1, work, total)
    xin = torch.full((cap, in_pad), 7.0, dtype=cd, device=dev)
    act_rows, idx = torch.empty(cap, A, device=dev), torch.empty(cap, dtype=torch.int64, device=dev)
    K.learn_compact(tr, work, cap, xin, 31, act_rows, idx, obs_norm=on)
    n_rows = int(total[0])
    assert n_rows == idx_ref.numel() and torch.equal(idx[:n_rows], idx_ref)
    assert torch.equal(xin[:n_rows, :S], want_cd)
    assert bool((xin[:n_rows, S:31] == 0).all()) and bool((xin[:n_rows, 31] == 1).all())
    assert torch.equal(act_rows[:n_rows], tr.act_rows().index_select(0, idx_ref))
    # ... and the plain kernel on the same trajectory still writes the raw observation
    xin_raw = torch.empty(cap, in_pad, dtype=cd, device=dev)
    K.learn_compact(tr, work, cap, xin_raw, 31, act_rows, idx)
    assert torch.equal(xin_raw[:n_rows, :S], x_valid.to(torch.float32).to(cd))
    # tg_obs_normalize_rows: row-major rows (PPO's s_final, the gather fallback), an SoA slot (the per-step path), no ones column
    out = torch.full((n_rows, in_pad), 7.0, dtype=cd, device=dev)
    K.obs_normalize_rows(x_valid.contiguous(), on, out, 31)
    assert torch.equal(out[:, :S], want_cd) and bool((out[:, S:31] == 0).all()) and bool((out[:, 31] == 1).all())
    slot = tr.obs[:, 3, :].t()                                                          # [n][S] view: row stride 1
    out = torch.full((tr.n, in_pad), 7.0, dtype=cd, device=dev)
    K.obs_normalize_rows(slot, on, out)
    assert torch.equal(out[:, :S], xn_torch(slot, on).to(cd)) and bool((out[:, S:] == 0).all())
    # GemmMLP.prepare_input(obs_norm=...): the same rows, and the ones column marked on the storage
    m = M.GemmMLP(pol.actor, cd)
    xp = m.prepare_input(x_valid, obs_norm=on)
    assert xp.shape == (n_rows, m.in_pad) and torch.equal(xp[:, :S], want_cd)
    assert M.has_ones_column(xp) == (m.in_pad == 32 and m._f32 is None)
    if M.has_ones_column(xp):
        assert bool((xp[:, 31] == 1).all())


# --------------------------------------------------------------------------------------------------------------------------------
# 4. the actor inside the fused kernels
# --------------------------------------------------------------------------------------------------------------------------------
FUSED = [("bf16", "ReLU", None, False), ("f32", "ReLU", 16, False), ("f32", "ReLU", 32, True), ("f32", "Tanh", 16, False),
         ("f32", "Tanh", 32, False)]


@pytest.mark.parametrize("kind,act,block_envs,randomized", FUSED, ids=[f"{k}-{a}-{b}{'-dr' if r else ''}" for k, a, b, r in FUSED])
def test_fused_actor_reads_the_normalised_observation(tg, dev, kind, act, block_envs, randomized):
    name = "QuadPole"
    S, A = DIMS[name]
    torch.manual_seed(11)
    hidden = (128, 128) if kind == "bf16" else (64, 64, 64)
    pol = tg.GaussianActor_NeuralNetwork(S, A, hidden, activation=act, cov=0.3, device=dev, normalize_obs=True, obs_clip=1.5)
    on = pol.obs_norm
    on.set(*distinct_stats(S, seed=2))
    on.freeze()
    ranges = {k: (0.7, 1.4) for k in tg.environments.ENV_CLASSES[name].RANDOMIZABLE} if randomized else None
    eng = tg.DeviceRollout(make_env(tg, name, T0, ranges), pol, G0, E0, seed=41,
                           compute_dtype=torch.bfloat16 if kind == "bf16" else None, fused=True)
    if block_envs:
        eng.f32_block_envs = block_envs
    assert eng.fused and eng._fused_f32 == (kind == "f32")
    tr = eng.run()
    torch.cuda.synchronize()
    eps = F.philox_draws(tg, make_env(tg, name, T0), pol, G0, E0, 41, dev)
    layers = F.actor_layers(pol)
    k1 = (S + 7) // 8 * 8
    seen = {}

    def mean_fn(x):                           # x: the recorded raw observation (exact in f64) -> xn, exact input to the bound
        xn = xn_torch(x.float(), on)
        seen["frac"] = float((xn.abs() == 1.5).float().mean())
        xn = xn.double()
        if kind == "bf16":
            return F.bf16_mean_and_bound(layers, xn)
        return (f32_tanh_mean_and_bound if act == "Tanh" else F.f32_mean_and_bound)(layers, xn, k1)

    F.check_actions(tr, eps, F.sigmas(eng), mean_fn, k_alive_min=G0 * E0 * 2)
    assert 0.0 < seen["frac"] < 1.0                                                      # the clamp was active, and not everywhere
    # the trajectory records the RAW observation: a plain policy's teacher-forced replay of these actions reproduces it
    plain = tg.GaussianActor_NeuralNetwork(S, A, hidden, activation=act, cov=0.3, device=dev)
    rep = tg.DeviceRollout(make_env(tg, name, T0, ranges), plain, G0, E0, seed=41, fused=False)
    rep._seed_host, rep._stream_host = 41, 0
    got = rep.run(initial_states=tr.obs[:, 0, :].t().cpu().numpy(), forced_actions=tr.act.permute(2, 1, 0).cpu().numpy())
    torch.cuda.synchronize()
    assert torch.equal(got.obs, tr.obs) and torch.equal(got.len, tr.len) and torch.equal(got.rew, tr.rew)


# --------------------------------------------------------------------------------------------------------------------------------
# 5. the learner is otherwise unchanged
# --------------------------------------------------------------------------------------------------------------------------------
LEARN = [("grpo", None, None), ("grpo", torch.bfloat16, None), ("ppo", None, None), ("ppo", torch.bfloat16, None), ("ppo", None, 512)]


@pytest.mark.parametrize("algo_name,cdt,batch", LEARN, ids=[f"{a}-{'bf16' if c else 'f32'}{'-mb' if b else ''}" for a, c, b in LEARN])
def test_frozen_normalised_learner_equals_a_plain_learner_on_normalised_observations(tg, dev, algo_name, cdt, batch):
    name = "QuadPole"
    S, A = DIMS[name]
    torch.manual_seed(17)
    cls = tg.GaussianActor_NeuralNetwork if algo_name == "grpo" else tg.GaussianActorCritic_NeuralNetwork
    plain = cls(S, A, (128, 128), cov=0.3, device=dev)
    pol = twin(tg, plain, obs_clip=1.5)
    pol.obs_norm.set(*distinct_stats(S, seed=4))
    pol.obs_norm.freeze()
    eng = tg.DeviceRollout(make_env(tg, name, T0), pol, G0, E0, seed=23, compute_dtype=cdt)
    tr = eng.run()
    torch.cuda.synchronize()
    tr2 = tg.rollout.DeviceTrajectory(S, A, T0, tr.n, G0, E0, torch.float32, dev)
    for k in ("act", "rew", "mask", "len", "counters"):
        getattr(tr2, k).copy_(getattr(tr, k))
    tr2.obs.copy_(xn_torch(tr.obs.permute(1, 2, 0), pol.obs_norm).permute(2, 0, 1))
    frac = float((tr2.obs.abs() == 1.5).float().mean())
    assert 0.0 < frac < 1.0

    def learner(p):
        opt = torch.optim.Adam(p.parameters(), lr=3e-4)
        if algo_name == "grpo":
            return tg.GRPO(0.2, 0.0, 0.99, p, opt, updates_per_iter=2, autocast_dtype=cdt)
        return tg.PPO(0.2, p, opt, None, 2, gamma=0.99, batch_size=batch, autocast_dtype=cdt, seed=5)

    a_on = learner(pol)
    before = [p.detach().clone() for p in pol.parameters()]
    stats_before = [t.clone() for t in (pol.obs_norm.count, pol.obs_norm.mean, pol.obs_norm.m2, pol.obs_norm.table)]
    a_on.learn(types.SimpleNamespace(device_traj=tr))
    # (built only now: GRPO folds the old-policy pass into the first update while "nothing has written a parameter since old_policy <-
    #  policy", which it tells from a process-wide count of raw parameter writes -- a learner built before another learner's Adam
    #  step would run the separate no-grad pass instead: the same numbers from another kernel, not the same launches)
    a_plain = learner(plain)
    a_plain.learn(types.SimpleNamespace(device_traj=tr2))
    torch.cuda.synchronize()
    assert sum(float((p.detach() - b).abs().sum()) for p, b in zip(pol.parameters(), before)) > 0
    for p, q in zip(pol.parameters(), plain.parameters()):
        assert torch.equal(p, q)
    for a, b in zip(stats_before, (pol.obs_norm.count, pol.obs_norm.mean, pol.obs_norm.m2, pol.obs_norm.table)):
        assert torch.equal(a, b)                                                         # frozen: not a bit moved
    assert a_on.last_stats["obs_count"] == 1000.0 and "obs_count" not in a_plain.last_stats
    m = a_on._mlp(pol.actor)
    assert m is not None and (cdt is not None or m._f32 is not None)                    # the native learners ran (fp32: the chain learner)


BOOT = [("f32", None, True), ("bf16", torch.bfloat16, True), ("torch", None, False)]


@pytest.mark.parametrize("label,cdt,fused_mlp", BOOT, ids=[b[0] for b in BOOT])
def test_bootstrap_rows_are_the_normalised_final_states(tg, dev, label, cdt, fused_mlp):
    """PPO(bootstrap_truncated=True) on time-limited episodes with an UNFROZEN normalised policy: the critic's input rows for
    s_final (`boot_xin`) are xn(s_final) under the table this learn() wrote at its entry, bit for bit, padding and ones column
    included; without a GemmMLP (fused_mlp=False) the bootstrap values are the critic on on.normalize(s_final), bit for bit."""
    K, M = tg.hip_ops, tg.mlp
    name, T, G, Eps = "QuadPole2D", 48, 4, 40
    S, A = DIMS[name]
    torch.manual_seed(23)
    pol = tg.GaussianActorCritic_NeuralNetwork(S, A, (128, 128, 128), cov=0.5, device=dev, normalize_obs=True, obs_clip=1.0)
    on = pol.obs_norm
    mgr = tg.RolloutManager(lambda: make_env(tg, name, T), pol, num_workers=G, num_episodes_per_worker=Eps, seed=9, compute_dtype=cdt)
    buf = tg.Rollout_Buffer(mgr)
    buf.sample()
    algo = tg.PPO(epsilon=0.2, policy=pol, optimizer=torch.optim.Adam(pol.parameters(), lr=2e-4), ref_model=None, updates_per_iter=1,
                  gamma=0.99, batch_size=None, autocast_dtype=cdt, fused_mlp=fused_mlp, bootstrap_truncated=True)
    critic_before = [p.detach().clone() for p in pol.critic.parameters()]
    algo.learn(buf)
    torch.cuda.synchronize()
    traj = buf.device_traj
    assert float(on.count) == float(traj.mask.sum()) > 0                                 # the table is this learn()'s own
    s_final, timeout = K.rollout_final_state(mgr.engine.params, traj)
    n = traj.n
    assert 0 < int(timeout.sum()) and algo.last_stats["n_bootstrapped"] == int(timeout.sum())   # some episodes timed out
    assert torch.equal(algo._small_bufs["boot_state"].view(n, S), s_final)
    want = xn_torch(s_final, on)
    frac = float((want.abs() == 1.0).float().mean())
    assert 0.0 < frac < 1.0
    m_c = algo._mlp(pol.critic)
    if fused_mlp:
        assert m_c is not None
        xin = algo._small_bufs["boot_xin"].view(n, m_c.in_pad)
        ones = m_c.in_pad == 32 and m_c._f32 is None
        assert xin.dtype == m_c.cd and torch.equal(xin[:, :S], want.to(m_c.cd))
        assert not torch.equal(xin[:, :S], s_final.to(m_c.cd))                           # (not the raw state)
        if ones:
            assert bool((xin[:, S:31] == 0).all()) and bool((xin[:, 31] == 1).all()) and M.has_ones_column(xin)
        else:
            assert bool((xin[:, S:] == 0).all())
    else:
        assert m_c is None and "boot_xin" not in algo._small_bufs
        critic0 = tg.policies.NeuralNetwork(S, 1, (128, 128, 128), "ReLU").to(dev)
        with torch.no_grad():
            for p, q in zip(critic0.parameters(), critic_before):
                p.copy_(q)
            v = critic0(want).reshape(-1) * timeout
        assert torch.equal(algo._small_bufs["boot_value"], v)


@pytest.mark.parametrize("cdt", [None, torch.bfloat16], ids=["f32", "bf16"])
def test_grpo_reference_policy_reads_states_through_its_own_statistics(tg, dev, cdt):
    """GRPO with beta != 0 and a reference policy whose statistics differ from the policy's: its input rows are the valid rows' RAW
    observations through ITS table (torch expression, bit for bit), its log-probabilities those of the learner's no-grad pass on such
    rows; learn() updates the policy's statistics and leaves the reference policy's alone."""
    import copy
    name = "QuadPole"
    S, A = DIMS[name]
    torch.manual_seed(27)
    pol = tg.GaussianActor_NeuralNetwork(S, A, (128, 128), cov=0.3, device=dev, normalize_obs=True, obs_clip=1.5)
    pol.obs_norm.set(*distinct_stats(S, seed=6))
    ref = copy.deepcopy(pol)                                                             # its own weights object AND its own statistics
    assert ref.obs_norm is not pol.obs_norm
    ref.obs_norm.set(*distinct_stats(S, seed=7))
    ref.obs_norm.freeze()
    with torch.no_grad():
        for p in ref.actor.parameters():
            p.add_(0.01 * torch.randn_like(p))
    mgr = tg.RolloutManager(lambda: make_env(tg, name, T0), pol, num_workers=G0, num_episodes_per_worker=E0, seed=33, compute_dtype=cdt)
    buf = tg.Rollout_Buffer(mgr)
    buf.sample()
    algo = tg.GRPO(0.2, 0.5, 0.99, pol, torch.optim.Adam(pol.parameters(), lr=3e-4), ref_model=ref, updates_per_iter=1, autocast_dtype=cdt)
    with pytest.raises(ValueError, match="shares"):
        shared = copy.deepcopy(pol)
        shared.obs_norm = pol.obs_norm
        tg.GRPO(0.2, 0.5, 0.99, pol, torch.optim.Adam(pol.parameters(), lr=3e-4), ref_model=shared)
    assert algo.old_policy.obs_norm is pol.obs_norm
    ref_stats = [t.clone() for t in (ref.obs_norm.count, ref.obs_norm.mean, ref.obs_norm.m2, ref.obs_norm.table)]
    pol_table = pol.obs_norm.table.clone()
    algo.learn(buf)
    torch.cuda.synchronize()
    traj = buf.device_traj
    for a, b in zip(ref_stats, (ref.obs_norm.count, ref.obs_norm.mean, ref.obs_norm.m2, ref.obs_norm.table)):
        assert torch.equal(a, b)
    assert not torch.equal(pol.obs_norm.table, pol_table) and float(pol.obs_norm.count) == 1000.0 + float(traj.mask.sum())
    idx = traj.mask.reshape(-1).nonzero().squeeze(1)
    rows, cap = idx.numel(), traj.T * traj.n
    x_raw = traj.obs_rows().index_select(0, idx)
    m_ref = algo._mlp(ref.actor)
    assert m_ref is not None
    xin_ref = algo._ws.get("xin_ref", rows, m_ref.in_pad, m_ref.cd, dev, cap)
    want = xn_torch(x_raw, ref.obs_norm)
    assert torch.equal(xin_ref[:, :S], want.to(m_ref.cd))
    assert not torch.equal(want, xn_torch(x_raw, pol.obs_norm))
    act = traj.act_rows().index_select(0, idx)
    m_ref.refresh(force=True)
    lp = algo._logp_nograd(ref.actor, m_ref.prepare_input(want), act, ref.var)
    got = algo._ws.get("ref_logp", rows, 1, torch.float32, dev, cap).view(-1)
    assert torch.equal(got, lp)
    assert np.isfinite(algo.last_stats["kl_ref"]).all() and algo.last_stats["kl_ref"][0] > 0


# --------------------------------------------------------------------------------------------------------------------------------
# 6. learn() updates, then uses
# --------------------------------------------------------------------------------------------------------------------------------
def test_learn_updates_the_statistics_first_and_freeze_holds_them(tg, dev):
    name = "QuadPole"
    S, A = DIMS[name]
    torch.manual_seed(19)
    pol = tg.GaussianActorCritic_NeuralNetwork(S, A, (64, 64), cov=0.3, device=dev, normalize_obs=True)
    on = pol.obs_norm
    mgr = tg.RolloutManager(lambda: make_env(tg, name, T0), pol, num_workers=G0, num_episodes_per_worker=E0, seed=29)
    buf = tg.Rollout_Buffer(mgr)
    algo = tg.PPO(0.2, pol, torch.optim.Adam(pol.parameters(), lr=3e-4), None, 1, gamma=0.99, batch_size=None)
    buf.sample()
    rows = valid_rows(mgr.engine.traj)
    algo.learn(buf)
    check_statistics(on, [rows], [np.zeros(S)])
    assert algo.last_stats["obs_count"] == float(rows.shape[0]) == algo.last_stats["n_valid"]
    on.freeze()
    kept = [t.clone() for t in (on.count, on.mean, on.m2, on.table)]
    buf.sample()
    algo.learn(buf)
    torch.cuda.synchronize()
    for a, b in zip(kept, (on.count, on.mean, on.m2, on.table)):
        assert torch.equal(a, b)
    assert algo.last_stats["obs_count"] == float(rows.shape[0])
    on.unfreeze()
    rows2 = valid_rows(mgr.engine.traj)
    mean_before = on.mean.cpu().numpy().copy()
    algo.learn(buf)
    check_statistics(on, [rows, rows2], [np.zeros(S), mean_before])


@pytest.mark.parametrize("cdt", [None, torch.bfloat16], ids=["f32", "bf16"])
def test_a_captured_per_step_graph_replays_with_the_rewritten_table(tg, dev, cdt):
    name = "CartPole"
    S, A = DIMS[name]
    torch.manual_seed(21)
    pol = tg.GaussianActor_NeuralNetwork(S, A, (64, 64), cov=0.3, device=dev, normalize_obs=True, obs_clip=2.0)
    engs = [tg.DeviceRollout(make_env(tg, name, T0), pol, G0, E0, seed=31, fused=False, use_graph=g, compute_dtype=cdt) for g in (True, False)]
    first = [snapshot(e.run()) for e in engs]
    assert same(first[0], first[1]) and engs[0]._graph is not None and engs[1]._graph is None
    graph = engs[0]._graph
    pol.obs_norm.update(engs[1].traj)                                                     # the table moves, in place
    torch.cuda.synchronize()
    assert float(pol.obs_norm.count) == float(first[1]["mask"].sum())
    second = [snapshot(e.run()) for e in engs]
    assert engs[0]._graph is graph                                                        # no recapture
    assert same(second[0], second[1])
    assert not torch.equal(second[0]["act"], first[0]["act"])


# --------------------------------------------------------------------------------------------------------------------------------
# 7. two ranks against one
# --------------------------------------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_ranks_reproduce_the_one_rank_statistics_and_step(tmp_path):
    """tests/obs_norm_dist_worker.py as fresh child processes (the harness of test_distributed_gpu.py / test_learned_std_gpu.py: gloo,
    both ranks on cuda:0, half the groups each).  The first rollouts are the one-rank rollout bit for bit (identity statistics);
    after one learn() both ranks hold the same bits; the two-rank statistics and the one-rank statistics are each within
    Y.merge_bounds of the exact statistics of the whole rollout's valid rows, count exact, each table within 1 ulp of the table of
    its own statistics and the two tables within 1 ulp of each other plus what the statistics' bounds allow; weights at that
    harness's bar (1e-6 in relative L2); where the tables are bit-equal the second rollout is the one-rank rollout bit for bit."""
    here = os.path.dirname(os.path.abspath(__file__))
    worker = os.path.join(here, "obs_norm_dist_worker.py")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="2")
    procs, outs = [], {}
    for world in (1, 2):
        port = _free_port()
        outs[world] = [str(tmp_path / f"w{world}_r{r}.pt") for r in range(world)]
        for r in range(world):
            procs.append(subprocess.Popen([sys.executable, worker, str(r), str(world), str(port), outs[world][r]],
                                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env))
    for p in procs:
        try:
            log, _ = p.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            pytest.fail("a rank did not finish in 300 s")
        assert p.returncode == 0, log.decode("utf-8", "replace")[-3000:]
    one = torch.load(outs[1][0], weights_only=False)
    two = [torch.load(f, weights_only=False) for f in outs[2]]
    for case, rec in one.items():
        a, b = two[0][case], two[1][case]
        assert torch.equal(torch.cat([a["actions0"], b["actions0"]], 0), rec["actions0"]), case
        for k in ("count", "mean", "m2", "table"):
            assert torch.equal(a[k], b[k]), (case, k)
        assert all(torch.equal(x, y) for x, y in zip(a["weights"], b["weights"]))
        rows = [a["rows"].numpy(), b["rows"].numpy()]
        allx = np.concatenate(rows).astype(np.longdouble)
        S = allx.shape[1]
        mean_ref = allx.mean(0).astype(np.float64)
        m2_ref = ((allx - allx.mean(0)) ** 2).sum(0).astype(np.float64)
        e_mean, e_m2 = Y.merge_bounds([np.concatenate(rows)], [np.zeros(S)])
        for r in (rec, a):
            mean, m2 = r["mean"].numpy(), r["m2"].numpy()
            assert float(r["count"]) == float(allx.shape[0]) == r["obs_count"]
            assert np.all(np.abs(mean - mean_ref) <= e_mean + Y.U * np.abs(mean)), case
            assert np.all(np.abs(m2 - m2_ref) <= e_m2 + Y.U * np.abs(m2)), case
            want = Y.table(float(r["count"]), mean, m2, r["eps"])
            assert np.all(np.abs(r["table"].numpy().astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64))
        t1, t2 = rec["table"].numpy(), a["table"].numpy()
        assert np.all(np.abs(t1.astype(np.float64) - t2.astype(np.float64)) <= np.spacing(np.maximum(np.abs(t1), np.abs(t2))).astype(np.float64)), case
        for x, y in zip(a["weights"], rec["weights"]):
            assert float((x.double() - y.double()).norm()) <= 1e-6 * float(y.double().norm()), case
        # the next rollout reads the merged table: where the two-rank table is the one-rank table (same weights: no optimizer step in
        # between), the ranks' rollouts are the one-rank rollout bit for bit
        u1, u2 = rec["upd_table"].numpy(), a["upd_table"].numpy()
        assert torch.equal(a["upd_table"], b["upd_table"])
        assert np.all(np.abs(u1.astype(np.float64) - u2.astype(np.float64)) <= np.spacing(np.maximum(np.abs(u1), np.abs(u2))).astype(np.float64)), case
        print(case, "tables bit-equal after update():", bool(np.array_equal(u1, u2)), "after learn():", bool(np.array_equal(t1, t2)))
        if np.array_equal(u1, u2):
            assert torch.equal(torch.cat([a["upd_actions"], b["upd_actions"]], 0), rec["upd_actions"]), case
        assert not torch.equal(rec["upd_actions"], rec["actions0"])
