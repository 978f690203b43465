"""Time-limit bootstrapping on the GPU (run with `-m gpu`): tg_rollout_final_state against tg_env_step (bits) and the fp64 oracle,
its classification against the fp64 restatement in tests/bootstrap_fp64.py, tg_ppo_returns_boot against tg_ppo_returns on rewards
the test augments itself (bits), and PPO(bootstrap_truncated=True).learn() against a flag-off learn() on such rewards (bits)."""
import ctypes as C
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import bootstrap_fp64 as B

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ENVS = ["CartPole", "Pendulum", "QuadPole2D", "QuadPole"]
DIMS = {"CartPole": (5, 1), "QuadPole2D": (10, 2), "QuadPole": (20, 4), "Pendulum": (3, 1)}
# test_gpu_parity.py::test_step_matches_oracle_on_seeded_batch's parametrisation: the step kernel against the fp64 oracle
STEP_TOL = [(torch.float64, 1e-11), (torch.float32, 2e-5)]


@pytest.fixture(scope="module")
def tg():
    import trajopt_grpo_amd as tg
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return tg


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def native_step(tg, env, state, action, steps, dtype, dev):
    """tg_env_step through the C ABI (as native_step of test_gpu_parity.py): state [n][S], action [n][A] f32, step counts BEFORE the
    step -> next state [n][S] in `dtype`, on the host."""
    Nn = tg._native
    p = env.native_params()
    n = state.shape[0]
    st = state.t().contiguous().to(dtype)
    ac = action.t().contiguous().float()
    nx = torch.empty_like(st)
    sp = torch.as_tensor(np.asarray(steps), dtype=torch.int32, device=dev)
    tb = torch.zeros(n, dtype=dtype, device=dev)
    rw = torch.empty(n, dtype=dtype, device=dev)
    tr = torch.empty(n, dtype=torch.uint8, device=dev)
    Nn.check(Nn.load().tg_env_step(C.byref(p), Nn.dtype_code(dtype), st.data_ptr(), n, ac.data_ptr(), n, nx.data_ptr(), n,
                                   sp.data_ptr(), tb.data_ptr(), rw.data_ptr(), tr.data_ptr(), n, Nn.stream_ptr(dev)))
    torch.cuda.synchronize()
    return nx.t().contiguous().cpu()


def last_transition(traj):
    """(obs[:, L-1, i] as [n][S], act[:, L-1, i] as [n][A], L) of a finished rollout."""
    L = traj.len.long()
    ar = torch.arange(traj.n, device=L.device)
    return traj.obs[:, L - 1, ar].t().contiguous(), traj.act[:, L - 1, ar].t().contiguous(), L


def make_env(tg, name, T, params):
    return tg.environments.ENV_CLASSES[name](max_steps=T, **params)


# --------------------------------------------------------------------------------------------------------------------------------
# 1. the final state, bits
# --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ENVS)
@pytest.mark.parametrize("dtype,tol", STEP_TOL)
@pytest.mark.parametrize("path", ["per_step", "auto"])
def test_final_state_is_the_step_kernels_bit_for_bit(tg, dev, name, dtype, tol, path):
    """Sampled rollouts on the per-step path and on the path the policy's shape takes by itself (the fp32 fused rollout for a float32
    trajectory).  s_final equals what tg_env_step returns for (obs[:, L-1], act[:, L-1], step count L-1), bit for bit -- an f64
    trajectory's state rounded to f32 once, which is the only form an f32 row can hold it in -- and that step agrees with the fp64
    oracle's at the step kernel's own tolerance for the dtype."""
    S, A = DIMS[name]
    T, G, Eps = 32, 3, 70                                        # n = 210: not a multiple of the wavefront
    torch.manual_seed(3)
    pol = tg.GaussianActor_NeuralNetwork(S, A, (64, 64), cov=0.4, device=dev)
    env = make_env(tg, name, T, {})
    eng = tg.DeviceRollout(env, pol, G, Eps, dtype=dtype, seed=11, fused=False if path == "per_step" else None)
    if path == "auto" and dtype == torch.float32:
        assert eng.fused, "the fp32 fused rollout was expected for this shape"
    traj = eng.run()
    before = [t.clone() for t in (traj.obs, traj.act, traj.rew, traj.mask, traj.len)]
    s_final, timeout = tg.hip_ops.rollout_final_state(eng.params, traj)
    torch.cuda.synchronize()
    for a, b in zip(before, (traj.obs, traj.act, traj.rew, traj.mask, traj.len)):
        assert torch.equal(a, b), "the trajectory is read, not written"
    obs_last, act_last, L = last_transition(traj)
    assert int(L.min()) >= 1 and int(L.max()) <= T
    nx = native_step(tg, env, obs_last, act_last, (L - 1).cpu().numpy(), dtype, dev)
    assert s_final.dtype == torch.float32 and s_final.shape == (G * Eps, S)
    assert torch.equal(s_final.cpu(), nx.float()), "s_final differs from tg_env_step's next state"
    ref = B.oracle_final_state(name, obs_last.double().cpu().numpy(), act_last.cpu().numpy(), L.cpu().numpy(), T, {})
    err = float(np.abs(nx.double().numpy() - ref).max())
    print(name, dtype, path, "max |step - oracle| =", err, "timeouts", int(timeout.sum()), "of", G * Eps)
    np.testing.assert_allclose(nx.double().numpy(), ref, rtol=tol, atol=tol)
    cls = B.classify(name, ref, L.cpu().numpy(), T)
    keep = ~B.near_bound(name, ref)
    assert np.array_equal(timeout.cpu().numpy().astype(bool)[keep], cls[keep])


# --------------------------------------------------------------------------------------------------------------------------------
# 2. classification
# --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ENVS)
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_timeout_is_the_fp64_classification(tg, dev, name, dtype):
    """Teacher-forced cases (tests/bootstrap_fp64.py::forced_case; their shares are confirmed by the oracle alone in
    test_bootstrap_cpu.py).  The oracle steps each episode's last recorded transition in fp64; the helper evaluates the failure test on
    that state and the time test on the step count, separately.  Conditions of the case, asserted here on what the GPU recorded:
    >= 10 % time-limited, >= 10 % ended otherwise, and (for the envs that can fail) an episode that fails exactly at step T, which
    must not count as a timeout.  Episodes whose fp64 final position lies within 1e-5 of the bound are left out: at most 1 %.
    Pendulum cannot fail: its second class is the balance terminal, and it has no boundary episode of this kind."""
    case = B.CASES[name]
    T, params = case["T"], case["params"]
    S, A = DIMS[name]
    init, act = B.forced_case(name)
    n = len(init)
    pol = tg.GaussianActor_NeuralNetwork(S, A, (8,), cov=0.5, device=dev)      # unused: actions are forced
    mgr = tg.RolloutManager(lambda: make_env(tg, name, T, params), pol, num_workers=1, num_episodes_per_worker=n, dtype=dtype)
    traj = mgr.rollout_device(initial_states=init, forced_actions=act)
    s_final, timeout = tg.hip_ops.rollout_final_state(mgr.engine.params, traj)
    obs_last, act_last, L = last_transition(traj)
    Lh = L.cpu().numpy()
    ref = B.oracle_final_state(name, obs_last.double().cpu().numpy(), act_last.cpu().numpy(), Lh, T, params)
    cls = B.classify(name, ref, Lh, T, params.get("timestep"))
    near = B.near_bound(name, ref)
    got = timeout.cpu().numpy().astype(bool)
    boundary = B.failed(name, ref) & (Lh == T) & ~near
    print(name, dtype, "timeout share", cls.mean(), "left out", int(near.sum()), "boundary episodes", int(boundary.sum()))
    assert near.mean() <= 0.01
    assert cls.mean() >= 0.10 and (~cls).mean() >= 0.10
    assert np.array_equal(got[~near], cls[~near])
    if name == "Pendulum":
        assert np.all(Lh[~cls] == 11) and not B.failed(name, ref).any()
    else:
        assert boundary.sum() >= 1 and not got[boundary].any()
    # a slot without a finished episode: zeros and 0, whatever its neighbours hold
    traj.len[5] = 0
    traj.len[6] = -3
    s2, t2 = tg.hip_ops.rollout_final_state(mgr.engine.params, traj)
    assert not s2[5:7].any() and not t2[5:7].any()
    keep = torch.ones(n, dtype=torch.bool, device=dev)
    keep[5:7] = False
    assert torch.equal(s2[keep], s_final[keep]) and torch.equal(t2[keep], timeout[keep])


# --------------------------------------------------------------------------------------------------------------------------------
# 3. returns, bits
# --------------------------------------------------------------------------------------------------------------------------------
def _ragged(dev, T, n, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    L = torch.randint(1, T + 1, (n,), generator=g)
    L[0], L[1], L[2] = 1, T, T
    mask = (torch.arange(T)[:, None] < L[None, :])
    zero = torch.zeros(T, n)
    rew = torch.where(mask, torch.randn(T, n, generator=g), zero)               # (no negative zeros)
    val = torch.where(mask, torch.randn(T, n, generator=g), zero)
    b = torch.randn(n, generator=g) * 3
    b[torch.rand(n, generator=g) < 0.4] = 0.0
    return (rew.to(dev), val.to(dev), mask.to(torch.uint8).to(dev), L.to(torch.int32).to(dev), b.to(dev))


@pytest.mark.parametrize("monte_carlo", [True, False], ids=["mc", "gae"])
@pytest.mark.parametrize("gamma", [0.5, 0.99, 0.999])
def test_returns_boot_equals_returns_on_augmented_rewards(tg, dev, monte_carlo, gamma):
    K = tg.hip_ops
    T, n = 45, 333                                              # ragged lengths incl. L = 1 and L = T; n not a multiple of 256
    rew, val, mask, L, b = _ragged(dev, T, n, 7)
    assert int((b == 0).sum()) > 0 and int((b != 0).sum()) > 0
    ar = torch.arange(n, device=dev)
    aug = rew.clone()
    bonus = b * gamma                                           # two separately rounded fp32 operations
    aug[L.long() - 1, ar] = rew[L.long() - 1, ar] + bonus
    out = {}
    for tag, call in (("ref", lambda a, r, w: K.ppo_returns(aug, val, mask, gamma, 0.95, monte_carlo, a, r, w)),
                      ("boot", lambda a, r, w: K.ppo_returns_boot(rew, val, mask, L, b, gamma, 0.95, monte_carlo, a, r, w)),
                      ("plain", lambda a, r, w: K.ppo_returns(rew, val, mask, gamma, 0.95, monte_carlo, a, r, w)),
                      ("boot0", lambda a, r, w: K.ppo_returns_boot(rew, val, mask, L, torch.zeros_like(b), gamma, 0.95, monte_carlo, a, r, w))):
        adv, ret = torch.full_like(rew, float("nan")), torch.full_like(rew, float("nan"))
        rew_before = rew.clone()
        mom = call(adv, ret, torch.empty(6 * n, dtype=torch.float64, device=dev))
        torch.cuda.synchronize()
        assert torch.equal(rew, rew_before)
        out[tag] = (adv, ret, mom)
    for x, y in (("boot", "ref"), ("boot0", "plain")):
        for p, q in zip(out[x], out[y]):
            assert torch.equal(p, q), (x, y)
    assert not torch.equal(out["boot"][1], out["plain"][1])     # (the bonus is there)


# --------------------------------------------------------------------------------------------------------------------------------
# 4. learn(), end to end
# --------------------------------------------------------------------------------------------------------------------------------
FACTORY = {"CartPole": (5, 1, (128, 128, 128), 0.5), "QuadPole2D": (10, 2, (128, 128, 128), 0.5)}


def _learner(tg, dev, name, flag, updates, monte_carlo, batch_size, forced=None, T=32, G=4, Eps=40):
    """Policy, manager, sampled (or teacher-forced) buffer and PPO, built from fixed seeds: two calls give bit-identical weights and
    trajectories -- the test's `deep copy` of learner and buffer."""
    S, A, hidden, cov = FACTORY[name]
    params = B.CASES[name]["params"]
    torch.manual_seed(5)
    pol = tg.GaussianActorCritic_NeuralNetwork(S, A, hidden, cov=cov, device=dev)
    mgr = tg.RolloutManager(lambda: make_env(tg, name, T, params), pol, num_workers=G, num_episodes_per_worker=Eps, seed=9)
    buf = tg.Rollout_Buffer(mgr)
    if forced is None:
        buf.sample()
    else:
        buf.device_traj = mgr.rollout_device(initial_states=forced[0], forced_actions=forced[1])
    algo = tg.PPO(epsilon=0.2, policy=pol, optimizer=torch.optim.Adam(pol.parameters(), lr=2e-4), ref_model=None,
                  updates_per_iter=updates, gamma=0.99, lam=0.95, batch_size=batch_size, monte_carlo=monte_carlo, seed=3,
                  bootstrap_truncated=flag)
    return pol, mgr, buf, algo


def _critic_values(tg, algo, s_final):
    """V(s_final) by the learner's own no-grad critic path on freshly built weight layouts: the pass _learn runs on these rows."""
    critic = algo.policy.critic
    m = algo._mlp(critic)
    if m is None:
        return algo._forward(critic, s_final).reshape(-1).clone()
    m.refresh(force=True)
    return m.forward(m.prepare_input(s_final), keep=False, padded=True)[:, 0].clone()


def _augment_on_device(tg, algo, mgr, traj):
    """traj.rew += gamma * V(s_final) * timeout at each episode's last step, from the new wrapper and the critic pass; -> timeout."""
    s_final, timeout = tg.hip_ops.rollout_final_state(mgr.engine.params, traj)
    b = _critic_values(tg, algo, s_final) * timeout
    L = traj.len.long()
    ar = torch.arange(traj.n, device=L.device)
    bonus = b * algo.gamma
    traj.rew[L - 1, ar] = traj.rew[L - 1, ar] + bonus
    return timeout, b


LEARN_CASES = [("CartPole", 1, True, None), ("CartPole", 2, False, None), ("QuadPole2D", 2, True, None), ("QuadPole2D", 1, False, None),
               ("CartPole", 2, True, 512)]


@pytest.mark.parametrize("name,updates,monte_carlo,batch_size", LEARN_CASES)
def test_learn_with_the_flag_equals_learn_without_it_on_augmented_rewards(tg, dev, name, updates, monte_carlo, batch_size):
    """The factories' net shapes (fp32), full batch and one minibatch case.  Everything downstream of the returns kernel is the same
    code, and the critic pass is the same kernel on the same rows and weights: the weights after learn() are compared bit for bit."""
    pol_on, mgr_on, buf_on, algo_on = _learner(tg, dev, name, True, updates, monte_carlo, batch_size)
    pol_off, mgr_off, buf_off, algo_off = _learner(tg, dev, name, False, updates, monte_carlo, batch_size)
    t_on, t_off = buf_on.device_traj, buf_off.device_traj
    for a, b in zip((t_on.obs, t_on.act, t_on.rew, t_on.len), (t_off.obs, t_off.act, t_off.rew, t_off.len)):
        assert torch.equal(a, b)
    for p, q in zip(pol_on.parameters(), pol_off.parameters()):
        assert torch.equal(p, q)
    rew_before = t_on.rew.clone()
    timeout, b = _augment_on_device(tg, algo_off, mgr_off, t_off)
    assert int(timeout.sum()) > 0 and float(b.abs().max()) > 0 and not torch.equal(t_off.rew, rew_before)
    algo_on.learn(buf_on)
    algo_off.learn(buf_off)
    torch.cuda.synchronize()
    assert torch.equal(t_on.rew, rew_before), "learn() must not modify the trajectory's rewards"
    assert torch.equal(algo_on.norm8, algo_off.norm8)
    for k, (p, q) in enumerate(zip(pol_on.parameters(), pol_off.parameters())):
        assert torch.equal(p, q), k
    stats_on, stats_off = algo_on.last_stats, algo_off.last_stats
    assert stats_on["n_bootstrapped"] == int(timeout.sum()) and "n_bootstrapped" not in stats_off
    assert stats_on["total_loss"] == stats_off["total_loss"]
    print(name, updates, monte_carlo, batch_size, "n_bootstrapped", stats_on["n_bootstrapped"], "of", t_on.n)


def test_a_buffer_without_timeouts_gives_the_flag_off_run(tg, dev):
    """Every episode fails before the horizon (large constant pushes): b = 0 everywhere, and rewards of a rollout hold no negative
    zeros, so flag on is flag off, bit for bit."""
    name = "CartPole"
    S, A = DIMS[name]
    T, n = 32, 160
    rng = np.random.default_rng(1)
    from oracle import envs as E
    init = E.sample_initial_states(name, n, rng).astype(np.float32).astype(np.float64)
    s = rng.uniform(0.6, 1.0, n) * rng.choice([-1.0, 1.0], n)
    act = np.broadcast_to(s[:, None, None], (n, T, A)).astype(np.float32).copy()
    runs = {}
    for flag in (True, False):
        pol, mgr, buf, algo = _learner(tg, dev, name, flag, 2, True, None, forced=(init, act))
        _, timeout = tg.hip_ops.rollout_final_state(mgr.engine.params, buf.device_traj)
        assert int(timeout.sum()) == 0 and int(buf.device_traj.len.max()) < T
        algo.learn(buf)
        torch.cuda.synchronize()
        runs[flag] = ([p.detach().clone() for p in pol.parameters()], algo.last_stats)
    for p, q in zip(runs[True][0], runs[False][0]):
        assert torch.equal(p, q)
    assert runs[True][1]["n_bootstrapped"] == 0


# --------------------------------------------------------------------------------------------------------------------------------
# 5. it changes what it should
# --------------------------------------------------------------------------------------------------------------------------------
def test_every_episode_time_limited_moves_the_last_return_by_gamma_v(tg, dev):
    name = "CartPole"
    S, A = DIMS[name]
    T, n = 32, 160
    rng = np.random.default_rng(2)
    from oracle import envs as E
    init = E.sample_initial_states(name, n, rng).astype(np.float32).astype(np.float64)
    act = np.zeros((n, T, A), dtype=np.float32)
    ret, mean, v = {}, {}, None
    for flag in (True, False):
        pol, mgr, buf, algo = _learner(tg, dev, name, flag, 1, True, None, forced=(init, act))
        traj = buf.device_traj
        s_final, timeout = tg.hip_ops.rollout_final_state(mgr.engine.params, traj)
        assert int(timeout.sum()) == n and int(traj.len.min()) == T
        if flag:
            v = _critic_values(tg, algo, s_final)
        algo.learn(buf)
        torch.cuda.synchronize()
        ret[flag] = algo._ws._buf["ret_full"][:T * n].view(T, n).clone()       # Monte Carlo: the pre-normalisation returns
        mean[flag] = float(algo.norm8[2])
        if flag:
            assert algo.last_stats["n_bootstrapped"] == n
    gv = (v * algo.gamma).double()
    diff = ret[True][T - 1].double() - ret[False][T - 1].double()
    scale = torch.maximum(torch.maximum(ret[True][T - 1].abs(), ret[False][T - 1].abs()), gv.abs().float()).double()
    print("max |diff - gamma V| / scale =", float(((diff - gv).abs() / scale).max()), "mean V", float(v.mean()), "ret mean", mean)
    assert torch.all((diff - gv).abs() <= 2.0 ** -23 * scale)                   # one fp32 rounding of r + gamma V
    assert float(v.mean()) != 0.0 and np.sign(mean[True] - mean[False]) == np.sign(float(v.mean()))


# --------------------------------------------------------------------------------------------------------------------------------
# 6. two ranks
# --------------------------------------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_ranks_with_the_flag_equal_one_rank(tmp_path):
    """tests/bootstrap_dist_worker.py as fresh child processes (the harness of test_distributed_gpu.py / test_grad_clip_gpu.py: gloo,
    both ranks on cuda:0, half the groups each): b is per env and local, so the two ranks reproduce the one-rank weights to that
    harness's 1e-6 (relative L2), and n_bootstrapped is the global count on every rank."""
    worker = os.path.join(HERE, "bootstrap_dist_worker.py")
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
        print(case, "n_bootstrapped", rec["n_bootstrapped"], "local", a["n_local"], b["n_local"])
        assert all(torch.equal(x, y) for x, y in zip(a["weights"], b["weights"]))
        assert 0 < rec["n_bootstrapped"] == rec["n_local"]
        assert a["n_bootstrapped"] == b["n_bootstrapped"] == a["n_local"] + b["n_local"] == rec["n_bootstrapped"]
        for x, y in zip(a["weights"], rec["weights"]):
            assert float((x.double() - y.double()).norm()) <= 1e-6 * float(y.double().norm()), case


# --------------------------------------------------------------------------------------------------------------------------------
# 7. refusals
# --------------------------------------------------------------------------------------------------------------------------------
def test_swarm_and_engineless_buffers_are_refused(tg, dev):
    torch.manual_seed(0)
    pol = tg.GaussianActorCritic_NeuralNetwork(20, 4, (64, 64), cov=0.3, device=dev)
    mgr = tg.RolloutManager(lambda: tg.QuadPoleSwarm(n_agents=4, max_steps=16), pol, num_workers=2, num_episodes_per_worker=4, seed=1)
    buf = tg.Rollout_Buffer(mgr)
    buf.sample()
    before = [p.detach().clone() for p in pol.parameters()]
    algo = tg.PPO(epsilon=0.2, policy=pol, optimizer=torch.optim.Adam(pol.parameters(), lr=3e-4), ref_model=None, updates_per_iter=1,
                  batch_size=None, bootstrap_truncated=True)
    with pytest.raises(ValueError, match="swarm"):
        algo.learn(buf)
    with pytest.raises(ValueError, match=r"swarm envs \(agents=4\) are not supported"):
        tg.hip_ops.rollout_final_state(mgr.engine.params, buf.device_traj)       # the native refusal itself
    # hand-built CPU tensors: no engine to take the env parameters from
    mgr1 = tg.RolloutManager(lambda: tg.QuadPole(max_steps=16), pol, num_workers=2, num_episodes_per_worker=4, seed=1)
    obs, act, rew, ln, mask = mgr1.rollout()
    hand = type("HandBuilt", (), dict(group_observations=obs, group_actions=act, group_rewards=rew, group_lengths=ln, group_masks=mask))()
    with pytest.raises(ValueError, match="no rollout engine"):
        algo.learn(hand)
    torch.cuda.synchronize()
    assert all(torch.equal(p, q) for p, q in zip(pol.parameters(), before)), "a refused learn() leaves the weights alone"
    # ... while the same buffer trains without the flag
    tg.PPO(epsilon=0.2, policy=pol, optimizer=torch.optim.Adam(pol.parameters(), lr=3e-4), ref_model=None, updates_per_iter=1,
           batch_size=None).learn(hand)
