"""Per-env domain randomisation on the MI355X (Env.randomize, tg_env_randomize and the `_dr` entry points):

  1. off means unchanged: every range (1, 1) gives the un-randomised rollout bit for bit, on every rollout path (tolerance zero:
     the device-built constants are the host-built ones);
  2. DeviceRollout.env_params equals the fp64 restatement of the draw (tests/domain_rand_fp64.py) bit for bit;
  3. each slot steps its own vehicle: 64 sampled slots replayed through the oracle step with the slot's parameters patched in, at
     the per-step fp64 tolerance of test_gpu_parity.py::test_step_matches_oracle_on_seeded_batch, lengths and masks exact;
  4. the teacher-forced one-launch replay, the per-step replay and tg_rollout_final_state_dr reproduce a fused randomised rollout
     bit for bit;
  5. two ranks reproduce the rows of one rank, bit for bit;
  6. PPO(bootstrap_truncated=True) re-steps with the slot's own parameters;
  7. different vehicles end in different states, the episodes of a restart group in identical ones."""
import ctypes as C
import os
import socket
import subprocess
import sys
from unittest import mock

import numpy as np
import pytest
import torch

from oracle import envs as E

import domain_rand_fp64 as DR

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DIMS = {"CartPole": (5, 1), "QuadPole2D": (10, 2), "QuadPole": (20, 4), "Pendulum": (3, 1)}
STEP_TOL_F64 = 1e-11        # test_gpu_parity.py::test_step_matches_oracle_on_seeded_batch, float64: states rtol = atol = tol, rewards atol 50 tol
WIDE = (0.5, 2.0)


@pytest.fixture(scope="module")
def tg():
    import trajopt_grpo_amd as tg
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return tg


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def make_env(tg, name, T, ranges=None, seed=0, **kw):
    env = tg.environments.ENV_CLASSES[name](max_steps=T, **kw)
    if ranges is not None:
        env.randomize(ranges, seed=seed)
    return env


def snapshot(tr):
    torch.cuda.synchronize()
    return {k: getattr(tr, k).clone() for k in ("obs", "act", "rew", "mask", "len")}


def same(a, b):
    return all(torch.equal(a[k], b[k]) for k in ("obs", "act", "rew", "mask", "len"))


def oracle_step(name, col, state, action, steps, T, time_balanced=0.0):
    """The oracle's step for ONE env whose p[] is `col` (its column of env_params): state [S], action [A], steps and time_balanced
    before the step -> (next state, reward, truncated, steps after, time_balanced after)."""
    st, ac, sp, tb = state[None, :], action[None, :], np.array([steps]), np.full(1, time_balanced)
    if name == "CartPole":
        return E.cartpole_step(st, ac, sp, tb, max_steps=T, masscart=col[0], masspole=col[1], length=col[2], gravity=col[3])
    if name == "Pendulum":
        return E.pendulum_step(st, ac, sp, tb, max_steps=T, mass=col[0], length=col[1], gravity=col[2])
    if name == "QuadPole2D":
        with mock.patch.dict(E.QP2D, dict(mq=col[0], mp=col[1], I=col[2], Lq=col[3], Lp=col[4], gravity=col[5])):
            return E.quadpole2d_step(st, ac, sp, tb, max_steps=T)
    with mock.patch.dict(E.QP3D, dict(mass=col[0], load_mass=col[1], gravity=col[2], tether=col[3], Ixx=col[4], Iyy=col[5], Izz=col[6],
                                      torque_constant=col[7], arm=col[8])):
        return E.quadpole_step(st, ac, sp, tb, max_steps=T)


# --------------------------------------------------------------------------------------------------------------------------------
# 1. off means unchanged
# --------------------------------------------------------------------------------------------------------------------------------
PATHS = ["per_step_f64", "per_step_f32", "forced", "fused_bf16", "f32_relu_16", "f32_relu_32", "f32_tanh_16", "f32_tanh_32"]


@pytest.mark.parametrize("name", ["CartPole", "Pendulum", "QuadPole2D", "QuadPole", "QuadPoleSwarm"])
@pytest.mark.parametrize("path", PATHS)
def test_unit_ranges_give_the_plain_rollout_bit_for_bit(tg, dev, name, path):
    base = "QuadPole" if name == "QuadPoleSwarm" else name
    S, A = DIMS[base]
    kw = {"n_agents": 4} if name == "QuadPoleSwarm" else {}
    T, G, Eps = 40, 6, 24
    torch.manual_seed(5)
    hidden = (128, 128) if path == "fused_bf16" else (64, 64)
    act = "Tanh" if "tanh" in path else "ReLU"
    pol = tg.GaussianActor_NeuralNetwork(S, A, hidden, activation=act, cov=0.3, device=dev)
    ekw = dict(seed=13)
    if path == "fused_bf16":
        ekw.update(compute_dtype=torch.bfloat16)
    elif path == "per_step_f64":
        ekw.update(dtype=torch.float64)
    elif path in ("per_step_f32", "forced"):
        ekw.update(fused=False)
    unit = {k: (1.0, 1.0) for k in tg.environments.ENV_CLASSES[name].RANDOMIZABLE}
    results = []
    for ranges in (None, unit):
        eng = tg.DeviceRollout(make_env(tg, name, T, ranges, **kw), pol, G, Eps, **ekw)
        if path.startswith("f32_"):
            eng.f32_block_envs = int(path[-2:])
        assert eng.fused == (path == "fused_bf16" or path.startswith("f32_"))
        if path == "forced":
            rng = np.random.default_rng(3)
            init = E.sample_initial_states(base, eng.n, rng)
            forced = rng.normal(size=(eng.n, T, A)).astype(np.float32) * 0.6
            tr = eng.run(initial_states=init, forced_actions=forced)
        else:
            tr = eng.run()
        results.append(snapshot(tr))
        if ranges is None:
            assert eng.env_params is None
        else:
            nominal = torch.tensor(list(eng.params.p), dtype=torch.float64, device=dev)
            assert torch.equal(eng.env_params, nominal[:, None].expand(12, eng.n))
    assert int(results[0]["len"].min()) >= 1 and float(results[0]["obs"].abs().sum()) > 0
    assert same(results[0], results[1])
    if path.startswith("f32_relu"):
        # the engine launches the `_act_dr` form; tg_fused_rollout_f32_dr itself (ReLU) on the same start, table and RNG stream
        Nn = tg._native
        tr = eng.traj
        nat = tr.native()
        st = Nn.stream_ptr(dev)
        Nn.check(Nn.load().tg_rollout_begin(C.byref(nat), S, A, st))
        tr.obs[:, 0, :].copy_(results[1]["obs"][:, 0, :])
        rng0 = torch.tensor([13, 0], dtype=torch.int64, device=dev)
        Nn.check(Nn.load().tg_fused_rollout_f32_dr(C.byref(eng.params), eng.env_params.data_ptr(), C.byref(nat), eng._frag.stream.data_ptr(),
                                                   eng._frag.table.data_ptr(), 64, 2, eng._f32_block_envs, eng._sigma, rng0.data_ptr(), 0, 0, T, st))
        assert same(snapshot(tr), results[1])


@pytest.mark.parametrize("use_graph", [True, False])
def test_switching_randomisation_off_on_a_live_engine_drops_the_table(tg, dev, use_graph):
    """A per-step engine (float64 trajectory; with use_graph its un-randomised rollouts are hipGraph replays): a randomised rollout,
    then randomize(None).  The next rollouts are a never-randomised engine's rollouts of the same stream ids bit for bit, with no
    table -- the graph is captured after the switch and must hold the plain launches."""
    T, G, Eps = 24, 4, 16
    torch.manual_seed(6)
    pol = tg.GaussianActor_NeuralNetwork(10, 2, (64, 64), cov=0.3, device=dev)
    env = make_env(tg, "QuadPole2D", T, {"mq": WIDE, "Lp": WIDE}, seed=4)
    eng = tg.DeviceRollout(env, pol, G, Eps, dtype=torch.float64, seed=77, use_graph=use_graph)
    ref = tg.DeviceRollout(make_env(tg, "QuadPole2D", T), pol, G, Eps, dtype=torch.float64, seed=77, use_graph=use_graph)
    assert not eng.fused and bool(eng.use_graph) == use_graph
    first, ref_first = snapshot(eng.run()), snapshot(ref.run())
    assert eng.env_params is not None and ref.env_params is None and not same(first, ref_first)
    env.randomize(None)
    for _ in range(2):                                                # (with use_graph: the capture, then a replay)
        got, want = snapshot(eng.run()), snapshot(ref.run())
        assert eng.env_params is None
        assert same(got, want)
    assert (eng._graph is not None) == use_graph
    env.randomize({"mq": WIDE})                                       # ... and on again: a table, other states
    again, want = snapshot(eng.run()), snapshot(ref.run())
    assert eng.env_params is not None and not same(again, want)


# --------------------------------------------------------------------------------------------------------------------------------
# 2. the draw
# --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["QuadPole", "CartPole"])
@pytest.mark.parametrize("restart", [False, True])
def test_env_params_equal_the_fp64_restatement_bit_for_bit(tg, dev, name, restart):
    S, A = DIMS[name]
    T, G, Eps = 4, 128, 32                                          # n = 4,096 slots
    ranges = {k: (0.5 + 0.05 * j, 1.5 + 0.1 * j) for j, k in enumerate(tg.environments.ENV_CLASSES[name].RANDOMIZABLE) if j != 1}
    torch.manual_seed(0)
    pol = tg.GaussianActor_NeuralNetwork(S, A, (64, 64), cov=0.3, device=dev)
    env = make_env(tg, name, T, ranges, seed=77)
    eng = tg.DeviceRollout(env, pol, G, Eps, restart=restart, seed=123456789, group_offset=3)
    nominal = list(eng.params.p)
    for stream in (0, 1):                                           # two rollouts = two stream ids: the parameters are re-drawn
        eng.run()
        torch.cuda.synchronize()
        ref = DR.table(nominal, DR.spec_of(env), 123456789, stream, eng.n, key_offset=3 * Eps, key_div=Eps if restart else 1,
                       randomize_seed=77)
        got = eng.env_params.cpu().numpy()
        assert got.shape == (12, eng.n) and got.dtype == np.float64
        assert np.array_equal(got, ref)
        for r in range(12):
            if r not in [s[0] for s in DR.spec_of(env)]:
                assert np.all(got[r] == nominal[r])                   # un-randomised rows: the nominal value, exactly
        if restart:
            assert np.all(got.reshape(12, G, Eps) == got.reshape(12, G, Eps)[:, :, :1])
        if stream == 0:
            first = got.copy()
    assert not np.array_equal(first[0], got[0])


# --------------------------------------------------------------------------------------------------------------------------------
# 3. each slot steps its own vehicle
# --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["QuadPole", "QuadPole2D", "CartPole", "Pendulum"])
def test_sampled_slots_replay_through_the_oracle_with_their_own_parameters(tg, dev, name):
    S, A = DIMS[name]
    T, G, Eps = 64, 16, 32
    ranges = {k: WIDE for k in tg.environments.ENV_CLASSES[name].RANDOMIZABLE}
    torch.manual_seed(2)
    pol = tg.GaussianActor_NeuralNetwork(S, A, (64, 64), cov=0.3, device=dev)
    eng = tg.DeviceRollout(make_env(tg, name, T, ranges, seed=1), pol, G, Eps, dtype=torch.float64, seed=17)
    tr = eng.run()
    torch.cuda.synchronize()
    obs, act, rew = tr.obs.cpu().numpy(), tr.act.cpu().numpy(), tr.rew.cpu().numpy()
    mask, ln, ptab = tr.mask.cpu().numpy(), tr.len.cpu().numpy(), eng.env_params.cpu().numpy()
    slots = np.random.default_rng(0).choice(eng.n, size=64, replace=False)
    worst_s = worst_r = 0.0
    compared = 0
    balance_limit = E.ENV_SPECS[name].get("balance_terminates")
    for i in slots:
        L = int(ln[i])
        assert 1 <= L <= T and np.array_equal(mask[:, i], (np.arange(T) < L).astype(np.uint8))
        tb = 0.0
        for t in range(L):
            nx, rw, trunc, _, tb_next = oracle_step(name, ptab[:, i], obs[:, t, i], act[:, t, i], t, T, tb)
            tb = float(tb_next[0])
            ended = bool(trunc[0]) or (balance_limit is not None and tb > balance_limit)      # Pendulum: the balance terminal too
            assert rw.shape == (1,)
            np.testing.assert_allclose(rew[t, i], rw[0], rtol=STEP_TOL_F64, atol=50 * STEP_TOL_F64)
            worst_r = max(worst_r, abs(rew[t, i] - rw[0]))
            if t + 1 < L:                                            # the episode went on: the oracle agrees, and on the state
                assert not ended, (name, i, t)
                np.testing.assert_allclose(obs[:, t + 1, i], nx[0], rtol=STEP_TOL_F64, atol=STEP_TOL_F64)
                worst_s = max(worst_s, float(np.abs(obs[:, t + 1, i] - nx[0]).max()))
                compared += 1
            else:                                                    # ... ended here: the oracle's flag, or the horizon
                assert ended or L == T, (name, i, t)
    assert compared >= 64 * 4, compared                               # whole episodes were replayed, not a handful of first steps
    print(name, "64 slots, none left out;", compared, "state comparisons; max |state - oracle|", worst_s, "max |reward - oracle|", worst_r)
    # the vehicles differ: a nominal-parameter oracle step is NOT the recorded one
    i = int(slots[0])
    nominal = np.array(list(eng.params.p))
    nx, *_ = oracle_step(name, nominal, obs[:, 0, i], act[:, 0, i], 0, T)
    assert float(np.abs(nx[0] - obs[:, 1, i]).max()) > 1e-6


# --------------------------------------------------------------------------------------------------------------------------------
# 4. all paths agree
# --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["quadpole_4096_f32", "quadpole_4096_bf16", "swarm8_f32"])
def test_forced_per_step_and_final_state_reproduce_the_fused_rollout(tg, dev, case):
    name, kw = ("QuadPoleSwarm", {"n_agents": 8}) if case.startswith("swarm") else ("QuadPole", {})
    G, Eps, T = (64, 64, 48) if not kw else (16, 8, 48)
    cdt, hidden = (torch.bfloat16, (128, 128)) if case.endswith("bf16") else (None, (64, 64))
    ranges = {"mass": (0.7, 1.4), "load_mass": WIDE, "Ixx": WIDE, "Iyy": WIDE, "tether_length": WIDE, "arm_length": (0.8, 1.25)}
    torch.manual_seed(11)
    pol = tg.GaussianActor_NeuralNetwork(20, 4, hidden, cov=0.3, device=dev)
    mk = lambda: make_env(tg, name, T, ranges, seed=3, **kw)
    eng = tg.DeviceRollout(mk(), pol, G, Eps, seed=31, compute_dtype=cdt)
    assert eng.fused
    fused = snapshot(eng.run())
    ptab = eng.env_params.clone()
    n = eng.n
    assert n == (4096 if not kw else 1024)
    ln = fused["len"]
    assert torch.equal(fused["mask"], (torch.arange(T, device=dev)[:, None] < ln[None, :]).to(torch.uint8))
    assert int(ln.min()) >= 1 and int(ln.min()) < T                  # some vehicles leave the bounds
    init, forced = fused["obs"][:, 0, :].t().cpu().numpy(), fused["act"].permute(2, 1, 0).cpu().numpy()
    for per_step in (True, False):
        # (a fresh engine per replay: the parameters are re-drawn with every rollout, and the fused rollout was a first one)
        plain = tg.DeviceRollout(mk(), pol, G, Eps, seed=31, compute_dtype=cdt, fused=False)
        plain.forced_per_step = per_step
        replay = snapshot(plain.run(initial_states=init, forced_actions=forced))
        assert torch.equal(plain.env_params, ptab)
        assert torch.equal(replay["len"], ln) and torch.equal(replay["mask"], fused["mask"]), per_step
        assert torch.equal(replay["rew"], fused["rew"]) and torch.equal(replay["obs"], fused["obs"]), per_step
    again = tg.DeviceRollout(mk(), pol, G, Eps, seed=31, compute_dtype=cdt)
    assert same(snapshot(again.run()), fused)
    if not kw:
        # tg_rollout_final_state_dr re-steps transition len - 1.  Told that every episode was one step shorter, it must return the
        # state the fused kernel recorded in slot len - 1, bit for bit (same step function, same table)
        s_final, timeout = tg.hip_ops.rollout_final_state(eng.params, eng.traj, env_params=ptab)
        L = ln.long()
        long_enough = L >= 2
        assert int(long_enough.sum()) > n // 2
        eng.traj.len.copy_(torch.where(long_enough, ln - 1, ln))
        s_prev, _ = tg.hip_ops.rollout_final_state(eng.params, eng.traj, env_params=ptab)
        eng.traj.len.copy_(ln)
        recorded = fused["obs"][:, L - 1, torch.arange(n, device=dev)].t()
        assert torch.equal(s_prev[long_enough], recorded[long_enough])
        nominal_final, _ = tg.hip_ops.rollout_final_state(eng.params, eng.traj)
        assert not torch.equal(nominal_final, s_final)
        assert torch.isfinite(s_final).all() and int(timeout.sum()) > 0


# --------------------------------------------------------------------------------------------------------------------------------
# 5. sharding
# --------------------------------------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_ranks_reproduce_the_rows_of_one_rank(tmp_path):
    worker = os.path.join(HERE, "domain_rand_dist_worker.py")
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
        Eg = rec["E"]
        for shard in two:
            lo, hi = shard[case]["groups"]
            assert hi > lo
            cols = slice(lo * Eg, hi * Eg)
            for k in range(2):
                whole, part = rec["runs"][k], shard[case]["runs"][k]
                assert torch.equal(part["env_params"], whole["env_params"][:, cols]), case
                for key in ("obs", "act", "rew", "mask"):
                    assert torch.equal(part[key], whole[key][..., cols]), (case, key)
                assert torch.equal(part["len"], whole["len"][cols]), case
        assert not torch.equal(rec["runs"][0]["env_params"], rec["runs"][1]["env_params"])
        assert two[0][case]["groups"][1] == two[1][case]["groups"][0]


# --------------------------------------------------------------------------------------------------------------------------------
# 6. bootstrap
# --------------------------------------------------------------------------------------------------------------------------------
def test_ppo_bootstrap_re_steps_each_slot_with_its_own_parameters(tg, dev):
    name, T, G, Eps = "QuadPole2D", 16, 8, 16
    ranges = {k: WIDE for k in tg.QuadPole2D.RANDOMIZABLE}
    torch.manual_seed(4)
    pol = tg.GaussianActorCritic_NeuralNetwork(10, 2, (64, 64), cov=0.3, device=dev)
    mgr = tg.RolloutManager(lambda: make_env(tg, name, T, ranges, seed=2), pol, num_workers=G, num_episodes_per_worker=Eps, seed=9,
                            dtype=torch.float64)
    buf = tg.Rollout_Buffer(mgr)
    buf.sample()
    algo = tg.PPO(epsilon=0.2, policy=pol, optimizer=torch.optim.Adam(pol.parameters(), lr=3e-4), ref_model=None, updates_per_iter=1,
                  gamma=0.99, batch_size=None, bootstrap_truncated=True)
    seen = {}
    plain = tg.hip_ops.rollout_final_state

    def spy(params, traj, s_final=None, timeout=None, env_params=None):
        out = plain(params, traj, s_final, timeout, env_params=env_params)
        torch.cuda.synchronize()
        seen.update(env_params=env_params, s_final=out[0].clone(), timeout=out[1].clone())
        return out

    with mock.patch.object(tg.algorithms.K, "rollout_final_state", spy):
        algo.learn(buf)
    eng, traj = mgr.engine, buf.device_traj
    assert seen["env_params"] is eng.env_params and eng.env_params is not None
    timeout = seen["timeout"].cpu().numpy().astype(bool)
    assert timeout.sum() > 0 and algo.last_stats["n_bootstrapped"] == int(timeout.sum())
    obs, act, ln = traj.obs.cpu().numpy(), traj.act.cpu().numpy(), traj.len.cpu().numpy()
    ptab, s_final = eng.env_params.cpu().numpy(), seen["s_final"].cpu().numpy()
    nominal_final, _ = plain(eng.params, traj)
    nominal_final = nominal_final.cpu().numpy()
    for i in np.nonzero(timeout)[0]:
        L = int(ln[i])
        nx, _, _, _, _ = oracle_step(name, ptab[:, i], obs[:, L - 1, i], act[:, L - 1, i], L - 1, T)
        # (s_final is the f64 step rounded to f32 once: the fp64 step tolerance plus half an ulp of float32)
        np.testing.assert_allclose(s_final[i], nx[0], rtol=STEP_TOL_F64 + 2.0 ** -24, atol=STEP_TOL_F64 + 2.0 ** -24)
    assert float(np.abs(nominal_final[timeout] - s_final[timeout]).max()) > 1e-4      # not the nominal vehicle's re-step


# --------------------------------------------------------------------------------------------------------------------------------
# 7. it does something
# --------------------------------------------------------------------------------------------------------------------------------
def test_different_vehicles_diverge_and_a_restart_group_does_not(tg, dev):
    T, G, Eps = 50, 4, 8
    ranges = {"Ixx": WIDE, "tether_length": WIDE}
    torch.manual_seed(0)
    pol = tg.GaussianActor_NeuralNetwork(20, 4, (64, 64), cov=0.3, device=dev)
    eng = tg.DeviceRollout(make_env(tg, "QuadPole", T, ranges, seed=8), pol, G, Eps, restart=True, dtype=torch.float64, seed=5)
    n = eng.n
    init = np.repeat(E.sample_initial_states("QuadPole", 1, np.random.default_rng(1)), n, axis=0)      # one shared initial state
    t = np.arange(T, dtype=np.float32)[None, :, None]
    forced = np.broadcast_to(0.05 * np.sin(0.3 * t + np.arange(4, dtype=np.float32)[None, None, :]) + np.array([0.02, -0.02, 0.01, 0.0], np.float32),
                             (n, T, 4)).copy()
    tr = eng.run(initial_states=init, forced_actions=forced)
    torch.cuda.synchronize()
    assert int(tr.len.min()) == T                                     # nobody left the bounds: slot T - 1 holds the state after 49 steps
    last = tr.obs[:, T - 1, :].cpu().numpy().T.reshape(G, Eps, 20)
    ptab = eng.env_params.cpu().numpy().reshape(12, G, Eps)
    assert np.all(last == last[:, :1, :])                             # one group = one vehicle: identical states
    assert np.all(ptab == ptab[:, :, :1])
    for g in range(1, G):
        assert ptab[4, g, 0] != ptab[4, 0, 0] and ptab[3, g, 0] != ptab[3, 0, 0]
        assert float(np.abs(last[g, 0] - last[0, 0]).max()) > 1e-6    # other parameters: another state
