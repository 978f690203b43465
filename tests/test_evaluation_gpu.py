"""GPU: deterministic evaluation and parameter sweeps.

1. DeviceRollout.run(deterministic=True) on every rollout path: the recorded action is the actor's mean of the recorded observation
   (the fp64 bounds of tests/test_fused_rollout_fp64.py, with sigma = 0 and no draw), independent of the engine's seed, zero at
   masked steps; sampling engines -- the captured hipGraph included -- are left as they were.
2. tg_env_param_grid, tg_eval_tile_states, tg_eval_cells against the NumPy restatements of tests/evaluation_fp64.py, bit for bit.
3. Evaluator end to end, and a training run that an evaluation in its middle does not move by a bit."""
import ctypes as C

import numpy as np
import pytest
import torch

import evaluation_fp64 as EV
from test_fused_rollout_fp64 import (DIMS, actor_layers, bf16_mean_and_bound, check_actions, f32_mean_and_bound, make_env, sigmas,
                                     staggered_initial_states)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tg():
    import trajopt_grpo_amd as tg
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return tg


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def snapshot(tr):
    return [x.clone() for x in (tr.obs, tr.act, tr.rew, tr.mask, tr.len)]


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------------------------------------
# 1. mean-action rollouts on every path
# ------------------------------------------------------------------------------------------------------------------------------
PATHS = {"step": ("CartPole", (64, 64), None, dict(fused=False, use_graph=False), None),
         "f32x16": ("CartPole", (64, 64), None, dict(fused=True), 16),
         "f32x32": ("CartPole", (64, 64), None, dict(fused=True), 32),
         "bf16": ("QuadPole", (128, 128), torch.bfloat16, dict(fused=True), None)}
G, EPS, T = 3, 32, 32                                     # 96 envs: ragged against the 32- and 64-env tiles of every path


def _policy(tg, dev, path, variant):
    name, hidden, _, _, _ = PATHS[path]
    S, A = DIMS[name]
    torch.manual_seed(300 + len(path))
    pol = tg.GaussianActor_NeuralNetwork(S, A, hidden, cov=0.3, device=dev, **({"learn_std": True} if variant == "learn_std" else {}),
                                         **({"normalize_obs": True} if variant == "normalize_obs" else {}))
    if variant == "normalize_obs":                        # statistics that move every feature, and a clamp that bites somewhere
        g = torch.Generator().manual_seed(1)
        pol.obs_norm.set(torch.randn(S, generator=g) * 0.2, torch.rand(S, generator=g) * 2.0 + 0.05, 1000.0)
    return pol


def _engine(tg, dev, path, pol, seed, **over):
    name, _, cdt, kw, block = PATHS[path]
    eng = tg.DeviceRollout(make_env(tg, name, T), pol, G, EPS, seed=seed, compute_dtype=cdt, **{**kw, **over})
    if block is not None:
        eng.f32_block_envs = block
    return eng


def _mean_fn(path, pol):
    """fp64 mean and error bound of the path's actor on the recorded observation: the fused kernels' own bounds
    (test_fused_rollout_fp64); the per-step path (tg_mlp_f32_forward or a GEMM chain: fp32 products, K <= 32 padded inputs plus the
    bias summed in fp32 in some order) is covered by the fp32 bound with K1 = 32, which holds for any order."""
    name, _, _, _, _ = PATHS[path]
    S = DIMS[name][0]
    layers = actor_layers(pol)
    on = pol.obs_norm

    def prep(x):                                           # what the actor reads: the fp32 normalised observation when normalize_obs is on
        return x if on is None else on.normalize(x.float()).double()
    if path == "bf16":
        return lambda x: bf16_mean_and_bound(layers, prep(x))
    k1 = 32 if path == "step" else (S + 7) // 8 * 8
    return lambda x: f32_mean_and_bound(layers, prep(x), k1)


@pytest.mark.parametrize("variant", ["plain", "normalize_obs", "learn_std"])
@pytest.mark.parametrize("path", list(PATHS))
def test_deterministic_actions_are_the_actor_mean_on_every_path(tg, dev, path, variant):
    name = PATHS[path][0]
    A = DIMS[name][1]
    pol = _policy(tg, dev, path, variant)
    init = staggered_initial_states(tg, name, T, G, EPS, dev, seed=21)
    # a sampling engine first: its bits must be the same after the deterministic runs below
    sampler = _engine(tg, dev, path, pol, seed=5)
    before = snapshot(sampler.run(initial_states=init))
    one, two = _engine(tg, dev, path, pol, seed=11), _engine(tg, dev, path, pol, seed=77)
    assert one.fused == (path != "step") and (not one.fused or one._fused_f32 == (path != "bf16"))
    tr = one.run(initial_states=init, deterministic=True)
    first = snapshot(tr)
    assert sigmas(one) == [0.0] * A
    if path.startswith("f32"):
        assert one._frag.block_envs == PATHS[path][4]
    assert same(first, snapshot(two.run(initial_states=init, deterministic=True))), "a mean-action rollout depends on the seed"
    assert same(first, snapshot(one.run(initial_states=init, deterministic=True)))          # ... or on the stream id
    mask = tr.mask.bool()
    assert int((tr.len < T).sum()) > 0 and int((tr.len == T).sum()) > 0 and tr.n == 96      # the premise: ragged lengths
    assert not bool(tr.act[:, ~mask].any()), "actions recorded at masked steps"
    check_actions(tr, torch.zeros_like(tr.act), [0.0] * A, _mean_fn(path, pol), k_alive_min=2 * tr.n)
    assert not same(first, before)                                                       # (the sampled rollout is another one)
    # the sampler, replayed from its first stream id, draws what it drew before
    sampler._stream_host = 0
    sampler.rng[1].zero_()
    assert same(before, snapshot(sampler.run(initial_states=init)))
    assert sigmas(sampler) != [0.0] * A


def test_deterministic_run_leaves_the_captured_graph_alone(tg, dev):
    """use_graph=True bakes sigma into the capture: a deterministic run takes the plain per-step launches, gives the same
    trajectory as an engine without a graph, and the captured sampling graph replays as before."""
    pol = _policy(tg, dev, "step", "plain")
    eng = _engine(tg, dev, "step", pol, seed=31, use_graph=True)
    before = snapshot(eng.run())
    graph, baked = eng._graph, eng._graph_baked
    assert graph is not None
    init = before[0][:, 0, :].t().cpu().numpy()
    det = snapshot(eng.run(initial_states=init, deterministic=True))
    det_fresh = snapshot(eng.run(deterministic=True))                                    # no initial states: the graph's own condition
    assert eng._graph is graph and eng._graph_baked == baked
    plain = _engine(tg, dev, "step", pol, seed=32)
    assert same(det, snapshot(plain.run(initial_states=init, deterministic=True)))
    assert not bool(det_fresh[1][:, ~det_fresh[3].bool()].any())
    eng._stream_host = 0
    eng.rng[1].zero_()
    assert same(before, snapshot(eng.run())) and eng._graph is graph


# ------------------------------------------------------------------------------------------------------------------------------
# 2. the three entry points against their restatements
# ------------------------------------------------------------------------------------------------------------------------------
def _quadpole_grid(tg, dev, sweep, E, n, env_offset=0):
    K = tg.hip_ops
    env = tg.QuadPole(max_steps=24)
    p = env.native_params()
    values = torch.tensor([v for _, f in sweep for v in f], dtype=torch.float64, device=dev)
    grid = K.param_grid([i for i, _ in sweep], [len(f) for _, f in sweep], values, E)
    out = torch.full((12, n), -7.0, dtype=torch.float64, device=dev)
    K.env_param_grid(p, grid, out, env_offset)
    torch.cuda.synchronize()
    return out.cpu().numpy(), EV.grid_table(list(p.p), sweep, E, n, env_offset), p, grid


def test_param_grid_matches_the_restatement_bit_for_bit(tg, dev):
    mass, tether = tg.QuadPole.RANDOMIZABLE["mass"], tg.QuadPole.RANDOMIZABLE["tether_length"]
    sweep = [(mass, [0.8, 1.0, 1.25]), (tether, [0.5, 1.7])]
    got, want, p, _ = _quadpole_grid(tg, dev, sweep, 5, 30)
    assert np.array_equal(got, want)
    assert np.array_equal(got[:, 10:15], np.repeat(np.array(list(p.p))[:, None], 5, axis=1)[:, :5] * np.where(
        np.arange(12)[:, None] == tether, 0.5, 1.0))                                    # cell 2 = (mass x 1.0, tether x 0.5): nominal bits elsewhere
    listed_backwards, _, _, _ = _quadpole_grid(tg, dev, list(reversed(sweep)), 5, 30)
    assert np.array_equal(listed_backwards, want)                                        # p[] order decides, not the listing
    shard, want_shard, _, _ = _quadpole_grid(tg, dev, sweep, 5, 20, env_offset=10)
    assert np.array_equal(shard, want_shard) and np.array_equal(shard, want[:, 10:])
    one, want_one, _, _ = _quadpole_grid(tg, dev, [(mass, [1.0])], 7, 7)                 # a 1 x 1 grid of factor 1: the nominal table
    assert np.array_equal(one, want_one) and np.array_equal(one, np.repeat(np.array(list(p.p))[:, None], 7, axis=1))
    none, want_none, _, _ = _quadpole_grid(tg, dev, [], 8, 8)                              # nothing swept: one cell
    assert np.array_equal(none, want_none)


def test_param_grid_refusals_return_arg_errors_with_device_pointers(tg, dev):
    Nn = tg._native
    lib = Nn.load()
    _, _, p, grid = _quadpole_grid(tg, dev, [(0, [0.8, 1.25]), (3, [0.5, 1.0, 2.0])], 5, 30)
    out = torch.full((12, 30), -7.0, dtype=torch.float64, device=dev)
    st = Nn.stream_ptr(dev)

    def call(g, n=30, off=0, tab=out.data_ptr()):
        return lib.tg_env_param_grid(C.byref(p), C.byref(g), tab, n, off, st)

    def edited(**kw):
        g = Nn.ParamGrid.from_buffer_copy(grid)
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(g, k)[v[0]] = v[1]
            else:
                setattr(g, k, v)
        return g
    assert call(grid, tab=None) == Nn.TG_ERR_ARG
    for g in (edited(count=13), edited(count=-1), edited(index=(1, 12)), edited(index=(1, -1)), edited(index=(1, 0)), edited(levels=(0, 0)),
              edited(d_values=None), edited(episodes_per_cell=4), edited(episodes_per_cell=0)):
        assert call(g) == Nn.TG_ERR_ARG
    assert call(grid, n=35) == Nn.TG_ERR_ARG and call(grid, off=5) == Nn.TG_ERR_ARG and call(grid, off=-5) == Nn.TG_ERR_ARG
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()), "a refused call wrote the table"


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_tile_states_copies_cell_zero_and_nothing_else(tg, dev, dtype):
    S, A, Tt, Cc, E = 5, 1, 24, 4, 5
    n = Cc * E
    traj = tg.DeviceTrajectory(S, A, Tt, n, Cc, E, dtype, dev)
    g = torch.Generator().manual_seed(2)
    traj.obs.copy_(torch.randn(S, Tt + 1, n, generator=g, dtype=torch.float64).to(dtype))
    before = traj.obs.clone()
    tg.hip_ops.eval_tile_states(traj, E)
    torch.cuda.synchronize()
    slot0 = traj.obs[:, 0, :].reshape(S, Cc, E)
    assert torch.equal(slot0, before[:, 0, :E].unsqueeze(1).expand(S, Cc, E))
    assert torch.equal(traj.obs[:, 1:, :], before[:, 1:, :]) and torch.equal(traj.obs[:, 0, :E], before[:, 0, :E])
    tg.hip_ops.eval_tile_states(traj, n)                                                 # one cell: nothing to do
    with pytest.raises(RuntimeError, match="not a multiple"):
        tg.hip_ops.eval_tile_states(traj, 3)


def _synthetic(tg, dev, dtype, Cc, E, Tt, seed, empty_cell=None):
    n = Cc * E
    rng = np.random.default_rng(seed)
    rew = (rng.standard_normal((Tt, n)) * 40.0)
    rew = rew.astype(np.float32) if dtype == torch.float32 else rew
    length = rng.integers(-3, Tt + 1, n).astype(np.int32)                               # 0 and negatives: still running
    length[[0, 1, E, n - 1]] = [1, Tt, Tt, 1]
    length[2] = Tt + 1                                                                    # out of range: not counted
    if empty_cell is not None:
        length[empty_cell * E:(empty_cell + 1) * E] = rng.integers(-2, 1, E)
    timeout = rng.integers(0, 2, n).astype(np.uint8)
    traj = tg.DeviceTrajectory(3, 1, Tt, n, Cc, E, dtype, dev)
    traj.rew.copy_(torch.from_numpy(rew))
    traj.len.copy_(torch.from_numpy(length))
    return traj, rew, length, timeout


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("Cc,E,empty", [(3, 70, None), (3, 70, 1), (2, 700, None)], ids=["3x70", "3x70-empty-cell", "2x700"])
def test_eval_cells_match_the_restatement_bit_for_bit(tg, dev, dtype, Cc, E, empty):
    """E = 70: fewer episodes than partials; E = 700: every partial folds two or three episodes before the tree."""
    Tt = 37
    traj, rew, length, timeout = _synthetic(tg, dev, dtype, Cc, E, Tt, seed=Cc * E + (empty or 0), empty_cell=empty)
    to = torch.from_numpy(timeout).to(dev)
    obs_before, rew_before = traj.obs.clone(), traj.rew.clone()
    returns, cells = tg.hip_ops.eval_cells(traj, to, E)
    torch.cuda.synchronize()
    want_r = EV.episode_returns(rew, length)
    want_c = EV.cell_stats(want_r, length, timeout, E, Tt)
    got_r, got_c = returns.cpu().numpy(), cells.cpu().numpy()
    assert np.array_equal(got_r.view(np.int64), want_r.view(np.int64))
    assert np.array_equal(got_c.view(np.int64), want_c.view(np.int64)), (got_c, want_c)
    assert np.all(got_c[:, 6] + got_c[:, 7] == got_c[:, 0]) and np.all(got_c[:, 0] <= E)
    if empty is not None:
        # a cell with no ended episode: zero episodes and sums, and the identities of min and max (+inf, -inf)
        assert list(got_c[empty]) == [0.0, 0.0, 0.0, np.inf, -np.inf, 0.0, 0.0, 0.0]
        assert np.all(got_r[empty * E:(empty + 1) * E] == 0.0)
    assert torch.equal(traj.obs, obs_before) and torch.equal(traj.rew, rew_before)


# ------------------------------------------------------------------------------------------------------------------------------
# 3. Evaluator end to end
# ------------------------------------------------------------------------------------------------------------------------------
def test_sweep_of_ones_is_the_plain_deterministic_rollout(tg, dev):
    """Every factor 1.0: the `_dr` kernels read a table whose columns are the nominal p[] and must give the plain kernels'
    trajectory bit for bit, in every cell (all cells start from cell 0's states)."""
    Tt, E = 32, 24
    torch.manual_seed(7)
    pol = tg.GaussianActor_NeuralNetwork(20, 4, (64, 64), cov=0.3, device=dev)
    ev = tg.Evaluator(tg.QuadPole(max_steps=Tt), pol, episodes=E, sweep={"mass": [1.0, 1.0], "tether_length": [1.0, 1.0]}, seed=13)
    ev.evaluate()                                                                         # builds the engine
    ev.engine.f32_block_envs = 32
    ev.engine._frag = None
    res = ev.evaluate()
    tr = ev.engine.traj
    assert ev.engine.fused and ev.engine._fused_f32 and ev.engine.env_params is not None and tr.n == 4 * E
    plain = tg.DeviceRollout(tg.QuadPole(max_steps=Tt), pol, 1, E, seed=13)
    plain.f32_block_envs = 32
    pt = plain.run(deterministic=True)
    assert plain.env_params is None
    for c in range(4):
        sl = slice(c * E, (c + 1) * E)
        assert torch.equal(tr.obs[:, :, sl], pt.obs) and torch.equal(tr.act[:, :, sl], pt.act), c
        assert torch.equal(tr.rew[:, sl], pt.rew) and torch.equal(tr.len[sl], pt.len) and torch.equal(tr.mask[:, sl], pt.mask), c
    assert len({tuple(r) for r in res.returns.tolist()}) == 1                            # ... so every cell has the same returns
    assert all(row["episodes"] == E for row in res.table)


@pytest.mark.parametrize("name,sweep,randomize", [("QuadPole", {"mass": [0.7, 1.0, 1.4], "tether_length": [0.5, 2.0]}, None),
                                                 ("CartPole", None, {"masspole": (0.5, 2.0)}), ("Pendulum", {"length": [0.8, 1.25]}, None)],
                         ids=["quadpole-3x2", "cartpole-randomised", "pendulum-1x2"])
def test_evaluate_is_repeatable_and_counts_every_episode(tg, dev, name, sweep, randomize):
    Tt, E = 40, 33
    S, A = DIMS[name]
    torch.manual_seed(8)
    pol = tg.GaussianActor_NeuralNetwork(S, A, (64, 64), cov=0.3, device=dev)
    env = make_env(tg, name, Tt)
    if randomize:
        env.randomize(randomize, seed=4)
    ev = tg.Evaluator(env, pol, episodes=E, sweep=sweep, seed=17)
    a = ev.evaluate()
    first_params = None if ev.engine.env_params is None else ev.engine.env_params.clone()
    b = ev.evaluate()
    assert a.table == b.table and np.array_equal(a.returns, b.returns) and a.summary == b.summary
    assert np.array_equal(a.cells.view(np.int64), b.cells.view(np.int64))
    assert len(a.table) == ev.cells == a.returns.shape[0] and a.returns.shape[1] == E
    for row in a.table:
        assert row["episodes"] == E and 1.0 <= row["length_mean"] <= Tt
        assert abs(row["timeout_frac"] + row["early_frac"] - 1.0) < 1e-12 and row["return_min"] <= row["return_mean"] <= row["return_max"]
    assert np.all(a.cells[:, 6] + a.cells[:, 7] == E)
    assert a.summary["episodes"] == ev.cells * E and a.early_name == ("balanced" if name == "Pendulum" else "failure")
    tr = ev.engine.traj
    assert not bool(tr.act[:, ~tr.mask.bool()].any())
    # the per-episode returns are the f64 sums of the recorded rewards, and every cell started from cell 0's states
    want = EV.episode_returns(tr.rew.cpu().numpy(), tr.len.cpu().numpy())
    assert np.array_equal(a.returns.reshape(-1).view(np.int64), want.view(np.int64))
    slot0 = tr.obs[:, 0, :].reshape(S, ev.cells, E)
    assert torch.equal(slot0, slot0[:, :1, :].expand_as(slot0))
    if sweep:
        p = env.native_params()
        listing = [(env.RANDOMIZABLE[k], v) for k, v in sweep.items()]
        assert np.array_equal(ev.engine.env_params.cpu().numpy(), EV.grid_table(list(p.p), listing, E, ev.cells * E))
        assert [row["factors"] for row in a.table] == [a.factors(c) for c in range(ev.cells)]
    else:
        # one cell of randomly drawn vehicles, the same ones in both evaluations; the caller's env is as it was
        assert ev.cells == 1 and torch.equal(first_params, ev.engine.env_params) and env.randomization == randomize
        col = ev.engine.env_params[env.RANDOMIZABLE["masspole"]]
        assert len(torch.unique(col)) > E // 2 and float(col.min()) >= 0.5 * env.masspole and float(col.max()) <= 2.0 * env.masspole


def _train(tg, dev, with_eval):
    Tt = 32
    torch.manual_seed(5)
    pol = tg.GaussianActorCritic_NeuralNetwork(5, 1, (64, 64), cov=0.5, device=dev, normalize_obs=True, normalize_value=True)
    mgr = tg.RolloutManager(lambda: tg.CartPole(max_steps=Tt), pol, num_workers=4, num_episodes_per_worker=32, seed=9)
    buf = tg.Rollout_Buffer(mgr)
    opt = torch.optim.Adam(pol.parameters(), lr=2e-4)
    algo = tg.PPO(epsilon=0.2, policy=pol, optimizer=opt, ref_model=None, updates_per_iter=2, gamma=0.99, lam=0.95, batch_size=None,
                  seed=3)
    ev = tg.Evaluator(tg.CartPole(max_steps=Tt), pol, episodes=16, sweep={"masspole": [0.8, 1.25]}, seed=2) if with_eval else None
    for it in range(2):
        buf.sample()
        algo.learn(buf)
        if ev is not None and it == 0:
            res = ev.evaluate()
            assert all(row["episodes"] == 16 for row in res.table)
    torch.cuda.synchronize()
    state = {f"param.{k}": p.detach().clone() for k, p in enumerate(pol.parameters())}
    for k, p in enumerate(pol.parameters()):
        for key, v in opt.state[p].items():
            state[f"adam.{k}.{key}"] = v.detach().clone() if torch.is_tensor(v) else torch.tensor(float(v))
    for key, t in (("obs", pol.obs_norm), ("value", pol.value_norm)):
        for f in ("count", "mean", "m2", "table"):
            state[f"{key}_norm.{f}"] = getattr(t, f).detach().clone()
    state["traj.act"] = mgr.engine.traj.act.clone()
    state["rng"] = mgr.engine.rng.clone()
    return state


def test_an_evaluation_between_two_updates_moves_no_bit_of_the_training(tg, dev):
    """Two learn() calls of a CartPole PPO with running observation and value normalisation, with and without an evaluate() of the
    same policy in between: weights, Adam moments and step counts, both running statistics, the training engine's RNG stream and its
    second rollout are identical bit for bit."""
    a, b = _train(tg, dev, False), _train(tg, dev, True)
    assert set(a) == set(b) and any(k.startswith("adam.") and k.endswith("exp_avg") for k in a)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert float(a["obs_norm.count"]) > 0 and float(a["value_norm.count"]) > 0
