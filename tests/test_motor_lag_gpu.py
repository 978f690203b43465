"""The actuator lag on the MI355X (run with `-m gpu`): Env.motor_time_constant, a first-order rotor lag in front of every physics
step, on every rollout path.

The yardstick is the plain one-launch kernel (tg_rollout_forced, pinned to the reference's goldens elsewhere): a lagged rollout
with commanded actions a[t] must be, bit for bit, the plain rollout of the same env over its k T physics steps fed the FILTERED
commands -- the filter restated in NumPy float32 by tests/motor_lag_ref.py (held to an exact case and a rounding bound by
tests/test_motor_lag_cpu.py) -- and read at every k-th step.

  1. the identity through sampled tg_rollout_step_lag launches, f32 and f64, k in {1, 3}, n in {1, 65, 300};
  2. every path (fused bf16, fused fp32 at 16 and 32 envs per workgroup, ReLU and Tanh, the graph) replays itself through
     tg_rollout_forced_lag and through per-step forced launches;
  3. split fused launches compose, across compactions that move motor states between lanes;
  4. per-env time constants from the parameter table; a uniform table; rank shards;
  5. an obs-norm table on the fused paths;
  6. tg_rollout_final_state_lag and PPO's bootstrap;
  7. an Evaluator sweep over the time constant;
  8. the scalar Env.step();
  9. refusals: error codes, nothing launched."""
import ctypes as C

import numpy as np
import pytest
import torch

import domain_rand_fp64 as DR
import motor_lag_ref as ML
import substeps_ref as SR
from test_fused_rollout_fp64 import f32_policy
from test_tanh_gpu import tanh_policy

pytestmark = pytest.mark.gpu

ENVS = ("QuadPole2D", "QuadPole")
T = 16
TAU = 0.05
DT = 0.02
DTYPES = {"f32": torch.float32, "f64": torch.float64}
KEYS = ("obs", "rew", "mask", "len", "act", "motor")


@pytest.fixture(scope="module")
def tg():
    import trajopt_grpo_amd as tg
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return tg


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


# ------------------------------------------------------------------------------------------------------------------------------
# helpers
# ------------------------------------------------------------------------------------------------------------------------------
def lag_env(tg, name, horizon=T, k=1, tau=TAU):
    env = tg.environments.ENV_CLASSES[name](max_steps=horizon)
    env.substeps = k
    env.motor_time_constant = tau
    return env


def plain_env(tg, name, horizon):
    return tg.environments.ENV_CLASSES[name](max_steps=horizon)


def new_traj(tg, name, horizon, n, dtype, dev, s0, actions=None, motor=False):
    """A zeroed trajectory with slot 0 = s0 (n, S), the action planes = actions (n, horizon, A) and, with `motor`, a zeroed record."""
    S, A = SR.DIMS[name]
    Nn = tg._native
    tr = tg.rollout.DeviceTrajectory(S, A, horizon, n, 1, n, dtype, dev)
    with torch.cuda.device(dev):
        Nn.check(Nn.load().tg_rollout_begin(C.byref(tr.native()), S, A, Nn.stream_ptr(dev)), "tg_rollout_begin")
    tr.obs[:, 0, :].copy_(torch.as_tensor(np.asarray(s0)[:n], dtype=dtype).t().to(dev))
    if actions is not None:
        tr.act.copy_(torch.as_tensor(np.asarray(actions)[:n]).permute(2, 1, 0).to(dev))
    if motor:
        tr.motor = torch.zeros(A, horizon + 1, n, dtype=torch.float32, device=dev)
    return tr


def snap(tr):
    torch.cuda.synchronize()
    out = {"obs": tr.obs.clone(), "rew": tr.rew.clone(), "mask": tr.mask.clone(), "len": tr.len.clone(), "act": tr.act.clone()}
    if getattr(tr, "motor", None) is not None:
        out["motor"] = tr.motor.clone()
    return out


def bits(x):
    x = x.detach().cpu().contiguous().numpy() if isinstance(x, torch.Tensor) else np.ascontiguousarray(x)
    return x.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[x.dtype.itemsize])


def assert_same(got, want, what, keys=("obs", "rew", "mask", "len")):
    for key in keys:
        assert got[key].dtype == want[key].dtype and torch.equal(got[key], want[key]), f"{what}: {key} differs"
        if key == "motor":
            assert np.array_equal(bits(got[key]), bits(want[key])), f"{what}: motor differs in a sign of zero"


def decimated(plain, k, horizon=T):
    """tests/substeps_ref.decimate on the device tensors: the plain rollout of k T steps read at every k-th step."""
    obs, rew, mask, L = plain["obs"], plain["rew"], plain["mask"], plain["len"].long()
    out = {"obs": obs[:, ::k, :].contiguous(), "mask": mask[::k].contiguous(), "len": (-(-L // k)).int()}
    rs = torch.zeros(horizon, rew.shape[1], dtype=rew.dtype, device=rew.device)
    for t in range(horizon):
        acc = rew[t * k].clone()
        for j in range(1, k):
            acc = torch.where((t * k + j) < L, acc + rew[t * k + j], acc)      # sequential, in the trajectory dtype; executed calls only
        rs[t] = acc
    out["rew"] = rs
    return out


def check_against_plain(tg, dev, name, k, got, dtype, al, horizon=T, ptab=None, what=""):
    """The deciding comparison.  `got`: a lagged rollout's snapshot.  Its recorded commanded actions are filtered by the restatement
    (every physics step, as if no episode ended: the filter is causal), the plain one-launch kernel rolls the k T physics steps
    under them from the same initial states, and the lagged rollout must be that run read at every k-th step; its motor record must
    be the restatement's, gated by the physics steps the PLAIN run executed."""
    Nn, lib = tg._native, tg._native.load()
    n = got["len"].numel()
    act = got["act"].cpu().numpy()                                                # [A][T][n], zeros behind an episode's end
    cmds = ML.free_commands(act, al, k)                                           # [A][k T][n]
    s0 = got["obs"][:, 0, :].t().cpu().numpy()
    tr = new_traj(tg, name, k * horizon, n, dtype, dev, s0, np.ascontiguousarray(cmds.transpose(2, 1, 0)))
    p = plain_env(tg, name, k * horizon).native_params()
    with torch.cuda.device(dev):
        if ptab is None:
            Nn.check(lib.tg_rollout_forced(C.byref(p), C.byref(tr.native()), 0, k * horizon, Nn.stream_ptr(dev)), "tg_rollout_forced")
        else:
            Nn.check(lib.tg_rollout_forced_dr(C.byref(p), ptab.data_ptr(), C.byref(tr.native()), 0, k * horizon, Nn.stream_ptr(dev)),
                     "tg_rollout_forced_dr")
    plain = snap(tr)
    assert_same(got, decimated(plain, k, horizon), f"{what}: against the plain rollout of the filtered commands")
    executed = ML.executed_from_plain_len(plain["len"].cpu().numpy(), k, horizon)
    _, motor = ML.filter(act, al, k, executed)
    assert got["motor"].dtype == torch.float32 and tuple(got["motor"].shape) == motor.shape
    assert np.array_equal(bits(got["motor"]), bits(motor)), f"{what}: motor record against the restatement"
    assert not bool(got["motor"][:, 0, :].any())
    return plain


def run_step_lag(tg, name, k, n, dtype, dev, ptab=None, sigma=0.3, seed=7, tau=TAU):
    """T launches of tg_rollout_step_lag, SAMPLING around means equal to the pinned action set."""
    Nn, lib = tg._native, tg._native.load()
    S, A = SR.DIMS[name]
    means = torch.as_tensor(SR.forced_actions(name, SR.N_MAX, T)[:n]).to(dev)     # (n, T, A)
    tr = new_traj(tg, name, T, n, dtype, dev, SR.initial_states(name), motor=True)
    p, nat, st = lag_env(tg, name, T, k, tau).physics_params(), tr.native(), Nn.stream_ptr(dev)
    rng = torch.tensor([seed, 0], dtype=torch.int64, device=dev)
    sg = (C.c_float * A)(*([sigma] * A))
    table = None if ptab is None else ptab.data_ptr()
    with torch.cuda.device(dev):
        for t in range(T):
            m = means[:, t, :].contiguous()
            Nn.check(lib.tg_rollout_step_lag(C.byref(p), table, C.byref(nat), t, m.data_ptr(), A, sg, rng.data_ptr(), 0, k,
                                             tr.motor.data_ptr(), st), "tg_rollout_step_lag")
    return tr


# ------------------------------------------------------------------------------------------------------------------------------
# 1. the identity
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 65, 300])
@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("name", ENVS)
def test_lagged_rollout_is_the_plain_rollout_of_the_filtered_commands(tg, dev, name, k, dt, n):
    dtype = DTYPES[dt]
    got = snap(run_step_lag(tg, name, k, n, dtype, dev))
    plain = check_against_plain(tg, dev, name, k, got, dtype, ML.alpha(TAU, DT), what=f"{name} k={k} {dt} n={n}")
    assert torch.equal(got["mask"].sum(0).int(), got["len"])
    if n >= 65:                                                          # the case does what it was chosen for, on THIS run
        assert bool((got["len"] < T).any()) and bool((got["len"] == T).any())
        assert bool((got["act"].abs() > 1).any())                        # commands beyond [-1, 1]: the filter's clip is exercised
        if k > 1:
            assert bool((plain["len"] % k != 0).any())                   # an episode that stops inside a control step
        # the lag is felt: the same commands without it give another trajectory
        direct = snap(run_step_lag(tg, name, k, n, dtype, dev, tau=1e-12))
        assert torch.equal(direct["act"][:, 0, :], got["act"][:, 0, :]) and not torch.equal(direct["obs"][:, 1, :], got["obs"][:, 1, :])


# ------------------------------------------------------------------------------------------------------------------------------
# 2. every path agrees
# ------------------------------------------------------------------------------------------------------------------------------
PATHS = ["bf16", "f32x16", "f32x32", "tanh"]
SHAPES = {1: (1, 1), 65: (1, 65), 300: (3, 100)}                         # n -> groups, episodes per group


def path_policy(tg, dev, name, path, seed=5):
    S, A = SR.DIMS[name]
    if path == "tanh":
        return tanh_policy(tg, S, A, (128, 128), dev, seed)
    return f32_policy(tg, S, A, (128, 128), dev, seed)


def path_engine(tg, dev, name, path, G, Eps, k, pol, seed=11, horizon=T, env=None, **kw):
    env = lag_env(tg, name, horizon, k) if env is None else env
    eng = tg.DeviceRollout(env, pol, G, Eps, seed=seed, compute_dtype=torch.bfloat16 if path == "bf16" else None, fused=True, **kw)
    if path != "bf16":
        eng.f32_block_envs = 32 if path == "f32x32" else 16
    assert eng.fused and eng._fused_f32 == (path != "bf16")
    return eng


def replay(tg, dev, env, got, G, Eps, pol, per_step=False):
    """The recorded initial states and COMMANDED actions through tg_rollout_forced_lag, or launch by launch."""
    eng = tg.DeviceRollout(env, pol, G, Eps, seed=1, fused=False, use_graph=False)
    eng.forced_per_step = per_step
    tr = eng.run(initial_states=got["obs"][:, 0, :].t().cpu().numpy(), forced_actions=got["act"].permute(2, 1, 0).cpu().numpy())
    assert eng.lag and tr.motor is not None
    return snap(tr)


@pytest.mark.parametrize("n", [1, 65, 300])
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", ENVS)
def test_every_fused_path_replays_itself(tg, dev, name, path, n):
    G, Eps = SHAPES[n]
    k = 3 if path in ("bf16", "f32x16") else 1
    pol = path_policy(tg, dev, name, path)
    eng = path_engine(tg, dev, name, path, G, Eps, k, pol)
    got = snap(eng.run(initial_states=SR.initial_states(name)[:n]))
    assert eng.lag and eng.substeps == k and float(eng.params.p[10]) == TAU
    assert torch.equal(got["mask"].sum(0).int(), got["len"]) and not bool(got["motor"][:, 0, :].any())
    if n >= 65:
        assert bool((got["len"] < T).any()) and bool((got["len"] == T).any()) and bool(got["motor"].any())
    env = lag_env(tg, name, T, k)
    assert_same(replay(tg, dev, env, got, G, Eps, pol), got, f"{path}: one-launch replay", keys=KEYS)
    assert_same(replay(tg, dev, env, got, G, Eps, pol, per_step=True), got, f"{path}: launch-by-launch replay", keys=KEYS)
    # ... and, through the replay, the yardstick itself
    check_against_plain(tg, dev, name, k, got, torch.float32, ML.alpha(TAU, DT), what=f"{path} fused")


@pytest.mark.parametrize("name", ENVS)
def test_the_graph_path_is_the_eager_path(tg, dev, name):
    k, G, Eps = 3, 3, 100
    pol = f32_policy(tg, *SR.DIMS[name], (128, 128), dev, seed=8)

    def engine(**kw):
        return tg.DeviceRollout(lag_env(tg, name, T, k), pol, G, Eps, seed=21, fused=False, **kw)

    eager = snap(engine(use_graph=False).run())
    graph = engine(use_graph=True)
    assert_same(snap(graph.run()), eager, "hipGraph replay", keys=KEYS)
    assert graph._graph is not None and bool(eager["motor"].any())
    check_against_plain(tg, dev, name, k, eager, torch.float32, ML.alpha(TAU, DT), what="per-step sampled (DeviceRollout)")
    # a deterministic run takes the same entries with sigma = 0
    det = engine(use_graph=False)
    d = snap(det.run(initial_states=SR.initial_states(name)[:G * Eps], deterministic=True))
    assert_same(replay(tg, dev, lag_env(tg, name, T, k), d, G, Eps, pol), d, "deterministic: replay", keys=KEYS)


# ------------------------------------------------------------------------------------------------------------------------------
# 3. split launches and compaction
# ------------------------------------------------------------------------------------------------------------------------------
def edge_states(name, n):
    """Every even slot one step from the spatial bound with outward velocity (it leaves at step 1); every odd slot the env's own
    reset state, at rest in the middle."""
    from oracle import envs as OE
    rng = np.random.Generator(np.random.PCG64(77))
    s0 = np.array(OE.sample_initial_states(name, n, rng), dtype=np.float64)
    _, bound, _ = SR.PUSH[name]
    vel = {"QuadPole2D": 2, "QuadPole": 3}[name]
    s0[0::2, 0] = bound - 1e-3
    s0[0::2, vel] = 5.0
    return s0


@pytest.mark.parametrize("name", ENVS)
def test_split_fused_launches_compose_across_compactions(tg, dev, name):
    horizon, cut, n = 24, 11, 300
    pol = path_policy(tg, dev, name, "bf16")
    s0 = edge_states(name, n)
    whole = snap(path_engine(tg, dev, name, "bf16", 3, 100, 1, pol, horizon=horizon).run(initial_states=s0))
    eng = path_engine(tg, dev, name, "bf16", 3, 100, 1, pol, horizon=horizon)
    launch = eng._enqueue_fused

    def in_two(lo, hi):
        launch(lo, cut)
        eng.rng[1] -= 1                                                  # (each launch's epilogue advances the stream: one rollout, one stream)
        launch(cut, hi)

    eng._enqueue_fused = in_two
    split = snap(eng.run(initial_states=s0))
    assert_same(split, whole, "[0, 24) against [0, 11) + [11, 24)", keys=KEYS)
    # the construction holds: the even slots ended at step 1, so every compaction (steps 8 and 16, or 19) moved envs between lanes ...
    L, motor = whole["len"].cpu().numpy(), whole["motor"].cpu().numpy()
    assert np.all(L[0::2] == 1)
    # ... and every wave's 32 envs keep a live odd slot past step 8 whose motor state is not zero
    for lo in range(0, n, 32):
        odd = np.arange(lo + 1, min(lo + 32, n), 2)
        assert np.any((L[odd] > 8) & np.any(motor[:, 9, odd] != 0.0, axis=0)), lo
    check_against_plain(tg, dev, name, 1, whole, torch.float32, ML.alpha(TAU, DT), horizon=horizon, what="fused bf16 with compaction")


# ------------------------------------------------------------------------------------------------------------------------------
# 4. per-env time constants
# ------------------------------------------------------------------------------------------------------------------------------
MASS = {"QuadPole2D": "mq", "QuadPole": "mass"}


def randomized_env(tg, name, k):
    env = lag_env(tg, name, T, k)
    env.randomize({"motor_time_constant": (0.5, 2.0), MASS[name]: (0.8, 1.25)}, seed=3)
    return env


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("name", ENVS)
def test_per_env_time_constants(tg, dev, name, k):
    G, Eps, seed = 3, 100, 21
    n = G * Eps
    pol = f32_policy(tg, *SR.DIMS[name], (128, 128), dev, seed=8)
    env = randomized_env(tg, name, k)
    eng = tg.DeviceRollout(env, pol, G, Eps, seed=seed, fused=False, use_graph=False)
    got = snap(eng.run(initial_states=SR.initial_states(name)[:n]))
    tab = eng.env_params.clone()
    p = env.physics_params()
    spec = sorted(((env.parameter_slots()[key], lo, hi) for key, (lo, hi) in env.randomization.items()), key=lambda e: e[0])
    want = DR.table([p.p[i] for i in range(12)], spec, seed, 0, n, randomize_seed=3)
    assert np.array_equal(bits(tab), bits(want))                         # row 10 = tau times the drawn factor, like every other row
    tau_i = tab[10].cpu().numpy()
    assert np.all((tau_i >= 0.5 * TAU) & (tau_i <= 2.0 * TAU)) and len(np.unique(tau_i)) > n // 2
    al = ML.alpha(tau_i, DT)                                             # every env's own gain, from the table's bits
    check_against_plain(tg, dev, name, k, got, torch.float32, al, ptab=tab, what="per-env tau")
    # the fused paths read the same table: they replay themselves through the per-step entries with it
    for path in ("bf16", "f32x16"):
        fe = path_engine(tg, dev, name, path, G, Eps, k, pol, env=randomized_env(tg, name, k), seed=seed)
        fgot = snap(fe.run(initial_states=SR.initial_states(name)[:n]))
        assert np.array_equal(bits(fe.env_params), bits(want))
        check_against_plain(tg, dev, name, k, fgot, torch.float32, al, ptab=tab, what=f"per-env tau, fused {path}")


@pytest.mark.parametrize("name", ENVS)
def test_a_uniform_table_is_the_tableless_result(tg, dev, name):
    n, k, dtype = 65, 3, torch.float32
    p = lag_env(tg, name, T, k).physics_params()
    tab = torch.tensor([float(v) for v in p.p], dtype=torch.float64, device=dev).reshape(12, 1).repeat(1, n).contiguous()
    assert float(tab[10, 0]) == TAU
    want = snap(run_step_lag(tg, name, k, n, dtype, dev))
    assert_same(snap(run_step_lag(tg, name, k, n, dtype, dev, ptab=tab)), want, "uniform table, per step", keys=KEYS)


@pytest.mark.parametrize("path", ["bf16", "f32x16"])
def test_two_shards_are_the_whole_run(tg, dev, path):
    name, k, G, Eps = "QuadPole", 3, 4, 33
    pol = f32_policy(tg, 20, 4, (128, 128), dev, seed=8)
    s0 = SR.initial_states(name)[:G * Eps]

    def engine(groups, **kw):
        return path_engine(tg, dev, name, path, groups, Eps, k, pol, env=randomized_env(tg, name, k), **kw)

    whole_eng = engine(G)
    whole = snap(whole_eng.run(initial_states=s0))
    half = G // 2 * Eps
    parts, tabs = [], []
    for r in range(2):
        eng = engine(G // 2, group_offset=r * (G // 2), global_groups=G)
        parts.append(snap(eng.run(initial_states=s0[r * half:(r + 1) * half])))
        tabs.append(eng.env_params.clone())
    for key in KEYS:
        assert torch.equal(torch.cat([parts[0][key], parts[1][key]], dim=-1), whole[key]), key
    assert torch.equal(torch.cat(tabs, dim=-1), whole_eng.env_params)
    assert bool((whole["len"] < T).any()) and bool(whole["motor"].any())


# ------------------------------------------------------------------------------------------------------------------------------
# 5. an obs-norm table
# ------------------------------------------------------------------------------------------------------------------------------
def normed_policy(tg, dev, name):
    S, A = SR.DIMS[name]
    torch.manual_seed(6)
    pol = tg.GaussianActor_NeuralNetwork(S, A, (128, 128), cov=0.3, device=dev, normalize_obs=True, obs_clip=1.5)
    rng = np.random.Generator(np.random.PCG64(9))
    pol.obs_norm.set(rng.normal(0.0, 0.3, S), rng.uniform(0.5, 2.0, S), 1000)
    pol.obs_norm.freeze()
    return pol


@pytest.mark.parametrize("path", ["bf16", "f32x16", "f32x32"])
def test_fused_lag_with_an_obs_norm_table(tg, dev, path):
    name, k, G, Eps = "QuadPole", 3, 2, 65
    pol = normed_policy(tg, dev, name)
    s0 = SR.initial_states(name)[:G * Eps]
    got = snap(path_engine(tg, dev, name, path, G, Eps, k, pol).run(initial_states=s0))
    assert bool((got["len"] < T).any()) and bool((got["len"] == T).any())
    # the trajectory records the raw observation and the dynamics never see the table: the replay identity and the yardstick hold
    assert_same(replay(tg, dev, lag_env(tg, name, T, k), got, G, Eps, pol), got, f"{path} with obs norm: replay", keys=KEYS)
    check_against_plain(tg, dev, name, k, got, torch.float32, ML.alpha(TAU, DT), what=f"{path} with obs norm")
    plain_pol = f32_policy(tg, *SR.DIMS[name], (128, 128), dev, seed=6)
    plain_pol.actor.load_state_dict(pol.actor.state_dict())
    other = snap(path_engine(tg, dev, name, path, G, Eps, k, plain_pol).run(initial_states=s0))
    assert not torch.equal(other["act"], got["act"])                    # the table does reach the actor


# ------------------------------------------------------------------------------------------------------------------------------
# 6. the final state of the last control step, and PPO's bootstrap
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("name", ENVS)
def test_final_state_lag_is_the_next_slot_of_a_longer_clock(tg, dev, name, k):
    """An episode the clock ended at T: the state its last control step produced is slot T of the same rollout (same seed, same
    initial states: the same draws and means up to step T - 1) under a clock of T + 1 control steps, which carries on there."""
    G, Eps = 3, 100
    n = G * Eps
    pol = f32_policy(tg, *SR.DIMS[name], (128, 128), dev, seed=8)
    s0 = SR.initial_states(name)[:n]
    short = tg.DeviceRollout(lag_env(tg, name, T, k), pol, G, Eps, seed=21, fused=False, use_graph=False)
    tr = short.run(initial_states=s0)
    s_final, timeout = tg.hip_ops.rollout_final_state(short.params, tr, substeps=k, motor=tr.motor)
    longer = tg.DeviceRollout(lag_env(tg, name, T + 1, k), pol, G, Eps, seed=21, fused=False, use_graph=False)
    ref = snap(longer.run(initial_states=s0))
    torch.cuda.synchronize()
    clock = timeout.bool()
    assert torch.equal(clock, (tr.len == T) & (ref["len"] == T + 1)) and 0 < int(clock.sum()) < n
    assert torch.equal(tr.obs[:, :T, :], ref["obs"][:, :T, :]) and torch.equal(tr.motor[:, :T, :], ref["motor"][:, :T, :])
    want = ref["obs"][:, T, :].t()                                       # (n, S)
    assert np.array_equal(bits(s_final[clock]), bits(want[clock]))
    # without the motor record the re-step would start from the commanded action: another state
    plain_final, _ = tg.hip_ops.rollout_final_state(short.params, tr, substeps=k)
    assert not torch.equal(plain_final[clock], s_final[clock])


def test_ppo_bootstraps_a_lagged_env(tg, dev):
    torch.manual_seed(4)
    pol = tg.GaussianActorCritic_NeuralNetwork(10, 2, (64, 64), cov=0.5, device=dev)
    mgr = tg.RolloutManager(lambda: lag_env(tg, "QuadPole2D", 24, 2), pol, num_workers=4, num_episodes_per_worker=32, seed=9)
    buf = tg.Rollout_Buffer(mgr)
    algo = tg.PPO(epsilon=0.2, policy=pol, optimizer=torch.optim.Adam(pol.parameters(), lr=3e-4), ref_model=None, updates_per_iter=2,
                  gamma=0.99, batch_size=None, bootstrap_truncated=True)
    for _ in range(2):
        buf.sample()
        algo.learn(buf)
        tr = mgr.engine.traj
        _, timeout = tg.hip_ops.rollout_final_state(mgr.engine.params, tr, substeps=2, motor=tr.motor)
        assert algo.last_stats["n_bootstrapped"] == int(timeout.sum()) > 0
    assert mgr.engine.lag and all(bool(torch.isfinite(q).all()) for q in pol.parameters())


# ------------------------------------------------------------------------------------------------------------------------------
# 7. an Evaluator sweep
# ------------------------------------------------------------------------------------------------------------------------------
def test_evaluator_sweeps_the_time_constant(tg, dev):
    name, E = "QuadPole2D", 64
    pol = f32_policy(tg, 10, 2, (64, 64), dev, seed=3)
    env = lag_env(tg, name, T, 2)
    factors = [0.5, 1, 2]
    ev = tg.Evaluator(env, pol, episodes=E, seed=2, sweep={"motor_time_constant": factors})
    res = ev.evaluate()
    tab = ev.engine.env_params.cpu().numpy()
    assert ev.cells == 3 and np.array_equal(tab[10], np.repeat(np.array([TAU * f for f in factors]), E))
    p = env.physics_params()
    assert all(np.all(tab[r] == p.p[r]) for r in range(12) if r != 10)
    swept = snap(ev.engine.traj)
    one = tg.Evaluator(env, pol, episodes=E, seed=2)
    ref = one.evaluate()
    unswept = snap(one.engine.traj)
    assert np.array_equal(bits(res.returns[1]), bits(ref.returns[0]))   # the factor-1 cell is the unswept evaluation
    for key in KEYS:
        assert torch.equal(swept[key][..., E:2 * E], unswept[key]), key
    assert not np.array_equal(res.returns[0], res.returns[1]) and not np.array_equal(res.returns[2], res.returns[1])
    # a training run beside the evaluator is what it is without one
    a = snap(tg.DeviceRollout(lag_env(tg, name, T, 2), pol, 2, 20, seed=5, fused=False, use_graph=False).run())
    ev.evaluate()
    b = snap(tg.DeviceRollout(lag_env(tg, name, T, 2), pol, 2, 20, seed=5, fused=False, use_graph=False).run())
    assert_same(a, b, "a training rollout beside an evaluation", keys=KEYS)


# ------------------------------------------------------------------------------------------------------------------------------
# 8. the scalar API
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("name", ENVS)
def test_scalar_env_step_follows_the_restatement(tg, dev, name, k):
    Nn, lib = tg._native, tg._native.load()
    steps, n = 8, 4
    acts = SR.forced_actions(name, SR.N_MAX, steps)
    tr = new_traj(tg, name, steps, n, torch.float64, dev, SR.initial_states(name), acts, motor=True)
    p = lag_env(tg, name, steps, k).physics_params()
    with torch.cuda.device(dev):
        Nn.check(lib.tg_rollout_forced_lag(C.byref(p), None, C.byref(tr.native()), 0, steps, k, tr.motor.data_ptr(), Nn.stream_ptr(dev)),
                 "tg_rollout_forced_lag")
    got = snap(tr)
    check_against_plain(tg, dev, name, k, got, torch.float64, ML.alpha(TAU, DT), horizon=steps, what="tg_rollout_forced_lag, f64")
    al = ML.alpha(TAU, DT)
    for i in range(n):
        env = lag_env(tg, name, steps, k)
        env.set_state(SR.initial_states(name)[i])
        L = int(got["len"][i])
        m = np.zeros(SR.DIMS[name][1], np.float32)
        for t in range(L):
            obs, r, _, trunc, _ = env.step(acts[i, t])
            c = np.clip(acts[i, t], np.float32(-1), np.float32(1))
            for _ in range(k if t + 1 < L else 0):
                m = ML.filter_step(m, c, al)
            assert r == float(got["rew"][t, i]) and trunc == (t + 1 == L)
            if t + 1 < L:
                assert np.array_equal(obs, got["obs"][:, t + 1, i].cpu().numpy())
                assert np.array_equal(bits(env._motor), bits(m)) and np.array_equal(bits(m), bits(got["motor"][:, t + 1, i]))
        env.restart()
        assert env._motor is None                                        # m = 0 again at the reset
    assert int(got["len"].max()) >= 2                                    # (a motor state was compared)


# ------------------------------------------------------------------------------------------------------------------------------
# 9. refusals
# ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(tg, dev):
    Nn, lib = tg._native, tg._native.load()
    name, n = "QuadPole", 65
    tr = new_traj(tg, name, T, n, torch.float32, dev, SR.initial_states(name), SR.forced_actions(name, SR.N_MAX, T), motor=True)
    cart = new_traj(tg, "CartPole", T, n, torch.float32, dev, SR.initial_states("CartPole"), SR.forced_actions("CartPole", SR.N_MAX, T), motor=True)
    before, before_cart = snap(tr), snap(cart)
    st = Nn.stream_ptr(dev)
    good = lag_env(tg, name, T).physics_params()
    off = lag_env(tg, name, T).physics_params()
    off.p[10] = 0.0
    cp = tg.CartPole(max_steps=T).native_params()
    cp.p[10] = TAU
    s_final, timeout = torch.zeros(n, 20, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev)
    cases = [(cp, cart, cart.motor.data_ptr(), Nn.TG_ERR_UNSUPPORTED), (good, tr, None, Nn.TG_ERR_ARG), (off, tr, tr.motor.data_ptr(), Nn.TG_ERR_ARG)]
    with torch.cuda.device(dev):
        for p, t, motor, code in cases:
            nat = t.native()
            assert lib.tg_rollout_step_lag(C.byref(p), None, C.byref(nat), 0, None, 0, None, None, 0, 1, motor, st) == code
            assert lib.tg_rollout_forced_lag(C.byref(p), None, C.byref(nat), 0, T, 1, motor, st) == code
            assert lib.tg_rollout_final_state_lag(C.byref(p), None, C.byref(nat), s_final.data_ptr(), timeout.data_ptr(), 1, motor, st) == code
    assert_same(snap(tr), before, "a refused call", keys=KEYS)
    assert_same(snap(cart), before_cart, "a refused call (CartPole)", keys=KEYS)
    assert not bool(s_final.any()) and not bool(timeout.any())
    # through the public surface: an env whose attribute was forced past the setter is refused by the library
    pol = f32_policy(tg, 5, 1, (128, 128), dev, seed=9)
    env = tg.CartPole(max_steps=T)
    env._motor_tau = TAU
    eng = tg.DeviceRollout(env, pol, 2, 4, seed=1)
    with pytest.raises(RuntimeError, match="no rotors"):
        eng.run()
    torch.cuda.synchronize()
    assert not bool(eng.traj.mask.any())
    # and with the lag off nothing of it exists
    eng = tg.DeviceRollout(tg.QuadPole2D(max_steps=T), f32_policy(tg, 10, 2, (128, 128), dev, seed=9), 2, 4, seed=1)
    assert eng.run().motor is None and not eng.lag
