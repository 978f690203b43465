"""Control decimation on the MI355X (run with `-m gpu`): Env.substeps = k physics steps per policy step, on every rollout path.

The yardstick is the plain per-step kernel (tg_rollout_step, pinned to the reference's goldens elsewhere): a rollout with
substeps = k, horizon T and forced actions a[t] must be, bit for bit, the plain rollout of the same env with max_steps = k T driven
with a[p // k] at physics step p and read at every k-th step (tests/substeps_ref.py states the rule over the oracle and pins the
cases; tests/test_substeps_cpu.py holds the conditions on them).

  1. the identity through tg_rollout_step_sub (forced, and with given means) and tg_rollout_forced_sub, f32 and f64, n in {1, 65, 300};
  2. tg_rollout_final_state_sub against tg_rollout_final_state on that plain run;
  3. k = 1 through every `_sub` entry equals the sibling entry (the fused ones in sampling mode with the same seed);
  4. the fused bf16 / fp32 kernels at k > 1: the sampled trajectory replays itself through tg_rollout_forced_sub, and its actions
     meet the fp64 bound of tests/test_fused_rollout_fp64.py on the recorded observations;
  5. composition with a parameter table, an obs-norm table and rank shards;
  6. DeviceRollout on every path through the public Env.substeps, an Evaluator run, PPO(bootstrap_truncated=True);
  7. refusals: error codes and ValueErrors, nothing launched."""
import ctypes as C

import numpy as np
import pytest
import torch

import substeps_ref as SR
from test_fused_rollout_fp64 import (actor_layers, bf16_mean_and_bound, check_actions, f32_mean_and_bound, f32_policy, philox_draws,
                                     sigmas)
from test_tanh_gpu import f32_tanh_mean_and_bound, tanh_policy

pytestmark = pytest.mark.gpu

T = SR.T
KS = SR.KS
DTYPES = {"f32": torch.float32, "f64": torch.float64}


@pytest.fixture(scope="module")
def tg():
    import trajopt_grpo_amd as tg
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return tg


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


# ------------------------------------------------------------------------------------------------------------------------------
# helpers: hand-driven trajectories
# ------------------------------------------------------------------------------------------------------------------------------
def env_of(tg, name, horizon, k=1, fine=False):
    """fine: the physics step is timestep / k -- the control period stays 0.02 s, as a user refining the integration would set it (a
    sampled rollout under a random policy then lasts as long as at k = 1, and some episodes still reach the horizon)."""
    env = tg.environments.ENV_CLASSES[name](max_steps=horizon)
    env.substeps = k
    if fine:
        env.timestep = env.timestep / k
    return env


def new_traj(tg, name, horizon, n, dtype, dev, s0, actions):
    """A zeroed trajectory with slot 0 = s0 (n, S) and the action planes = actions (n, horizon, A)."""
    S, A = SR.DIMS[name]
    Nn = tg._native
    tr = tg.rollout.DeviceTrajectory(S, A, horizon, n, 1, n, dtype, dev)
    with torch.cuda.device(dev):
        Nn.check(Nn.load().tg_rollout_begin(C.byref(tr.native()), S, A, Nn.stream_ptr(dev)), "tg_rollout_begin")
    tr.obs[:, 0, :].copy_(torch.as_tensor(s0[:n], dtype=dtype).t().to(dev))
    if actions is not None:
        tr.act.copy_(torch.as_tensor(actions[:n]).permute(2, 1, 0).to(dev))
    return tr


def snap(tr):
    torch.cuda.synchronize()
    return {"obs": tr.obs.clone(), "rew": tr.rew.clone(), "mask": tr.mask.clone(), "len": tr.len.clone(), "act": tr.act.clone()}


def plain_run(tg, name, k, n, dtype, dev, ptab=None):
    """The yardstick: tg_rollout_step (tg_rollout_step_dr with a table) over k T steps under the held actions."""
    Nn, lib = tg._native, tg._native.load()
    P = k * T
    tr = new_traj(tg, name, P, n, dtype, dev, SR.initial_states(name), SR.hold(SR.forced_actions(name), k))
    p, nat, st = env_of(tg, name, P).native_params(), tr.native(), Nn.stream_ptr(dev)
    with torch.cuda.device(dev):
        for t in range(P):
            if ptab is None:
                Nn.check(lib.tg_rollout_step(C.byref(p), C.byref(nat), t, None, 0, None, None, 0, st), "tg_rollout_step")
            else:
                Nn.check(lib.tg_rollout_step_dr(C.byref(p), ptab.data_ptr(), C.byref(nat), t, None, 0, None, None, 0, st), "tg_rollout_step_dr")
    return tr


_PLAIN = {}


def plain_cached(tg, name, k, n, dtype, dev):
    """One yardstick run per (env, k, n, dtype), shared by the tests and left unchanged."""
    key = (name, k, n, dtype)
    if key not in _PLAIN:
        tr = plain_run(tg, name, k, n, dtype, dev)
        _PLAIN[key] = (tr, snap(tr))
    return _PLAIN[key]


def decimated(plain, k):
    """substeps_ref.decimate on the device tensors ([.][time][env] layout): what the substepped rollout must hold."""
    obs, rew, mask, L = plain["obs"], plain["rew"], plain["mask"], plain["len"].long()
    out = {"obs": obs[:, ::k, :].contiguous(), "mask": mask[::k].contiguous(), "len": (-(-L // k)).int()}
    rs = torch.zeros(T, rew.shape[1], dtype=rew.dtype, device=rew.device)
    for t in range(T):
        acc = rew[t * k].clone()
        for j in range(1, k):
            acc = torch.where((t * k + j) < L, acc + rew[t * k + j], acc)      # sequential, in the trajectory dtype; executed calls only
        rs[t] = acc
    out["rew"] = rs
    return out


def assert_same(got, want, what, keys=("obs", "rew", "mask", "len")):
    for key in keys:
        assert got[key].dtype == want[key].dtype and torch.equal(got[key], want[key]), f"{what}: {key} differs"


def sub_params(tg, name, k):
    return env_of(tg, name, T, k).physics_params()


def run_step_sub(tg, name, k, n, dtype, dev, ptab=None, means=False):
    """T launches of tg_rollout_step_sub: teacher-forced, or (means) sampling with sigma = 0 around means equal to the actions."""
    Nn, lib = tg._native, tg._native.load()
    S, A = SR.DIMS[name]
    acts = SR.forced_actions(name)
    tr = new_traj(tg, name, T, n, dtype, dev, SR.initial_states(name), None if means else acts)
    p, nat, st = sub_params(tg, name, k), tr.native(), Nn.stream_ptr(dev)
    table = None if ptab is None else ptab.data_ptr()
    rng = torch.tensor([7, 0], dtype=torch.int64, device=dev)
    zero = (C.c_float * A)(*([0.0] * A))
    mean = torch.as_tensor(acts[:n]).to(dev)                            # (n, T, A)
    with torch.cuda.device(dev):
        for t in range(T):
            if means:
                m = mean[:, t, :].contiguous()
                Nn.check(lib.tg_rollout_step_sub(C.byref(p), table, C.byref(nat), t, m.data_ptr(), A, zero, rng.data_ptr(), 0, k, st),
                         "tg_rollout_step_sub")
            else:
                Nn.check(lib.tg_rollout_step_sub(C.byref(p), table, C.byref(nat), t, None, 0, None, None, 0, k, st), "tg_rollout_step_sub")
    return tr


def run_forced_sub(tg, name, k, n, dtype, dev, ptab=None, split=None):
    Nn, lib = tg._native, tg._native.load()
    tr = new_traj(tg, name, T, n, dtype, dev, SR.initial_states(name), SR.forced_actions(name))
    p, nat, st = sub_params(tg, name, k), tr.native(), Nn.stream_ptr(dev)
    table = None if ptab is None else ptab.data_ptr()
    with torch.cuda.device(dev):
        for lo, hi in ([(0, T)] if split is None else [(0, split), (split, T)]):
            Nn.check(lib.tg_rollout_forced_sub(C.byref(p), table, C.byref(nat), lo, hi, k, st), "tg_rollout_forced_sub")
    return tr


# ------------------------------------------------------------------------------------------------------------------------------
# 1. the identity
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 65, 300])
@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", SR.ENVS)
def test_substepped_rollout_is_the_plain_rollout_read_at_every_kth_step(tg, dev, name, k, dt, n):
    dtype = DTYPES[dt]
    _, plain = plain_cached(tg, name, k, n, dtype, dev)
    if n >= 65:                                                          # the cases do what they were chosen for, on THIS run's lengths
        early, mid, full = SR.ending_shares(plain["len"].cpu().numpy(), k)
        assert early >= 0.25 and full >= 1 and (k == 1 or mid >= 0.125), (early, mid, full)
    want = decimated(plain, k)
    assert_same(snap(run_step_sub(tg, name, k, n, dtype, dev)), want, "tg_rollout_step_sub (forced)")
    got = snap(run_step_sub(tg, name, k, n, dtype, dev, means=True))
    assert_same(got, want, "tg_rollout_step_sub (means, sigma 0)")
    acts = torch.as_tensor(SR.forced_actions(name)[:n]).permute(2, 1, 0).to(dev)
    alive = want["mask"].bool()
    assert torch.equal(got["act"][:, alive], acts[:, alive]) and not bool(got["act"][:, ~alive].any())
    assert_same(snap(run_forced_sub(tg, name, k, n, dtype, dev)), want, "tg_rollout_forced_sub")
    assert_same(snap(run_forced_sub(tg, name, k, n, dtype, dev, split=11)), want, "tg_rollout_forced_sub in two launches")
    assert torch.equal(want["mask"].sum(0).int(), want["len"])


# ------------------------------------------------------------------------------------------------------------------------------
# 2. the final state of the last control step
# ------------------------------------------------------------------------------------------------------------------------------
def final_plain(tg, name, k, tr_plain, dev):
    return tg.hip_ops.rollout_final_state(env_of(tg, name, k * T).native_params(), tr_plain)


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", SR.ENVS)
def test_final_state_sub_is_the_plain_final_state(tg, dev, name, k, dt):
    n, dtype = 300, DTYPES[dt]
    tr_plain, plain = plain_cached(tg, name, k, n, dtype, dev)
    s_ref, to_ref = final_plain(tg, name, k, tr_plain, dev)
    tr = run_forced_sub(tg, name, k, n, dtype, dev)
    s_got, to_got = tg.hip_ops.rollout_final_state(sub_params(tg, name, k), tr, substeps=k)
    torch.cuda.synchronize()
    assert torch.equal(s_got, s_ref) and torch.equal(to_got, to_ref)
    assert 0 < int(to_ref.sum()) < n                                    # both ends of the classification occur
    assert_same(snap(tr_plain), plain, "the yardstick is left unchanged")


# ------------------------------------------------------------------------------------------------------------------------------
# 3. k = 1 through every `_sub` entry
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("name", SR.ENVS)
def test_one_substep_through_the_per_step_sub_entries_is_the_sibling(tg, dev, name, dt):
    n, dtype = 300, DTYPES[dt]
    tr_plain, plain = plain_cached(tg, name, 1, n, dtype, dev)
    assert_same(snap(run_step_sub(tg, name, 1, n, dtype, dev)), plain, "tg_rollout_step_sub, k = 1")
    tr = run_forced_sub(tg, name, 1, n, dtype, dev)
    assert_same(snap(tr), plain, "tg_rollout_forced_sub, k = 1")
    # ... and against the sibling's own one-launch replay
    Nn = tg._native
    sib = new_traj(tg, name, T, n, dtype, dev, SR.initial_states(name), SR.forced_actions(name))
    with torch.cuda.device(dev):
        Nn.check(Nn.load().tg_rollout_forced(C.byref(env_of(tg, name, T).native_params()), C.byref(sib.native()), 0, T, Nn.stream_ptr(dev)),
                 "tg_rollout_forced")
    assert_same(snap(tr), snap(sib), "tg_rollout_forced_sub against tg_rollout_forced")
    s_ref, to_ref = final_plain(tg, name, 1, tr_plain, dev)
    s_got, to_got = (x.clone() for x in tg.hip_ops.rollout_final_state(sub_params(tg, name, 1), tr, substeps=1))
    p1 = sub_params(tg, name, 1)
    s_sub, to_sub = torch.empty_like(s_ref), torch.empty_like(to_ref)
    with torch.cuda.device(dev):
        Nn.check(Nn.load().tg_rollout_final_state_sub(C.byref(p1), None, C.byref(tr.native()), s_sub.data_ptr(), to_sub.data_ptr(), 1,
                                                      Nn.stream_ptr(dev)), "tg_rollout_final_state_sub")
    torch.cuda.synchronize()
    assert torch.equal(s_got, s_ref) and torch.equal(to_got, to_ref) and torch.equal(s_sub, s_ref) and torch.equal(to_sub, to_ref)


def force_sub_entry(monkeypatch, tg):
    """DeviceRollout picks the `_sub` entry with substeps = 1 (what it never does by itself): the fused launches of the engine go
    through tg_fused_rollout_sub / tg_fused_rollout_f32_sub with every other argument unchanged."""
    def entry(f32, act, ptab, obs_norm, substeps=1):
        base = "tg_fused_rollout_f32" if f32 else "tg_fused_rollout"
        return base + "_sub", (ptab,), ((act,) if f32 else ()) + (tuple(obs_norm) if obs_norm is not None else (None, 0.0)) + (1,)
    monkeypatch.setattr(tg.rollout, "fused_entry", entry)


FUSED = [("bf16", None, 2, 65), ("f32", 16, 2, 20), ("f32", 32, 2, 20)]           # kind, envs per workgroup, groups, episodes per group


def fused_engine(tg, dev, name, kind, block, G, Eps, k, pol, seed=11, **kw):
    eng = tg.DeviceRollout(env_of(tg, name, T, k, fine=True), pol, G, Eps, seed=seed,
                           compute_dtype=torch.bfloat16 if kind == "bf16" else None, fused=True, **kw)
    if kind != "bf16":
        eng.f32_block_envs = block
    assert eng.fused and eng._fused_f32 == (kind != "bf16")
    return eng


def fused_policy(tg, dev, name, kind, tanh=False, seed=5):
    S, A = SR.DIMS[name]
    hidden = (256, 256) if kind == "bf16" else (128, 128)
    return tanh_policy(tg, S, A, hidden, dev, seed) if tanh else f32_policy(tg, S, A, hidden, dev, seed)


@pytest.mark.parametrize("kind,block,G,Eps", FUSED, ids=["bf16", "f32x16", "f32x32"])
@pytest.mark.parametrize("name", SR.ENVS)
def test_one_substep_through_the_fused_sub_entries_is_the_sibling(tg, dev, monkeypatch, name, kind, block, G, Eps):
    pol = fused_policy(tg, dev, name, kind)
    s0 = SR.initial_states(name)[:G * Eps]
    ref = snap(fused_engine(tg, dev, name, kind, block, G, Eps, 1, pol).run(initial_states=s0))
    force_sub_entry(monkeypatch, tg)
    got = snap(fused_engine(tg, dev, name, kind, block, G, Eps, 1, pol).run(initial_states=s0))
    assert_same(got, ref, "fused `_sub`, k = 1, sampling", keys=("obs", "rew", "mask", "len", "act"))
    assert bool((ref["len"] < T).any()) and bool((ref["len"] == T).any())


# ------------------------------------------------------------------------------------------------------------------------------
# 4. the fused kernels at k > 1
# ------------------------------------------------------------------------------------------------------------------------------
def replay(tg, dev, name, k, sampled, G, Eps, pol, ranges_env=None, env_params=None):
    """The recorded initial states and actions through tg_rollout_forced_sub (DeviceRollout's one-launch teacher-forced path)."""
    env = env_of(tg, name, T, k, fine=True) if ranges_env is None else ranges_env
    eng = tg.DeviceRollout(env, pol, G, Eps, seed=1, fused=False, use_graph=False)
    n = G * Eps
    tr = eng.run(initial_states=sampled["obs"][:, 0, :].t().cpu().numpy(), forced_actions=sampled["act"].permute(2, 1, 0).cpu().numpy())
    assert eng.substeps == k
    return snap(tr)


def check_fused(tg, dev, name, kind, block, G, Eps, k, tanh=False):
    S, A = SR.DIMS[name]
    pol = fused_policy(tg, dev, name, kind, tanh)
    eng = fused_engine(tg, dev, name, kind, block, G, Eps, k, pol)
    tr = eng.run(initial_states=SR.initial_states(name)[:G * Eps])
    got = snap(tr)
    assert eng.substeps == k and int(eng.params.max_steps) == k * T and eng.params.timestep == 0.02 / k
    assert bool((got["len"] < T).any()) and bool((got["len"] == T).any()) and torch.equal(got["mask"].sum(0).int(), got["len"])
    # the dynamics: the sampled trajectory replays itself
    assert_same(replay(tg, dev, name, k, got, G, Eps, pol), got, f"{kind} fused rollout, k = {k}: teacher-forced replay")
    # the actor: one evaluation per CONTROL step on the recorded observation, with the (env, t) draw
    eps = philox_draws(tg, env_of(tg, name, T), pol, G, Eps, 11, dev)
    layers = actor_layers(pol)
    if kind == "bf16":
        mean_fn = lambda x: bf16_mean_and_bound(layers, x)
    elif tanh:
        mean_fn = lambda x: f32_tanh_mean_and_bound(layers, x, (S + 7) // 8 * 8)
    else:
        mean_fn = lambda x: f32_mean_and_bound(layers, x, (S + 7) // 8 * 8)
    check_actions(tr, eps, sigmas(eng), mean_fn, k_alive_min=G * Eps * 2)


@pytest.mark.parametrize("k", [2, 3, 5])
@pytest.mark.parametrize("name", SR.ENVS)
def test_fused_bf16_with_substeps(tg, dev, name, k):
    check_fused(tg, dev, name, "bf16", None, 2, 65, k)                  # n = 130: two partly filled 128-env workgroups


@pytest.mark.parametrize("block", [16, 32])
@pytest.mark.parametrize("k", [2, 3, 5])
@pytest.mark.parametrize("name", SR.ENVS)
def test_fused_f32_with_substeps(tg, dev, name, k, block):
    check_fused(tg, dev, name, "f32", block, 2, 20, k)                  # n = 40: ragged last workgroup at both block sizes


@pytest.mark.parametrize("block", [16, 32])
@pytest.mark.parametrize("name", SR.ENVS)
def test_fused_f32_tanh_with_substeps(tg, dev, name, block):
    check_fused(tg, dev, name, "f32", block, 2, 20, 3, tanh=True)


# ------------------------------------------------------------------------------------------------------------------------------
# 5. composition
# ------------------------------------------------------------------------------------------------------------------------------
def drawn_table(tg, name, n, dev):
    """A per-env parameter table: every randomisable parameter scaled by a factor of [0.7, 1.4], drawn by tg_env_randomize."""
    Nn = tg._native
    env = env_of(tg, name, T)
    env.randomize({key: (0.7, 1.4) for key in env.RANDOMIZABLE}, seed=3)
    spec, p = env.randomize_spec(), env.native_params()
    tab = torch.empty(12, n, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        Nn.check(Nn.load().tg_env_randomize(C.byref(p), C.byref(spec), tab.data_ptr(), n, 5, 0, 0, 1, Nn.stream_ptr(dev)), "tg_env_randomize")
    return tab


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("k", [2, 3, 5])
@pytest.mark.parametrize("name", SR.ENVS)
def test_identity_with_a_parameter_table(tg, dev, name, k, dt):
    n, dtype = 65, DTYPES[dt]
    tab = drawn_table(tg, name, n, dev)
    plain = snap(plain_run(tg, name, k, n, dtype, dev, ptab=tab))
    assert not torch.equal(plain["obs"], plain_cached(tg, name, k, n, dtype, dev)[1]["obs"])      # the vehicles do differ
    want = decimated(plain, k)
    assert_same(snap(run_step_sub(tg, name, k, n, dtype, dev, ptab=tab)), want, "tg_rollout_step_sub with a table")
    tr = run_forced_sub(tg, name, k, n, dtype, dev, ptab=tab)
    assert_same(snap(tr), want, "tg_rollout_forced_sub with a table")
    tr_plain = plain_run(tg, name, k, n, dtype, dev, ptab=tab)
    s_ref, to_ref = tg.hip_ops.rollout_final_state(env_of(tg, name, k * T).native_params(), tr_plain, env_params=tab)
    s_got, to_got = tg.hip_ops.rollout_final_state(sub_params(tg, name, k), tr, env_params=tab, substeps=k)
    torch.cuda.synchronize()
    assert torch.equal(s_got, s_ref) and torch.equal(to_got, to_ref)


@pytest.mark.parametrize("name", SR.ENVS)
def test_a_uniform_table_is_the_tableless_result(tg, dev, name):
    n, k, dtype = 65, 3, torch.float32
    p = sub_params(tg, name, k)
    tab = torch.tensor([float(v) for v in p.p], dtype=torch.float64, device=dev).reshape(12, 1).repeat(1, n).contiguous()
    want = decimated(plain_cached(tg, name, k, n, dtype, dev)[1], k)
    assert_same(snap(run_step_sub(tg, name, k, n, dtype, dev, ptab=tab)), want, "uniform table, per step")
    assert_same(snap(run_forced_sub(tg, name, k, n, dtype, dev, ptab=tab)), want, "uniform table, one launch")


def normed_policy(tg, dev, name, kind):
    S, A = SR.DIMS[name]
    torch.manual_seed(6)
    pol = tg.GaussianActor_NeuralNetwork(S, A, (256, 256) if kind == "bf16" else (128, 128), cov=0.3, device=dev, normalize_obs=True,
                                         obs_clip=1.5)
    rng = np.random.Generator(np.random.PCG64(9))
    pol.obs_norm.set(rng.normal(0.0, 0.3, S), rng.uniform(0.5, 2.0, S), 1000)
    pol.obs_norm.freeze()
    return pol


@pytest.mark.parametrize("kind,block,G,Eps", FUSED, ids=["bf16", "f32x16", "f32x32"])
def test_fused_sub_with_an_obs_norm_table(tg, dev, monkeypatch, kind, block, G, Eps):
    name = "QuadPole"
    pol = normed_policy(tg, dev, name, kind)
    s0 = SR.initial_states(name)[:G * Eps]
    # k > 1: the replay identity (the trajectory records the raw observation; the dynamics never see the table)
    k = 3
    got = snap(fused_engine(tg, dev, name, kind, block, G, Eps, k, pol).run(initial_states=s0))
    assert bool((got["len"] < T).any()) and bool((got["len"] == T).any())
    assert_same(replay(tg, dev, name, k, got, G, Eps, pol), got, f"{kind} fused rollout with obs norm, k = {k}: replay")
    plain_pol = fused_policy(tg, dev, name, kind, seed=6)
    plain_pol.actor.load_state_dict(pol.actor.state_dict())
    other = snap(fused_engine(tg, dev, name, kind, block, G, Eps, k, plain_pol).run(initial_states=s0))
    assert not torch.equal(other["act"], got["act"])                    # the table does reach the actor
    # k = 1: tg_fused_rollout_on / tg_fused_rollout_f32_on
    ref = snap(fused_engine(tg, dev, name, kind, block, G, Eps, 1, pol).run(initial_states=s0))
    force_sub_entry(monkeypatch, tg)
    one = snap(fused_engine(tg, dev, name, kind, block, G, Eps, 1, pol).run(initial_states=s0))
    assert_same(one, ref, "fused `_sub` with obs norm, k = 1", keys=("obs", "rew", "mask", "len", "act"))


@pytest.mark.parametrize("kind,block,G,Eps", [("bf16", None, 4, 33), ("f32", 16, 4, 10), ("f32", 32, 4, 10)], ids=["bf16", "f32x16", "f32x32"])
def test_fused_sub_in_two_shards_is_the_whole_run(tg, dev, kind, block, G, Eps):
    name, k = "QuadPole", 3
    pol = fused_policy(tg, dev, name, kind)
    s0 = SR.initial_states(name)[:G * Eps]
    whole = snap(fused_engine(tg, dev, name, kind, block, G, Eps, k, pol).run(initial_states=s0))
    half = G // 2 * Eps
    parts = []
    for r in range(2):
        eng = fused_engine(tg, dev, name, kind, block, G // 2, Eps, k, pol, group_offset=r * (G // 2), global_groups=G)
        parts.append(snap(eng.run(initial_states=s0[r * half:(r + 1) * half])))
    for key in ("obs", "rew", "mask", "len", "act"):
        assert torch.equal(torch.cat([parts[0][key], parts[1][key]], dim=-1), whole[key]), key
    assert bool((whole["len"] < T).any())


# ------------------------------------------------------------------------------------------------------------------------------
# 6. end to end
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SR.ENVS)
def test_device_rollout_on_every_path(tg, dev, name):
    k, G, Eps = 3, 2, 20
    S, A = SR.DIMS[name]
    pol = f32_policy(tg, S, A, (128, 128), dev, seed=8)
    s0 = SR.initial_states(name)[:G * Eps]

    def engine(**kw):
        return tg.DeviceRollout(env_of(tg, name, T, k, fine=True), pol, G, Eps, seed=21, **kw)

    # per-step launches, sampled; their replay one launch and launch by launch
    per_step = snap(engine(fused=False, use_graph=False).run(initial_states=s0))
    assert bool((per_step["len"] < T).any()) and bool((per_step["len"] == T).any())
    assert_same(replay(tg, dev, name, k, per_step, G, Eps, pol), per_step, "per-step path: one-launch replay")
    eng = engine(fused=False, use_graph=False)
    eng.forced_per_step = True
    by_step = snap(eng.run(initial_states=s0, forced_actions=per_step["act"].permute(2, 1, 0).cpu().numpy()))
    assert_same(by_step, per_step, "per-step path: launch-by-launch replay")
    # the same rollout from its own resets: the graph replays what the plain launches do
    eager = snap(engine(fused=False, use_graph=False).run())
    graph = engine(fused=False, use_graph=True)
    assert_same(snap(graph.run()), eager, "hipGraph replay", keys=("obs", "rew", "mask", "len", "act"))
    assert graph._graph is not None
    # fused fp32 (auto-selected) and bf16, and deterministic runs of both: replay identities
    for kw in (dict(), dict(compute_dtype=torch.bfloat16)):
        cpol = pol if not kw else f32_policy(tg, S, A, (256, 256), dev, seed=8)
        for det in (False, True):
            e = tg.DeviceRollout(env_of(tg, name, T, k, fine=True), cpol, G, Eps, seed=21, **kw)
            assert e.fused
            got = snap(e.run(initial_states=s0, deterministic=det))
            assert_same(replay(tg, dev, name, k, got, G, Eps, cpol), got, f"fused {kw} deterministic={det}: replay")
            if det:
                again = snap(e.run(initial_states=s0, deterministic=True))
                assert_same(again, got, "deterministic runs repeat", keys=("obs", "rew", "mask", "len", "act"))


def test_scalar_env_step_follows_the_rule(tg, dev):
    """Env.step() of a substepped env: a host loop over tg_env_step -- the summed reward and the state of one control step of the
    device rollout, the truncation at the same control step."""
    name, k, n = "QuadPole", 3, 8
    tr = run_forced_sub(tg, name, k, n, torch.float64, dev)
    got = snap(tr)
    acts = SR.forced_actions(name)
    for i in range(n):
        env = env_of(tg, name, T, k)
        env.set_state(SR.initial_states(name)[i])
        L = int(got["len"][i])
        for t in range(L):
            obs, r, _, trunc, _ = env.step(acts[i, t])
            assert r == float(got["rew"][t, i])
            assert trunc == (t + 1 == L)                            # (QuadPole's own clock truncates at k T physics steps)
            if t + 1 < L:
                assert np.array_equal(obs, got["obs"][:, t + 1, i].cpu().numpy())


def test_evaluator_inherits_substeps(tg, dev):
    name, k = "CartPole", 3
    pol = f32_policy(tg, 5, 1, (64, 64), dev, seed=3)
    ev = tg.Evaluator(env_of(tg, name, T, k), pol, episodes=64, seed=2)
    res = ev.evaluate()
    s = res.summary
    assert ev.engine.substeps == k and int(ev.engine.params.max_steps) == k * T
    assert s["episodes"] == 64 and 1 <= s["length_mean"] <= T and np.isfinite(s["return_mean"])
    # the clock / failure split is the plain classification of the same trajectory run at the physics rate
    traj = ev.engine.traj
    held = np.repeat(traj.act.permute(2, 1, 0).cpu().numpy(), k, axis=1)
    plain = new_traj(tg, name, k * T, traj.n, torch.float32, dev, traj.obs[:, 0, :].t().cpu().numpy(), held)
    Nn = tg._native
    p = env_of(tg, name, k * T).native_params()
    with torch.cuda.device(dev):
        for t in range(k * T):
            Nn.check(Nn.load().tg_rollout_step(C.byref(p), C.byref(plain.native()), t, None, 0, None, None, 0, Nn.stream_ptr(dev)), "tg_rollout_step")
    _, timeout = tg.hip_ops.rollout_final_state(p, plain)
    assert abs(s["timeout_frac"] - float(timeout.float().mean())) < 1e-12


def ppo_run(tg, dev, env_fn, learns=2):
    torch.manual_seed(4)
    pol = tg.GaussianActorCritic_NeuralNetwork(5, 1, (64, 64), cov=0.5, device=dev)
    mgr = tg.RolloutManager(env_fn, pol, num_workers=4, num_episodes_per_worker=32, seed=9)
    buf = tg.Rollout_Buffer(mgr)
    algo = tg.PPO(epsilon=0.2, policy=pol, optimizer=torch.optim.Adam(pol.parameters(), lr=3e-4), ref_model=None, updates_per_iter=2,
                  gamma=0.99, batch_size=None, bootstrap_truncated=True)
    boots = []
    for _ in range(learns):
        buf.sample()
        algo.learn(buf)
        boots.append((algo.last_stats["n_bootstrapped"], snap(buf.device_traj)))
    return pol, boots


def test_ppo_bootstraps_a_substepped_env(tg, dev):
    k, horizon = 3, 40
    pol, boots = ppo_run(tg, dev, lambda: env_of(tg, "CartPole", horizon, k))
    Nn = tg._native
    p = env_of(tg, "CartPole", k * horizon).native_params()
    for n_boot, tr in boots:
        # the yardstick of case 2: the recorded trajectory run at the physics rate by the plain kernel, classified by the plain entry
        n = tr["len"].numel()
        held = np.repeat(tr["act"].permute(2, 1, 0).cpu().numpy(), k, axis=1)
        S, A = 5, 1
        plain = tg.rollout.DeviceTrajectory(S, A, k * horizon, n, 1, n, torch.float32, dev)
        plain.obs[:, 0, :].copy_(tr["obs"][:, 0, :])
        plain.act.copy_(torch.as_tensor(held).permute(2, 1, 0).to(dev))
        with torch.cuda.device(dev):
            for t in range(k * horizon):
                Nn.check(Nn.load().tg_rollout_step(C.byref(p), C.byref(plain.native()), t, None, 0, None, None, 0, Nn.stream_ptr(dev)),
                         "tg_rollout_step")
        _, timeout = tg.hip_ops.rollout_final_state(p, plain)
        assert n_boot == int(timeout.sum()) and 0 < n_boot
    assert all(bool(torch.isfinite(q).all()) for q in pol.parameters())


def test_ppo_with_one_substep_never_heard_of_the_attribute(tg, dev):
    class Unaware(tg.CartPole):
        """A CartPole without the attribute: reading it raises AttributeError, as on an env written before it existed."""
        substeps = property(lambda self: (_ for _ in ()).throw(AttributeError("substeps")))

    horizon = 40
    pol_a, boots_a = ppo_run(tg, dev, lambda: Unaware(max_steps=horizon))
    pol_b, boots_b = ppo_run(tg, dev, lambda: env_of(tg, "CartPole", horizon, 1))
    for (na, ta), (nb, tb) in zip(boots_a, boots_b):
        assert na == nb
        assert_same(ta, tb, "substeps = 1", keys=("obs", "rew", "mask", "len", "act"))
    for a, b in zip(pol_a.parameters(), pol_b.parameters()):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------------------------------
# 7. refusals
# ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(tg, dev):
    Nn, lib = tg._native, tg._native.load()
    name, n = "QuadPole", 65
    with pytest.raises(ValueError, match="Pendulum"):
        tg.Pendulum().substeps = 2
    with pytest.raises(ValueError, match="swarm"):
        tg.QuadPoleSwarm(n_agents=2).substeps = 2
    tr = new_traj(tg, name, T, n, torch.float32, dev, SR.initial_states(name), SR.forced_actions(name))
    before = snap(tr)
    st = Nn.stream_ptr(dev)
    p2 = sub_params(tg, name, 2)
    cases = [(p2, 0, Nn.TG_ERR_ARG), (p2, 65, Nn.TG_ERR_ARG), (p2, 3, Nn.TG_ERR_ARG), (env_of(tg, name, T).native_params(), 2, Nn.TG_ERR_ARG),
             (tg.Pendulum(max_steps=2 * T).native_params(), 2, Nn.TG_ERR_UNSUPPORTED),
             (tg.QuadPoleSwarm(n_agents=2, max_steps=2 * T).native_params(), 2, Nn.TG_ERR_UNSUPPORTED)]
    s_final, timeout = torch.zeros(n, 20, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        for p, k, code in cases:
            nat = tr.native()
            assert lib.tg_rollout_step_sub(C.byref(p), None, C.byref(nat), 0, None, 0, None, None, 0, k, st) == code
            assert lib.tg_rollout_forced_sub(C.byref(p), None, C.byref(nat), 0, T, k, st) == code
            assert lib.tg_rollout_final_state_sub(C.byref(p), None, C.byref(nat), s_final.data_ptr(), timeout.data_ptr(), k, st) == code
    assert_same(snap(tr), before, "a refused call", keys=("obs", "rew", "mask", "len", "act"))
    assert not bool(s_final.any()) and not bool(timeout.any())
    # through the public surface: a swarm whose attribute was forced past the setter is refused by the library
    pol = f32_policy(tg, 20, 4, (128, 128), dev, seed=9)
    swarm = tg.QuadPoleSwarm(n_agents=2, max_steps=T)
    swarm._substeps = 2
    eng = tg.DeviceRollout(swarm, pol, 2, 4, seed=1)
    with pytest.raises(RuntimeError, match="swarm"):
        eng.run()
    torch.cuda.synchronize()
    assert not bool(eng.traj.mask.any())
