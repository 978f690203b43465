"""Control decimation (Env.substeps), host side (no GPU): the rule restated over the oracle against the identity the GPU tests use,
the pinned forced-action sets of those tests with their conditions (asserted on the oracle alone), the setter's refusals, the entry
selection, the physics-clock parameters, the metadata key, and the new symbols with their refusals (checked before anything is
launched: the pointers below are never dereferenced)."""
import ctypes as C
import itertools
import os
import re
import warnings

import numpy as np
import pytest

import substeps_ref as SR
import trajopt_grpo_amd as tg

N = tg._native
R = tg.rollout
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 256
NEW_ENTRIES = ["tg_rollout_step_sub", "tg_rollout_forced_sub", "tg_rollout_final_state_sub", "tg_fused_rollout_sub",
               "tg_fused_rollout_f32_sub"]
# sha256 (first 16 hex digits) of the pinned (initial states, forced actions) of each env: PCG64 streams, stable across NumPy versions
PINNED = {"CartPole": "b28f5e51e0a1a39f", "QuadPole2D": "10d686afed0050de", "QuadPole": "f91a335622c5f867"}


@pytest.fixture(scope="module")
def plain_runs():
    """{(env, k): the oracle's plain rollout of horizon k T under the held actions}, computed once."""
    out = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)             # (the oracle normalises the zero quaternion of an ended env's padding)
        for name in SR.ENVS:
            s0, a = SR.initial_states(name), SR.forced_actions(name)
            for k in SR.KS:
                out[name, k] = SR.plain_rollout(name, s0, SR.hold(a, k), SR.T * k)
    return out


# ---- the rule and the identity, on the oracle ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SR.ENVS)
def test_the_pinned_sets_are_what_they_were(name):
    assert SR.digest(SR.initial_states(name), SR.forced_actions(name)) == PINNED[name]
    # n in {1, 65, 300} of the GPU tests are prefixes of one set
    assert np.array_equal(SR.forced_actions(name)[:65], SR.forced_actions(name, SR.N_MAX)[:65])


@pytest.mark.parametrize("k", SR.KS)
@pytest.mark.parametrize("name", SR.ENVS)
def test_the_rule_is_the_plain_rollout_read_at_every_kth_step(plain_runs, name, k):
    """substep_rollout (a loop of the oracle's own step: up to k calls, stop at truncation, summed reward) against decimate() of the
    plain rollout with max_steps = k T: bit for bit in fp64."""
    s0, a = SR.initial_states(name), SR.forced_actions(name)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        sub = SR.substep_rollout(name, s0, a, SR.T, k)
    want = SR.decimate(*plain_runs[name, k], k)
    for got, ref, what in zip(sub, want, ("obs", "rew", "mask", "len")):
        assert np.array_equal(got, ref), what
    assert np.array_equal(sub[2].sum(1), sub[3])                       # mask and len agree, in control steps


@pytest.mark.parametrize("k", SR.KS)
@pytest.mark.parametrize("name", SR.ENVS)
def test_the_pinned_sets_end_early_midway_and_never(plain_runs, name, k):
    """At least a quarter of the episodes end before the horizon, at least one in eight at a physics step that is not the last
    substep of its control step (k > 1), at least one runs the full horizon -- for the whole set and for its 65-env prefix."""
    L = plain_runs[name, k][3]
    for n in (65, SR.N_MAX):
        early, mid, full = SR.ending_shares(L[:n], k)
        assert early >= 0.25 and full >= 1, (n, early, full)
        assert k == 1 or mid >= 0.125, (n, mid)


def test_the_issues_two_estimates():
    """A CartPole at rest under a constant +1 command leaves |x| <= 1 near physics step 45 (measured: 45), a QuadPole at rest with
    zero thrust (a = -1) falls through its 1.5 m bound near step 28 (measured: 28) -- at dt = 0.02, on the oracle."""
    s0 = np.array([[0.0, 0.0, 0.0, 1.0, 0.0]])                          # hanging or upright matters little to the cart's push
    L = SR.plain_rollout("CartPole", s0, np.ones((1, 100, 1), np.float32), 100)[3]
    assert 40 <= int(L[0]) <= 50
    q0 = np.zeros((1, 20)); q0[0, 6] = 1.0; q0[0, 13] = 1.0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        L = SR.plain_rollout("QuadPole", q0, -np.ones((1, 100, 4), np.float32), 100)[3]
    assert 25 <= int(L[0]) <= 31


# ---- Env.substeps ---------------------------------------------------------------------------------------------------------------
def test_substeps_defaults_to_one_and_validates():
    for cls in (tg.CartPole, tg.QuadPole2D, tg.QuadPole, tg.Pendulum):
        env = cls()
        assert env.substeps == 1 and env.control_timestep == env.timestep
        env.substeps = 1                                               # the default is accepted everywhere
    env = tg.QuadPole(max_steps=20)
    for k in (1, 2, 64, np.int32(5)):
        env.substeps = k
        assert env.substeps == int(k) and isinstance(env.substeps, int)
        assert env.control_timestep == env.timestep * int(k) and env.max_steps == 20
    for bad in (0, -1, 65, 2.0, "2", None, True):
        with pytest.raises(ValueError, match="substeps"):
            env.substeps = bad
    assert env.substeps == 5                                           # a refused value changes nothing
    with pytest.raises(AttributeError):
        env.control_timestep = 0.1


def test_substeps_refuses_pendulum_and_swarms():
    with pytest.raises(ValueError, match="Pendulum"):
        tg.Pendulum().substeps = 2
    with pytest.raises(ValueError, match="swarm"):
        tg.QuadPoleSwarm(n_agents=4).substeps = 2
    one = tg.QuadPoleSwarm(n_agents=1)
    one.substeps = 3                                                   # n_agents = 1 is exactly QuadPole
    assert one.substeps == 3


@pytest.mark.parametrize("name", SR.ENVS)
def test_physics_params_are_the_plain_env_of_k_times_the_steps(name):
    cls = tg.environments.ENV_CLASSES[name]
    env = cls(max_steps=SR.T)
    before = bytes(env.native_params())
    assert bytes(env.physics_params()) == before                        # substeps == 1: native_params()
    for k in (2, 3, 5):
        env.substeps = k
        assert bytes(env.native_params()) == before                     # native_params() keeps returning what it returns today
        p, want = env.physics_params(), cls(max_steps=SR.T * k).native_params()
        assert bytes(p) == bytes(want)
        assert p.max_steps == SR.T * k and p.timestep == env.timestep
    if name == "CartPole":                                             # finalised: the fp64-accumulated clock of k T steps
        from oracle import envs as OE
        assert p.time_trunc_step == OE.cartpole_time_trunc_step(SR.T * 5, env.timestep)


# ---- entry selection ----------------------------------------------------------------------------------------------------------
def _fits(name, n_args):
    assert len(N.SIGNATURES[name][1]) == n_args, name


def test_entry_selection_with_one_substep_is_todays():
    PT, ON = 0x1000, (0x2000, 5.0)
    RELU, TANH = N.TG_ACT_RELU, N.TG_ACT_TANH
    # (f32?, parameter table?, obs_norm?) -> (entry, arguments after the env parameters, tail): the selector's table before `substeps`
    today = {
        (False, False, False): lambda act: ("tg_fused_rollout", (), ()),
        (False, True, False): lambda act: ("tg_fused_rollout_dr", (PT,), ()),
        (False, False, True): lambda act: ("tg_fused_rollout_on", (None,), ON),
        (False, True, True): lambda act: ("tg_fused_rollout_on", (PT,), ON),
        (True, False, False): lambda act: ("tg_fused_rollout_f32", (), ()) if act == RELU else ("tg_fused_rollout_f32_act", (), (act,)),
        (True, True, False): lambda act: ("tg_fused_rollout_f32_act_dr", (PT,), (act,)),
        (True, False, True): lambda act: ("tg_fused_rollout_f32_on", (None,), (act,) + ON),
        (True, True, True): lambda act: ("tg_fused_rollout_f32_on", (PT,), (act,) + ON),
    }
    for f32, act, pt, on in itertools.product((False, True), (RELU, TANH), (False, True), (False, True)):
        args = (f32, act, PT if pt else None, ON if on else None)
        assert R.fused_entry(*args, 1) == R.fused_entry(*args) == today[f32, pt, on](act), args
    want = {(False, False): ("tg_rollout_step", ()), (False, True): ("tg_rollout_step_dr", (PT,)),
            (True, False): ("tg_rollout_forced", ()), (True, True): ("tg_rollout_forced_dr", (PT,))}
    for (forced, pt), w in want.items():
        assert R.step_entry(forced, PT if pt else None, 1) == R.step_entry(forced, PT if pt else None) == w
    assert R.sub_tail(1) == ()


def test_entry_selection_with_substeps():
    PT, ON = 0x1000, (0x2000, 5.0)
    RELU, TANH = N.TG_ACT_RELU, N.TG_ACT_TANH
    for f32, act, pt, on in itertools.product((False, True), (RELU, TANH), (False, True), (False, True)):
        name, table, tail = R.fused_entry(f32, act, PT if pt else None, ON if on else None, 3)
        assert name == ("tg_fused_rollout_f32_sub" if f32 else "tg_fused_rollout_sub")
        assert table == (PT if pt else None,)
        assert tail == ((act,) if f32 else ()) + (ON if on else (None, 0.0)) + (3,)
        _fits(name, 1 + len(table) + (11 if f32 else 10) + len(tail) + 1)
    for forced, pt in itertools.product((False, True), (False, True)):
        name, table = R.step_entry(forced, PT if pt else None, 4)
        assert name == ("tg_rollout_forced_sub" if forced else "tg_rollout_step_sub") and table == (PT if pt else None,)
        _fits(name, 1 + len(table) + (3 if forced else 7) + len(R.sub_tail(4)) + 1)
    assert R.sub_tail(4) == (4,)
    _fits("tg_rollout_final_state_sub", 7)


# ---- metadata -----------------------------------------------------------------------------------------------------------------
def test_metadata_gains_substeps_only_when_it_is_not_one():
    class Stub:
        def metadata(self):
            return {}

    def meta(env):
        pipe = tg.pipelines.Pipeline.__new__(tg.pipelines.Pipeline)
        pipe.test_name = pipe.checkpoint_name = pipe.today = pipe.env_name = "x"
        pipe.policy = pipe.algorithm = pipe.buffer = Stub()
        pipe.visualizer = pipe.publisher = pipe.logger = None
        pipe.env = env
        return pipe.get_metadata()

    env = tg.CartPole()
    assert "substeps" not in meta(env)
    env.substeps = 4
    assert meta(env)["substeps"] == 4


def test_train_ppo_takes_substeps():
    src = open(os.path.join(REPO, "tools", "train_ppo.py")).read()
    assert "--substeps" in src and "env.substeps = substeps" in src


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_and_bound():
    header = open(os.path.join(REPO, "include", "trajopt_grpo_hip.h")).read()
    lib = N.load()
    for name in NEW_ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in N.SIGNATURES and hasattr(lib, name)
        assert N.SIGNATURES[name][1][-2] == C.c_int32                   # `substeps` is the last argument before the stream
    assert C.sizeof(N.EnvParams) == 4 * 4 + 8 + 12 * 8                  # k travels as an argument, not in the struct
    assert "agents > 1" in header and "Pendulum" in header and "[1, 64]" in header


def _traj(T, n=4, dtype=N.TG_F32):
    t = N.Traj()
    t.d_obs = t.d_act = t.d_rew = t.d_mask = t.d_len = t.d_counters = FAKE
    t.n, t.horizon, t.dtype = n, T, dtype
    return t


def _call(name, p, tr, k):
    lib, sg = N.load(), (C.c_float * 4)(0.1, 0.1, 0.1, 0.1)
    if name == "tg_rollout_step_sub":
        return lib.tg_rollout_step_sub(C.byref(p), None, C.byref(tr), 0, None, 0, None, None, 0, k, None)
    if name == "tg_rollout_forced_sub":
        return lib.tg_rollout_forced_sub(C.byref(p), None, C.byref(tr), 0, tr.horizon, k, None)
    if name == "tg_rollout_final_state_sub":
        return lib.tg_rollout_final_state_sub(C.byref(p), None, C.byref(tr), FAKE, FAKE, k, None)
    if name == "tg_fused_rollout_sub":
        return lib.tg_fused_rollout_sub(C.byref(p), None, C.byref(tr), FAKE, FAKE, 128, 2, sg, FAKE, 0, 0, tr.horizon, None, 0.0, k, None)
    return lib.tg_fused_rollout_f32_sub(C.byref(p), None, C.byref(tr), FAKE, FAKE, 128, 2, 32, sg, FAKE, 0, 0, tr.horizon, N.TG_ACT_RELU,
                                        None, 0.0, k, None)


@pytest.mark.parametrize("name", NEW_ENTRIES)
def test_refusals_come_before_any_launch(name):
    T = 8
    env = tg.QuadPole(max_steps=T)
    env.substeps = 2
    p, tr = env.physics_params(), _traj(T)
    for k in (0, -3, 65):
        assert _call(name, p, tr, k) == N.TG_ERR_ARG
        assert "substeps" in N.load().tg_last_error().decode()
    # a p whose max_steps is not horizon * k: the control-clock params, or another k
    assert _call(name, env.native_params(), tr, 2) == N.TG_ERR_ARG
    assert _call(name, p, tr, 3) == N.TG_ERR_ARG
    assert "physics clock" in N.load().tg_last_error().decode()
    swarm = tg.QuadPoleSwarm(n_agents=4, max_steps=2 * T).native_params()
    assert _call(name, swarm, tr, 2) == N.TG_ERR_UNSUPPORTED
    assert "swarm" in N.load().tg_last_error().decode()
    pend = tg.Pendulum(max_steps=2 * T).native_params()
    assert _call(name, pend, tr, 2) == N.TG_ERR_UNSUPPORTED
    assert "Pendulum" in N.load().tg_last_error().decode()


def test_plain_entries_refuse_the_physics_clock_params():
    """The entries without `_sub` keep their horizon == max_steps check: they cannot be handed a substepped env's params by mistake."""
    T = 8
    env = tg.QuadPole(max_steps=T)
    env.substeps = 2
    p, tr = env.physics_params(), _traj(T)
    lib = N.load()
    assert lib.tg_rollout_step(C.byref(p), C.byref(tr), 0, None, 0, None, None, 0, None) == N.TG_ERR_ARG
    assert lib.tg_rollout_forced(C.byref(p), C.byref(tr), 0, T, None) == N.TG_ERR_ARG
    assert lib.tg_rollout_final_state(C.byref(p), C.byref(tr), FAKE, FAKE, None) == N.TG_ERR_ARG
