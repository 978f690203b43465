"""The actuator lag (Env.motor_time_constant), host side (no GPU): the NumPy float32 restatement of the filter against an exact
case and a rounding bound, the entry selection, the setter's and the library's refusals (checked before anything is launched: the
pointers below are never dereferenced), the randomisation slot, the metadata key and the new symbols."""
import ctypes as C
import itertools
import math
import os
import re

import numpy as np
import pytest

import motor_lag_ref as ML
import trajopt_grpo_amd as tg

N = tg._native
R = tg.rollout
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 256
NEW_ENTRIES = ["tg_rollout_step_lag", "tg_rollout_forced_lag", "tg_rollout_final_state_lag", "tg_fused_rollout_lag",
               "tg_fused_rollout_f32_lag"]


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def test_alpha_is_one_double_divide_rounded_once():
    assert ML.alpha(0.02, 0.02) == np.float32(0.5) and ML.alpha(0.0, 0.02) == np.float32(1.0)
    assert ML.alpha(0.05, 0.02) == np.float32(0.02 / (0.05 + 0.02)) and ML.alpha(0.05, 0.02).dtype == np.float32
    taus = np.array([0.01, 0.05, 0.3])
    assert np.array_equal(ML.alpha(taus, 0.02), np.array([np.float32(0.02 / (t + 0.02)) for t in taus]))
    env = tg.QuadPole2D()
    env.motor_time_constant = 0.05
    assert env.motor_alpha() == ML.alpha(0.05, env.timestep) and isinstance(env.motor_alpha(), np.float32)


@pytest.mark.parametrize("k,T", [(1, 16), (3, 5), (4, 4)])
def test_exact_filter_case(k, T):
    """tau = dt, so alpha = 0.5; actions are multiples of 1/8 in [-1, 1]; T k <= 16 physics steps.  After j steps m is a multiple of
    2^-(3 + j) of magnitude <= 1: at most 20 significant bits, so every float32 operation of the filter is exact and the restatement
    must EQUAL the closed form m_j = sum_{i <= j} c_i 2^-(j - i + 1), evaluated in fp64 (exact there too)."""
    assert T * k <= 16
    A, n = 2, 9
    rng = np.random.Generator(np.random.PCG64(5))
    act = (rng.integers(-12, 13, size=(A, T, n)) / 8.0).astype(np.float32)          # some beyond [-1, 1]: the clip is part of the rule
    al = ML.alpha(0.02, 0.02)
    assert al == np.float32(0.5)
    cmds, motor = ML.filter(act, al, k, np.full((T, n), k))
    c = np.repeat(np.clip(act.astype(np.float64), -1.0, 1.0), k, axis=1)             # the command held over a control step's k steps
    want = np.zeros((A, T * k, n))
    for j in range(T * k):
        for i in range(j + 1):
            want[:, j] += c[:, i] * 0.5 ** (j - i + 1)
    assert np.array_equal(cmds.astype(np.float64), want)
    assert np.array_equal(motor[:, 1:T].astype(np.float64), want[:, k - 1:(T - 1) * k:k])   # slot t + 1: m after control step t
    assert not motor[:, 0].any() and not motor[:, T].any()                           # the reset, and the slot behind the horizon


def test_rounding_bound():
    """On random actions and gains, |m_float32 - m_fp64| <= 3 j 2^-24 after j steps, m_fp64 the same recurrence in fp64 with the
    same float32 alpha and the same clipped float32 commands.  Derivation: |c|, |m| <= 1 (m stays in [-1, 1]: d = c - m is exact
    near c by Sterbenz, fl(alpha d) <= d, so m + e never passes c).  One step rounds three times: d = c - m with |d| <= 2 errs by at
    most 2^-24 and reaches m scaled by alpha <= 1; e = alpha d with |e| <= 2 errs by at most 2^-24; m + e with |m + e| <= 1 errs by
    at most 2^-25: under 3 2^-24 per step.  The exact map m -> (1 - alpha) m + alpha c is a contraction (0 <= 1 - alpha <= 1), so
    earlier errors do not grow: the bound is the sum."""
    A, T, n, k = 4, 40, 64, 3
    rng = np.random.Generator(np.random.PCG64(6))
    act = np.clip(rng.normal(0.0, 0.7, size=(A, T, n)), -1.5, 1.5).astype(np.float32)
    al = ML.alpha(rng.uniform(0.0, 0.3, n), 0.02)
    cmds, _ = ML.filter(act, al, k, np.full((T, n), k))
    assert float(np.abs(cmds).max()) <= 1.0
    c = np.repeat(np.clip(act, np.float32(-1), np.float32(1)).astype(np.float64), k, axis=1)
    m = np.zeros((A, n))
    worst = 0.0
    for j in range(T * k):
        m = m + al.astype(np.float64)[None, :] * (c[:, j] - m)
        err = float(np.abs(cmds[:, j].astype(np.float64) - m).max())
        assert err <= 3 * (j + 1) * 2.0 ** -24, (j, err)
        worst = max(worst, err)
    assert worst > 0.0                                                               # (the case does round)


def test_a_stopped_lane_filters_no_more():
    A, T, n, k = 2, 4, 3, 3
    act = np.full((A, T, n), 0.75, np.float32)
    executed = np.array([[3, 3, 3], [3, 2, 3], [3, 0, 1], [3, 0, 0]])               # env 1 stops inside step 1, env 2 inside step 2
    cmds, motor = ML.filter(act, ML.alpha(0.05, 0.02), k, executed)
    free = ML.free_commands(act, ML.alpha(0.05, 0.02), k)
    for t, i in itertools.product(range(T), range(n)):
        e = executed[t, i]
        assert np.array_equal(cmds[:, t * k:t * k + e, i], free[:, t * k:t * k + e, i])      # causal: the run steps are the free ones
        assert not cmds[:, t * k + e:(t + 1) * k, i].any()
    assert motor[:, 1, 1].any() and not motor[:, 2:, 1].any()                        # zeros once the env does not carry on
    assert motor[:, 2, 2].any() and not motor[:, 3:, 2].any()
    assert np.array_equal(ML.executed_from_plain_len([12, 5, 7], k, T), executed)


# ---- Env.motor_time_constant ----------------------------------------------------------------------------------------------------
def test_the_attribute_defaults_to_off_and_validates():
    for cls in (tg.CartPole, tg.QuadPole2D, tg.QuadPole, tg.Pendulum):
        env = cls()
        assert env.motor_time_constant == 0.0
        env.motor_time_constant = 0.0                                                # the default is accepted everywhere
        assert env.native_params().p[10] == 0.0
    env = tg.QuadPole(max_steps=20)
    for tau in (0.05, 1, np.float32(0.25), 0.0):
        env.motor_time_constant = tau
        assert env.motor_time_constant == float(tau) and isinstance(env.motor_time_constant, float)
    env.motor_time_constant = 0.04
    for bad in (-0.01, float("nan"), float("inf"), -float("inf"), "0.1", None, True):
        with pytest.raises(ValueError, match="motor_time_constant"):
            env.motor_time_constant = bad
    assert env.motor_time_constant == 0.04                                           # a refused value changes nothing


def test_only_the_rotor_envs_take_it():
    for env in (tg.CartPole(), tg.Pendulum()):
        with pytest.raises(ValueError, match="no rotors"):
            env.motor_time_constant = 0.05
    with pytest.raises(ValueError, match="swarm"):
        tg.QuadPoleSwarm(n_agents=4).motor_time_constant = 0.05
    one = tg.QuadPoleSwarm(n_agents=1)
    one.motor_time_constant = 0.05                                                   # n_agents = 1 is exactly QuadPole
    assert one.motor_time_constant == 0.05


@pytest.mark.parametrize("cls", [tg.QuadPole2D, tg.QuadPole])
def test_the_params_carry_it_in_slot_ten(cls):
    env = cls(max_steps=16)
    before, before_phys = bytes(env.native_params()), bytes(env.physics_params())
    env.motor_time_constant = 0.05
    p = env.native_params()
    assert p.p[10] == 0.05 and p.p[11] == 0.0
    env.substeps = 3
    q = env.physics_params()
    assert q.p[10] == 0.05 and q.max_steps == 48
    assert [p.p[i] for i in range(10)] == [q.p[i] for i in range(10)]
    env.motor_time_constant = 0.0
    env.substeps = 1
    assert bytes(env.native_params()) == before and bytes(env.physics_params()) == before_phys


# ---- entry selection ------------------------------------------------------------------------------------------------------------
def _fits(name, n_args):
    assert len(N.SIGNATURES[name][1]) == n_args, name


def test_entry_selection_without_a_motor_is_todays():
    PT, ON = 0x1000, (0x2000, 5.0)
    for f32, act, pt, on, k in itertools.product((False, True), (N.TG_ACT_RELU, N.TG_ACT_TANH), (False, True), (False, True), (1, 3)):
        args = (f32, act, PT if pt else None, ON if on else None, k)
        assert R.fused_entry(*args) == R.fused_entry(*args, motor=None)
        assert not R.fused_entry(*args)[0].endswith("_lag")
    for forced, pt, k in itertools.product((False, True), (False, True), (1, 3)):
        assert R.step_entry(forced, PT if pt else None, k) == R.step_entry(forced, PT if pt else None, k, motor=None)
        assert not R.step_entry(forced, PT if pt else None, k)[0].endswith("_lag")
    assert R.sub_tail(1) == R.sub_tail(1, motor=None) == () and R.sub_tail(4) == R.sub_tail(4, motor=None) == (4,)
    assert R.fused_entry(False, N.TG_ACT_RELU, None, None) == ("tg_fused_rollout", (), ())
    assert R.step_entry(False, None) == ("tg_rollout_step", ()) and R.step_entry(True, None) == ("tg_rollout_forced", ())


def test_entry_selection_with_a_motor():
    PT, ON, MO = 0x1000, (0x2000, 5.0), 0x3000
    for f32, act, pt, on, k in itertools.product((False, True), (N.TG_ACT_RELU, N.TG_ACT_TANH), (False, True), (False, True), (1, 3)):
        name, table, tail = R.fused_entry(f32, act, PT if pt else None, ON if on else None, k, motor=MO)
        assert name == ("tg_fused_rollout_f32_lag" if f32 else "tg_fused_rollout_lag")
        assert table == (PT if pt else None,)
        assert tail == ((act,) if f32 else ()) + (ON if on else (None, 0.0)) + (k, MO)
        _fits(name, 1 + len(table) + (11 if f32 else 10) + len(tail) + 1)
    for forced, pt, k in itertools.product((False, True), (False, True), (1, 4)):
        name, table = R.step_entry(forced, PT if pt else None, k, motor=MO)
        assert name == ("tg_rollout_forced_lag" if forced else "tg_rollout_step_lag") and table == (PT if pt else None,)
        _fits(name, 1 + len(table) + (3 if forced else 7) + len(R.sub_tail(k, motor=MO)) + 1)
        assert R.sub_tail(k, motor=MO) == (k, MO)
    _fits("tg_rollout_final_state_lag", 8)


# ---- the randomisation slot -----------------------------------------------------------------------------------------------------
def test_the_randomise_name_exists_only_while_the_lag_is_on():
    env = tg.QuadPole(max_steps=8)
    names = list(env.RANDOMIZABLE)
    assert env.parameter_slots() == env.RANDOMIZABLE
    with pytest.raises(ValueError, match="motor_time_constant"):
        env.randomize({"motor_time_constant": (0.5, 2.0)})
    with pytest.raises(ValueError, match="motor_time_constant"):
        tg.evaluation.check_sweep(env, {"motor_time_constant": [0.5, 1.0]})
    env.motor_time_constant = 0.05
    assert env.parameter_slots() == {**env.RANDOMIZABLE, "motor_time_constant": 10}
    assert list(env.RANDOMIZABLE) == names == list(tg.QuadPole.RANDOMIZABLE) and "motor_time_constant" not in tg.QuadPole.RANDOMIZABLE
    env.randomize({"motor_time_constant": (0.5, 2.0), "mass": (0.8, 1.25), "arm_length": (0.9, 1.1)}, seed=3)
    spec = env.randomize_spec()
    assert spec.count == 3 and [spec.index[i] for i in range(3)] == [0, 8, 10]          # p[] order: slot 10 sorts last
    assert (spec.lo[2], spec.hi[2]) == (0.5, 2.0) and spec.seed == 3
    assert tg.evaluation.check_sweep(env, {"motor_time_constant": [0.5, 1, 2], "mass": [1.0]}) == \
        [("mass", 0, [1.0]), ("motor_time_constant", 10, [0.5, 1.0, 2.0])]
    assert env.randomize_metadata() == {"ranges": {"motor_time_constant": [0.5, 2.0], "mass": [0.8, 1.25], "arm_length": [0.9, 1.1]},
                                        "seed": 3}
    env.motor_time_constant = 0.0                                                    # off again: the name is gone, and the spec says so
    with pytest.raises(ValueError, match="motor_time_constant"):
        env.randomize_spec()


def test_privileged_spec_takes_the_name():
    env = tg.QuadPole2D(max_steps=8)
    env.motor_time_constant = 0.05
    pol = tg.GaussianActorCritic_NeuralNetwork(10, 2, (64, 64), cov=0.3, device="cpu",
                                               privileged_critic={"motor_time_constant": (0.5, 2.0), "mq": (0.8, 1.25)})
    spec = tg.algorithms.privileged_spec(pol, env)
    assert spec.count == 2 and [spec.index[i] for i in range(2)] == [10, 0] and spec.nominal[0] == 0.05
    env.motor_time_constant = 0.0
    with pytest.raises(ValueError, match="motor_time_constant"):
        tg.algorithms.privileged_spec(pol, env)


# ---- metadata and the tool ------------------------------------------------------------------------------------------------------
def test_metadata_round_trip():
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

    env = tg.QuadPole2D()
    assert "motor_time_constant" not in meta(env)
    env.motor_time_constant = 0.035
    m = meta(env)
    assert m["motor_time_constant"] == 0.035
    other = tg.QuadPole2D()
    other.motor_time_constant = m["motor_time_constant"]
    assert bytes(other.native_params()) == bytes(env.native_params())
    assert "motor_time_constant" not in meta(tg.CartPole())


def test_train_ppo_takes_motor_tau():
    import importlib.util
    spec = importlib.util.spec_from_file_location("train_ppo_tool", os.path.join(REPO, "tools", "train_ppo.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    assert tool.pop_motor_tau(["3", "QuadPole", "--motor-tau", "0.05", "--gae"]) == (0.05, ["3", "QuadPole", "--gae"])
    assert tool.pop_motor_tau(["3", "QuadPole"]) == (0.0, ["3", "QuadPole"])
    with pytest.raises(SystemExit, match="motor-tau"):
        tool.pop_motor_tau(["--motor-tau", "fast"])
    ranges, rest = tool.pop_randomize(["--randomize", "motor_time_constant=0.5:2", "--randomize", "mass=0.8:1.25"])
    env = tool.build_env("QuadPole", ranges, 2, 0.05)                                 # the lag is on before the name is ranged
    assert env.motor_time_constant == 0.05 and env.substeps == 2 and env.timestep == 0.01
    assert env.randomization == {"motor_time_constant": (0.5, 2.0), "mass": (0.8, 1.25)} and env.physics_params().p[10] == 0.05
    with pytest.raises(ValueError, match="motor_time_constant"):
        tool.build_env("QuadPole", ranges)                                            # off: the name is unknown
    with pytest.raises(ValueError, match="no rotors"):
        tool.build_env("CartPole", {}, 1, 0.05)
    plain = tool.build_env("QuadPole", {})
    assert plain.motor_time_constant == 0.0 and plain.randomization is None


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_and_bound():
    header = open(os.path.join(REPO, "include", "trajopt_grpo_hip.h")).read()
    lib = N.load()
    assert N.ABI_VERSION == lib.tg_abi_version()                                      # (additions only: no signature changed)
    for name in NEW_ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in N.SIGNATURES and hasattr(lib, name)
        sub = N.SIGNATURES[name[:-4] + "_sub"][1]
        assert N.SIGNATURES[name][1] == sub[:-1] + [C.c_void_p, sub[-1]]              # the `_sub` sibling plus d_motor before the stream
    assert C.sizeof(N.EnvParams) == 4 * 4 + 8 + 12 * 8                                # tau travels in p[10]: the struct is what it was


def _traj(T, n=4, dtype=N.TG_F32):
    t = N.Traj()
    t.d_obs = t.d_act = t.d_rew = t.d_mask = t.d_len = t.d_counters = FAKE
    t.n, t.horizon, t.dtype = n, T, dtype
    return t


def _call(name, p, tr, k=1, motor=FAKE, ptab=None):
    lib, sg = N.load(), (C.c_float * 4)(0.1, 0.1, 0.1, 0.1)
    if name == "tg_rollout_step_lag":
        return lib.tg_rollout_step_lag(C.byref(p), ptab, C.byref(tr), 0, None, 0, None, None, 0, k, motor, None)
    if name == "tg_rollout_forced_lag":
        return lib.tg_rollout_forced_lag(C.byref(p), ptab, C.byref(tr), 0, tr.horizon, k, motor, None)
    if name == "tg_rollout_final_state_lag":
        return lib.tg_rollout_final_state_lag(C.byref(p), ptab, C.byref(tr), FAKE, FAKE, k, motor, None)
    if name == "tg_fused_rollout_lag":
        return lib.tg_fused_rollout_lag(C.byref(p), ptab, C.byref(tr), FAKE, FAKE, 128, 2, sg, FAKE, 0, 0, tr.horizon, None, 0.0, k, motor, None)
    return lib.tg_fused_rollout_f32_lag(C.byref(p), ptab, C.byref(tr), FAKE, FAKE, 128, 2, 32, sg, FAKE, 0, 0, tr.horizon, N.TG_ACT_RELU,
                                        None, 0.0, k, motor, None)


def _lagged(cls, T, tau=0.05, k=1):
    env = cls(max_steps=T)
    env.motor_time_constant = tau
    env.substeps = k
    return env


@pytest.mark.parametrize("name", NEW_ENTRIES)
def test_refusals_come_before_any_launch(name):
    T = 8
    tr = _traj(T)
    err = lambda: N.load().tg_last_error().decode()
    good = _lagged(tg.QuadPole, T).physics_params()
    # envs without rotors, and swarms: the parameters are forced past the setter
    for cls in (tg.CartPole, tg.Pendulum):
        p = cls(max_steps=T).native_params()
        p.p[10] = 0.05
        assert _call(name, p, tr) == N.TG_ERR_UNSUPPORTED and "no rotors" in err()
    swarm = tg.QuadPoleSwarm(n_agents=4, max_steps=T).native_params()
    swarm.p[10] = 0.05
    assert _call(name, swarm, tr) == N.TG_ERR_UNSUPPORTED and "swarm" in err()
    # a null motor record
    assert _call(name, good, tr, motor=None) == N.TG_ERR_ARG and "motor" in err()
    # the time constant: off without a table, negative, not finite (with a table too)
    for tau, ptab in ((0.0, None), (-0.01, None), (-0.01, FAKE), (math.nan, None), (math.inf, None), (math.nan, FAKE), (-math.inf, FAKE)):
        p = _lagged(tg.QuadPole, T).physics_params()
        p.p[10] = tau
        assert _call(name, p, tr, ptab=ptab) == N.TG_ERR_ARG and "p[10]" in err(), (tau, ptab)
    # `_sub`'s own limits still hold behind the lag's
    assert _call(name, good, tr, k=0) == N.TG_ERR_ARG and "substeps" in err()
    assert _call(name, good, tr, k=2) == N.TG_ERR_ARG and "physics clock" in err()
