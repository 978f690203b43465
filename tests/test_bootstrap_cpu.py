"""Time-limit bootstrapping, host side (no GPU): the fp64 restatement the GPU tests compare against, the teacher-forced cases of the
classification test (their class shares, confirmed with the oracle alone), the `bootstrap_truncated` keyword of PPO and of the
factories, and the two new entry points of the C ABI with their refusals (checked before anything is launched: the pointers below
are never dereferenced)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import bootstrap_fp64 as B
import trajopt_grpo_amd as tg
from oracle import learner as L

N = tg._native
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 256
NEW_ENTRIES = ["tg_rollout_final_state", "tg_ppo_returns_boot"]


# ---- the fp64 restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("monte_carlo", [True, False], ids=["mc", "gae"])
def test_a_zero_bootstrap_is_ppo_advantages_on_the_untouched_rewards(monte_carlo):
    rng = np.random.default_rng(0)
    G, Eps, T = 3, 5, 17
    length = rng.integers(1, T + 1, (G, Eps))
    mask = (np.arange(T) < length[..., None]).astype(np.float32)
    rew = (rng.normal(size=(G, Eps, T)) * mask).astype(np.float32)
    val = (rng.normal(size=(G, Eps, T)) * mask).astype(np.float32)
    assert np.array_equal(B.augment(rew, length, np.zeros((G, Eps)), 0.99), rew.astype(np.float64))
    got = B.bootstrapped_advantages(rew, mask, val, length, np.zeros((G, Eps)), 0.99, 0.95, monte_carlo)
    ref = L.ppo_advantages(torch.from_numpy(rew.astype(np.float64)), torch.from_numpy(mask), torch.from_numpy(val), 0.99, 0.95, monte_carlo)
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
    # a length outside [1, T] adds nothing either
    assert np.array_equal(B.augment(rew, np.zeros((G, Eps)), np.ones((G, Eps)), 0.99), rew.astype(np.float64))


def test_hand_computed_two_envs_four_steps():
    """gamma = lam = 1/2 and dyadic numbers: every operation is exact in fp32, so the textbook values are matched exactly.
    Env 0 runs to the horizon (L = 4) and is bootstrapped with V(s_4) = 8; env 1 ends at L = 2 with V(s_2) = 4: the bonus lands on
    step L - 1 = 1, not on the horizon's last step.  R_{L-1} = r + gamma V(s_L); delta_{L-1} = r + gamma V(s_L) - V(s_{L-1})."""
    gamma = lam = 0.5
    rew = np.array([[1.0, 2.0, 3.0, 4.0], [1.0, -2.0, 0.0, 0.0]])
    mask = np.array([[1.0, 1, 1, 1], [1, 1, 0, 0]], dtype=np.float32)
    val = np.array([[1.0, 1, 1, 1], [2, 1, 0, 0]], dtype=np.float32)
    length, b = np.array([4, 2]), np.array([8.0, 4.0])
    aug = B.augment(rew, length, b, gamma)
    assert np.array_equal(aug, [[1, 2, 3, 8], [1, 0, 0, 0]])
    # Monte Carlo: R_3 = 4 + 8/2 = 8, R_2 = 3 + 8/2 = 7, R_1 = 2 + 7/2, R_0 = 1 + 5.5/2; env 1: R_1 = -2 + 4/2 = 0, R_0 = 1
    R = np.array([[3.75, 5.5, 7.0, 8.0], [1.0, 0.0, 0.0, 0.0]])
    rtg = L.rtg_scan(torch.from_numpy(aug), torch.from_numpy(mask), gamma)
    assert np.array_equal(rtg.numpy(), R)
    # GAE: env 0: A_3 = 8 - 1 = 7; A_2 = (3 + 1/2 - 1) + 7/4; A_1 = (2 + 1/2 - 1) + 4.25/4; A_0 = (1 + 1/2 - 1) + 2.5625/4
    #      env 1: A_1 = delta_1 = -2 + 4/2 - 1 = -1; A_0 = (1 + 1/2 - 2) + (-1)/4
    A = np.array([[1.140625, 2.5625, 4.25, 7.0], [-0.75, -1.0, 0.0, 0.0]])
    adv, ret = L.gae_scan(torch.from_numpy(aug).float(), torch.from_numpy(val), torch.from_numpy(mask), gamma, lam)
    assert np.array_equal(adv.numpy(), A) and np.array_equal(ret.numpy(), A + val)
    # ... and through ppo_advantages: the valid entries, each normalised by its own mean / (unbiased std + 1e-8)
    valid = mask.reshape(-1) > 0
    for mc, (a_raw, r_raw) in ((True, (R - val, R)), (False, (A, A + val))):
        a, r = B.bootstrapped_advantages(rew, mask, val, length, b, gamma, lam, mc)
        for got, raw in ((a, a_raw), (r, r_raw)):
            v = torch.from_numpy(raw.reshape(-1)[valid]).double()
            assert torch.allclose(got.double(), (v - v.mean()) / (v.std() + 1e-8), rtol=1e-6, atol=1e-6)
    # without the bootstrap the cut returns are what the learner computes today
    assert np.array_equal(L.rtg_scan(torch.from_numpy(rew), torch.from_numpy(mask), gamma).numpy(), [[3.25, 4.5, 5.0, 4.0], [0.0, -2.0, 0.0, 0.0]])


@pytest.mark.parametrize("name", list(B.CASES))
def test_forced_cases_hold_both_classes_by_the_oracle_alone(name):
    """The inputs of the GPU classification test, rolled out by the oracle: at least 10 % of the episodes time-limited, at least 10 %
    ended otherwise (failed; Pendulum: balance-terminated), none within 1e-5 of a bound, and -- for the envs that can fail -- episodes
    that fail exactly at step T (timeout = 0 although L == T)."""
    case = B.CASES[name]
    T, params = case["T"], case["params"]
    init, act = B.forced_case(name)
    n = len(init)
    assert n == B.N_RANDOM + B.N_SCAN and n % 64 != 0
    length, s_final, obs_last = B.oracle_rollout(name, init, act, T, params)
    timeout = B.classify(name, s_final, length, T, params.get("timestep"))
    assert timeout.mean() >= 0.10 and (~timeout).mean() >= 0.10
    assert B.near_bound(name, s_final).mean() <= 0.01
    fails = B.failed(name, s_final)
    if name == "Pendulum":
        assert not fails.any()
        ended_by_balance = ~timeout
        assert np.all(length[ended_by_balance] == 11) and T > 11          # 5 s of balance at 0.5 s per step
    else:
        assert np.array_equal(~timeout, fails)                              # these envs end by failure or by the clock
        boundary = fails & (length == T)
        assert boundary.sum() >= 2 and not timeout[boundary].any()
    # the re-step from the last recorded transition is the state the rollout dropped
    again = B.oracle_final_state(name, obs_last, act[np.arange(n), length - 1], length, T, params)
    assert np.array_equal(again, s_final)


# ---- the keyword ----------------------------------------------------------------------------------------------------------------
def _ppo(**kw):
    pol = tg.GaussianActorCritic_NeuralNetwork(5, 1, (64, 64), cov=0.5, device="cpu")
    return tg.PPO(0.2, pol, torch.optim.Adam(pol.parameters(), lr=3e-4), None, 2, batch_size=None, **kw)


def test_bootstrap_truncated_is_validated_at_construction():
    for bad in (1, 0, "yes", None, 1.0):
        with pytest.raises(ValueError, match="bootstrap_truncated"):
            _ppo(bootstrap_truncated=bad)
    assert _ppo().bootstrap_truncated is False and _ppo(bootstrap_truncated=True).bootstrap_truncated is True
    sig = inspect.signature(tg.PPO.__init__).parameters
    assert sig["bootstrap_truncated"].kind is inspect.Parameter.KEYWORD_ONLY and sig["bootstrap_truncated"].default is False
    assert list(sig).index("bootstrap_truncated") == list(sig).index("max_grad_norm") + 1
    assert "bootstrap_truncated" not in inspect.signature(tg.GRPO.__init__).parameters


def test_metadata_gains_the_key_only_when_set():
    plain = {"algorithm": "PPO", "epsilon": 0.2, "c1": 0.5, "kl_coeff": 0.5, "gamma": 0.99, "lam": 0.95, "entropy": 0.01,
             "batch_size": None, "updates_per_iter": 2}
    assert _ppo().metadata() == plain and _ppo(bootstrap_truncated=False).metadata() == plain
    assert _ppo(bootstrap_truncated=True).metadata() == {**plain, "bootstrap_truncated": True}
    assert _ppo(bootstrap_truncated=True, max_grad_norm=1.0).metadata() == {**plain, "max_grad_norm": 1.0, "bootstrap_truncated": True}


def test_a_buffer_without_an_engine_is_refused_before_anything_runs():
    algo = _ppo(bootstrap_truncated=True)
    buf = type("HandBuilt", (), {"device_traj": None})()
    with pytest.raises(ValueError, match="no rollout engine"):
        algo._bootstrap_params(buf)
    swarm = N.default_params(N.TG_ENV_QUADPOLE, 16)
    swarm.agents = 4
    buf.rollout_manager = type("Mgr", (), {"engine": type("Eng", (), {"params": swarm})()})()
    with pytest.raises(ValueError, match="swarm"):
        algo._bootstrap_params(buf)
    swarm.agents = 1
    assert algo._bootstrap_params(buf) is swarm


@pytest.mark.parametrize("factory", ["create_cartpole_pipeline_ppo", "create_quadpole2d_pipeline_ppo", "create_quadpole_pipeline_ppo"])
def test_factories_take_the_keyword(factory):
    fn = getattr(tg.pipelines, factory)
    p = inspect.signature(fn).parameters["bootstrap_truncated"]
    assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY
    assert inspect.signature(tg.pipelines._ppo_pipeline).parameters["bootstrap_truncated"].default is False
    # the factory hands it to the PPO it builds (caught at the constructor: no rollout manager is built on a box without a GPU)
    seen = {}

    class Stop(Exception):
        pass

    def fake_ppo(**kw):
        seen.update(kw)
        raise Stop

    orig = tg.pipelines.PPO
    tg.pipelines.PPO = fake_ppo
    try:
        for flag in (False, True):
            pol = tg.GaussianActorCritic_NeuralNetwork(5, 1, (8,), cov=0.5, device="cpu")
            with pytest.raises(Stop):
                fn("t", "c", policy=pol, bootstrap_truncated=flag)
            assert seen["bootstrap_truncated"] is flag
    finally:
        tg.pipelines.PPO = orig


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
def test_new_entry_points_are_declared_bound_and_exported_and_the_abi_is_13():
    lib = N.load()
    header = open(os.path.join(REPO, "include", "trajopt_grpo_hip.h")).read()
    declared = set(re.findall(r"\b(tg_[a-z0-9_]+)\s*\(", header))
    for name in NEW_ENTRIES:
        assert name in declared and name in N.SIGNATURES and hasattr(lib, name), name
    assert len(N.SIGNATURES["tg_rollout_final_state"][1]) == 5 and len(N.SIGNATURES["tg_ppo_returns_boot"][1]) == 15
    assert hasattr(tg.hip_ops, "rollout_final_state") and hasattr(tg.hip_ops, "ppo_returns_boot")
    assert lib.tg_abi_version() == N.ABI_VERSION == 13 == int(re.search(r"#define\s+TG_ABI_VERSION\s+(\d+)", header).group(1))


def _traj(n=8, T=16, dtype=N.TG_F32):
    tr = N.Traj()
    tr.d_obs = tr.d_act = tr.d_rew = tr.d_mask = tr.d_len = tr.d_counters = FAKE
    tr.n, tr.horizon, tr.dtype = n, T, dtype
    return tr


def test_final_state_refusals():
    lib = N.load()
    p = N.default_params(N.TG_ENV_CARTPOLE, 16)
    tr = _traj()
    assert lib.tg_rollout_final_state(None, C.byref(tr), FAKE, FAKE, None) == -1 and b"null pointer" in lib.tg_last_error()
    assert lib.tg_rollout_final_state(C.byref(p), C.byref(tr), None, FAKE, None) == -1 and b"null pointer" in lib.tg_last_error()
    assert lib.tg_rollout_final_state(C.byref(p), C.byref(tr), FAKE, None, None) == -1 and b"null pointer" in lib.tg_last_error()
    hole = _traj()
    hole.d_len = None
    assert lib.tg_rollout_final_state(C.byref(p), C.byref(hole), FAKE, FAKE, None) == -1 and b"null pointer" in lib.tg_last_error()
    assert lib.tg_rollout_final_state(C.byref(p), C.byref(_traj(n=0)), FAKE, FAKE, None) == -1 and b"bad sizes" in lib.tg_last_error()
    assert lib.tg_rollout_final_state(C.byref(p), C.byref(_traj(T=8)), FAKE, FAKE, None) == -1
    assert b"horizon 8 != env.max_steps 16" in lib.tg_last_error()
    # a swarm: an error status of its own and the reason
    swarm = N.default_params(N.TG_ENV_QUADPOLE, 16)
    swarm.agents = 8
    assert lib.tg_rollout_final_state(C.byref(swarm), C.byref(tr), FAKE, FAKE, None) == N.TG_ERR_UNSUPPORTED == -3
    assert b"swarm envs (agents=8) are not supported" in lib.tg_last_error()
    # the 12-state quadrotor has no episodes; an unknown dtype
    q12 = N.default_params(N.TG_ENV_QUADROTOR12, 16)
    assert lib.tg_rollout_final_state(C.byref(q12), C.byref(tr), FAKE, FAKE, None) == -3 and b"unsupported env_id" in lib.tg_last_error()
    assert lib.tg_rollout_final_state(C.byref(p), C.byref(_traj(dtype=7)), FAKE, FAKE, None) == -3


def test_ppo_returns_boot_refusals():
    lib = N.load()
    ok = [FAKE, FAKE, FAKE, FAKE, FAKE, 0.99, 0.95, 1, FAKE, FAKE + 64, 8, 16, FAKE, FAKE, None]
    for hole in (0, 1, 2, 3, 4, 8, 9, 12, 13):
        args = list(ok)
        args[hole] = None
        assert lib.tg_ppo_returns_boot(*args) == -1 and b"tg_ppo_returns_boot: null pointer" in lib.tg_last_error(), hole
    for n, T in ((0, 16), (-1, 16), (8, 0)):
        args = list(ok)
        args[10], args[11] = n, T
        assert lib.tg_ppo_returns_boot(*args) == -1 and b"tg_ppo_returns_boot: bad sizes" in lib.tg_last_error()
    args = list(ok)
    args[9] = args[8]
    assert lib.tg_ppo_returns_boot(*args) == -1 and b"distinct buffers" in lib.tg_last_error()
