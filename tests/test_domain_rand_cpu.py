"""CPU: per-env domain randomisation -- Env.randomize() validation and metadata, the new entry points in header / exports /
binding and their argument refusals (no launch), and the self-consistency of the fp64 restatement of the draw."""
import ctypes as C
import json
import math
import os
import re

import numpy as np
import pytest

import trajopt_grpo_amd as tg

import domain_rand_fp64 as DR

N = tg._native
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENVS = {"CartPole": tg.CartPole, "Pendulum": tg.Pendulum, "QuadPole2D": tg.QuadPole2D, "QuadPole": tg.QuadPole,
        "QuadPoleSwarm": tg.QuadPoleSwarm}
NAMES = {"CartPole": "masscart masspole length gravity", "Pendulum": "mass length gravity",
         "QuadPole2D": "mq mp I Lq Lp gravity",
         "QuadPole": "mass load_mass gravity tether_length Ixx Iyy Izz torque_constant arm_length",
         "QuadPoleSwarm": "mass load_mass gravity tether_length Ixx Iyy Izz torque_constant arm_length"}
NEW_SYMBOLS = ["tg_env_randomize", "tg_rollout_step_dr", "tg_rollout_forced_dr", "tg_rollout_final_state_dr", "tg_fused_rollout_dr",
               "tg_fused_rollout_f32_dr", "tg_fused_rollout_f32_act_dr"]


@pytest.mark.parametrize("name", sorted(ENVS))
def test_randomize_accepts_exactly_the_physical_parameters(name):
    env = ENVS[name]()
    assert list(env.RANDOMIZABLE) == NAMES[name].split()
    p = env.native_params()
    for attr, idx in env.RANDOMIZABLE.items():                    # the names are the attributes _fill_params reads, at their p[] index
        assert p.p[idx] == getattr(env, attr)
    assert env.randomization is None and env.randomize_spec() is None and env.randomize_metadata() is None
    ranges = {k: (0.5, 2.0) for k in env.RANDOMIZABLE}
    assert env.randomize(ranges, seed=7) is env
    assert env.randomization == ranges
    spec = env.randomize_spec()
    assert spec.count == len(ranges) and spec.seed == 7
    assert list(spec.index)[:spec.count] == sorted(env.RANDOMIZABLE.values())
    assert all(spec.lo[k] == 0.5 and spec.hi[k] == 2.0 for k in range(spec.count))
    for off in ({}, None):
        env.randomize(ranges)
        env.randomize(off)
        assert env.randomization is None and env.randomize_spec() is None


@pytest.mark.parametrize("name", sorted(ENVS))
def test_randomize_refuses_everything_else_at_call_time(name):
    env = ENVS[name]()
    good = next(iter(env.RANDOMIZABLE))
    for key in ("spatial_bounds", "bound", "balance_radius", "swingup", "timestep", "max_steps", "no_such_parameter", "tether", "arm"):
        with pytest.raises(ValueError, match=re.escape(repr(key))):
            env.randomize({good: (0.9, 1.1), key: (0.9, 1.1)})
    for bad in ((0.0, 1.0), (-1.0, 1.0), (1.2, 1.1), (1.0, math.inf), (math.nan, 1.0), (1.0,), "ab", 3.0):
        with pytest.raises(ValueError, match=re.escape(repr(good))):
            env.randomize({good: bad})
    assert env.randomization is None                                  # a refused call leaves randomisation as it was
    env.randomize({good: (1.0, 1.0)})                                 # lo == hi is a range
    with pytest.raises(ValueError):
        env.randomize({good: (0.5, 0.4)})
    assert env.randomization == {good: (1.0, 1.0)}


def test_native_params_errors_come_first():
    env = tg.QuadPole()
    env.randomize({"mass": (0.5, 2.0)})
    env.spatial_bounds = ((-1.0, 1.5), (-1.5, 1.5), (-1.5, 1.5))
    with pytest.raises(ValueError, match="symmetric"):
        env.native_params()


def test_metadata_round_trip():
    env = tg.QuadPole2D()
    assert env.randomize_metadata() is None
    env.randomize({"mp": (0.5, 2.0), "I": (0.8, 1.25)}, seed=11)
    entry = json.loads(json.dumps(env.randomize_metadata()))
    other = tg.QuadPole2D()
    other.randomize(**entry)
    assert other.randomization == env.randomization and other.randomize_spec().seed == 11
    assert bytes(other.randomize_spec()) == bytes(env.randomize_spec())

    class Stub:
        def metadata(self):
            return {}
    pipe = tg.pipelines.Pipeline.__new__(tg.pipelines.Pipeline)
    pipe.test_name = pipe.checkpoint_name = pipe.today = "x"
    pipe.env_name = "QuadPole2D"
    pipe.policy = pipe.algorithm = pipe.buffer = Stub()
    pipe.visualizer = pipe.publisher = pipe.logger = None
    pipe.env = tg.QuadPole2D()
    assert "randomize" not in pipe.get_metadata()                     # only when it is on
    pipe.env = env
    assert pipe.get_metadata()["randomize"] == env.randomize_metadata()


def test_header_exports_and_binding_agree_on_the_new_symbols():
    lib = N.load()
    header = open(os.path.join(REPO, "include", "trajopt_grpo_hip.h")).read()
    declared = set(re.findall(r"\b(tg_[a-z0-9_]+)\s*\(", header))
    for name in NEW_SYMBOLS:
        assert name in declared and name in N.SIGNATURES and hasattr(lib, name), name
    assert lib.tg_abi_version() == 13 == N.ABI_VERSION
    assert C.sizeof(N.EnvParams) == 4 * 4 + 8 + 12 * 8 and C.sizeof(N.Traj) == 6 * 8 + 8 + 4 + 4      # layouts kept
    assert C.sizeof(N.RandomizeSpec) == 4 + 12 * 4 + 4 + 12 * 8 + 12 * 8 + 8 and N.RandomizeSpec.lo.offset == 56   # (4 B of padding)


def _spec(count=1, index=0, lo=0.5, hi=2.0):
    s = N.RandomizeSpec()
    s.count = count
    for k in range(min(count, 12)):
        s.index[k], s.lo[k], s.hi[k] = (index + k) % 12, lo, hi
    return s


def test_new_entry_points_refuse_bad_arguments_without_a_launch():
    lib = N.load()
    p = N.default_params(N.TG_ENV_QUADPOLE, 16)
    fake = C.c_void_p(4096)                                           # never dereferenced: every call below is refused on the host
    rc = lib.tg_env_randomize(C.byref(p), C.byref(_spec()), None, 8, 0, 0, 0, 1, None)
    assert rc == N.TG_ERR_ARG and b"null parameter table" in lib.tg_last_error()
    rc = lib.tg_env_randomize(C.byref(p), C.byref(_spec(count=13)), fake, 8, 0, 0, 0, 1, None)
    assert rc == N.TG_ERR_ARG and b"count" in lib.tg_last_error()
    rc = lib.tg_env_randomize(C.byref(p), C.byref(_spec(lo=1.5, hi=1.0)), fake, 8, 0, 0, 0, 1, None)
    assert rc == N.TG_ERR_ARG and b"lo <= hi" in lib.tg_last_error()
    for lo in (0.0, -0.5, math.nan):
        rc = lib.tg_env_randomize(C.byref(p), C.byref(_spec(lo=lo)), fake, 8, 0, 0, 0, 1, None)
        assert rc == N.TG_ERR_ARG and b"0 < lo" in lib.tg_last_error()
    rc = lib.tg_env_randomize(C.byref(p), C.byref(_spec(hi=math.inf)), fake, 8, 0, 0, 0, 1, None)
    assert rc == N.TG_ERR_ARG
    s = _spec(count=2)
    s.index[1] = s.index[0]
    rc = lib.tg_env_randomize(C.byref(p), C.byref(s), fake, 8, 0, 0, 0, 1, None)
    assert rc == N.TG_ERR_ARG and b"twice" in lib.tg_last_error()
    s = _spec()
    s.index[0] = 12
    assert lib.tg_env_randomize(C.byref(p), C.byref(s), fake, 8, 0, 0, 0, 1, None) == N.TG_ERR_ARG
    assert lib.tg_env_randomize(C.byref(p), C.byref(_spec()), fake, 8, 0, 0, 0, 0, None) == N.TG_ERR_ARG     # key_div < 1
    assert lib.tg_env_randomize(C.byref(p), None, fake, 8, 0, 0, 0, 1, None) == N.TG_ERR_ARG
    # the `_dr` siblings: a null table is refused before anything else is looked at
    tr = N.Traj()
    sigma = (C.c_float * 4)(1, 1, 1, 1)
    assert lib.tg_rollout_step_dr(C.byref(p), None, C.byref(tr), 0, None, 0, None, None, 0, None) == N.TG_ERR_ARG
    assert b"null parameter table" in lib.tg_last_error()
    assert lib.tg_rollout_forced_dr(C.byref(p), None, C.byref(tr), 0, 1, None) == N.TG_ERR_ARG
    assert lib.tg_rollout_final_state_dr(C.byref(p), None, C.byref(tr), None, None, None) == N.TG_ERR_ARG
    assert lib.tg_fused_rollout_dr(C.byref(p), None, C.byref(tr), None, None, 128, 2, sigma, None, 0, 0, 1, None) == N.TG_ERR_ARG
    assert lib.tg_fused_rollout_f32_dr(C.byref(p), None, C.byref(tr), None, None, 64, 2, 32, sigma, None, 0, 0, 1, None) == N.TG_ERR_ARG
    assert lib.tg_fused_rollout_f32_act_dr(C.byref(p), None, C.byref(tr), None, None, 64, 2, 32, sigma, None, 0, 0, 1, 0, None) == N.TG_ERR_ARG
    # ... and with a table, what the plain entry points refuse is still refused (null trajectory pointers here)
    assert lib.tg_rollout_step_dr(C.byref(p), fake, C.byref(tr), 0, None, 0, None, None, 0, None) == N.TG_ERR_ARG
    assert lib.tg_rollout_forced_dr(C.byref(p), fake, C.byref(tr), 0, 1, None) == N.TG_ERR_ARG
    assert lib.tg_rollout_final_state_dr(C.byref(p), fake, C.byref(tr), None, None, None) == N.TG_ERR_ARG
    assert lib.tg_fused_rollout_f32_act_dr(C.byref(p), fake, C.byref(tr), None, None, 64, 2, 32, sigma, None, 0, 0, 1, 7, None) == N.TG_ERR_ARG


# ---- the fp64 restatement of the draw ----
SPEC = [(0, 0.5, 2.0), (1, 0.8, 1.25), (3, 1.0, 1.0), (4, 0.25, 4.0), (8, 0.9, 0.95)]
NOMINAL = [1.5, 0.5, 9.80665, 0.5, 0.4, 0.4, 0.25, 0.1, 0.5, 1.5, 0.0, 0.0]


def test_restated_factors_lie_in_their_ranges_and_fill_them():
    f = DR.factors(SPEC, seed=3, stream=5, n=4096)
    for k, (_, lo, hi) in enumerate(SPEC):
        assert f[k].min() >= lo and f[k].max() <= hi
        if hi > lo:
            assert f[k].min() < lo + 0.01 * (hi - lo) and f[k].max() > hi - 0.01 * (hi - lo)     # 4,096 uniform draws
            assert abs(f[k].mean() - 0.5 * (lo + hi)) < 4 * (hi - lo) / math.sqrt(12 * 4096)
    assert np.all(f[2] == 1.0)
    # the two parameters of one draw, and the draws of different sub values, are different numbers
    u = [(f[k] - lo) / (hi - lo) for k, (_, lo, hi) in enumerate(SPEC) if hi > lo]
    for a in range(len(u)):
        for b in range(a + 1, len(u)):
            assert abs(np.corrcoef(u[a], u[b])[0, 1]) < 0.08
    tab = DR.table(NOMINAL, SPEC, 3, 5, 4096)
    for r in range(12):
        if r not in [s[0] for s in SPEC] or r == 3:
            assert np.all(tab[r] == NOMINAL[r])                        # un-randomised rows (and a (1, 1) range): the nominal value, exactly


def test_restated_draw_changes_with_every_key_word():
    base = DR.factors(SPEC, seed=3, stream=5, n=256)
    assert not np.array_equal(base[0], DR.factors(SPEC, seed=4, stream=5, n=256)[0])
    assert not np.array_equal(base[0], DR.factors(SPEC, seed=3, stream=6, n=256)[0])           # re-drawn every rollout
    assert not np.array_equal(base[0], DR.factors(SPEC, seed=3, stream=5, n=256, randomize_seed=1)[0])
    assert DR.combined_seed(3, 0) == 3
    # the sub values are not the reset's, nor a time step's
    assert DR.SUB_FIRST - (12 // 2 - 1) > 2 ** 31 and DR.SUB_FIRST < 0xFFFFFFFF


def test_restated_draw_shares_a_group_and_ignores_sharding():
    E, G = 8, 32
    n = E * G
    f = DR.factors(SPEC, seed=9, stream=2, n=n, key_div=E)
    g = f.reshape(len(SPEC), G, E)
    assert np.all(g == g[:, :, :1])                                    # restart: the E episodes of a group share one vehicle
    assert len(np.unique(g[0, :, 0])) == G
    for key_div in (1, E):
        whole = DR.table(NOMINAL, SPEC, 9, 2, n, key_div=key_div)
        lo = DR.table(NOMINAL, SPEC, 9, 2, 96, key_offset=0, key_div=key_div)
        hi = DR.table(NOMINAL, SPEC, 9, 2, n - 96, key_offset=96, key_div=key_div)
        assert np.array_equal(np.concatenate([lo, hi], axis=1), whole)
