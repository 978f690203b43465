"""CPU: the vector env's ABI (tg_vec_env, tg_vec_env_step, tg_vec_env_reset_all) and DeviceVecEnv's host side -- symbols, struct
layout, every host-side refusal (code and message, nothing launched: the pointers handed over are not device memory), the spaces."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import trajopt_grpo_amd as tg

N = tg._native
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(REPO, "include", "trajopt_grpo_hip.h")).read()
FAKE = 0x10000          # a non-null, 16-byte aligned address no refused call may touch


def test_symbols_are_declared_bound_and_exported_and_the_abi_is_still_13():
    lib = N.load()
    for name in ("tg_vec_env_step", "tg_vec_env_reset_all"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", HEADER), f"{name} is not declared"
        assert name in N.SIGNATURES and hasattr(lib, name)
    assert "typedef struct tg_vec_env {" in HEADER
    assert lib.tg_abi_version() == N.ABI_VERSION == 13
    assert int(re.search(r"#define\s+TG_ABI_VERSION\s+(\d+)", HEADER).group(1)) == 13
    assert tg.DeviceVecEnv is tg.vector.DeviceVecEnv and "DeviceVecEnv" in tg.__all__


def test_vec_env_struct_layout_matches_the_header():
    body = re.search(r"typedef struct tg_vec_env \{(.*?)\} tg_vec_env;", HEADER, re.S).group(1)
    fields = re.findall(r"^\s*([A-Za-z0-9_]+\s*\*?)\s+([a-z_]+);", body, re.M)
    size = {"void*": 8, "int32_t*": 8, "double*": 8, "uint32_t*": 8, "int64_t": 8, "uint64_t": 8, "int32_t": 4}
    assert [name for _, name in fields] == [name for name, _ in N.VecEnv._fields_]
    off = 0
    for ctype, name in fields:
        width = size[ctype.replace(" ", "")]
        off = (off + width - 1) // width * width
        assert getattr(N.VecEnv, name).offset == off and getattr(N.VecEnv, name).size == width, name
        off += width
    assert C.sizeof(N.VecEnv) == off == 72
    assert N.VecEnv.n.offset == 40 and N.VecEnv.seed.offset == 56 and N.VecEnv.horizon.offset == 64 and N.VecEnv.dtype.offset == 68


def make_vec(n=8, horizon=16, dtype=N.TG_F32, env_offset=0, **null):
    v = N.VecEnv()
    for name in ("d_state", "d_steps", "d_balanced", "d_ep_return", "d_episode"):
        setattr(v, name, None if null.get(name) else FAKE)
    v.n, v.env_offset, v.seed, v.horizon, v.dtype = n, env_offset, 1, horizon, dtype
    return v


def step(p, v, *, ptab=None, substeps=1, motor=None, actions=FAKE, outs=None):
    outs = [FAKE] * 7 if outs is None else outs
    rc = N.load().tg_vec_env_step(None if p is None else C.byref(p), ptab, substeps, motor, None if v is None else C.byref(v), actions,
                                  *outs, None)
    return rc, N.load().tg_last_error().decode()


def params(env_id, max_steps=16):
    return N.default_params(env_id, max_steps)


def test_step_refuses_null_pointers():
    p = params(N.TG_ENV_CARTPOLE)
    for rc, msg in (step(None, make_vec()), step(p, None), step(p, make_vec(), actions=None),
                    *(step(p, make_vec(), outs=[None if j == k else FAKE for j in range(7)]) for k in range(7)),
                    *(step(p, make_vec(**{name: True})) for name in ("d_state", "d_steps", "d_balanced", "d_ep_return", "d_episode"))):
        assert rc == N.TG_ERR_ARG and "tg_vec_env_step: null pointer" in msg, (rc, msg)


def test_step_refuses_bad_sizes_and_alignment():
    p = params(N.TG_ENV_QUADPOLE)
    for v in (make_vec(n=0), make_vec(n=-3), make_vec(horizon=0), make_vec(env_offset=-1)):
        rc, msg = step(p, v)
        assert rc == N.TG_ERR_ARG and "bad sizes" in msg, (rc, msg)
    rc, msg = step(p, make_vec(horizon=15))
    assert rc == N.TG_ERR_ARG and "horizon 15 x substeps 1 != env.max_steps 16" in msg
    rc, msg = step(p, make_vec(), actions=FAKE + 8)
    assert rc == N.TG_ERR_ARG and "d_actions must be aligned to a row (16 bytes)" in msg
    rc, msg = step(p, make_vec(), outs=[FAKE + 4] + [FAKE] * 6)
    assert rc == N.TG_ERR_ARG and "16-byte aligned" in msg


def test_step_refuses_swarms_unknown_envs_and_dtypes():
    p = params(N.TG_ENV_QUADPOLE)
    p.agents = 8
    rc, msg = step(p, make_vec())
    assert rc == N.TG_ERR_UNSUPPORTED and "swarm envs (agents=8) are not supported" in msg
    p = params(N.TG_ENV_QUADROTOR12)
    rc, msg = step(p, make_vec(horizon=p.max_steps))
    assert rc == N.TG_ERR_UNSUPPORTED and "unsupported env_id 3" in msg
    p = params(N.TG_ENV_CARTPOLE)
    p.env_id = 9
    rc, msg = step(p, make_vec())
    assert rc == N.TG_ERR_UNSUPPORTED and "unsupported env_id 9" in msg
    rc, msg = step(params(N.TG_ENV_CARTPOLE), make_vec(dtype=2))
    assert rc == N.TG_ERR_UNSUPPORTED and "unsupported dtype 2" in msg


def test_step_refuses_substeps_out_of_range_and_on_pendulum():
    p = params(N.TG_ENV_QUADPOLE2D)
    for k in (0, -1, 65):
        rc, msg = step(p, make_vec(), substeps=k)
        assert rc == N.TG_ERR_ARG and f"substeps={k} outside [1, 64]" in msg, (rc, msg)
    rc, msg = step(params(N.TG_ENV_QUADPOLE2D, 48), make_vec(horizon=16), substeps=2)
    assert rc == N.TG_ERR_ARG and "horizon 16 x substeps 2 != env.max_steps 48" in msg
    pend = params(N.TG_ENV_PENDULUM, 32)
    rc, msg = step(pend, make_vec(horizon=16), substeps=2)
    assert rc == N.TG_ERR_UNSUPPORTED and "Pendulum takes substeps = 1 only" in msg


def test_step_refuses_a_motor_state_where_there_is_no_rotor_or_no_time_constant():
    for env_id in (N.TG_ENV_CARTPOLE, N.TG_ENV_PENDULUM):
        rc, msg = step(params(env_id), make_vec(), motor=FAKE)
        assert rc == N.TG_ERR_UNSUPPORTED and "has no rotors to lag" in msg, (rc, msg)
    p = params(N.TG_ENV_QUADPOLE)                       # p[10] == 0 without a table: the lag is off, a motor state is a mistake
    rc, msg = step(p, make_vec(), motor=FAKE)
    assert rc == N.TG_ERR_ARG and "motor time constant" in msg


def test_reset_all_refusals():
    lib = N.load()

    def reset(p, v, motor=None, obs=FAKE):
        rc = lib.tg_vec_env_reset_all(None if p is None else C.byref(p), motor, None if v is None else C.byref(v), 1, obs, None)
        return rc, lib.tg_last_error().decode()

    p = params(N.TG_ENV_CARTPOLE)
    for rc, msg in (reset(None, make_vec()), reset(p, None), reset(p, make_vec(), obs=None), reset(p, make_vec(d_episode=True))):
        assert rc == N.TG_ERR_ARG and "tg_vec_env_reset_all: null pointer" in msg, (rc, msg)
    rc, msg = reset(p, make_vec(n=0))
    assert rc == N.TG_ERR_ARG and "bad sizes" in msg
    rc, msg = reset(p, make_vec(), motor=FAKE)
    assert rc == N.TG_ERR_UNSUPPORTED and "has no rotors to lag" in msg
    rc, msg = reset(p, make_vec(dtype=5))
    assert rc == N.TG_ERR_UNSUPPORTED and "unsupported dtype 5" in msg
    rc, msg = reset(p, make_vec(), obs=FAKE + 4)
    assert rc == N.TG_ERR_ARG and "16-byte aligned" in msg
    q = params(N.TG_ENV_QUADPOLE)
    q.agents = 2
    rc, msg = reset(q, make_vec())
    assert rc == N.TG_ERR_UNSUPPORTED and "swarm envs" in msg


def test_device_vec_env_has_no_cpu_fallback_and_refuses_swarms():
    with pytest.raises(N.NativeLibraryError, match="no CPU fallback"):
        tg.DeviceVecEnv(tg.CartPole(max_steps=8), 4, device="cpu")
    with pytest.raises(ValueError, match="swarm"):
        tg.DeviceVecEnv(tg.QuadPoleSwarm(n_agents=4, max_steps=8), 4, device="cpu")
    with pytest.raises(ValueError, match="num_envs"):
        tg.DeviceVecEnv(tg.CartPole(max_steps=8), 0, device="cpu")


@pytest.mark.parametrize("name, S, A", [("CartPole", 5, 1), ("Pendulum", 3, 1), ("QuadPole2D", 10, 2), ("QuadPole", 20, 4)])
def test_spaces_have_the_envs_shapes_and_bounds(name, S, A):
    env = tg.environments.ENV_CLASSES[name]()
    single_obs, single_act, obs, act = tg.vector.vector_spaces(env, 7)
    assert single_obs is env.observation_space and single_act is env.action_space
    assert single_obs.shape == (S,) and single_act.shape == (A,) and obs.shape == (7, S) and act.shape == (7, A)
    assert obs.dtype == single_obs.dtype and act.dtype == np.float32
    for k in range(7):
        assert np.array_equal(obs.low[k], single_obs.low) and np.array_equal(obs.high[k], single_obs.high)
        assert np.array_equal(act.low[k], single_act.low) and np.array_equal(act.high[k], single_act.high)
    if name in ("CartPole", "Pendulum"):                 # (the quadrotors declare the reference's [0, 20] thrust box)
        assert np.all(act.low == -1) and np.all(act.high == 1) and np.all(obs.low == -1) and np.all(obs.high == 1)
    else:
        assert np.all(act.low == 0) and np.all(act.high == 20) and np.all(np.isinf(obs.low)) and np.all(np.isinf(obs.high))
    inside = np.broadcast_to(single_act.high, (7, A)).astype(np.float32)
    assert act.contains(inside) and not act.contains(inside + 1) and not act.contains(inside[:6])
    assert act.sample().shape == (7, A)
