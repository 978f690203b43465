"""The sampling and reset kernels against the fp64 restatement of their draws (tests/philox_fp64.py).

Every other parity test replays the kernels' own draws, so none of them can see a wrong draw.  Here:
  * tg_rollout_step with mean 0 and sigma 1 records eps itself; every (env, t, k) must equal the fp64 Box-Muller of the
    restated Philox words within a bound derived from the hardware instructions' errors (below);
  * every sampling path (eager per-step, captured graph, fp32 fused at 16 and 32 envs per workgroup, bf16 fused in both wave
    variants) must, on three successive rollouts, draw stream k's noise and reset from host stream k, rollout k differing from
    rollout k - 1;
  * tg_env_reset of every env, fp64 and fp32, against the fp64 reset maps, and a KS test of a 2^20-env reset's own angles
    against the reference's ranges.

Error bound of one eps component, eps = sqrt(-2 ln u) * cos(2 pi v) in fp32 (env_kernels.hip): with d_ln = ln2 LOG2_ABS_ERR
+ 2 u |ln u| the error of the computed ln u (v_log_f32, then the product with ln 2 rounded to fp32), r^2 = -2 ln u is off by
at most 2 d_ln, so r = sqrt(r^2) is off by at most min(2 d_ln / r, sqrt(2 d_ln)) (the second term rules as u -> 1, where r -> 0)
plus v_sqrt_f32's 1 ulp; the product with cos / sin adds r TRIG_ABS_ERR and one rounding.

The two instruction constants are ASSUMED, not measured: no accuracy figure of v_log_f32 / v_sin_f32 / v_cos_f32 on gfx950 is
published.  Each test prints the largest error it observed; an observed error beyond the assumption is to be examined, not
absorbed by a wider bound."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import philox_fp64 as P

pytestmark = pytest.mark.gpu

U = 2.0 ** -24                      # fp32 unit roundoff
LOG2_ABS_ERR = 2.0 ** -19           # assumed |v_log_f32(u) - log2(u)| for u in [2^-24, 1]: 1 ulp of |log2 u| <= 24
TRIG_ABS_ERR = 2.0 ** -20           # assumed |v_sin_f32(v) - sin(2 pi v)|, |v_cos_f32(v) - cos(2 pi v)| for v in (0, 1] (revolutions)
SQRT_REL_ERR = 2.0 ** -23           # v_sqrt_f32: 1 ulp
EPS_MAX = math.sqrt(-2.0 * math.log(2.0 ** -24))      # ~5.77: u01 has 24 bits, so no |eps| can exceed this (intrinsic)

OBSERVED = {}                        # largest |kernel - fp64| per path, printed by every test that adds to it


@pytest.fixture(scope="module")
def tg():
    import trajopt_grpo_amd as tg
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return tg


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def eps_bound(eps, ur, ut, is_sin):
    """Bound on |fp32 kernel eps - fp64 eps| per component (module docstring)."""
    lnu = np.log(ur)
    r = np.sqrt(-2.0 * lnu)
    d_r2 = 2.0 * (math.log(2.0) * LOG2_ABS_ERR + 2.0 * U * np.abs(lnu))
    with np.errstate(divide="ignore"):
        e_rad = np.minimum(np.where(r > 0, d_r2 / np.where(r > 0, r, 1.0), np.inf), np.sqrt(d_r2))
    e_rad = e_rad + SQRT_REL_ERR * (r + e_rad)
    trig = np.where(is_sin > 0, np.abs(np.sin(2 * math.pi * ut)), np.abs(np.cos(2 * math.pi * ut)))
    rad_max = r + e_rad
    b = e_rad * (trig + TRIG_ABS_ERR) + rad_max * TRIG_ABS_ERR
    return (b + U * (np.abs(eps) + b)) * (1.0 + 1e-6)


def check_eps(got, seed, stream, env_offset, mask, tag):
    """got: the recorded actions [A][T][n] (mean 0, sigma 1); mask [T][n] of the steps to check (the rest must be 0)."""
    A, T, n = got.shape
    want, ur, ut, is_sin = P.sample_eps(seed, stream, env_offset + np.arange(n), T, A)
    m = np.broadcast_to(mask, got.shape)
    assert not got[~m].any(), f"{tag}: a step that was not alive holds an action"
    err = np.abs(got - want)[m]
    bound = eps_bound(want, ur, ut, is_sin)[m]
    bad = err > bound
    j = int(np.argmax(err / bound))
    assert not bad.any(), (f"{tag}: {int(bad.sum())} of {bad.size} eps out of bound; worst |err| {err[j]:.3e} at bound {bound[j]:.3e} "
                           f"(u_radius {ur[m][j]:.9g}, u_angle {ut[m][j]:.9g}, fp64 eps {want[m][j]:.6g})")
    assert np.abs(got[m]).max() <= EPS_MAX * (1 + U) + bound.max()
    OBSERVED[tag] = max(OBSERVED.get(tag, 0.0), float(err.max()))
    print(f"\n[rng] {tag}: max |eps - fp64| = {err.max():.3e} (max err / bound {float((err / bound).max()):.3f}) over {err.size} "
          f"draws; assumed LOG2_ABS_ERR = 2^{math.log2(LOG2_ABS_ERR):.0f}, TRIG_ABS_ERR = 2^{math.log2(TRIG_ABS_ERR):.0f}")
    return err.max()


def kernel_draws(tg, eng, seed, stream, env_offset, dev):
    """eps [A][T][n] of tg_rollout_step with mean 0 and sigma 1 (it records rn_add(0, rn_mul(1, eps)) == eps), every env made
    alive again in front of each step, with the device RNG state (seed, stream) and global env offset given."""
    Nn = tg._native
    A, T, n = eng.A, eng.T, eng.n
    zeros, ones = torch.zeros(n, A, device=dev), (C.c_float * A)(*([1.0] * A))
    lib, st = Nn.load(), Nn.stream_ptr(dev)
    eng._seed_host, eng._stream_host = 0, 0
    rng = torch.tensor([seed, stream], dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        eng._enqueue_prepare(None)
        tr = eng.traj.native()
        for t in range(T):
            eng.traj.len.zero_()
            Nn.check(lib.tg_rollout_step(C.byref(eng.params), C.byref(tr), t, zeros.data_ptr(), A, ones, rng.data_ptr(),
                                         env_offset, st), "tg_rollout_step")
    torch.cuda.synchronize()
    return eng.traj.act.clone()


def zero_policy(tg, S, A, hidden, dev):
    torch.manual_seed(0)
    pol = tg.GaussianActor_NeuralNetwork(S, A, hidden, cov=1.0, device=dev)
    with torch.no_grad():
        for p in pol.actor.parameters():
            p.zero_()
    return pol


# ------------------------------------------------------------------------------------------------------------------------------
# 2. the per-step sampling kernel
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["CartPole", "QuadPole2D", "QuadPole"])
def test_per_step_kernel_draws_are_the_fp64_box_muller_of_philox(tg, dev, name):
    """A = 1, 2, 4 (all four words), n = 300 (not a multiple of 64), 64-bit seeds and env offsets, several streams."""
    env = tg.environments.ENV_CLASSES[name](max_steps=6)
    S, A = env.obs_dim, env.act_dim
    eng = tg.DeviceRollout(env, zero_policy(tg, S, A, (64,), dev), 3, 100, fused=False, use_graph=False)
    assert eng.n % 64 != 0
    mask = np.ones((eng.T, eng.n), dtype=bool)
    for seed in (0, 5, 2 ** 40 + 3):
        for env_offset in (0, 2 ** 32 + 7):
            for stream in (0, 1, 7):
                got = kernel_draws(tg, eng, seed, stream, env_offset, dev).double().cpu().numpy()
                check_eps(got, seed, stream, env_offset, mask, f"per-step {name}")


# ------------------------------------------------------------------------------------------------------------------------------
# 3. successive rollouts on every sampling path
# ------------------------------------------------------------------------------------------------------------------------------
def reset_bound_f32(name, ang):
    """fp32 reset: the angle rounded to fp32 (U |angle|), sincosf (2 ulp), and for QuadPole the quaternion product, norm and
    division (a few ulp more)."""
    a = np.abs(ang.get("theta", ang.get("alpha")))
    return (2.0 * U * a + 8.0 * U) if name != "QuadPole" else np.full_like(a, 32.0 * U)


PATHS = [  # (path, restart, group_offset, seed)
    ("eager", False, 0, 77), ("eager", True, 2, 2 ** 40 + 3),
    ("graph", False, 3, 78), ("graph", True, 0, 79),
    ("f32x16", True, 1, 80), ("f32x32", False, 2, 81),
    ("bf16-4wave", True, 1, 82), ("bf16-8wave", False, 1, 83),
]


@pytest.mark.parametrize("path,restart,group_offset,seed", PATHS, ids=[f"{p[0]}-restart{int(p[1])}-go{p[2]}" for p in PATHS])
def test_successive_rollouts_draw_stream_k(tg, dev, path, restart, group_offset, seed):
    """A policy whose actor weights and biases are zero (mean exactly 0) with cov = 1: the recorded actions ARE the draws.  For
    rollouts k = 0, 1, 2 of one engine: every alive action is the fp64 eps of stream k (and bit for bit the per-step kernel's
    draw of stream k), the initial states are the fp64 reset of host stream k, and nothing repeats rollout k - 1."""
    name, S, A = "QuadPole", 20, 4
    G, E, T = (8, 4100, 6) if path == "bf16-8wave" else (3, 37, 12)
    env = tg.QuadPole(max_steps=T)
    if path.startswith("bf16"):
        pol = zero_policy(tg, S, A, (128, 128), dev)
        kw = dict(compute_dtype=torch.bfloat16, fused=True)
    else:
        pol = zero_policy(tg, S, A, (64, 64), dev)
        kw = dict(fused=True) if path.startswith("f32") else dict(fused=False, use_graph=(path == "graph"))
    eng = tg.DeviceRollout(env, pol, G, E, restart=restart, seed=seed, group_offset=group_offset,
                           global_groups=G + group_offset, **kw)
    if path.startswith("f32"):
        eng.f32_block_envs = 16 if path == "f32x16" else 32
    assert eng.fused == (path not in ("eager", "graph")) and [float(v) for v in eng._sigma] == [1.0] * A
    if path == "bf16-8wave":
        assert eng.n >= 32768 and eng.n % 256 != 0
    elif path == "bf16-4wave":
        assert eng.n < 32768
    helper = tg.DeviceRollout(tg.QuadPole(max_steps=T), pol, G, E, fused=False, use_graph=False)
    n, off = eng.n, group_offset * eng.E
    prev = None
    for k in range(3):
        tr = eng.run()
        torch.cuda.synchronize()
        act, mask, obs0 = tr.act.clone(), tr.mask.bool().clone(), tr.obs[:, 0, :].double().cpu().numpy()
        if path.startswith("f32"):
            assert eng._f32_block_envs == eng.f32_block_envs
        assert bool(mask[0].all())
        check_eps(act.double().cpu().numpy(), seed, k, off, mask.cpu().numpy(), path)
        draws = kernel_draws(tg, helper, seed, k, off, dev)
        assert torch.equal(act[:, mask], draws[:, mask]), f"rollout {k}: not the per-step kernel's draws of stream {k}"
        want, ang = P.reset_states(name, seed, k, n, key_offset=off, key_div=eng.E if restart else 1)
        err = np.abs(obs0 - want)
        assert (err <= reset_bound_f32(name, ang)[None, :]).all(), f"rollout {k}: initial states off by {err.max():.3e}"
        if restart:
            assert np.array_equal(obs0[:, :eng.E], np.repeat(obs0[:, :1], eng.E, axis=1))
        if prev is not None:
            assert bool((act[:, 0, :] != prev[0][:, 0, :]).all()), f"rollout {k} repeats noise of rollout {k - 1}"
            assert (obs0 != prev[1]).any(axis=0).all(), f"rollout {k} repeats initial states of rollout {k - 1}"
        prev = (act, obs0)


# ------------------------------------------------------------------------------------------------------------------------------
# 4. the reset kernel
# ------------------------------------------------------------------------------------------------------------------------------
RESET_ENVS = ["CartPole", "QuadPole2D", "QuadPole", "Pendulum", "PendulumSwingup"]


def make_env(tg, name, T=8, **kw):
    if name == "PendulumSwingup":
        return tg.Pendulum(swingup=True, max_steps=T, **kw)
    return tg.environments.ENV_CLASSES[name](max_steps=T, **kw)


def kernel_reset(tg, dev, name, dtype, n, seed, stream, key_offset, key_div):
    Nn = tg._native
    env = make_env(tg, name)
    p = env.native_params()
    state = torch.full((env.obs_dim, n), float("nan"), dtype=dtype, device=dev)
    with torch.cuda.device(dev):
        Nn.check(Nn.load().tg_env_reset(C.byref(p), Nn.dtype_code(dtype), state.data_ptr(), n, n, seed, stream, key_offset,
                                        key_div, Nn.stream_ptr(dev)), "tg_env_reset")
    torch.cuda.synchronize()
    return state.double().cpu().numpy()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", RESET_ENVS)
def test_reset_kernel_matches_the_fp64_maps(tg, dev, name, dtype):
    """tg_env_reset against the fp64 maps: fp64 within a few ulp, fp32 within the rounding of the fp32 angle and sincosf; 64-bit
    seeds and key offsets, key_div > 1, and Pendulum's swingup passed through the env params."""
    n = 1000
    worst = 0.0
    for seed, stream, key_offset, key_div in [(7, 0, 0, 1), (2 ** 40 + 3, 5, 2 ** 32 + 11, 1), (123, 2, 2 ** 32 + 5, 7),
                                              (0, 3, 64, 25)]:
        got = kernel_reset(tg, dev, name, dtype, n, seed, stream, key_offset, key_div)
        want, ang = P.reset_states(name, seed, stream, n, key_offset, key_div)
        err = np.abs(got - want)
        if dtype == torch.float64:
            tol = np.full(n, 8e-15 if name == "QuadPole" else 4e-15)
        else:
            tol = reset_bound_f32(name, ang)
        assert (err <= tol[None, :]).all(), (seed, stream, key_offset, key_div, float(err.max()))
        worst = max(worst, float(err.max()))
    print(f"\n[rng] reset {name} {dtype}: max |state - fp64| = {worst:.3e}")


@pytest.mark.parametrize("name", ["CartPole", "QuadPole", "PendulumSwingup"])
def test_scalar_env_reset_draws_stream_reset_count(tg, dev, name):
    """Env.reset(): the k-th call draws host stream k (k = 1, 2, ...) of the env's `_seed`, key 0 (environments.py)."""
    env = make_env(tg, name, device=dev)
    assert 0 <= env._seed < 2 ** 31
    env._seed = 2 ** 33 + 17
    for k in (1, 2, 3):
        obs, _ = env.reset()
        want, _ = P.reset_states(name, env._seed, k, 1)
        assert np.abs(obs - want[:, 0]).max() <= 8e-15, (k, obs, want[:, 0])
    env.restart()
    assert np.array_equal(env._obs_np(), obs)


def recovered_angles(name, o):
    if name == "CartPole":
        return {"theta": np.arctan2(o[2], o[3])}
    if name == "QuadPole2D":
        return {"theta": np.arctan2(o[7], o[8])}
    if name == "PendulumSwingup":
        return {"theta": np.arctan2(o[0], o[1])}
    if name == "Pendulum":
        return {"theta": math.pi + np.arctan2(-o[0], -o[1])}
    return {"alpha": 2.0 * np.arctan2(o[14], o[13]), "beta": 2.0 * np.arctan2(o[15], o[13])}


KS_RANGES = {"CartPole": {"theta": (-math.pi, math.pi)}, "QuadPole2D": {"theta": (-math.pi, math.pi)},
             "PendulumSwingup": {"theta": (-math.pi, math.pi)}, "Pendulum": {"theta": (math.pi - 0.05, math.pi + 0.05)},
             "QuadPole": {"alpha": (-1.0, 1.0), "beta": (-1.0, 1.0)}}


@pytest.mark.parametrize("name", RESET_ENVS)
def test_large_reset_angles_follow_the_reference_ranges(tg, dev, name):
    """End to end, without the restatement: the angles of a 2^20-env fp64 reset, read back from the kernel's own states, against
    the reference's uniform ranges (cartpole_env.py:103, quadrotor_env.py:543-544 and :951, pendulum_env.py:89-91)."""
    n = 1 << 20
    o = kernel_reset(tg, dev, name, torch.float64, n, 2024, 1, 0, 1)
    ang = recovered_angles(name, o)
    for k, (lo, hi) in KS_RANGES[name].items():
        a = ang[k]
        assert a.min() >= lo - 1e-12 and a.max() <= hi + 1e-12, (k, a.min(), a.max())
        D, p = P.ks_pvalue(a, P.uniform_cdf(lo, hi))
        assert p > 1e-3, (k, D, p)
    if name == "QuadPole":
        assert abs(np.corrcoef(ang["alpha"], ang["beta"])[0, 1]) < 6.0 / math.sqrt(n)


# ------------------------------------------------------------------------------------------------------------------------------
# 5. a covariance the kernels cannot honour
# ------------------------------------------------------------------------------------------------------------------------------
def test_rollout_refuses_a_non_diagonal_covariance(tg, dev):
    pol = tg.GaussianActor_NeuralNetwork(10, 2, (64,), cov=[0.3, 0.2], device=dev)
    eng = tg.DeviceRollout(tg.QuadPole2D(max_steps=4), pol, 1, 8, fused=False, use_graph=False)
    eng.run()
    pol.cov = torch.tensor([[0.3, 0.1], [0.1, 0.2]])
    with pytest.raises(ValueError, match="diagonal"):
        eng.run()
