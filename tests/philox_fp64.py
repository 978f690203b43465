"""Plain restatement of the project's random draws (csrc/tg_common.hpp, env_kernels.hip, env_dynamics.hpp), for the tests.

Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC 2011) in Python integers and in
vectorised numpy uint64, with the counter and key of `Philox::draw`:

    counter = (idx lo, idx hi, sub, stream),  key = (seed lo, seed hi)
    sub = t for the sampling draw of step t,  sub = 0xFFFFFFFF for a reset

then the uniforms `u01` / `u01d`, the Box-Muller transform of the sampling kernels evaluated in fp64, and every env's reset map
in fp64.  Nothing here calls the library: the GPU tests compare the kernels with these functions."""
import math

import numpy as np

MASK = 0xFFFFFFFF
M0, M1 = 0xD2511F53, 0xCD9E8D57            # round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85            # Weyl key increments
SUB_RESET = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """One block: ctr = 4 words, key = 2 words, all Python ints < 2^32 -> 4 words."""
    c0, c1, c2, c3 = (int(x) & MASK for x in ctr)
    k0, k1 = (int(x) & MASK for x in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return [c0, c1, c2, c3]


def philox4x32_10_np(c0, c1, c2, c3, k0, k1):
    """The same block on arrays (any broadcastable shapes of values < 2^32) -> 4 uint64 arrays of words."""
    m = np.uint64(MASK)
    c = [np.asarray(x, dtype=np.uint64) & m for x in (c0, c1, c2, c3)]
    c0, c1, c2, c3 = np.broadcast_arrays(*c)
    k0 = np.asarray(k0, dtype=np.uint64) & m
    k1 = np.asarray(k1, dtype=np.uint64) & m
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2           # < 2^64: exact in uint64
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & m, (p0 >> s32) ^ c3 ^ k1, p0 & m
        k0, k1 = (k0 + np.uint64(W0)) & m, (k1 + np.uint64(W1)) & m
    return c0, c1, c2, c3


def draw(seed, idx, sub, stream):
    """Philox::draw for one (seed, idx, sub, stream) -> 4 words."""
    return philox4x32_10((idx & MASK, (idx >> 32) & MASK, sub, stream), (seed & MASK, (seed >> 32) & MASK))


def draw_np(seed, idx, sub, stream):
    """Philox::draw on arrays: seed and idx are 64-bit (uint64 or Python ints), sub and stream 32-bit."""
    seed = np.asarray(seed, dtype=np.uint64)
    idx = np.asarray(idx, dtype=np.uint64)
    m, s32 = np.uint64(MASK), np.uint64(32)
    return philox4x32_10_np(idx & m, idx >> s32, sub, stream, seed & m, seed >> s32)


def u01(w):
    """Philox::u01: the top 24 bits of a word, uniform in (0, 1] (exact in fp32 and fp64)."""
    return ((np.asarray(w, dtype=np.uint64) >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24


def u01d(a, b):
    """Philox::u01d: 53 bits of two words, uniform in [0, 1)."""
    a, b = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)
    return (((a << np.uint64(32)) | b) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def box_muller(words, A):
    """fp64 eps[k] of one draw's 4 words (arrays): eps[2h] = sqrt(-2 ln u01(w[2h])) cos(2 pi u01(w[2h+1])), eps[2h+1] the same
    with sin.  -> list of A arrays, and the (u_radius, u_angle) of each component for the error bound."""
    eps, us = [], []
    for h in range((A + 1) // 2):
        ur, ut = u01(words[2 * h]), u01(words[2 * h + 1])
        rad = np.sqrt(-2.0 * np.log(ur))
        eps += [rad * np.cos(2.0 * math.pi * ut), rad * np.sin(2.0 * math.pi * ut)]
        us += [(ur, ut, 0), (ur, ut, 1)]
    return eps[:A], us[:A]


def sample_eps(seed, stream, env_idx, T, A):
    """eps of the sampling kernels for global env indices `env_idx` (1-D) and steps 0..T-1 -> fp64 [A][T][n] (the layout of
    the trajectory's `act`), plus u_radius, u_angle, is_sin of the same shape."""
    idx = np.asarray(env_idx, dtype=np.uint64)[None, :]
    t = np.arange(T, dtype=np.uint64)[:, None]
    words = draw_np(seed, idx, t, stream & MASK)
    eps, us = box_muller(words, A)
    return (np.stack(eps), np.stack([u[0] for u in us]), np.stack([u[1] for u in us]),
            np.stack([np.full_like(u[0], u[2]) for u in us]))


# ---- reset maps (env_dynamics.hpp, after the reference's cartpole_env.py:102-119, quadrotor_env.py:530-576 and :930-961,
# pendulum_env.py:86-106) ----
ENV_DIMS = {"CartPole": 5, "QuadPole2D": 10, "QuadPole": 20, "Pendulum": 3, "PendulumSwingup": 3}


def reset_angles(name, words):
    """The sampled angles of a reset: {name: fp64 array}."""
    u = u01d(words[0], words[1])
    if name in ("CartPole", "QuadPole2D", "PendulumSwingup"):
        return {"theta": -math.pi + 2.0 * math.pi * u}
    if name == "Pendulum":
        return {"theta": (math.pi - 0.05) + 0.1 * u}
    if name == "QuadPole":
        return {"alpha": -1.0 + 2.0 * u, "beta": -1.0 + 2.0 * u01d(words[2], words[3])}
    raise KeyError(name)


def reset_states(name, seed, stream, n, key_offset=0, key_div=1):
    """fp64 initial states [S][n] of envs 0..n-1 of a tg_env_reset(seed, stream, key_offset, key_div), and the angles."""
    i = np.arange(n, dtype=np.uint64)
    idx = (np.uint64(key_offset) + i) // np.uint64(key_div)
    words = draw_np(seed, idx, SUB_RESET, stream & MASK)
    ang = reset_angles(name, words)
    o = np.zeros((ENV_DIMS[name], n))
    if name in ("CartPole", "QuadPole2D", "Pendulum", "PendulumSwingup"):
        th = ang["theta"]
        at = {"CartPole": (2, 3), "QuadPole2D": (7, 8)}.get(name, (0, 1))
        o[at[0]], o[at[1]] = np.sin(th), np.cos(th)
        if name == "QuadPole2D":
            o[5] = 1.0
    else:
        sa, ca = np.sin(ang["alpha"] / 2), np.cos(ang["alpha"] / 2)
        sb, cb = np.sin(ang["beta"] / 2), np.cos(ang["beta"] / 2)
        q = np.stack([cb * ca, cb * sa, sb * ca, -sb * sa])           # q_y (x) q_x, quadrotor_env.py:196-201
        o[6] = 1.0
        o[13:17] = q / np.sqrt((q * q).sum(0))
    return o, ang


# ---- statistics without scipy ----
def normal_cdf(x):
    erf = np.frompyfunc(math.erf, 1, 1)
    return 0.5 * (1.0 + erf(np.asarray(x, dtype=np.float64) / math.sqrt(2.0)).astype(np.float64))


def ks_pvalue(x, cdf):
    """One-sample Kolmogorov-Smirnov test of x against `cdf`: (D, asymptotic p-value with Stephens' small-n correction)."""
    x = np.sort(np.asarray(x, dtype=np.float64))
    n = x.size
    F = cdf(x)
    k = np.arange(1, n + 1, dtype=np.float64)
    D = float(max((k / n - F).max(), (F - (k - 1) / n).max()))
    lam = (math.sqrt(n) + 0.12 + 0.11 / math.sqrt(n)) * D
    if lam < 0.2:
        return D, 1.0
    p = 2.0 * sum((-1) ** (j - 1) * math.exp(-2.0 * j * j * lam * lam) for j in range(1, 101))
    return D, min(max(p, 0.0), 1.0)


def uniform_cdf(lo, hi):
    return lambda x: np.clip((x - lo) / (hi - lo), 0.0, 1.0)
