"""Control decimation (Env.substeps) restated over the oracle's own step functions, and the pinned cases of the GPU tests.

The rule: an env with substeps = k applies each policy action for up to k consecutive calls of its own step and stops after the
first call that reports `truncated`; call j (from 0) of control step t runs with steps_after = t k + j + 1.  Transition t records the
observation before the first call, the summed reward (left to right, in the trajectory dtype) and the state after the last call.

The identity: that rollout with horizon T and forced actions a[t] is the plain rollout of the same env with max_steps = k T, driven
with a[p // k] at physics step p and read at every k-th step (`decimate`).  `substep_rollout` states the rule, `plain_rollout` is
the rollout kernels' loop over one oracle step per time step; tests/test_substeps_cpu.py holds one against the other.

Nothing here touches the GPU or the library under test."""
import hashlib

import numpy as np

from oracle import envs as OE

ENVS = ("CartPole", "QuadPole2D", "QuadPole")
KS = (1, 2, 3, 5)
T = 20                      # control steps: crosses the forced kernel's 8-step prefetch block and two fused compactions
N_MAX = 300                 # one lane, a second wave, a second 256-thread block: n in {1, 65, 300} are prefixes of one set
TIMESTEP = 0.02
# where the x velocity sits in the state, the bound x leaves through, and the fastest push: an env pushed at v m/s leaves after about
# bound / (v dt) physics steps, so speeds spread over [0, VMAX] end episodes at every step from ~5 on and leave the slow ones running
PUSH = {"CartPole": (1, 1.0, 12.0), "QuadPole2D": (2, 2.0, 20.0), "QuadPole": (3, 1.5, 16.0)}


STEP = {"CartPole": OE.cartpole_step, "QuadPole2D": OE.quadpole2d_step, "QuadPole": OE.quadpole_step}
DIMS = {"CartPole": (5, 1), "QuadPole2D": (10, 2), "QuadPole": (20, 4)}


def initial_states(name, n=N_MAX, seed=0):
    """(n, S) float64: the env's own reset distribution, then pushed along x at speeds spread over [0, VMAX] (quadratically: more slow ones, which run to the horizon) with alternating
    sign, shuffled over the envs (a prefix of the set has the same spread)."""
    rng = np.random.Generator(np.random.PCG64(1000 + seed + 17 * ENVS.index(name)))
    s0 = np.array(OE.sample_initial_states(name, n, rng), dtype=np.float64)
    col, _, vmax = PUSH[name]
    v = np.linspace(0.0, 1.0, n) ** 2 * vmax * np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    s0[:, col] = rng.permutation(v)
    return s0


def forced_actions(name, n=N_MAX, horizon=T, seed=0):
    """(n, T, A) float32: a third of the envs under a constant extreme command (+1, -1 in turn: full thrust / zero thrust, a full
    push either way), the rest N(0, 0.5) clipped to [-1.5, 1.5] (so the kernels' own clip to [-1, 1] is exercised as well)."""
    S, A = DIMS[name]
    rng = np.random.Generator(np.random.PCG64(2000 + seed + 17 * ENVS.index(name)))
    a = np.clip(rng.normal(0.0, 0.5, size=(n, horizon, A)), -1.5, 1.5).astype(np.float32)
    const = np.arange(n) % 3 == 0
    sign = np.where((np.arange(n) // 3) % 2 == 0, 1.0, -1.0).astype(np.float32)
    a[const] = sign[const][:, None, None]
    return a


def digest(*arrays):
    h = hashlib.sha256()
    for x in arrays:
        h.update(np.ascontiguousarray(x).tobytes())
    return h.hexdigest()[:16]


def plain_rollout(name, s0, actions, horizon, timestep=TIMESTEP, dtype=np.float64):
    """The rollout kernels' loop over the oracle's step, one call per time step: actions (n, horizon, A).
    -> obs (n, horizon + 1, S), rew (n, horizon), mask (n, horizon) u8, len (n,) -- zeros beyond an episode's end, as the kernels pad."""
    n, S = s0.shape
    obs = np.zeros((n, horizon + 1, S), dtype)
    rew = np.zeros((n, horizon), dtype)
    mask = np.zeros((n, horizon), np.uint8)
    length = np.zeros(n, np.int64)
    obs[:, 0] = s0.astype(dtype)
    alive = np.ones(n, bool)
    tb = np.zeros(n, dtype)
    for p in range(horizon):
        nxt, r, trunc, _, tb = STEP[name](obs[:, p], actions[:, p], np.full(n, p, np.int64), tb, max_steps=horizon, timestep=timestep,
                                          dtype=dtype)
        done = np.asarray(trunc, bool) | (p + 1 >= horizon)
        rew[alive, p] = np.asarray(r, dtype)[alive]
        mask[alive, p] = 1
        carry = alive & ~done
        obs[carry, p + 1] = np.asarray(nxt, dtype)[carry]
        length[alive & done] = p + 1
        alive = carry
    return obs, rew, mask, length


def substep_rollout(name, s0, actions, horizon, k, timestep=TIMESTEP, dtype=np.float64):
    """The rule itself: actions (n, horizon, A), one per CONTROL step; the env's clock is horizon * k physics steps of `timestep`."""
    n, S = s0.shape
    obs = np.zeros((n, horizon + 1, S), dtype)
    rew = np.zeros((n, horizon), dtype)
    mask = np.zeros((n, horizon), np.uint8)
    length = np.zeros(n, np.int64)
    obs[:, 0] = s0.astype(dtype)
    alive = np.ones(n, bool)
    tb = np.zeros(n, dtype)
    for t in range(horizon):
        cur = obs[:, t].copy()
        total = np.zeros(n, dtype)
        running = alive.copy()
        ended = np.zeros(n, bool)
        for j in range(k):
            nxt, r, trunc, _, tb = STEP[name](cur, actions[:, t], np.full(n, t * k + j, np.int64), tb, max_steps=horizon * k,
                                              timestep=timestep, dtype=dtype)
            r, nxt, trunc = np.asarray(r, dtype), np.asarray(nxt, dtype), np.asarray(trunc, bool)
            total[running] = r[running] if j == 0 else (total[running] + r[running]).astype(dtype)
            cur[running] = nxt[running]
            ended |= running & trunc
            running = running & ~trunc
        done = ended | (t + 1 >= horizon)
        rew[alive, t] = total[alive]
        mask[alive, t] = 1
        carry = alive & ~done
        obs[carry, t + 1] = cur[carry]
        length[alive & done] = t + 1
        alive = carry
    return obs, rew, mask, length


def hold(actions, k):
    """a[p // k]: (n, T, A) -> (n, k T, A)."""
    return np.repeat(actions, k, axis=1)


def decimate(obs, rew, mask, length, k):
    """A plain rollout of horizon k T (arrays with the env axis FIRST) read at every k-th step: what the substepped rollout must be.
    rew_sub[t] is the sequential sum, in the arrays' dtype, of rew[t k .. min(t k + k, L) - 1]; len_sub = ceil(L / k)."""
    n, P = rew.shape
    horizon = P // k
    assert horizon * k == P
    obs_s = np.ascontiguousarray(obs[:, ::k])
    mask_s = np.ascontiguousarray(mask[:, ::k])
    rew_s = np.zeros((n, horizon), rew.dtype)
    for t in range(horizon):
        acc = rew[:, t * k].copy()
        for j in range(1, k):
            live = (t * k + j) < length                       # only the executed calls are summed (the padding is zero, but -0.0 + 0.0
            acc = np.where(live, (acc + rew[:, t * k + j]).astype(rew.dtype), acc)        # would turn a -0.0 sum into +0.0)
        rew_s[:, t] = acc
    return obs_s, rew_s, mask_s, -(-length // k)


def ending_shares(len_plain, k, horizon=T):
    """(share that ends before the horizon, share that ends at a physics step that is not the last substep of its control step,
    number that runs the full horizon) of a plain run of horizon k T."""
    L = np.asarray(len_plain)
    early = L < k * horizon
    return float(early.mean()), float((early & (L % k != 0)).mean()), int((L == k * horizon).sum())
