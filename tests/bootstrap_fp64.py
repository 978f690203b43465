"""fp64 restatement of time-limit bootstrapping (PPO(bootstrap_truncated=True)), for tests/test_bootstrap_cpu.py and
tests/test_bootstrap_gpu.py.  Nothing here touches the GPU or the package under test: NumPy / torch-CPU and the oracle only.

Definition ("Time-limit bootstrapping").  For an episode of length L in a trajectory of horizon T:
  s_final = Env.step(obs[L-1], act[L-1]) with step count L;
  timeout = !failed(s_final) && (time_rule(L) || L == T);
  b       = timeout ? V(s_final) : 0;
  returns / advantages = those of the rewards with gamma * b added to the reward of step L - 1.
"""
import numpy as np
import torch

from oracle import envs as E
from oracle import learner as L

# position bound of each failing env and the state columns it applies to (test_gpu_parity.py:97-98)
BOUNDS = {"CartPole": (1.0, 1), "QuadPole2D": (2.0, 2), "QuadPole": (1.5, 3)}
NEAR = 1e-5           # a final position this close to its bound may classify either way in fp32 (test_gpu_parity.py:99)

# the teacher-forced cases of the classification test: horizon, constructor arguments (the oracle's step takes the same keywords),
# |action| ranges of the part meant to survive and of the part meant to fail.  CartPole: a constant push of 5 s N moves the cart by
# ~ 3.2 s m in 32 steps of 0.05 s.  QuadPole2D / QuadPole: both (all four) rotors at hover * (1 + s) climb by ~ 4.5 s m in 48 steps.
# Pendulum never fails; its other class is the balance terminal: with timestep 0.5 s, 5 s of balance are 11 steps, and with a weak
# gravity an upright start under tiny torques stays within cos(theta) <= -0.99 that long, in fp32 too.
CASES = {
    "CartPole": dict(T=32, params=dict(timestep=0.05), stay=(0.0, 0.2), fail=(0.5, 1.0)),
    "QuadPole2D": dict(T=48, params={}, stay=(0.0, 0.2), fail=(0.6, 1.0)),
    "QuadPole": dict(T=48, params={}, stay=(0.0, 0.15), fail=(0.6, 1.0)),
    "Pendulum": dict(T=24, params=dict(gravity=0.1, timestep=0.5), stay=None, fail=None),
}
N_RANDOM, N_SCAN = 300, 256          # n = 556: not a multiple of 64 or 256


def augment(rew, length, b, gamma):
    """rew [..., T] with gamma * b[...] added at step length[...] - 1 (fp64; nothing added where length is outside [1, T])."""
    out = np.array(rew, dtype=np.float64, copy=True)
    length, b = np.asarray(length).astype(np.int64), np.asarray(b, dtype=np.float64)
    T = out.shape[-1]
    flat, lf, bf = out.reshape(-1, T), length.reshape(-1), b.reshape(-1)
    for i in range(flat.shape[0]):
        if 1 <= lf[i] <= T:
            flat[i, lf[i] - 1] += gamma * bf[i]
    return out


def bootstrapped_advantages(rew, mask, values, length, b, gamma, lam=0.95, monte_carlo=True):
    """oracle.learner.ppo_advantages on the augmented rewards: (normalised advantages, normalised returns) of the valid steps."""
    r = torch.from_numpy(augment(rew, length, b, gamma))
    return L.ppo_advantages(r, torch.as_tensor(mask), torch.as_tensor(values), gamma, lam, monte_carlo)


def failed(name, state):
    """The env's own failure test on fp64 next states [N][S]: out of its position bound; Pendulum: never."""
    state = np.asarray(state, dtype=np.float64)
    if name not in BOUNDS:
        return np.zeros(len(state), dtype=bool)
    bound, k = BOUNDS[name]
    return (np.abs(state[:, :k]) > bound).any(axis=1)


def near_bound(name, state):
    state = np.asarray(state, dtype=np.float64)
    if name not in BOUNDS:
        return np.zeros(len(state), dtype=bool)
    bound, k = BOUNDS[name]
    return (np.abs(np.abs(state[:, :k]) - bound) < NEAR).any(axis=1)


def time_rule(name, steps_after, max_steps, timestep=None):
    """The env's own clock test on the step count: CartPole / Pendulum compare the fp64-accumulated time, the quadrotors the count."""
    steps_after = np.asarray(steps_after)
    if name in ("CartPole", "Pendulum"):
        dt = E.ENV_SPECS[name]["timestep"] if timestep is None else timestep
        return steps_after >= E.cartpole_time_trunc_step(max_steps, dt)
    return steps_after >= max_steps


def classify(name, s_final, length, T, timestep=None):
    """timeout [N] bool from fp64 final states and episode lengths, the two clauses evaluated separately."""
    length = np.asarray(length)
    return ~failed(name, s_final) & (time_rule(name, length, T, timestep) | (length == T))


def oracle_final_state(name, obs_last, act_last, length, T, params):
    """The oracle's fp64 Env.step on each episode's last recorded transition: obs_last [N][S], act_last [N][A] f32, step count
    length - 1 before the step."""
    steps = np.asarray(length).astype(np.int64) - 1
    return E.ENV_SPECS[name]["step"](np.asarray(obs_last, dtype=np.float64), np.asarray(act_last, dtype=np.float32), steps,
                                     np.zeros(len(steps)), max_steps=T, **params)[0]


def oracle_rollout(name, init, actions, T, params):
    """The oracle alone over teacher-forced actions [N][T][A], all N envs at once: (length [N], s_final [N][S] fp64, obs_last [N][S]).
    An episode ends on `truncated`, on Pendulum's balance rule, or at the horizon (rollout/rollout_worker.py:51)."""
    spec = E.ENV_SPECS[name]
    state = np.array(init, dtype=np.float64, copy=True)
    n = len(state)
    tb, length = np.zeros(n), np.zeros(n, dtype=np.int64)
    s_final, obs_last = np.zeros_like(state), np.zeros_like(state)
    alive = np.ones(n, dtype=bool)
    limit = spec.get("balance_terminates")
    for t in range(T):
        nxt, _, trunc, _, tb = spec["step"](state, actions[:, t], np.full(n, t), tb, max_steps=T, **params)
        done = trunc | (t + 1 >= T)
        if limit is not None:
            done = done | (tb > limit)
        end = alive & done
        length[end], s_final[end], obs_last[end] = t + 1, nxt[end], state[end]
        alive &= ~done
        state = nxt
    return length, s_final, obs_last


def forced_case(name, seed=0):
    """(init [n][S] fp64 holding float32 values, actions [n][T][A] f32) of one classification case: N_RANDOM episodes under a constant
    action from the `stay` or the `fail` range (Pendulum: upright starts under tiny torques, or anywhere under large ones), then N_SCAN
    episodes from ONE initial state whose constant action sweeps the whole range: the first failure moves across the horizon along
    the sweep, so some of them fail exactly at step T."""
    case = CASES[name]
    T = case["T"]
    rng = np.random.default_rng(seed)
    S, A = E.ENV_SPECS[name]["obs_dim"], E.ENV_SPECS[name]["act_dim"]
    n = N_RANDOM + N_SCAN
    if name == "Pendulum":
        upright = rng.random(n) < 0.4
        theta = np.where(upright, np.pi + rng.uniform(-0.02, 0.02, n), rng.uniform(-2.5, 2.5, n))
        init = E.pendulum_reset(theta)
        scale = np.where(upright, 0.002, 0.5)
        actions = (rng.uniform(-1, 1, (n, T, A)) * scale[:, None, None]).astype(np.float32)
    else:
        init = E.sample_initial_states(name, n, rng)
        init[N_RANDOM:] = init[N_RANDOM]
        lo_s, hi_s = case["stay"]
        lo_f, hi_f = case["fail"]
        fails = rng.random(N_RANDOM) < 0.5
        s = np.where(fails, rng.uniform(lo_f, hi_f, N_RANDOM), rng.uniform(lo_s, hi_s, N_RANDOM)) * rng.choice([-1.0, 1.0], N_RANDOM)
        s = np.concatenate([s, np.linspace(0.0, 1.0, N_SCAN)])
        actions = np.broadcast_to(s[:, None, None], (n, T, A)).astype(np.float32).copy()
    return init.astype(np.float32).astype(np.float64), actions
