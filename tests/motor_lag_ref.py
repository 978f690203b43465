"""The actuator lag (Env.motor_time_constant) restated in NumPy float32, one operation per line.

The rule: every env carries a motor state m (float32, normalised action units, 0 = hover thrust, 0 at the reset).  With
alpha = float32(dt / (tau + dt)) -- one double add and one double divide, rounded to float32 once -- the filter

    d = clip(a, -1, 1) - m
    e = alpha * d
    m = m + e

runs in front of EVERY executed physics step, and the env's own step receives m in place of the action.  With substeps = k the
action of control step t is held for its up to k physics steps; a lane that has stopped filters no more.

`filter` turns the commanded actions of a rollout into (the command each physics step received, the motor record the trajectory
keeps).  It needs to know how many physics steps each control step executed; the GPU tests read that from the plain kernel's own
rollout of the filtered commands (the filter is causal: the commands up to an episode's end do not depend on where it ends).

Nothing here touches the GPU or the library under test."""
import numpy as np

F32 = np.float32


def alpha(tau, dt):
    """float32(dt / (tau + dt)) -- scalars or arrays of doubles; tau = 0 gives 1 (the command passes through)."""
    tau = np.asarray(tau, dtype=np.float64)
    dt = np.asarray(dt, dtype=np.float64)
    s = tau + dt
    q = dt / s
    return q.astype(F32)


def filter_step(m, cmd, al):
    """One application of the filter: three float32 operations, each rounded on its own."""
    assert m.dtype == F32 and cmd.dtype == F32 and al.dtype == F32
    d = cmd - m
    e = al * d
    out = m + e
    assert d.dtype == F32 and e.dtype == F32 and out.dtype == F32
    return out


def filter(act, al, k, executed):
    """act f32 [A][T][n]: the commanded actions; al f32 [n] (or a scalar): every env's gain; k: physics steps per control step;
    executed int [T][n]: how many of them control step t of env i ran (0: the episode was over).
    -> (commands f32 [A][T k][n]: what physics step t k + j received, zero where it did not run;
        motor f32 [A][T + 1][n]: slot 0 zeros, slot t + 1 = m after control step t while the env carries on, else zeros)."""
    act = np.asarray(act)
    assert act.dtype == F32
    A, T, n = act.shape
    al = np.broadcast_to(np.asarray(al, dtype=F32), (n,))
    executed = np.asarray(executed)
    assert executed.shape == (T, n)
    cmds = np.zeros((A, T * k, n), F32)
    motor = np.zeros((A, T + 1, n), F32)
    m = np.zeros((A, n), F32)
    lo = F32(-1.0)
    hi = F32(1.0)
    for t in range(T):
        c = np.minimum(np.maximum(act[:, t, :], lo), hi)
        for j in range(k):
            run = j < executed[t]
            nxt = filter_step(m, c, al[None, :])
            m = np.where(run[None, :], nxt, m)
            cmds[:, t * k + j, :] = np.where(run[None, :], nxt, F32(0.0))
        carry = (executed[t + 1] > 0) if t + 1 < T else np.zeros(n, bool)
        m = np.where(carry[None, :], m, F32(0.0))
        motor[:, t + 1, :] = m
    return cmds, motor


def free_commands(act, al, k):
    """The commands of a rollout in which every physics step runs: what the plain kernel is fed before the lengths are known."""
    A, T, n = np.asarray(act).shape
    return filter(act, al, k, np.full((T, n), k))[0]


def executed_from_plain_len(L_plain, k, T):
    """executed[t][i] = the physics steps of control step t inside a plain episode of L_plain[i] physics steps."""
    L = np.asarray(L_plain, dtype=np.int64)
    t = np.arange(T, dtype=np.int64)[:, None]
    return np.clip(L[None, :] - t * k, 0, k)


def closed_form(cmd, al, j):
    """fp64: m after j steps under a CONSTANT command from m = 0 is cmd (1 - (1 - alpha)^j)."""
    return np.float64(cmd) * (1.0 - (1.0 - np.float64(al)) ** j)
