"""NumPy restatements of the evaluation kernels (include/trajopt_grpo_hip.h, "Deterministic evaluation and parameter sweeps"):
tg_env_param_grid's decode and tg_eval_cells' per-episode returns and per-cell statistics, operation for operation in IEEE double,
so the device results can be compared bit for bit.  No GPU, no library."""
import numpy as np

PARTIALS = 256                    # threads of the cell reduction (kCellThreads)


def decode_cell(cell, levels):
    """Level of every swept parameter for `cell`: row-major over the parameters in the order given (p[] order), the last fastest."""
    out, rem = [], int(cell)
    for lv in reversed(levels):
        out.append(rem % lv)
        rem //= lv
    return list(reversed(out))


def grid_table(nominal, sweep, episodes_per_cell, n, env_offset=0):
    """f64 [12][n].  sweep: [(p index, [factor, ...]), ...] in ANY listing order; the decode sorts by p index."""
    nominal = np.asarray(nominal, dtype=np.float64)
    assert nominal.shape == (12,)
    by_index = sorted(sweep, key=lambda item: item[0])
    levels = [len(f) for _, f in by_index]
    tab = np.repeat(nominal[:, None], n, axis=1)
    for i in range(n):
        lv = decode_cell((env_offset + i) // episodes_per_cell, levels)
        for (r, factors), l in zip(by_index, lv):
            tab[r, i] = nominal[r] * np.float64(factors[l])
    return tab


def episode_returns(rew, length):
    """f64 [n]: sum of rew[t][i] for t < len[i], t ascending, each reward converted to f64 first; 0 for len outside [1, T]."""
    rew = np.asarray(rew)
    T, n = rew.shape
    r64 = rew.astype(np.float64)
    out = np.zeros(n, dtype=np.float64)
    counted = (length >= 1) & (length <= T)
    for t in range(T):                                              # (vectorised over envs; the order within an env is t ascending)
        live = counted & (t < length)
        out[live] = out[live] + r64[t, live]
    return out


def _tree(partial):
    """partial[j] += partial[j + s] for s = 128, 64, ..., 1 -> partial[0]."""
    p = partial.copy()
    s = PARTIALS // 2
    while s > 0:
        p[:s] = p[:s] + p[s:2 * s]
        s //= 2
    return p[0]


def _strided(values, counted):
    """256 partials: partial j = 0.0 plus the counted entries e = j, j + 256, ... added in that order."""
    E = values.shape[0]
    rows = -(-E // PARTIALS)
    v = np.zeros(rows * PARTIALS, dtype=np.float64)
    v[:E] = np.where(counted, values, 0.0)                          # (adding +0.0 for an uncounted slot changes no bit: the sums never are -0.0)
    v = v.reshape(rows, PARTIALS)
    p = np.zeros(PARTIALS, dtype=np.float64)
    for k in range(rows):
        p = p + v[k]
    return p


def cell_stats(returns, length, timeout, episodes_per_cell, T):
    """f64 [C][8] = {episodes, sum of returns, sum of squared returns, min, max, sum of lengths, clock-ended, ended early}."""
    E = int(episodes_per_cell)
    n = returns.shape[0]
    assert n % E == 0
    out = np.zeros((n // E, 8), dtype=np.float64)
    for c in range(n // E):
        sl = slice(c * E, (c + 1) * E)
        r, L, to = returns[sl], length[sl], timeout[sl]
        counted = (L >= 1) & (L <= T)
        out[c, 0] = counted.sum()
        out[c, 1] = _tree(_strided(r, counted))
        out[c, 2] = _tree(_strided(r * r, counted))
        out[c, 3] = r[counted].min() if counted.any() else np.inf
        out[c, 4] = r[counted].max() if counted.any() else -np.inf
        out[c, 5] = L[counted].astype(np.int64).sum()
        out[c, 6] = ((to != 0) & counted).sum()
        out[c, 7] = out[c, 0] - out[c, 6]
    return out
