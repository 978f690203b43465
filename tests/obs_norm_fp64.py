"""NumPy restatement of the running observation normalisation (policies.ObsNorm, tg_obs_moments, tg_obs_norm_merge): the moments of
a batch about a centre, Chan's merge, the derived f32 table and the normalised observation -- the yardstick of
test_obs_norm_cpu.py / test_obs_norm_gpu.py.

Error model of the device's moments (u = 2^-53).  The kernels add N f64 terms in SOME fixed order; any order of recursive summation
of terms t_i satisfies |computed - exact| <= gamma_{N-1} sum |t_i| with gamma_k = k u / (1 - k u) (Higham, Accuracy and Stability
of Numerical Algorithms, (4.4)).  For sum d the terms d_i = x_i - c carry one rounding each when x is f64 (none for an f32
observation: the difference of a float and a double near it is not exact in general, so one is counted); for sum d^2 each term is
d_i^2 with a fused multiply-add (one rounding per step, already counted by the summation) on a d_i carrying one: (1 + u)^2.  Hence
    |S1 - S1*| <= gamma_{N+1} sum |d_i|,        |S2 - S2*| <= gamma_{N+3} sum d_i^2.
The merge adds a fixed handful of f64 operations (divide, multiplies, adds): MERGE_OPS roundings, each relative to the magnitude
of its result, bounded by the sums of absolute values that moments_bound() carries through the same formulas."""
import numpy as np

U = 2.0 ** -53
MERGE_OPS = 8                  # roundings between the batch sums and a merged statistic (count them in merge() below)


def gamma(k: int) -> float:
    return k * U / (1.0 - k * U)


def moments(x: np.ndarray, center: np.ndarray) -> np.ndarray:
    """x f64 [N][S] (the valid rows), center f64 [S] -> f64 [S][3] = {N, sum (x - c), sum (x - c)^2}, summed in extended precision."""
    d = x.astype(np.longdouble) - center.astype(np.longdouble)
    n = np.full(x.shape[1], float(x.shape[0]))
    return np.stack([n, d.sum(0).astype(np.float64), (d * d).sum(0).astype(np.float64)], axis=1)


def abs_moments(x: np.ndarray, center: np.ndarray):
    """(sum |x - c|, sum (x - c)^2) per feature: what the reordering bounds multiply."""
    d = np.abs(x.astype(np.float64) - center)
    return d.sum(0), (d * d).sum(0)


def merge(count: float, mean: np.ndarray, m2: np.ndarray, batch: np.ndarray):
    """Chan's merge of batch [S][3] (deviations taken from `mean`) -> (count, mean, m2), the kernel's operations in its order."""
    nb = float(batch[0, 0])
    if nb <= 0:
        return float(count), mean.copy(), m2.copy()
    na, sd, sq = float(count), batch[:, 1], batch[:, 2]
    n = na + nb
    db = sd / nb
    m2b = np.maximum(sq - sd * db, 0.0)
    return n, mean + db * (nb / n), (m2 + m2b) + (db * db) * (na * (nb / n))


def table(count: float, mean: np.ndarray, m2: np.ndarray, eps: float) -> np.ndarray:
    """f32 [2][S] = {(float)mean, (float)(1 / sqrt(m2 / count + eps))}; count == 0: {0, 1}."""
    S = mean.shape[0]
    if count <= 0:
        return np.stack([np.zeros(S, np.float32), np.ones(S, np.float32)])
    return np.stack([mean.astype(np.float32), (1.0 / np.sqrt(m2 / count + eps)).astype(np.float32)])


def normalize(x: np.ndarray, tab: np.ndarray, clip) -> np.ndarray:
    """xn = clamp((x - mean32) * rstd32, -clip, +clip) in float32, each operation rounded on its own; x is rounded to f32 first."""
    x32 = np.asarray(x).astype(np.float32)
    xn = (x32 - tab[0].astype(np.float32)).astype(np.float32) * tab[1].astype(np.float32)
    xn = xn.astype(np.float32)
    return xn if clip is None else np.clip(xn, np.float32(-clip), np.float32(clip)).astype(np.float32)


def statistics(batches, eps: float):
    """Successive merges of the row batches (each f64 [N_i][S]) from empty statistics -> (count, mean, m2, table)."""
    S = batches[0].shape[1]
    count, mean, m2 = 0.0, np.zeros(S), np.zeros(S)
    for x in batches:
        count, mean, m2 = merge(count, mean, m2, moments(x, mean))
    return count, mean, m2, table(count, mean, m2, eps)


def merge_bounds(batches, means_before):
    """Bounds on |mean - mean*| and |m2 - m2*| per feature after merging `batches` in turn, the device having used the centres
    `means_before[i]` (its own running means) for batch i.  Each merge contributes: the reordering bound of its sums pushed through
    the merge formulas (first order; the derivative of mean w.r.t. S1 is 1 / n, of m2 w.r.t. S2 is 1 and w.r.t. S1 is at most
    2 |db|), plus MERGE_OPS roundings of the merged magnitudes.  Errors of earlier merges carry over with factor 1."""
    S = batches[0].shape[1]
    e_mean, e_m2, tot_m2 = np.zeros(S), np.zeros(S), np.zeros(S)
    count = 0.0
    for x, c in zip(batches, means_before):
        N = x.shape[0]
        a1, a2 = abs_moments(x, c)
        n = count + N
        db = np.abs((x - c).sum(0)) / N
        e1, e2 = gamma(N + 1) * a1, gamma(N + 3) * a2
        # a centre off by e_mean shifts every deviation: the batch is merged about the device's own mean, consistently, so the
        # merged mean moves by at most e_mean and m2 by at most 2 a1 e_mean (first order)
        mag_mean = np.abs(c) + db
        tot_m2 = tot_m2 + a2 + a1 * db + db * db * N          # (an upper bound of every intermediate of the m2 update)
        mag_m2 = tot_m2
        e_m2 = e_m2 + e2 + 2.0 * db * e1 + 2.0 * a1 * e_mean + MERGE_OPS * U * (mag_m2 + np.abs(e_m2))
        e_mean = e_mean + e1 / n + MERGE_OPS * U * mag_mean
        count = n
    return e_mean, e_m2
