"""NumPy restatement of the running value normalisation (policies.ValueNorm, tg_value_norm_merge, tg_scatter_rows_affine,
tg_boot_values_affine): the moments {n, sum, sum of squares} of a batch of returns, Chan's merge of them into {count, mean, m2}, the
derived f32 table {mean, sigma, 1 / sigma, 0} and the two fp32 expressions denormalize / normalize -- the yardstick of
test_value_norm_cpu.py / test_value_norm_gpu.py, written as tests/obs_norm_fp64.py is.

merge() runs the kernel's f64 operations in the kernel's order (NumPy float64 scalars round every operation on its own, as the
kernel does with contraction off and IEEE divide / sqrt), so a device merge of GIVEN moments is compared bit for bit.

Error model against the exact statistics of the concatenated data (u = 2^-53).  The batch enters UNCENTRED, as S1 = sum r and
S2 = sum r^2 -- the form the learner's prologue has already all-reduced -- so the batch's squared deviations S2 - S1^2 / n are a
difference of two numbers of size S2: every relative error of S1 and S2 is paid at the magnitude of S2, not of the variance.
  sums   any order of recursive f64 summation of N terms t_i errs by at most gamma_{N-1} sum |t_i|, gamma_k = k u / (1 - k u)
         (Higham, Accuracy and Stability of Numerical Algorithms, (4.4)); as in obs_norm_fp64.py one more rounding is counted per term
         of S1 and three per term of S2 (the square of a rounded term, its own rounding):
             |S1 - S1*| <= e1 = gamma_{N+1} sum |r_i|,      |S2 - S2*| <= e2 = gamma_{N+3} sum r_i^2.
         The same bound covers the sum of two ranks' partial sums (one more addition: N + 1 <= N + 3 terms' worth).
  merge  mb = S1 / n_b, m2b = S2 - S1 mb, w = n_b / n, db = mb - mean, mean' = mean + db w, m2' = (m2 + m2b) + db^2 (n_a w):
         MERGE_OPS = 12 roundings in all (count them in merge(): 1 + 2 + 1 + 1 + 2 for the mean's chain and m2b, 5 for m2'; the
         count n_a + n_b is an integer below 2^53: exact).  First order in the input errors,
             d mean' <= d mean + e1 / n,
             d m2'   <= d m2 + e2 + 2 |mb| e1 + 2 |db| (n_a w) (e1 / n_b + d mean),
         and every rounding is charged u times an upper bound of the magnitude it rounds: |mean| + |mb| for the mean's chain,
         2 S2 + (everything added to m2 so far) for m2's (S1 mb <= S2 by Cauchy-Schwarz).  Errors of earlier merges carry over with
         factor 1 (the merged mean is a convex combination; m2 is a sum)."""
import numpy as np

U = 2.0 ** -53
MERGE_OPS = 12                 # f64 roundings between the batch sums and the merged statistics (count them in merge() below)


def gamma(k: int) -> float:
    return k * U / (1.0 - k * U)


def moments(r: np.ndarray) -> np.ndarray:
    """r [N] (the valid returns) -> f64 [3] = {N, sum r, sum r^2}, summed in extended precision and rounded once."""
    x = np.asarray(r).reshape(-1).astype(np.longdouble)
    return np.array([float(x.size), float(x.sum()), float((x * x).sum())], dtype=np.float64)


def abs_moments(r: np.ndarray):
    """(sum |r|, sum r^2): what the reordering bounds multiply."""
    x = np.abs(np.asarray(r, dtype=np.float64).reshape(-1))
    return float(x.sum()), float((x * x).sum())


def merge(count: float, mean: float, m2: float, mom) -> tuple:
    """Chan's merge of mom = {n_b, S1, S2} into (count, mean, m2): tg_value_norm_merge's operations in its order."""
    f = np.float64
    na, mu, q = f(count), f(mean), f(m2)
    nb = f(mom[0])
    if not nb > 0.0:
        return float(na), float(mu), float(q)
    s1, s2 = f(mom[1]), f(mom[2])
    mb = s1 / nb                                   # 1
    m2b = s2 - s1 * mb                             # 2, 3
    m2b = m2b if m2b > 0.0 else f(0.0)
    n = na + nb                                    # (integers: exact)
    w = nb / n                                     # 4
    db = mb - mu                                   # 5
    mu = mu + db * w                               # 6, 7
    q = (q + m2b) + (db * db) * (na * w)           # 8 | 9, 10, 11 | 12
    return float(n), float(mu), float(q)


def table(count: float, mean: float, m2: float, eps: float) -> np.ndarray:
    """f32 [4] = {(float)mean, (float)sigma, (float)(1 / sigma), 0}, sigma = sqrt(m2 / count + eps) in f64; count == 0: {0, 1, 1, 0}."""
    if not count > 0:
        return np.array([0.0, 1.0, 1.0, 0.0], dtype=np.float32)
    sigma = np.sqrt(np.float64(m2) / np.float64(count) + np.float64(eps))
    return np.array([np.float32(mean), np.float32(sigma), np.float32(np.float64(1.0) / sigma), 0.0], dtype=np.float32)


def denormalize(v: np.ndarray, tab: np.ndarray) -> np.ndarray:
    """v * table[1] + table[0] in float32: the multiply and the add each rounded on its own (no FMA)."""
    v32 = np.asarray(v).astype(np.float32)
    return ((v32 * np.float32(tab[1])).astype(np.float32) + np.float32(tab[0])).astype(np.float32)


def normalize(r: np.ndarray, tab: np.ndarray) -> np.ndarray:
    """(r - table[0]) * table[2] in float32, each operation rounded on its own: the critic's regression target."""
    r32 = np.asarray(r).astype(np.float32)
    return ((r32 - np.float32(tab[0])).astype(np.float32) * np.float32(tab[2])).astype(np.float32)


def statistics(batches, eps: float):
    """Successive merges of the batches of returns from empty statistics -> (count, mean, m2, table)."""
    count, mean, m2 = 0.0, 0.0, 0.0
    for r in batches:
        count, mean, m2 = merge(count, mean, m2, moments(r))
    return count, mean, m2, table(count, mean, m2, eps)


def exact(batches):
    """(count, mean, m2) of the concatenated batches: two passes in extended precision."""
    x = np.concatenate([np.asarray(r).reshape(-1) for r in batches]).astype(np.longdouble)
    mean = x.mean()
    return float(x.size), float(mean), float(((x - mean) ** 2).sum())


def merge_bounds(batches):
    """(bound on |mean - mean*|, bound on |m2 - m2*|) after merging `batches` in turn, each through its sums {N, S1, S2} formed in
    f64 in any order -- the module docstring's error model carried through the merges."""
    e_mean = e_m2 = tot = 0.0
    count = mean = 0.0
    for r in batches:
        x = np.asarray(r, dtype=np.float64).reshape(-1)
        N = float(x.size)
        a1, a2 = abs_moments(x)
        e1, e2 = gamma(int(N) + 1) * a1, gamma(int(N) + 3) * a2
        n = count + N
        w = N / n
        mb = float(x.astype(np.longdouble).sum()) / N
        db = abs(mb - mean)
        cross = db * db * count * w
        tot = tot + a2 + cross                                  # (an upper bound of everything added to m2 so far)
        e_m2 = e_m2 + e2 + 2.0 * abs(mb) * e1 + 2.0 * db * count * w * (e1 / N + e_mean) + MERGE_OPS * U * (2.0 * a2 + tot + e_m2)
        e_mean = e_mean + e1 / n + MERGE_OPS * U * (abs(mean) + abs(mb) + e_mean)
        mean = mean + (mb - mean) * w
        count = n
    return e_mean, e_m2
