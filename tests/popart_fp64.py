"""NumPy restatement of PopArt's rescale of the critic head (policies.ValueNorm(popart=True), tg_value_norm_merge_popart) -- the
yardstick of test_popart_cpu.py / test_popart_gpu.py, written as tests/value_norm_fp64.py is and using its merge().

When the return statistics move from (mean_a, sigma_a) to (mean_n, sigma_n), sigma = sqrt(m2 / count + eps) in f64 (the table's
expression), the critic's last layer w f32 [H], b f32 [1] becomes
    r = sigma_a / sigma_n,   w'_k = f32(f64(w_k) * r),   b' = f32(((f64(b) * sigma_a) + (mean_a - mean_n)) / sigma_n).
rescale() runs these f64 operations in the kernel's order (NumPy float64 scalars round every operation on its own, as the kernel does
with contraction off and IEEE divide / sqrt; f64 -> f32 is one rounding to nearest even in both), so a device head is compared bit
for bit.  The head keeps its bits when no batch was merged, when the statistics were empty before the merge, or when either sigma is
not a positive finite number.

Preservation bound.  For a hidden vector h let
    y  = sigma_a (w  . h + b ) + mean_a,      y' = sigma_n (w' . h + b') + mean_n,
both evaluated exactly on the STORED f32 weights and the f64 statistics.  Write u = 2^-53, v = 2^-24, and use the form
x = fl(x) (1 + d), |d| <= unit roundoff, of a rounding to nearest (Higham, Accuracy and Stability of Numerical Algorithms, Theorem
2.3), which holds as long as nothing overflows or underflows in f32 (or f64).
  weights  sigma_a / sigma_n = r (1 + d1);  w_k r = t_k (1 + d2);  t_k = w'_k (1 + e_k), |d| <= u, |e| <= v.  So
               sigma_a w_k = sigma_n w'_k (1 + e_k)(1 + d1)(1 + d2),
               |sigma_a w_k h_k - sigma_n w'_k h_k| <= sigma_n |w'_k h_k| ((1 + v)(1 + u)^2 - 1) <= sigma_n |w'_k h_k| (v + 3 u):
           two f64 roundings per weight (the quotient r, the product), the third u covers the cross terms 2 u v + u^2 (1 + v) < u.
  bias     p = fl(b sigma_a), d = fl(mean_a - mean_n), s = fl(p + d), q = fl(s / sigma_n), b' = f32(q): four f64 roundings,
               b sigma_a = p (1 + d3),  mean_a - mean_n = d (1 + d6),  p + d = s (1 + d4),  s = sigma_n q (1 + d5),  q = b' (1 + e_b),
               sigma_a b + mean_a - mean_n = s (1 + d4) + p d3 + d d6 = sigma_n b' (1 + e_b)(1 + d5)(1 + d4) + p d3 + d d6,
               |sigma_a b + mean_a - mean_n - sigma_n b'| <= sigma_n |b'| (v + 3 u) + u (|p| + |d|).
  together |y' - y| <= v sigma_n (sum_k |w'_k h_k| + |b'|)  +  u (HEAD_OPS sigma_n (sum_k |w'_k h_k| + |b'|) + |p| + |d|),
           HEAD_OPS = 3 (count them above: 2 roundings + 1 for the cross terms, on the weights and on the bias' quotient chain alike),
           and one u each on |p| and |d| (their own roundings).  preservation_bound() evaluates exactly this; the un-rescaled head
           read with the new statistics misses it by (sigma_n - sigma_a)(w . h + b) + (mean_n - mean_a), of the size of sigma."""
import numpy as np

import value_norm_fp64 as Y

U = 2.0 ** -53
V = 2.0 ** -24
HEAD_OPS = 3                   # f64 roundings (cross terms included) charged to sigma_n (sum |w' h| + |b'|): count them in the docstring


def sigma(stats, eps: float):
    """sqrt(m2 / count + eps) in f64 of stats = (count, mean, m2); None for empty statistics."""
    count, _, m2 = stats
    if not count > 0:
        return None
    with np.errstate(all="ignore"):
        return np.sqrt(np.float64(m2) / np.float64(count) + np.float64(eps))


def rescaled(stats_before, stats_after, eps: float) -> bool:
    """The skip rules: a batch was merged (the count moved), into statistics that were not empty, and both sigmas are positive and
    finite."""
    if not stats_before[0] > 0 or not stats_after[0] > stats_before[0]:
        return False
    sa, sn = sigma(stats_before, eps), sigma(stats_after, eps)
    return bool(np.isfinite(sa) and sa > 0 and np.isfinite(sn) and sn > 0)


def rescale(w, b, stats_before, stats_after, eps: float):
    """(w', b') f32 of the head w [H] (or [1][H]), b [1] (or a scalar): the kernel's operations in its order; the inputs' bits when
    the rescale is skipped."""
    w32, b32 = np.asarray(w, dtype=np.float32), np.asarray(b, dtype=np.float32)
    if not rescaled(stats_before, stats_after, eps):
        return w32.copy(), b32.copy()
    f = np.float64
    sa, sn = sigma(stats_before, eps), sigma(stats_after, eps)
    mean_a, mean_n = f(stats_before[1]), f(stats_after[1])
    r = sa / sn                                                    # 1
    w_new = (w32.astype(np.float64) * r).astype(np.float32)        # 2 | one rounding to f32
    p = b32.astype(np.float64) * sa                                # 1
    d = mean_a - mean_n                                            # 2
    b_new = ((p + d) / sn).astype(np.float32)                      # 3, 4 | one rounding to f32
    return w_new, b_new


def merge_and_rescale(count, mean, m2, mom, eps, w, b):
    """tg_value_norm_merge_popart as a whole: ((count', mean', m2'), table', w', b'); mom None: nothing to merge."""
    before = (float(count), float(mean), float(m2))
    after = before if mom is None else Y.merge(count, mean, m2, mom)
    w_new, b_new = rescale(w, b, before, after, eps)
    return after, Y.table(*after, eps), w_new, b_new


def predict(w, b, stats, eps, h):
    """sigma (w . h + b) + mean in extended precision on the stored f32 weights, h [rows][H] -> [rows]."""
    L = np.longdouble
    s = sigma(stats, eps)
    s, m = (L(1.0), L(0.0)) if s is None else (L(s), L(stats[1]))
    z = (np.asarray(h, dtype=np.float32).astype(L) * np.asarray(w, dtype=np.float32).reshape(1, -1).astype(L)).sum(1)
    return s * (z + L(np.asarray(b, dtype=np.float32).reshape(-1)[0])) + m


def preservation_bound(w_new, b_new, b_old, stats_before, stats_after, eps, h):
    """The docstring's bound on |y' - y| per row of h [rows][H], for a head that WAS rescaled."""
    sa, sn = float(sigma(stats_before, eps)), float(sigma(stats_after, eps))
    b_new = float(np.asarray(b_new, dtype=np.float32).reshape(-1)[0])
    b_old = float(np.asarray(b_old, dtype=np.float32).reshape(-1)[0])
    a = np.abs(np.asarray(h, dtype=np.float64) * np.asarray(w_new, dtype=np.float64).reshape(1, -1)).sum(1) + abs(b_new)
    p, d = abs(b_old * sa), abs(stats_before[1] - stats_after[1])
    return V * sn * a + U * (HEAD_OPS * sn * a + p + d)
