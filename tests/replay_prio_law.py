"""The definition the prioritised sampler is held to: row i is drawn with probability p_i / sum p.  In float64, from the leaves alone:

    C = cumsum(leaves)                                  C[i] = the mass of rows 0 .. i, C[n - 1] = T the total
    t_b = (b + u_b) / B * float64(root)                 the stratified targets, u_b = u01d(w0, w1) of the Philox draw
                                                        (seed, idx = b, sub = ordinal >> 32, stream = ordinal & 0xffffffff)
    row_b = the i with C[i - 1] <= t_b < C[i]           = searchsorted(C, t_b, side="right"), C[-1] read as 0

`root` is the float32 the tree stores.  Nothing here calls the library or the restatement's scan, node sum or descent
(tests/replay_prio_ref.py): there is no tree in this file, only a cumulative sum.

exact_rows() is for integer leaves of total < 2^24: every float32 sum of them, in any order, is exact, so the stored root is T, every
prefix the descent forms is a C[i], every `t -= before` is exact, and the drawn row IS row_b.

check_draws() is for any leaves: the tree's sums and prefixes are rounded, so the drawn row may be a neighbour of row_b where t_b falls
within `tol` of a boundary.  It asks C[idx_b - 1] - tol <= t_b T / root <= C[idx_b] + tol (the target rescaled to the exact total), and

    tol = (gamma(3 L (L + 3)) (1 + gamma(6 L)) + (n + 8) 2^-53) root,      gamma(k) = k u / (1 - k u),  u = 2^-24,

for a tree of n leaves and L levels above them.  Derivation (all leaves >= 0, so every bound is relative to a sum of its own terms;
a product of k factors (1 + d), |d| <= u, is 1 + theta with |theta| <= gamma(k), and gamma(a) + gamma(b) <= gamma(a + b)):
  * a node is the sum of its 64 children by a butterfly in which every term passes through 6 float32 additions, so a level-l node is its
    exact mass times (1 + theta), |theta| <= gamma(6 l): leaves (l = 0) are exact, the root is T (1 + theta), |theta| <= gamma(6 L);
  * the inclusive prefix over the 64 children of a node (Kogge-Stone) passes every term through at most 6 more additions, so a prefix
    over level-l children is within e_l = gamma(6 (l + 1)) T of the exact mass it stands for;
  * write g = (exact mass left of the current node) + t.  One step of the descent, `t -= prefix before the chosen child`, moves g by
    the error of that one prefix, at most e_l; the comparison that chose the child ("the first child > 0 whose prefix > t") places g
    within e_l of that child's exact interval on the side(s) it decides: below the interval's end when some prefix exceeded t, above its
    start when an earlier positive child was passed over.  Where it decides nothing -- the chosen child is the first positive one, or the
    fallback "last positive child" was taken -- the child's interval starts, or ends, where its parent's does, and the bound is the one of
    the nearest level above that did decide; at the root it is 0 <= t <= root;
  * so the drawn leaf's interval [C[idx - 1], C[idx]] holds t to within e_0 + e_1 + .. + e_(L-1) <= gamma(6 (1 + 2 + .. + L)) T
    = gamma(3 L (L + 1)) T: the levels the target was carried through, each counted once, whichever of them decided;
  * rescaling t by T / root moves it by at most gamma(6 L) T, and T <= (1 + gamma(6 L)) root: together gamma(3 L (L + 3)) (1 + gamma(6 L)) root;
  * the float64 steps (three to form t, one subtraction per level, this file's own cumulative sum of n terms) add at most (n + 8) 2^-53 root.
To first order this is 3 L (L + 3) 2^-24 root.  Non-monotone prefixes (two lanes of the scan group the same terms differently) need no
separate term: only the distance of each prefix from the exact mass is used.  Nothing in `tol` was measured on a device."""
import numpy as np

import philox_fp64 as P

U = 2.0 ** -24


def levels_above(n):
    """Levels above n leaves in the fan-out-64 tree: always at least one."""
    n, L = -(-int(n) // 64), 1
    while n > 1:
        n, L = -(-n // 64), L + 1
    return L


def gamma(k):
    return k * U / (1.0 - k * U)


def tolerance(n, root):
    L = levels_above(n)
    return (gamma(3 * L * (L + 3)) * (1.0 + gamma(6 * L)) + (n + 8) * 2.0 ** -53) * float(root)


def targets(root, seed, ordinal, B):
    """t_b, b = 0 .. B - 1, float64."""
    b = np.arange(B, dtype=np.uint64)
    w = P.draw_np(seed, b, (int(ordinal) >> 32) & P.MASK, int(ordinal) & P.MASK)
    return (b.astype(np.float64) + P.u01d(w[0], w[1])) / np.float64(B) * np.float64(root)


def rows_at(C, t):
    """The row whose interval [C[i - 1], C[i]) holds t."""
    return np.searchsorted(C, t, side="right").astype(np.int64)


def exact_rows(leaves, root, seed, ordinal, B):
    """The rows the law draws from integer leaves of total < 2^24 (asserted, and that the stored root is that total)."""
    leaves64 = np.asarray(leaves, dtype=np.float32).astype(np.float64)
    C = np.cumsum(leaves64)
    assert (leaves64 >= 0).all() and (leaves64 == np.floor(leaves64)).all() and 0 < C[-1] < 2 ** 24, "exact_rows needs integer leaves, total < 2^24"
    assert float(root) == C[-1], f"the stored root {float(root)} is not the exact total {C[-1]}"
    return rows_at(C, targets(root, seed, ordinal, B))


def check_draws(idx, leaves, root, seed, ordinal, B, rows, t=None):
    """The largest distance of a target from its drawn row's interval, over tol: <= 1 passes.  inf where a drawn row has no mass or lies
    outside the `rows` stored ones.  `t`: targets given directly instead of the Philox draw's."""
    leaves64 = np.asarray(leaves, dtype=np.float32).astype(np.float64)
    idx = np.asarray(idx, dtype=np.int64)
    assert idx.shape == (B,)
    if idx.min() < 0 or idx.max() >= min(rows, len(leaves64)) or not (leaves64[idx] > 0).all():
        return np.inf
    C = np.cumsum(leaves64)
    t = targets(root, seed, ordinal, B) if t is None else np.asarray(t, dtype=np.float64)
    t = t * (C[-1] / np.float64(root))
    below = np.where(idx > 0, C[np.maximum(idx - 1, 0)], 0.0)
    worst = np.maximum(np.maximum(below - t, t - C[idx]), 0.0).max()
    return float(worst / tolerance(len(leaves64), root))


# ---- the leaf sets of the tests: float32 [R] each, R = the stored rows (the leaves beyond them, up to the capacity, are 0) ----
def integer_leaf_sets(R, rng):
    """{name: leaves in 0 .. 31}, at least one positive."""
    node = np.arange(R) // 64
    last = (R - 1) // 64
    some = rng.integers(1, 32, R).astype(np.float32)
    sets = {"random, 30 % zeros": some * (rng.random(R) >= 0.3)}
    if not sets["random, 30 % zeros"].any():
        sets["random, 30 % zeros"][0] = 7
    for name, row in (("only row 0", 0), ("only row R - 1", R - 1), ("only the first leaf of the last level-1 node", last * 64)):
        sets[name] = np.zeros(R, np.float32)
        sets[name][row] = 1 + row % 31
    sets["alternate level-1 nodes zero"] = some * (node % 2 == 0)
    if R >= 3 * 4096:
        sets["one level-2 subtree zero"] = some * (np.arange(R) // 4096 != R // 4096 // 2)
    sets["all mass in the last level-1 node"] = some * (node == last)
    sets["total 3"] = np.zeros(R, np.float32)
    np.add.at(sets["total 3"], [0, R // 2, R - 1], 1)
    assert all(v.dtype == np.float32 and v.shape == (R,) and v.max() <= 31 and 0 < v.astype(np.float64).sum() < 2 ** 24 for v in sets.values())
    return sets


def real_leaf_sets(R, rng):
    return {"uniform [0.5, 2)": rng.uniform(0.5, 2.0, R).astype(np.float32),
            "log-uniform 2^-40 .. 2^20": (2.0 ** rng.uniform(-40.0, 20.0, R)).astype(np.float32)}
