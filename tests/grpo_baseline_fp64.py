"""GRPO's per-time-step group baseline (tg_grpo_step_advantage, csrc/grpo_baseline.hip) restated in NumPy, twice, with the input
recipes the CPU and GPU tests share.  numpy only; imports no GPU code.

R is float32 [T][n], mask uint8 [T][n] (non-zero = valid, any byte pattern), n = G E; segment (g, t) = the E consecutive entries at
t n + g E.  Per segment, over its valid entries V (c = |V|): s1 = sum (double)R, mean = s1 / c, b = (float)mean, d = R - b in one
float32 subtraction (+0 where invalid), q = sum (double)d (double)d.  Per group, ascending t: Q = sum q, C = sum c, K = #{t: c >= 1},
std = sqrt(Q / (C - K)) (0 when C - K <= 0).  A = d / ((float)std + 1e-8f) in two float32 operations ("std"), A = d ("none").

kernel_order(): the kernel's own order, to be met bit for bit.  A segment is cut into quads of 4 consecutive entries; W = min(64,
smallest power of two >= number of quads) lanes; lane l adds the entries of quads l, l + W, ... in ascending index to a sum that
starts at +0 (an invalid entry adds +0); a tree with offsets W / 2, ..., 1 adds lane l + off into lane l; lane 0 has the sum.

order_free(): the same quantities with exact segment sums (math.fsum) and float64 everywhere else, and the bounds below on what
any float32 evaluation in the kernel's FORM (whatever its summation order) may differ by.  u = 2^-24, v = 2^-53; magnitudes come
from the float64 values, the kernel's own intermediates differ from them in second order: every bound is multiplied by
SLACK = 1 + 2^-10 for that and for nothing else.
    mean:  recursive summation of c terms in any order is off by at most (c - 1) v sum|R|; the division adds v |mean|:
               e_mean = (c - 1) v sum_V |R| / c + v |mean|
    d:     b = (float)mean adds u |mean|, the subtraction u |d|:
               e_d = e_mean + u |mean| + u |d|                                   (0 where invalid: both are +0)
    Q:     each square is off by at most 2 |d| e_d + e_d^2, the products are exact, the sums over a segment and then over t are
           one recursive summation of C terms of Q:   e_Q = sum (2 |d| e_d + e_d^2) + C v Q
    std:   division and square root add v each; the root halves the relative error of its argument:
               r_std = e_Q / (2 Q) + 2 v                                         (Q = 0: every d is exactly 0, std = 0 exactly)
    A:     (float)std, the float32 sum with 1e-8f (taken as the float32 constant: no term of its own) and the division add u
           each, and std / (std + 1e-8f) <= 1:
               e_A = e_d / den + |A| (r_std + 3 u),   den = std + 1e-8f.
"""
import math

import numpy as np

U = 2.0 ** -24
V = 2.0 ** -53
SLACK = 1.0 + 2.0 ** -10
EPS32 = np.float32(1e-8)
GARBAGE = np.float32(1e30)            # finite, large: what may lie under a zero mask byte

# (T, G, E): the issue's nine, then E = 1 groups, a vector-load shape and a scalar-load shape whose second launch cuts the horizon
# into several chunks of more than one step (8192 / E steps each)
SHAPES = [(1, 1, 1), (3, 2, 2), (16, 3, 5), (9, 2, 63), (9, 2, 64), (9, 2, 65), (5, 1, 257), (4, 1, 4100), (130, 2, 8),
          (7, 5, 1), (40, 2, 512), (37, 1, 1001)]
MASKS = ["all", "prefix", "holes", "one_live", "none_live"]
VALUES = ["normal", "offset", "constant", "zeros"]


def lanes(E):
    nq, w = (E + 3) // 4, 1
    while w < 64 and w < nq:
        w *= 2
    return w


def make_mask(kind, T, G, E, rng):
    n = G * E
    if kind == "all":
        return np.ones((T, n), dtype=np.uint8)
    if kind == "prefix":                                                # episode lengths in [0, T]; env 0 never lives
        ln = rng.integers(0, T + 1, size=n)
        ln[0] = 0
        return (np.arange(T)[:, None] < ln[None, :]).astype(np.uint8)
    if kind == "holes":                                                 # any byte pattern: the non-zero bytes are not all 1
        m = rng.integers(1, 256, size=(T, n)).astype(np.uint8)
        m[rng.random((T, n)) < 0.4] = 0
        return m
    m = np.ones((T, n), dtype=np.uint8)
    t_star = T // 2
    m[t_star, :] = 0
    if kind == "one_live":                                              # exactly one live episode per group at t_star
        for g in range(G):
            m[t_star, g * E + int(rng.integers(0, E))] = 1
        return m
    assert kind == "none_live"
    return m


def make_values(kind, T, n, rng):
    if kind == "normal":
        return rng.standard_normal((T, n)).astype(np.float32)
    if kind == "offset":                                                # cancellation: |mean| / std ~ 1e4
        return (1e4 + rng.standard_normal((T, n))).astype(np.float32)
    if kind == "constant":
        return np.ones((T, n), dtype=np.float32)
    assert kind == "zeros"
    return np.zeros((T, n), dtype=np.float32)


def case(shape, mask_kind, value_kind, seed=0):
    """-> (R float32 [T][n], mask uint8 [T][n], E).  Under the zero bytes of a "holes" mask lies GARBAGE: the kernel must not look."""
    T, G, E = shape
    rng = np.random.default_rng([seed, T, G, E, MASKS.index(mask_kind), VALUES.index(value_kind)])
    mask = make_mask(mask_kind, T, G, E, rng)
    R = make_values(value_kind, T, G * E, rng)
    if mask_kind == "holes":
        R = np.where(mask != 0, R, GARBAGE).astype(np.float32)
    return R, mask, E


def cases():
    for shape in SHAPES:
        for mk in MASKS:
            for vk in VALUES:
                yield shape, mk, vk


def _segment_sums(x, W):
    """x float64 [S][E] (zeros where nothing is added) -> [S]: the kernel's lane-strided sums and shuffle tree."""
    S, E = x.shape
    nq = (E + 3) // 4
    iters = (nq + W - 1) // W
    pad = np.zeros((S, iters * W * 4), dtype=np.float64)
    pad[:, :E] = x
    pad = pad.reshape(S, iters, W, 4)
    p = np.zeros((S, W), dtype=np.float64)
    for it in range(iters):
        for j in range(4):
            p = p + pad[:, it, :, j]
    off = W // 2
    while off > 0:
        p[:, :off] = p[:, :off] + p[:, off:2 * off]
        off //= 2
    return p[:, 0].copy()


def kernel_order(R, mask, E, scale=True):
    """-> (A float32 [T][n], group float64 [G][3] = {Q, C, K}, tab float64 [3][G][T] = {c, mean, q}) in the kernel's order."""
    T, n = R.shape
    G = n // E
    W = lanes(E)
    valid = (mask != 0).reshape(T * G, E)
    r32 = R.reshape(T * G, E)
    s1 = _segment_sums(np.where(valid, r32.astype(np.float64), 0.0), W)
    c = _segment_sums(valid.astype(np.float64), W)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = np.where(c > 0.0, s1 / c, 0.0)
    b = mean.astype(np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        d = np.where(valid, r32 - b[:, None], np.float32(0.0)).astype(np.float32)
    d64 = d.astype(np.float64)
    q = _segment_sums(d64 * d64, W)
    c_tg, q_tg = c.reshape(T, G), q.reshape(T, G)
    Q, C, K = np.zeros(G), np.zeros(G), np.zeros(G)
    for t in range(T):                                                  # ascending t, one addition per step
        Q = Q + q_tg[t]
        C = C + c_tg[t]
        K = K + (c_tg[t] >= 1.0)
    dof = C - K
    with np.errstate(divide="ignore", invalid="ignore"):
        std = np.where(dof > 0.0, np.sqrt(Q / np.where(dof > 0.0, dof, 1.0)), 0.0)
    d = d.reshape(T, G, E)
    if scale:
        den = (std.astype(np.float32) + EPS32).astype(np.float32)
        A = (d / den[None, :, None]).astype(np.float32)
    else:
        A = d
    tab = np.stack([c_tg.T, mean.reshape(T, G).T, q_tg.T])
    return A.reshape(T, n), np.stack([Q, C, K], axis=1), tab


def order_free(R, mask, E, scale=True):
    """-> dict(A, e_A, d, e_d, Q, e_Q, C, K): float64 values from exact segment sums and the module's bounds (SLACK included)."""
    T, n = R.shape
    G = n // E
    valid = (mask != 0).reshape(T, G, E)
    r = np.where(valid, R.reshape(T, G, E).astype(np.float64), 0.0)
    c = valid.sum(axis=2).astype(np.float64)
    s1 = np.array([[math.fsum(r[t, g]) for g in range(G)] for t in range(T)], dtype=np.float64).reshape(T, G)
    sabs = np.abs(r).sum(axis=2)
    cc = np.maximum(c, 1.0)
    mean = np.where(c > 0, s1 / cc, 0.0)
    e_mean = np.maximum(c - 1.0, 0.0) * V * sabs / cc + V * np.abs(mean)
    d = np.where(valid, r - mean[:, :, None], 0.0)
    e_d = np.where(valid, e_mean[:, :, None] + U * np.abs(mean)[:, :, None] + U * np.abs(d), 0.0)
    C = c.sum(axis=0)
    K = (c >= 1).sum(axis=0).astype(np.float64)
    Q = np.array([math.fsum((d[:, g, :] ** 2).ravel()) for g in range(G)], dtype=np.float64)
    e_Q = (2.0 * np.abs(d) * e_d + e_d ** 2).sum(axis=(0, 2)) + C * V * Q
    dof = C - K
    std = np.where(dof > 0, np.sqrt(Q / np.where(dof > 0, dof, 1.0)), 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        r_std = np.where(Q > 0, e_Q / (2.0 * np.where(Q > 0, Q, 1.0)), 0.0) + 2.0 * V
    if scale:
        den = std + float(EPS32)
        A = d / den[None, :, None]
        e_A = e_d / den[None, :, None] + np.abs(A) * (r_std[None, :, None] + 3.0 * U)
    else:
        A, e_A = d, e_d
    return {"A": A.reshape(T, n), "e_A": (SLACK * e_A).reshape(T, n), "d": d.reshape(T, n), "e_d": (SLACK * e_d).reshape(T, n),
            "Q": Q, "e_Q": SLACK * e_Q, "C": C, "K": K}


def hold(tag, got, want, bound):
    """|got - want| <= bound everywhere and got finite; raises with the worst element; returns max err / bound."""
    got, want, bound = (np.asarray(a, dtype=np.float64) for a in (got, want, bound))
    assert got.shape == want.shape == bound.shape, (tag, got.shape, want.shape, bound.shape)
    assert np.isfinite(got).all(), f"{tag}: {int((~np.isfinite(got)).sum())} non-finite entries"
    err = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0.0, 0.0, err / bound)
    if ratio.size and not ratio.max() <= 1.0:
        j = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        raise AssertionError(f"{tag}: {int((ratio > 1.0).sum())} of {ratio.size} out of bound; worst at {j}: got {got[j]!r} want {want[j]!r} "
                             f"|err| {err[j]:.3e} bound {bound[j]:.3e}")
    return float(ratio.max()) if ratio.size else 0.0


def check_against_order_free(tag, A, group, R, mask, E, scale):
    """A float32 [T][n] and group [G][3] (the kernel's, or kernel_order()'s) against order_free() within its bounds."""
    ref = order_free(R, mask, E, scale)
    worst = hold(tag + ": A", A, ref["A"], ref["e_A"])
    hold(tag + ": Q", group[:, 0], ref["Q"], ref["e_Q"])
    assert np.array_equal(group[:, 1], ref["C"]) and np.array_equal(group[:, 2], ref["K"]), tag
    assert not (np.asarray(A)[mask == 0].view(np.uint32) != 0).any(), f"{tag}: an invalid entry is not +0"
    return worst
