"""float64 / NumPy restatement of the policy-shift measurement and the KL-adaptive learning-rate rule (csrc/policy_shift.hip), with
the bounds the tests hold the kernels to.  No GPU, no native library.

tg_lr_adapt: IEEE double `/`, `*` and comparisons, one operation each -- restated bit for bit (lr_rule()).

tg_policy_shift, per row: lp in float32 (gaussian_logp(): the bound of tests/returns_loss_fp64.py::logp_fp64), then in float64
    d = lp - logp_old            exact: the difference of two float32 numbers whose exponents lie < 29 apart
    k3 = expm1(d) - d            expm1: HIP's math documentation states 1 ulp for double; EXPM1_ULPS = 2 is twice that (as EXPF_ULPS is
                                 for expf), and NumPy's own expm1 lives inside it; the subtraction adds one rounding of |k3| <=
                                 |expm1 d| + |d|, the reference's another:
        |k3 - truth| <= (EXPM1_ULPS + 2) 2^-53 (|expm1 d| + |d|)
    clipped = d < log_lo || d > log_hi     exact given d; log_lo / log_hi are the host's doubles, the same here and there.
Sums of n terms added in ANY order differ from the exact sum by at most (n - 1) 2^-53 sum |term| (first order; SLACK covers the
rest); the reference sums are math.fsum's (exact, rounded once).  `rows` and `clipped rows` are sums of 0 / 1 below 2^53: exact.

Exact inputs (dyadic_inputs()): variance 1, means and actions multiples of 2^-6 below 4 in magnitude.  a - mu, its square and the sum
of up to 4 squares (< 256, multiples of 2^-12: 20 bits) are exact in float32 with or without FMA contraction, -0.5 * quad is exact,
and lp = fl32(-0.5 quad + fl32(const)) is ONE correctly rounded operation: NumPy reproduces lp, hence d, bit for bit, and only the
k3 bound and the reordering remain.

General inputs: lp carries e_lp (logp_fp64's bound; with a device log_std, inv_var = expf(-2 log_std) adds 2 EXPF_ULPS u to every
quadratic term and the constant -A/2 fl32(log 2 pi) - sum log_std is formed in float32: (A + 2) u (A/2 log 2 pi + sum |log_std|)).
d moves by at most e_lp, k3 by at most |expm1 d| e_lp + e^d e_lp^2 / 2 (Taylor; d k3 / dd = expm1 d), and a row whose float64 d lies
within e_lp of log_lo or log_hi may fall on either side: such rows are counted apart (at most EDGE_CAP of the rows)."""
import math

import numpy as np

from returns_loss_fp64 import EDGE_CAP, EXPF_ULPS, LOG_2PI, SLACK, U, logp_fp64

U53 = 2.0 ** -53
EXPM1_ULPS = 2.0
ROWS_PER_BLOCK, MAX_BLOCKS = 4096, 1024
EXACT_ROWS = [0, 1, 63, 64, 65, 4095, 4096, 4097, 1024 * 4096 + 1]


def blocks(rows):
    """tg_policy_shift_blocks."""
    return 0 if rows <= 0 else min(-(-rows // ROWS_PER_BLOCK), MAX_BLOCKS)


def log_bounds(epsilon):
    """(log_lo, log_hi) as the learners pass them."""
    return math.log1p(-float(epsilon)), math.log1p(float(epsilon))


def lr_rule(sums, desired_kl, factor, lr_min, lr_max, lr):
    """tg_lr_adapt: float64 [4] = {kl, clip_fraction, lr_in, lr_out}."""
    s = np.asarray(sums, dtype=np.float64)
    desired_kl, factor, lr_min, lr_max, lr = (np.float64(v) for v in (desired_kl, factor, lr_min, lr_max, lr))
    with np.errstate(divide="ignore", invalid="ignore"):
        kl, cf = s[1] / s[0], s[2] / s[0]
    out = lr
    if desired_kl > 0.0 and s[0] > 0.0:
        if kl > np.float64(2.0) * desired_kl:
            out = np.fmax(lr / factor, lr_min)
        elif kl < np.float64(0.5) * desired_kl:
            out = np.fmin(lr * factor, lr_max)
    return np.array([kl, cf, lr, out], dtype=np.float64)


LR_CASES = {  # name -> (sums, desired_kl, factor, lr_min, lr_max, lr) -> expected lr_out
    "above": ((100.0, 3.0, 10.0, -1.0), 0.01, 1.5, 1e-5, 1e-2, 1e-3),
    "below": ((100.0, 0.1, 0.0, 0.2), 0.01, 1.5, 1e-5, 1e-2, 1e-3),
    "between": ((100.0, 1.0, 5.0, 0.0), 0.01, 1.5, 1e-5, 1e-2, 1e-3),
    "at_upper_threshold": ((100.0, 2.0, 5.0, 0.0), 0.01, 1.5, 1e-5, 1e-2, 1e-3),
    "at_lower_threshold": ((128.0, 0.64, 5.0, 0.0), 0.01, 1.5, 1e-5, 1e-2, 1e-3),
    "clamp_min": ((100.0, 3.0, 10.0, -1.0), 0.01, 1.5, 1e-5, 1e-2, 1.2e-5),
    "clamp_max": ((100.0, 0.1, 0.0, 0.2), 0.01, 1.5, 1e-5, 1e-2, 9e-3),
    "no_rows": ((0.0, 0.0, 0.0, 0.0), 0.01, 1.5, 1e-5, 1e-2, 1e-3),
    "nan_sum": ((100.0, float("nan"), 1.0, 0.0), 0.01, 1.5, 1e-5, 1e-2, 1e-3),
    "measure_only": ((100.0, 3.0, 10.0, -1.0), 0.0, 1.5, 1e-5, 1e-2, 1e-3),
    "factor_2": ((7.0, 3.0, 1.0, 0.5), 0.05, 2.0, 1e-6, 1.0, 0.3),
}


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def k3_of(d):
    d = np.asarray(d, dtype=np.float64)
    return np.expm1(d) - d


def shift_sums(d, log_lo, log_hi, e_d=None):
    """From float64 d [n] (and its per-row error e_d, default exact) -> dict: sums float64 [4] = {rows, sum k3, clipped rows, sum d}
    of the rows that are not `edge`, bound_k3, bound_d on the two floating-point sums, n_edge."""
    d = np.asarray(d, dtype=np.float64)
    n = d.size
    e_d = np.zeros(n) if e_d is None else np.asarray(e_d, dtype=np.float64)
    em1 = np.expm1(d)
    k3 = em1 - d
    edge = (np.abs(d - log_lo) <= e_d) | (np.abs(d - log_hi) <= e_d)
    clipped = (d < log_lo) | (d > log_hi)
    row_k3 = (EXPM1_ULPS + 2) * U53 * (np.abs(em1) + np.abs(d)) + np.abs(em1) * e_d + 0.5 * np.exp(d + e_d) * e_d * e_d
    bound_k3 = (math.fsum(row_k3) + max(n - 1, 0) * U53 * math.fsum(np.abs(k3) + row_k3)) * SLACK
    bound_d = (math.fsum(e_d) + max(n - 1, 0) * U53 * math.fsum(np.abs(d) + e_d)) * SLACK
    return {"sums": np.array([float(n), math.fsum(k3), float((clipped & ~edge).sum()), math.fsum(d)]), "bound_k3": bound_k3,
            "bound_d": bound_d, "n_edge": int(edge.sum()), "d": d}


def check_sums(got, ref, tag=""):
    """got float64 [4] against shift_sums()'s dict: counts exact (edge rows may or may not be clipped), sums within the bounds."""
    got = np.asarray(got, dtype=np.float64)
    s = ref["sums"]
    assert got[0] == s[0], (tag, "rows", got[0], s[0])
    assert ref["n_edge"] <= EDGE_CAP * max(s[0], 1.0), (tag, "edge rows", ref["n_edge"], s[0])
    assert s[2] <= got[2] <= s[2] + ref["n_edge"], (tag, "clipped rows", got[2], s[2], ref["n_edge"])
    for j, key in ((1, "bound_k3"), (3, "bound_d")):
        err = abs(got[j] - s[j])
        print(f"{tag} sums[{j}] got {got[j]!r} want {s[j]!r} |err| {err:.3e} bound {ref[key]:.3e}")
        assert np.isfinite(got[j]) and err <= ref[key], (tag, j, got[j], s[j], err, ref[key])
    assert got[1] >= 0.0 or abs(got[1]) <= ref["bound_k3"], (tag, "k3 >= 0", got[1])


# ---- exact inputs ----
def dyadic_inputs(A, rows, seed=0):
    """means, actions float32 [rows][A] (multiples of 2^-6 below 4), logp_old float32 [rows] = fl32(lp + delta), delta a multiple of
    2^-10 in [-1/2, 1/2] (so that both clip sides occur at epsilon = 0.2), var = ones."""
    rng = np.random.default_rng(1000 * A + seed + rows % 997)
    mean = (rng.integers(-255, 256, size=(rows, A)) / 64.0).astype(np.float32)
    act = (rng.integers(-255, 256, size=(rows, A)) / 64.0).astype(np.float32)
    lp = dyadic_logp(mean, act)
    delta = (rng.integers(-512, 513, size=rows) / 1024.0).astype(np.float32)
    return mean, act, (lp + delta).astype(np.float32), np.ones(A, dtype=np.float32)


def dyadic_logp(mean, act):
    """The kernel's float32 lp for dyadic inputs at variance 1, bit for bit: one rounded addition."""
    A = mean.shape[1]
    quad = ((act.astype(np.float64) - mean.astype(np.float64)) ** 2).sum(1)
    assert np.all(quad == quad.astype(np.float32)) and np.all(quad < 256.0)
    const = np.float32(-0.5 * A * math.log(2.0 * 3.141592653589793))
    return (np.float32(-0.5) * quad.astype(np.float32) + const).astype(np.float32)


def dyadic_reference(mean, act, logp_old, epsilon):
    lo, hi = log_bounds(epsilon)
    d = dyadic_logp(mean, act).astype(np.float64) - logp_old.astype(np.float64)
    return shift_sums(d, lo, hi)


# ---- general inputs ----
def logp_reference(mean, act, var=None, log_std=None):
    """-> (lp float64 [rows], e_lp): the float64 log-probability and the bound on the kernel's float32 one."""
    mean, act = np.asarray(mean, dtype=np.float32), np.asarray(act, dtype=np.float32)
    if log_std is None:
        return logp_fp64(mean, act, var)
    ls = np.asarray(log_std, dtype=np.float32).astype(np.float64)
    A = ls.size
    v = np.exp(2.0 * ls)
    d = act.astype(np.float64) - mean.astype(np.float64)
    quad = (d * d / v).sum(1)
    const = -0.5 * A * LOG_2PI - ls.sum()
    lp = -0.5 * quad + const
    e = U * ((A + 4 + 2 * EXPF_ULPS) * quad / 2 + (A + 2) * (0.5 * A * LOG_2PI + np.abs(ls).sum()) + np.abs(lp)) * SLACK
    return lp, e


def general_reference(mean, act, logp_old, epsilon, var=None, log_std=None):
    lo, hi = log_bounds(epsilon)
    lp, e = logp_reference(mean, act, var, log_std)
    return shift_sums(lp - np.asarray(logp_old, dtype=np.float32).astype(np.float64), lo, hi, e)


GENERAL_CASES = {  # name -> (A, rows, row stride of the means, learned log_std?, actions transposed?)
    "a8_fixed": (8, 10007, 8, False, False),
    "a8_fixed_strided": (8, 4097, 11, False, True),
    "a4_log_std_stride8": (4, 10007, 8, True, False),
    "a4_log_std_strided_act": (4, 4097, 8, True, True),
    "a3_fixed": (3, 5000, 3, False, False),
}
GENERAL_EPSILON = 0.2


def general_inputs(name):
    """-> dict(mean_buf float32 [rows][stride] (the kernel reads [:, :A]), act float32 [rows][A], act_t (store the actions [A][rows] and
    pass the transposed view), logp_old, var | log_std).  logp_old = fl32(lp64 + delta) with |delta| uniform in [0, 0.4] and kept
    at least 1e-3 away from both clip edges, far beyond e_lp (~1e-6): the float64 reference has no edge rows (asserted on the CPU)."""
    A, rows, stride, learned, act_t = GENERAL_CASES[name]
    rng = np.random.default_rng(sorted(GENERAL_CASES).index(name) + 77)
    buf = rng.standard_normal((rows, stride)).astype(np.float32)
    mean = buf[:, :A]
    out = {"mean_buf": buf, "A": A, "act_t": act_t}
    if learned:
        out["log_std"] = rng.uniform(-0.7, 0.3, size=A).astype(np.float32)
        sigma = np.exp(out["log_std"].astype(np.float64))
    else:
        out["var"] = rng.uniform(0.2, 1.5, size=A).astype(np.float32)
        sigma = np.sqrt(out["var"].astype(np.float64))
    out["act"] = (mean + sigma * rng.standard_normal((rows, A))).astype(np.float32)
    lp, _ = logp_reference(mean, out["act"], out.get("var"), out.get("log_std"))
    lo, hi = log_bounds(GENERAL_EPSILON)
    delta = rng.uniform(-0.4, 0.4, size=rows)
    for edge in (lo, hi):                       # (d = lp - old = -delta)
        near = np.abs(-delta - edge) < 1e-3
        delta[near] += 4e-3
    out["logp_old"] = (lp + delta).astype(np.float32)
    return out
