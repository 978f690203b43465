"""float64 restatements of the scalar side of learn() -- reward-to-go, GAE, masked group moments, group normalisation, the
Gaussian log-probability and the clipped-surrogate loss head -- with the checkers that hold a kernel's output (plain arrays)
against them, and the input recipes the CPU and GPU tests share.  numpy / torch-CPU only; imports no GPU code.

The restatements take the float32 inputs as given (every float32 is exact in float64) and evaluate in float64; the moments sum
in np.longdouble.  Layout is the device trajectory's: [T][n], env index fastest; a loss row is one sample.

Every bound below follows from the operations the kernel performs (csrc/returns_kernels.hip, csrc/loss_kernels.hip), with
u = 2^-24 the float32 unit roundoff and one u |result| per individually rounded operation (rn_add / rn_sub / rn_mul / rn_div).
Magnitudes are taken from the float64 restatement; the kernel's own intermediates differ from them by O(u), which is second
order: every bound is multiplied by SLACK = 1 + 2^-10 for that and for nothing else.  A product with the mask (0.0 or 1.0) is
exact and gets no term.

Reward-to-go (rtg_scan_kernel, returns_moments_kernel, ppo_returns_kernel<false>):
    R_t = rn_add(rn_mul(r_t, m_t), carry),  carry = rn_mul(rn_mul(g, R_{t+1}), m_{t+1}),  g = fl32(gamma):
    E_t = g E_{t+1} m_{t+1} + u (|g R_{t+1}| m_{t+1} + |R_t|).
    Monte-Carlo advantage A_t = rn_sub(R_t, V_t):  E_t + u |A_t|.

GAE (gae_scan_kernel, ppo_returns_kernel<true>), c the coefficient of A_{t+1}:
    p = rn_mul(g, V_{t+1} m_{t+1});  s = rn_add(r_t, p);  delta = rn_sub(s, V_t);  A_t = rn_add(delta, q),
    q = rn_mul(rn_mul(c, A_{t+1}), m_{t+1});  last step A = rn_sub(r, V);  ret_t = rn_add(V_t, A_t):
    E_t = c E_{t+1} m_{t+1} + u (|p| + |s| + |delta| + |A_t| + (1 + COEF_ULPS) |c A_{t+1}| m_{t+1}),   ret: E_t + u |ret_t|.
    The restatement's c is the reference's, fl32(gamma * lam) (the double product rounded once, algorithms/ppo.py:119); the
    kernel forms rn_mul(fl32(gamma), fl32(lam)).  Both lie within (1 + u)^3 resp. (1 + u) of gamma * lam, hence within
    COEF_ULPS = 4 u of each other: that is the extra term on |c A_{t+1}|.  (They are equal for most pairs, and differ by one
    float32 ulp at (0.995, 0.97).)

Masked moments (env_moments_kernel / lane_moments + group_moments_kernel): float64 sums of float32 values (x * x is exact in
    float64).  The count must be exact; |s1 - sum x| <= N 2^-53 sum |x| and |s2 - sum x^2| <= N 2^-53 sum x^2, the bound of
    recursive summation of N terms in any order (N the count; the kernel's tree is shallower).

Group normalisation (group_normalize_kernel): mean = s1 / cnt, var = (s2 - s1 mean) / (cnt - 1) in float64, then
    meanf = (float) mean, stdf = (float) sqrt(var), den = stdf (mode 0) or rn_add(stdf, 1e-8f) (mode 1),
    out = rn_div(rn_sub(x, meanf), den).  The kernel's sums are nested (T steps per lane, ceil(group / 256) strided terms, a
    6-step shuffle tree, 3 adds): depth D = T + ceil(group / 256) + 9, so s1, s2 are off by at most D 2^-53 of their sums of
    magnitudes, and the one-pass variance by e_var = (3 D + 4) 2^-53 sum x^2 / ((cnt - 1) var) relatively -- the term that
    grows like (mean / std)^2.  The input recipe keeps |mean| / std <= ~100 and checker asserts e_var < u.  Then
        |out - truth| <= (u + D 2^-53 sum|x| / |s1|) |mean| / den + |truth| (u [sub] + u [div] + u [(float) std] + e_var / 2
                          + (mode 1: 2 u, the rounding of 1e-8f and of the sum)).
    A group of one valid entry gives 0 / 0 = NaN on that entry, as torch.std does; a group of none leaves zeros.  A group of
    zero variance is OUT OF SCOPE: the one-pass variance need not round to exactly 0 there, and x / 0 amplifies whatever is left.

Gaussian log-probability (gaussian_logp(), make_var()): d_k = a_k - mu_k (u), d_k * d_k (u), * inv_var_k (u) with inv_var_k =
    1.0f / var_k (u) -- 5 u relative per term counting d twice --, A - 1 rounded additions of partial sums <= quad, * -0.5
    exact, + logp_const rounded (u |lp|), logp_const = (float)(float64 expression) (u |const|):
        |lp - truth| <= u ((A + 4) quad / 2 + |const| + |lp|).      FMA contraction only removes roundings.

Loss head (surrogate_loss_kernel): expf has no published accuracy on this target, so the gradients, the std rows and the loss
    sums are held to the project's yardstick from tests/test_learned_std_gpu.py -- the ONE assumed quantity here: the error
    against float64 may be at most BAR_FACTOR = 4 times the error of torch's own float32 evaluation of the same expressions on
    the same inputs, floored at 4 x 2^-23 of the largest reference magnitude.  Gradients: max over the compared rows.  Sums:
    the kernel adds float32 per-row terms in float64, so the bar is on sum_i |term32_i - term64_i| of torch's rows, floored at
    4 x 2^-23 sum_i |term64_i|.  A one-row launch (M = 1) is a row of the M = 255 case and is held to that case's bars (its one
    term per sum to the bar on max_i |term32_i - term64_i|): a single row says nothing about torch's error.
    Rows near a clip edge: the kernel's rho is exp(x + e_x) (1 + e_exp) with |e_x| <= (log-prob bound) + u |lp - lp_old|, and
    lo / hi = rn(1 -+ eps) carry u.  A row whose float64 rho is within  delta = EDGE_FACTOR (e_x + (2 EXPF_ULPS + 1) u)  of an
    edge, relatively, may take either branch (one ulp is up to 2 u).  EXPF_ULPS = 2 (HIP documents 1) enters ONLY the width of this band, and
    EDGE_FACTOR = 2 leaves room for torch's float32 rows (two more roundings in the constant) to stay on the float64 branch
    outside it -- the checker verifies that they do.  Such rows are excluded from the bar and from the comparison; their
    gradient must equal one of the two branch values within the bar, and they may be at most EDGE_CAP = 0.1 % of the valid rows
    (x is uniform, so the expected share is 4 delta / 3 ~ 1e-5).
"""
import math

import numpy as np
import torch

U = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -10
COEF_ULPS = 4.0
BAR_FACTOR = 4.0
EXPF_ULPS = 2.0
EDGE_FACTOR = 2.0
EDGE_CAP = 1e-3
CELL_MIN = 0.05
LOG_2PI = math.log(2.0 * math.pi)
GARBAGE = 1e30                        # finite, large: what lies beyond an episode's end where the reference never looks


def coef_reference(gamma, lam):
    """fl32(gamma * lam): the double product rounded once (the reference, algorithms/ppo.py:119)."""
    return np.float32(float(gamma) * float(lam))


def coef_kernel(gamma, lam):
    """rn_mul(fl32(gamma), fl32(lam)): what gae_scan_kernel / ppo_returns_kernel form."""
    return np.float32(np.float32(gamma) * np.float32(lam))


# ------------------------------------------------------------------------------------------------------------------------------
# checkers' common part
# ------------------------------------------------------------------------------------------------------------------------------
def _hold(tag, got, want, bound, where=None):
    """|got - want| <= bound on `where` (default everywhere); raises with the worst element; returns max err / bound."""
    got, want, bound = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    bound = np.broadcast_to(bound, want.shape)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    sel = np.ones(want.shape, dtype=bool) if where is None else np.broadcast_to(where, want.shape)
    if not sel.any():
        return 0.0
    g, w, b = got[sel], want[sel], bound[sel]
    err = np.abs(g - w)
    err = np.where(np.isfinite(g), err, np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0.0, 0.0, err / b)
    j = int(np.argmax(ratio))
    if not ratio[j] <= 1.0:
        idx = tuple(int(v[j]) for v in np.nonzero(sel))
        raise AssertionError(f"{tag}: {int((ratio > 1.0).sum())} of {ratio.size} out of bound; worst at {idx}: got {g[j]!r} want {w[j]!r} "
                             f"|err| {err[j]:.3e} bound {b[j]:.3e}")
    return float(ratio[j])


# ------------------------------------------------------------------------------------------------------------------------------
# the two scans
# ------------------------------------------------------------------------------------------------------------------------------
def rtg_fp64(rew, mask, gamma):
    """-> (R, E) float64 [T][n]: reward-to-go and the propagated bound on a float32 kernel's error."""
    r, m = rew.astype(np.float64), mask.astype(np.float64)
    g = float(np.float32(gamma))
    T = r.shape[0]
    R, E = np.zeros_like(r), np.zeros_like(r)
    for t in range(T - 1, -1, -1):
        if t == T - 1:
            R[t] = r[t] * m[t]
            E[t] = 0.0                                                   # r * m is exact, and so is + 0
        else:
            c = g * R[t + 1] * m[t + 1]
            R[t] = r[t] * m[t] + c
            E[t] = g * E[t + 1] * m[t + 1] + U * (np.abs(c) + np.abs(R[t]))
    return R, E * SLACK


def gae_fp64(rew, val, mask, gamma, lam, coef=None, masked_reward=False):
    """-> (A, ret, E_A, E_ret) float64 [T][n].  coef: the coefficient of A_{t+1} (default the reference's fl32(gamma * lam)).
    masked_reward: the WRONG delta (r_t m_t) -- for the mutation tests only."""
    r, v, m = rew.astype(np.float64), val.astype(np.float64), mask.astype(np.float64)
    if masked_reward:
        r = r * m
    g = float(np.float32(gamma))
    c = float(coef_reference(gamma, lam) if coef is None else coef)
    T = r.shape[0]
    A, E = np.zeros_like(r), np.zeros_like(r)
    for t in range(T - 1, -1, -1):
        if t == T - 1:
            A[t] = r[t] - v[t]
            E[t] = U * np.abs(A[t])
        else:
            p = g * (v[t + 1] * m[t + 1])
            s = r[t] + p
            delta = s - v[t]
            q = c * A[t + 1] * m[t + 1]
            A[t] = delta + q
            E[t] = c * E[t + 1] * m[t + 1] + U * (np.abs(p) + np.abs(s) + np.abs(delta) + np.abs(A[t]) + (1.0 + COEF_ULPS) * np.abs(q))
    ret = v + A
    return A, ret, E * SLACK, (E + U * np.abs(ret)) * SLACK


def rtg_scan_f32(rew, mask, gamma):
    """The kernel's operation order in numpy float32 (no FMA): bit for bit oracle.learner.rtg_scan."""
    r, m, g = rew.astype(np.float32), mask.astype(np.float32), np.float32(gamma)
    R = np.zeros_like(r)
    carry = np.zeros(r.shape[1:], dtype=np.float32)
    for t in range(r.shape[0] - 1, -1, -1):
        R[t] = r[t] * m[t] + carry
        carry = (g * R[t]) * m[t]
    return R


def gae_scan_f32(rew, val, mask, gamma, coef):
    """The kernel's operation order in numpy float32 with the float32 coefficient `coef` given: with coef_reference() it is
    oracle.learner.gae_scan bit for bit, with coef_kernel() the kernel.  -> (adv, ret)."""
    r, v, m = rew.astype(np.float32), val.astype(np.float32), mask.astype(np.float32)
    g, c = np.float32(gamma), np.float32(coef)
    T = r.shape[0]
    A = np.zeros_like(r)
    nvm = np.zeros(r.shape[1:], dtype=np.float32)
    nam = np.zeros(r.shape[1:], dtype=np.float32)
    for t in range(T - 1, -1, -1):
        A[t] = r[t] - v[t] if t == T - 1 else ((r[t] + g * nvm) - v[t]) + nam
        nvm = v[t] * m[t]
        nam = (c * A[t]) * m[t]
    return A, v + A


def check_rtg(got, rew, mask, gamma, tag="rtg"):
    """got [T][n] against the float64 reward-to-go, everywhere (a masked reward is multiplied by 0: garbage there is ignored)."""
    R, E = rtg_fp64(rew, mask, gamma)
    return _hold(tag, got, R, E)


def check_mc_adv(got_adv, rew, val, mask, gamma, tag="mc adv"):
    R, E = rtg_fp64(rew, mask, gamma)
    A = R - val.astype(np.float64)
    return _hold(tag, got_adv, A, (E + U * np.abs(A)) * SLACK)


def check_gae(got_adv, got_ret, rew, val, mask, gamma, lam, tag="gae"):
    """Everywhere: beyond an episode's end the reference never reads A or ret, but the kernel documents what it writes there
    (delta from the UNMASKED reward), and only there can a delta from the masked reward be told from the right one."""
    A, ret, EA, Er = gae_fp64(rew, val, mask, gamma, lam)
    return max(_hold(tag + " adv", got_adv, A, EA), _hold(tag + " ret", got_ret, ret, Er))


# ------------------------------------------------------------------------------------------------------------------------------
# masked moments and group normalisation
# ------------------------------------------------------------------------------------------------------------------------------
def _groups(a, group_size):
    """[T][n] -> [G][T * group_size] (group g = envs [g * group_size, (g + 1) * group_size))."""
    T, n = a.shape
    return a.reshape(T, n // group_size, group_size).transpose(1, 0, 2).reshape(n // group_size, -1)


def moments_fp64(x, mask, group_size):
    """-> (count int64 [G], s1, s2, sum |x| : np.longdouble [G]) over the valid entries of each group."""
    xg = _groups(x, group_size).astype(np.longdouble)
    mg = _groups(mask, group_size).astype(bool)
    xg = np.where(mg, xg, np.longdouble(0))
    return mg.sum(1).astype(np.int64), xg.sum(1), (xg * xg).sum(1), np.abs(xg).sum(1)


def moments_plain(x, mask, group_size, base_stride=None, max_e=None):
    """Plain float64 torch sums, [G][3].  base_stride / max_e: the WRONG kernels of the mutation tests -- group g read from env
    g * base_stride on, and entries e >= max_e of a group dropped."""
    T, n = x.shape
    G = n // group_size
    xt, mt = torch.from_numpy(x.astype(np.float64)), torch.from_numpy(mask.astype(bool))
    out = torch.zeros(G, 3, dtype=torch.float64)
    for g in range(G):
        b = g * (group_size if base_stride is None else base_stride)
        e = group_size if max_e is None else min(group_size, max_e)
        v = xt[:, b:b + e][mt[:, b:b + e]]
        out[g] = torch.stack([torch.tensor(float(v.numel()), dtype=torch.float64), v.sum(), (v * v).sum()])
    return out.numpy()


def check_moments(got, x, mask, group_size, tag="moments"):
    """got f64 [G][3] = (count, sum, sum of squares)."""
    cnt, s1, s2, sa = moments_fp64(x, mask, group_size)
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == (cnt.size, 3), (tag, got.shape)
    bad = np.nonzero(got[:, 0] != cnt.astype(np.float64))[0]
    if bad.size:
        raise AssertionError(f"{tag}: count of group {int(bad[0])} is {got[bad[0], 0]!r}, want {int(cnt[bad[0]])}")
    N = cnt.astype(np.float64)
    r1 = _hold(tag + " s1", got[:, 1], s1.astype(np.float64), N * 2.0 ** -53 * sa.astype(np.float64) * SLACK)
    r2 = _hold(tag + " s2", got[:, 2], s2.astype(np.float64), N * 2.0 ** -53 * s2.astype(np.float64) * SLACK)
    return max(r1, r2)


def normalize_fp64(x, mask, group_size, mode, biased=False, no_eps=False):
    """-> (truth, bound, count of the entry's group: float64 [T][n]; e_var [G]); truth is 0 on masked entries and NaN in a group of < 2 valid ones.
    biased / no_eps: the WRONG kernels of the mutation tests."""
    T, n = x.shape
    cnt, s1, s2, sa = moments_fp64(x, mask, group_size)
    N = cnt.astype(np.longdouble)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = s1 / N
        xg = _groups(x, group_size).astype(np.longdouble)
        mg = _groups(mask, group_size).astype(bool)
        dev2 = (np.where(mg, xg - mean[:, None], 0) ** 2).sum(1)             # two-pass
        var = dev2 / (N if biased else N - 1)
        std = np.sqrt(var)
        den = std + (np.longdouble(1e-8) if mode == 1 and not no_eps else 0)
        D = T + -(-group_size // 256) + 9
        e_mean = U + D * 2.0 ** -53 * sa / np.abs(s1)
        e_var = (3 * D + 4) * 2.0 ** -53 * s2 / ((N - 1) * var)
        per = lambda a: np.repeat(a.astype(np.float64), group_size)[None, :]
        truth = (x.astype(np.float64) - per(mean)) / per(den)
        rel = 3 * U + per(e_var) / 2 + (2 * U if mode == 1 else 0.0)
        bound = (np.where(per(mean) == 0, 0.0, per(e_mean) * np.abs(per(mean))) / per(den) + np.abs(truth) * rel) * SLACK
    w = mask.astype(bool)
    truth = np.where(w, truth, 0.0)
    return truth, bound, per(cnt) + np.zeros((T, 1)), e_var.astype(np.float64)


def check_normalize(got, x, mask, group_size, mode, tag="normalize"):
    truth, bound, cnt, e_var = normalize_fp64(x, mask, group_size, mode)
    got = np.asarray(got, dtype=np.float64)
    w = mask.astype(bool)
    if not np.array_equal(got[~w], np.zeros(int((~w).sum()))):
        raise AssertionError(f"{tag}: a masked entry is not exactly 0")
    one = w & (cnt == 1)
    if not np.isnan(got[one]).all():
        raise AssertionError(f"{tag}: the valid entry of a one-entry group must be NaN, as torch.std makes it")
    cmp = w & (cnt >= 2)
    groups = np.unique((np.nonzero(cmp)[1] // group_size)) if cmp.any() else []
    for g in groups:
        assert e_var[g] < U, f"{tag}: the input recipe must keep the one-pass variance term below 2^-24 (group {g}: {e_var[g]:.3e})"
    return _hold(f"{tag} mode {mode}", got, truth, bound, where=cmp)


def normalize_oracle32(x, mask, group_size, mode, biased=False, no_eps=False):
    """torch float32 element-wise operations on float64 group statistics (torch.mean / torch.std of the float64 values): what
    the kernel's design is.  torch's all-float32 mean carries log2(N) u |mean| of summation error, which at |mean| / std = 100
    is outside a bound derived for float64 moments -- that is why the statistics are not float32 here."""
    T, n = x.shape
    out = np.zeros((T, n), dtype=np.float32)
    for g in range(n // group_size):
        sl = slice(g * group_size, (g + 1) * group_size)
        m = torch.from_numpy(mask[:, sl].astype(bool))
        v = torch.from_numpy(x[:, sl])[m]
        if v.numel() == 0:
            continue
        mean = v.double().mean().float()
        std = v.double().std(unbiased=not biased).float() if v.numel() > 1 or biased else torch.tensor(float("nan"))
        den = std if mode == 0 or no_eps else std + 1e-8
        o = torch.zeros(T, group_size)
        o[m] = (v - mean) / den
        out[:, sl] = o.numpy()
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# Gaussian log-probability
# ------------------------------------------------------------------------------------------------------------------------------
def logp_fp64(mean, act, var):
    """-> (lp, bound) float64 [M]; var float32 [A] as given."""
    v = np.asarray(var, dtype=np.float32).astype(np.float64)
    A = v.size
    d = act.astype(np.float64) - mean.astype(np.float64)
    quad = (d * d / v).sum(1)
    const = -0.5 * A * LOG_2PI - 0.5 * np.log(v).sum()
    lp = -0.5 * quad + const
    return lp, U * ((A + 4) * quad / 2 + abs(const) + np.abs(lp)) * SLACK


def check_logp(got, mean, act, var, tag="logp", extra=0.0):
    """extra: an allowance on top of the kernel's bound, for an evaluation that rounds more often than the kernel (torch's)."""
    lp, b = logp_fp64(mean, act, var)
    return _hold(tag, got, lp, b + extra)


def logp_oracle32(mean, act, var, drop_column=None):
    """oracle.learner.gaussian_log_prob in torch float32.  drop_column: the WRONG kernel that skips one action column."""
    from oracle.learner import gaussian_log_prob
    lp = gaussian_log_prob(torch.from_numpy(mean), torch.from_numpy(act), torch.from_numpy(np.asarray(var, dtype=np.float32)))
    if drop_column is not None:
        k = drop_column
        lp = lp + 0.5 * (torch.from_numpy(act[:, k]) - torch.from_numpy(mean[:, k])) ** 2 / float(var[k])
    return lp.numpy()


# ------------------------------------------------------------------------------------------------------------------------------
# the loss head
# ------------------------------------------------------------------------------------------------------------------------------
def _clean(inp):
    """The inputs with hidden rows' entries replaced by 0 (the reference never reads them; they hold NaN)."""
    m = inp["mask"].astype(bool)
    out = dict(inp)
    for k in ("mean", "act", "logp_old", "adv", "value", "ret", "logp_ref"):
        if inp.get(k) is not None:
            a = inp[k]
            out[k] = np.where(m.reshape((-1,) + (1,) * (a.ndim - 1)), a, np.float32(0))
    return out, m


def loss_fp64(inp, mutate=None, dtype=np.float64):
    """The loss head in closed form.  inp: dict of float32 arrays / scalars as the kernel gets them (loss_inputs()).  -> dict with
    sums f64 [4] = (sum surrogate, sum squared error, sum KL term, valid count), grad_mean [M][A], grad_value [M] | None,
    std_rows [M][4] | None, and the per-row pieces the checker needs.
    dtype=np.float32 evaluates the same closed form in numpy float32 (an emulation of a correct kernel, for the CPU tests);
    mutate: "keep_neg_below" / "drop_neg_above" / "ignore_mask" -- the WRONG kernels of the mutation tests; "flip": every
    row takes the branch on the other side of its nearer clip edge (the alternative value of a row near an edge)."""
    c, valid = _clean(inp)
    if mutate == "ignore_mask":
        c, valid = dict(inp), np.ones_like(valid)
    f = dtype
    mean, act, lpo, adv = (c[k].astype(f) for k in ("mean", "act", "logp_old", "adv"))
    M, A = mean.shape
    if c.get("log_std") is not None:
        ls = c["log_std"].astype(f)
        inv_var = np.exp(f(-2.0) * ls)
        const = f(f(-0.5 * A) * f(np.float32(1.8378770664093453)) - ls.sum(dtype=f)) if f is np.float32 else -0.5 * A * LOG_2PI - ls.sum()
    else:
        v = c["var"].astype(f)
        inv_var = f(1.0) / v
        const = f(-0.5 * A * LOG_2PI - 0.5 * np.log(c["var"].astype(np.float64)).sum())
    d = act - mean
    quad = (d * d * inv_var).sum(1, dtype=f)
    lp = f(-0.5) * quad + const
    am, ai, rm, ri = (f(t) for t in (c["norm"] if c.get("norm") is not None else (0.0, 1.0, 0.0, 1.0)))
    advn = (adv - am) * ai if c.get("norm") is not None else adv
    surr_coef, critic_coef, kl_coef = (f(t) for t in c["coefs"])
    eps = f(c["epsilon"])
    lo, hi = f(1.0) - eps, f(1.0) + eps
    rho = np.exp(lp - lpo)
    s1, s2 = rho * advn, np.clip(rho, lo, hi) * advn
    inside = (rho >= lo) & (rho <= hi)
    w = np.where(inside, True, s1 < s2)
    if mutate == "keep_neg_below":
        w = w | ((advn < 0) & (rho < lo))
    elif mutate == "drop_neg_above":
        w = w & ~((advn < 0) & (rho > hi))
    elif mutate == "flip":                                   # an inside row seen as outside (beyond the nearer edge), and the reverse
        w = np.where(inside, np.where(np.abs(rho - hi) < np.abs(rho - lo), advn < 0, advn > 0), True)
    surr = np.minimum(s1, s2)
    dlp = surr_coef * advn * rho * w.astype(f)
    kl = np.zeros(M, dtype=f)
    if kl_coef != 0:
        eo = np.exp(lpo)
        kl = eo * (lpo - lp)
        dlp = dlp - kl_coef * eo
    if c.get("logp_ref") is not None:
        x = c["logp_ref"].astype(f) - lp
        em1 = np.expm1(x) if f is np.float64 else np.exp(x) - f(1.0)
        kl = kl + (em1 - x)
        dlp = dlp + f(c["ref_coef"]) * em1
    g = dlp[:, None] * d * inv_var
    out = dict(valid=valid, rho=rho.astype(np.float64), advn=advn.astype(np.float64), inside=inside, quad=quad.astype(np.float64),
               lp=lp.astype(np.float64), const=float(const))
    vz = valid.astype(f)
    out["grad_mean"] = (g * vz[:, None]).astype(np.float64)
    terms = [surr * vz, np.zeros(M, dtype=f), kl * vz]
    out["grad_value"] = None
    if c.get("value") is not None:
        dv = c["value"].astype(f) - (c["ret"].astype(f) - rm) * ri
        terms[1] = dv * dv * vz
        out["grad_value"] = (critic_coef * f(2.0) * dv * vz).astype(np.float64)
    out["std_rows"] = None
    if c.get("log_std") is not None:
        rows = np.zeros((M, 4), dtype=np.float64)
        rows[:, :A] = dlp[:, None] * (d * d * inv_var - f(1.0)) * vz[:, None]
        out["std_rows"] = rows
    out["terms"] = [t.astype(np.float64) for t in terms]
    out["sums"] = np.array([math.fsum(t) for t in out["terms"]] + [float(valid.sum())])
    return out


def loss_torch32(inp):
    """torch's float32 evaluation of the same expressions (oracle.learner.grpo_objective / ppo_loss's formulae, sums instead of
    means, the coefficients applied as the kernel gets them) with autograd for d / d mean and d / d value.  Same dict as
    loss_fp64()."""
    c, valid = _clean(inp)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    mean = t(c["mean"]).requires_grad_(True)
    act, lpo, adv = t(c["act"]), t(c["logp_old"]), t(c["adv"])
    M, A = mean.shape
    vz = t(valid.astype(np.float32))
    if c.get("log_std") is not None:
        ls = t(c["log_std"])
        inv_var = torch.exp(-2.0 * ls)
        lp = -0.5 * ((act - mean) ** 2 * inv_var).sum(1) - 0.5 * A * LOG_2PI - ls.sum()
    else:
        var = t(c["var"])
        inv_var = 1.0 / var
        lp = -0.5 * (((act - mean) ** 2) / var).sum(1) - 0.5 * A * LOG_2PI - 0.5 * torch.log(var).sum()
    lp.retain_grad()
    eps = float(np.float32(c["epsilon"]))
    sc, cc, kc = (torch.tensor(np.float32(v)) for v in c["coefs"])
    if c.get("norm") is not None:
        am, ai, rm, ri = (torch.tensor(np.float32(v)) for v in c["norm"])
        advn = (adv - am) * ai
    else:
        advn = adv
    rho = torch.exp(lp - lpo)
    lo, hi = torch.tensor(1.0) - torch.tensor(np.float32(c["epsilon"])), torch.tensor(1.0) + torch.tensor(np.float32(c["epsilon"]))
    surr = torch.min(rho * advn, torch.clamp(rho, float(lo), float(hi)) * advn) * vz
    total = sc * surr.sum()
    terms = [surr, torch.zeros(M), torch.zeros(M)]
    if float(kc) != 0.0:
        terms[2] = torch.exp(lpo) * (lpo - lp) * vz
        total = total + kc * terms[2].sum()
    if c.get("logp_ref") is not None:
        x = t(c["logp_ref"]) - lp
        terms[2] = (torch.exp(x) - x - 1.0) * vz
        total = total - torch.tensor(np.float32(c["ref_coef"])) * terms[2].sum()
    value = None
    if c.get("value") is not None:
        value = t(c["value"]).requires_grad_(True)
        terms[1] = (value - (t(c["ret"]) - rm) * ri) ** 2 * vz
        total = total + cc * terms[1].sum()
    total.backward()
    out = dict(valid=valid, rho=rho.detach().double().numpy(), grad_mean=mean.grad.double().numpy(),
               grad_value=None if value is None else value.grad.double().numpy(), std_rows=None)
    if c.get("log_std") is not None:
        rows = np.zeros((M, 4))
        d = (act - mean).detach()
        rows[:, :A] = (lp.grad[:, None] * (d * d * inv_var - 1.0)).double().numpy()
        out["std_rows"] = rows
    out["terms"] = [x_.detach().double().numpy() for x_ in terms]
    out["sums"] = np.array([math.fsum(x_) for x_ in out["terms"]] + [float(valid.sum())])
    return out


def clip_cells(ref):
    """Share of the valid rows in each (sign of the advantage) x (rho below / inside / above the clip range) cell, float64."""
    v, rho, a = ref["valid"], ref["rho"], ref["advn"]
    lo, hi = ref["lo"], ref["hi"]
    n = max(int(v.sum()), 1)
    pos = {"below": rho < lo, "inside": (rho >= lo) & (rho <= hi), "above": rho > hi}
    return {(s, k): float((v & sg & p).sum()) / n for s, sg in (("neg", a < 0), ("pos", a > 0)) for k, p in pos.items()}


def loss_reference(inp):
    """float64 restatement, torch's float32 rows, the edge band and every bar of one loss case: computed once, shared."""
    ref, t32, alt = loss_fp64(inp), loss_torch32(inp), loss_fp64(inp, mutate="flip")
    eps = float(np.float32(inp["epsilon"]))
    ref["lo"], ref["hi"] = 1.0 - eps, 1.0 + eps
    A = inp["mean"].shape[1]
    c, _ = _clean(inp)
    e_lp = U * ((A + 4) * ref["quad"] / 2 + abs(ref["const"]) + np.abs(ref["lp"]))
    if inp.get("log_std") is not None:                                   # inv_var = expf(-2 log_std): EXPF_ULPS more on every term
        e_lp = e_lp + 2 * EXPF_ULPS * U * ref["quad"] / 2
    e_x = e_lp + U * np.abs(ref["lp"] - c["logp_old"].astype(np.float64))
    delta = EDGE_FACTOR * (e_x + (2 * EXPF_ULPS + 1) * U) * SLACK
    rho = ref["rho"]
    edge = ref["valid"] & ((np.abs(rho / ref["lo"] - 1) <= delta) | (np.abs(rho / ref["hi"] - 1) <= delta))
    cmp = ref["valid"] & ~edge
    # torch's float32 rows take the float64 branch outside the band (else its error would not be a rounding error)
    lo32, hi32 = float(np.float32(1.0) - np.float32(inp["epsilon"])), float(np.float32(1.0) + np.float32(inp["epsilon"]))
    in32 = (t32["rho"] >= lo32) & (t32["rho"] <= hi32)
    below32 = t32["rho"] < lo32
    assert np.array_equal(in32[cmp], ref["inside"][cmp]) and np.array_equal(below32[cmp], (rho < ref["lo"])[cmp]), \
        "torch float32 takes another clip branch outside the edge band"
    bars = {}
    for k in ("grad_mean", "grad_value", "std_rows"):
        if ref[k] is None:
            continue
        r, t = ref[k][cmp], t32[k][cmp]
        e32 = float(np.abs(t - r).max()) if r.size else 0.0
        mag = float(np.abs(r).max()) if r.size else 0.0
        bars[k] = (BAR_FACTOR * max(e32, 2.0 ** -23 * mag), e32)
    for j, k in enumerate(("surr", "crit", "kl")):
        d, r = np.abs(t32["terms"][j] - ref["terms"][j]), np.abs(ref["terms"][j])
        bars["sum_" + k] = (BAR_FACTOR * max(float(d.sum()), 2.0 ** -23 * float(r.sum())), float(d.sum()))
        bars["term_" + k] = (BAR_FACTOR * max(float(d[cmp].max(initial=0.0)), 2.0 ** -23 * float(r[cmp].max(initial=0.0))), float(d[cmp].max(initial=0.0)))
    return dict(ref=ref, t32=t32, alt=alt, edge=edge, cmp=cmp, bars=bars)


def check_loss(got, R, tag="loss", require_cells=True):
    """got: dict(sums [4], grad_mean [M][A], grad_value [M] | None, std_rows [M][4] | None) of a kernel; R = loss_reference(inp).
    -> {quantity: err / bar}."""
    ref, edge, cmp, bars = R["ref"], R["edge"], R["cmp"], R["bars"]
    valid = ref["valid"]
    nv = int(valid.sum())
    if require_cells:
        for cell, share in clip_cells(ref).items():
            assert share >= CELL_MIN, f"{tag}: clip cell {cell} holds {share:.3%} of the valid rows: the inputs do not exercise it"
    assert int(edge.sum()) <= EDGE_CAP * nv, f"{tag}: {int(edge.sum())} of {nv} valid rows lie in the clip-edge band (cap {EDGE_CAP:.1%})"
    sums = np.asarray(got["sums"], dtype=np.float64)
    if not np.isfinite(sums).all():
        raise AssertionError(f"{tag}: a loss sum is not finite: {sums.tolist()} (a hidden row was read)")
    if sums[3] != nv:
        raise AssertionError(f"{tag}: sums[3] = {sums[3]!r}, the valid count is {nv}")
    seen = {}
    for k in ("grad_mean", "grad_value", "std_rows"):
        if ref[k] is None:
            continue
        g = np.asarray(got[k], dtype=np.float64)
        assert g.shape == ref[k].shape, (tag, k, g.shape)
        if not np.array_equal(g[~valid], np.zeros_like(g[~valid])):
            raise AssertionError(f"{tag}: {k} of a hidden row is not exactly 0")
        bar = bars[k][0]
        seen[k] = _hold(f"{tag} {k} (bar {bar:.3e}, torch float32 err {bars[k][1]:.3e})", g, ref[k], bar, where=cmp if g.ndim == 1 else cmp[:, None])
        if edge.any():
            ge, a, b = g[edge].reshape(int(edge.sum()), -1), ref[k][edge].reshape(int(edge.sum()), -1), R["alt"][k][edge].reshape(int(edge.sum()), -1)
            err = np.minimum(np.abs(ge - a).max(1), np.abs(ge - b).max(1))
            if not (err <= bar).all():
                raise AssertionError(f"{tag}: {k} of a clip-edge row equals neither branch value: |err| {err.max():.3e} bar {bar:.3e}")
    for j, k in enumerate(("sum_surr", "sum_crit", "sum_kl")):
        seen[k] = _hold(f"{tag} {k} (torch float32 err {bars[k][1]:.3e})", sums[j:j + 1], ref["sums"][j:j + 1], bars[k][0])
    return seen


def loss_row(inp, j):
    """The one-row case M = 1: row j of `inp` alone (valid), every scalar input as it is."""
    out = dict(inp)
    for k in ("mean", "act", "logp_old", "adv", "value", "ret", "logp_ref", "mask"):
        if inp.get(k) is not None:
            out[k] = np.ascontiguousarray(inp[k][j:j + 1])
    return out


def single_rows(inp):
    """The first valid row of each of the seven strata of loss_inputs(): the M = 1 cases."""
    valid = inp["mask"].astype(bool)
    return [int(np.nonzero(valid & (np.arange(valid.size) % 7 == c))[0][0]) for c in range(7)]


def check_loss_row(got, R, j, tag="loss row"):
    """A one-row launch on row j of the case behind R: one row says nothing about torch's error, so the row is held to the
    bars of the case it was taken from (torch's float32 error over all of that case's rows, this one among them) -- the gradient
    to the gradients' bar, each sum (one term) to the per-row terms' bar, sums[3] == 1."""
    ref, bars = R["ref"], R["bars"]
    sums = np.asarray(got["sums"], dtype=np.float64)
    if not np.isfinite(sums).all() or sums[3] != 1.0:
        raise AssertionError(f"{tag}: sums {sums.tolist()} of one valid row")
    seen = {}
    for k in ("grad_mean", "grad_value", "std_rows"):
        if ref[k] is None:
            continue
        g = np.asarray(got[k], dtype=np.float64).reshape(-1)
        a, b = ref[k][j].reshape(-1), R["alt"][k][j].reshape(-1)
        err = np.abs(g - a).max() if not R["edge"][j] else min(np.abs(g - a).max(), np.abs(g - b).max())
        if not err <= bars[k][0]:
            raise AssertionError(f"{tag}: {k} of row {j}: got {g.tolist()} want {a.tolist()} |err| {err:.3e} bar {bars[k][0]:.3e}")
        seen[k] = float(err / bars[k][0])
    for i, k in enumerate(("term_surr", "term_crit", "term_kl")):
        seen[k] = _hold(f"{tag} row {j} {k} (torch float32 err {bars[k][1]:.3e})", sums[i:i + 1], ref["terms"][i][j:j + 1], bars[k][0])
    return seen


# ------------------------------------------------------------------------------------------------------------------------------
# the inputs, shared by the CPU and GPU tests: same seeds, same arrays
# ------------------------------------------------------------------------------------------------------------------------------
SCAN_SHAPES = [(1, 1), (31, 65), (32, 64), (33, 63), (64, 257), (97, 300), (3, 2 ** 18 + 65)]          # (T, n)
GAMMAS = [0.5, 0.999, 1.0]
LAMS = [0.0, 0.95, 1.0]
ODD_PAIR = (0.995, 0.97)                       # rn_mul(fl32(gamma), fl32(lam)) != fl32(gamma * lam), by one ulp
GAE_PAIRS = [(g, l) for g in GAMMAS for l in LAMS] + [ODD_PAIR]
GROUP_SIZES = [1, 63, 64, 65, 255, 256, 257, 1000, 4100]
MOMENT_HORIZONS = [1, 33, 70]
LOGP_CASES = [(A, M) for A in range(1, 9) for M in (1, 255, 1000)] + [(1, 4096 * 256 + 3)]
LOSS_ROWS = [255, 10007]                     # (M = 1: single rows of the M = 255 case)
LOSS_BIG = (8, 1024 * 256 + 257)               # past one pass of the 1024 x 256 grid-stride loop


def _garbage(rng, shape):
    return (rng.choice([-1.0, 1.0], size=shape) * rng.uniform(0.1, 1.0, size=shape) * GARBAGE).astype(np.float32)


def scan_inputs(T, n):
    """-> rew, val float32 [T][n], mask uint8 [T][n], lens.  Ragged episodes with length 1 and length T present (n >= 2); beyond
    its end an odd env holds garbage rewards and values, an even env zero rewards; envs [64, 128) are short and zero-padded
    (tg_returns_moments stops its scan early in such a block)."""
    rng = np.random.default_rng(1000 * T + n % 1000)
    lens = rng.integers(1, T + 1, size=n)
    if n >= 2:
        lens[0], lens[1] = 1, T
    if n > 128 and T >= 33:
        lens[64:128] = rng.integers(1, T // 3 + 1, size=64)
    mask = (np.arange(T)[:, None] < lens[None, :]).astype(np.uint8)
    rew = (3.0 * rng.normal(size=(T, n))).astype(np.float32)
    val = (2.0 * rng.normal(size=(T, n))).astype(np.float32)
    dead = mask == 0
    odd = (np.arange(n) % 2 == 1)[None, :] & ~((np.arange(n) >= 64) & (np.arange(n) < 128))[None, :]
    rew = np.where(dead, np.where(odd, _garbage(rng, (T, n)), np.float32(0)), rew).astype(np.float32)
    val = np.where(dead, _garbage(rng, (T, n)), val).astype(np.float32)
    return rew, val, mask, lens


def moments_inputs(group_size, T, special=False):
    """-> x float32 [T][n], mask uint8 [T][n], n = 3 group_size.  Group g has scale (1e-3, 1, 30)[g] and |mean| / std about
    (0, 10, 100)[g]; an arbitrary (not prefix) mask hides ~30 %, every group keeping >= 2 valid entries where it has two;
    hidden entries hold garbage.  special: group 1 keeps exactly one valid entry, group 2 none."""
    n = 3 * group_size
    rng = np.random.default_rng(7000 + 10 * group_size + T)
    scale = np.repeat(np.array([1e-3, 1.0, 30.0]), group_size)
    ratio = np.repeat(np.array([0.0, 10.0, 100.0]), group_size)
    x = (scale[None, :] * (ratio[None, :] + rng.normal(size=(T, n)))).astype(np.float32)
    mask = (rng.uniform(size=(T, n)) < 0.7).astype(np.uint8)
    for g in range(3):
        sl = slice(g * group_size, (g + 1) * group_size)
        mask[0, sl.start] = 1
        if group_size > 1:
            mask[T - 1, sl.stop - 1] = 1
        elif T > 1:
            mask[T - 1, sl.start] = 1
    if special:
        mask[:, group_size:] = 0
        mask[T // 2, group_size + group_size // 2] = 1
    x = np.where(mask == 0, _garbage(rng, (T, n)), x).astype(np.float32)
    return x, mask


def logp_inputs(A, M):
    """-> mean, act float32 [M][A], var float32 [A] log-uniform on [1e-2, 10]."""
    rng = np.random.default_rng(300 + 17 * A + M % 1000)
    var = np.exp(rng.uniform(math.log(1e-2), math.log(10.0), size=A)).astype(np.float32)
    if A >= 2:
        var[0], var[-1] = np.float32(1e-2), np.float32(10.0)
    mean = rng.normal(size=(M, A)).astype(np.float32)
    act = (mean + 1.5 * np.sqrt(var)[None, :] * rng.normal(size=(M, A))).astype(np.float32)
    return mean, act, var


LOSS_VARIANTS = {  # name -> (PPO form (value / return, norm and coefficients as the device holds them), reference penalty, learned std)
    "grpo": (False, False, False), "ppo": (True, False, False), "grpo_ref": (False, True, False),
    "grpo_std": (False, False, True), "ppo_std": (True, False, True), "grpo_ref_std": (False, True, True),
}


LOSS_PARAMS = [(v, A) for v, (_, _, std) in LOSS_VARIANTS.items() for A in range(1, 5 if std else 9)]      # the learned std: A <= 4


def loss_inputs(variant, A, M):
    """One loss case: dict of float32 arrays as the kernel gets them.  Row i is planted in stratum i % 7: strata 0..5 are the six
    (advantage sign) x (below / inside / above) cells -- x = lp64 - logp_old uniform on that cell's part of [-1.5, 1.5], the parts
    abutting at ln(1 -+ eps), so x is piecewise uniform on the whole interval with the edges inside it -- and stratum 6 is the
    block of exactly zero advantages (x uniform on all of [-1.5, 1.5]).
    20 % of the rows are hidden (mask 0) and hold NaN in mean, act, logp_old, adv, value, ret, logp_ref.
    The M = 1 cases are single rows of the M = 255 case, one per stratum (single_rows(), loss_row())."""
    ppo, ref, std = LOSS_VARIANTS[variant]
    rng = np.random.default_rng(50000 + 1000 * sorted(LOSS_VARIANTS).index(variant) + 100 * A + M % 97)
    eps = np.float32(0.2)
    inp = dict(epsilon=eps, variant=variant)
    if std:
        inp["log_std"] = rng.uniform(-1.5, 0.5, size=A).astype(np.float32)
        sigma = np.exp(inp["log_std"].astype(np.float64))
        inp["var"] = None
    else:
        inp["var"] = rng.uniform(0.2, 0.6, size=A).astype(np.float32)
        sigma = np.sqrt(inp["var"].astype(np.float64))
    mean = rng.normal(size=(M, A)).astype(np.float32)
    act = (mean + sigma[None, :] * rng.normal(size=(M, A))).astype(np.float32)
    stratum = np.arange(M) % 7
    sign = np.where(stratum % 2 == 0, -1.0, 1.0)
    adv = np.where(stratum == 6, 0.0, sign * rng.uniform(0.2, 2.0, size=M)).astype(np.float32)
    lo_x, hi_x = math.log(1.0 - float(eps)), math.log(1.0 + float(eps))
    part = np.where(stratum == 6, 3, (stratum % 6) // 2)
    a_x = np.choose(part, [-1.5, lo_x, hi_x, -1.5])
    b_x = np.choose(part, [lo_x, hi_x, 1.5, 1.5])
    x = rng.uniform(a_x, b_x)
    inp.update(mean=mean, act=act, adv=adv)
    base = dict(inp, logp_old=np.zeros(M, dtype=np.float32), mask=np.ones(M, dtype=np.uint8), coefs=(1.0, 0.0, 0.0), norm=None)
    lp64 = loss_fp64(base)["lp"]
    inp["logp_old"] = (lp64 - x).astype(np.float32)
    mask = (rng.uniform(size=M) < 0.8).astype(np.uint8)
    nv = float(mask.sum())
    inp["mask"] = mask
    inp["value"] = inp["ret"] = inp["norm"] = inp["logp_ref"] = None
    inp["ref_coef"] = np.float32(0.0)
    if ppo:
        inp["value"] = rng.normal(size=M).astype(np.float32)
        inp["ret"] = (1.5 * rng.normal(size=M) + 0.3).astype(np.float32)
        inp["norm"] = np.array([0.1, 1.7, -0.2, 0.6], dtype=np.float32)      # |adv| >= 0.2 > 0.1: the planted signs survive
        inp["coefs"] = tuple(np.float32(v) for v in (-1.0 / nv, 0.5 / nv, 0.5 / nv))
    else:
        inp["coefs"] = (np.float32(1.0 / 3.0), np.float32(0.0), np.float32(0.0))
    if ref:
        inp["logp_ref"] = (lp64 + rng.uniform(-1.0, 1.0, size=M)).astype(np.float32)
        inp["ref_coef"] = np.float32(0.04)
    hidden = mask == 0
    for k in ("mean", "act", "logp_old", "adv", "value", "ret", "logp_ref"):
        if inp[k] is not None:
            inp[k] = inp[k].copy()
            inp[k][hidden] = np.nan
    return inp


def loss_cases(variant, A):
    """[(tag, inputs)] of one (variant, A): M = 255, M = 10007, and at A = 8 the case past one grid-stride pass.  (M = 1: rows of
    the first.)"""
    out = [(f"{variant} A={A} M={M}", loss_inputs(variant, A, M)) for M in LOSS_ROWS]
    if A == LOSS_BIG[0]:
        out.append((f"{variant} A={A} M={LOSS_BIG[1]}", loss_inputs(variant, *LOSS_BIG)))
    return out
