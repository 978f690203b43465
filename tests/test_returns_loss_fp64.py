"""tests/returns_loss_fp64.py validated without a GPU:
  1. the float64 restatements reproduce the record (tests/golden/rtg_adv.npz, policy_actor*.npz) and, for the loss head, float64
     torch autograd of oracle.learner.grpo_objective / ppo_loss's formulae;
  2. the float32 oracle alone (oracle.learner.rtg_scan / gae_scan, torch float32 for the rest) stays inside every bound on the
     very inputs tests/test_returns_loss_fp64_gpu.py feeds the kernels, and the clip-edge exclusion stays under its cap;
  3. every listed mutation of the oracle's output -- a plausible wrong kernel -- is rejected by its checker."""
import math

import numpy as np
import pytest
import torch

import returns_loss_fp64 as F
from conftest import load_golden
from oracle import learner as L


def tn(a):
    """[G][E][T] of the goldens -> the kernels' [T][n]."""
    return np.ascontiguousarray(a.reshape(-1, a.shape[-1]).T)


def oracle_rtg(rew, mask, gamma):
    return L.rtg_scan(torch.from_numpy(rew.T.copy()), torch.from_numpy(mask.T.astype(np.float32)), gamma).numpy().T


def oracle_gae(rew, val, mask, gamma, lam):
    a, r = L.gae_scan(torch.from_numpy(rew.T.copy()), torch.from_numpy(val.T.copy()), torch.from_numpy(mask.T.astype(np.float32)), gamma, lam)
    return a.numpy().T, r.numpy().T


# ------------------------------------------------------------------------------------------------------------------------------
# 1. the restatements against the record
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gamma", [0.5, 0.99, 0.999])
def test_scans_and_normalisation_reproduce_the_recorded_reference(gamma):
    """The goldens are the reference's own float32 results: the same operations as the kernels, so the kernels' bound holds them.
    The recorded normalised advantages come from torch's all-float32 mean / std: N-term float32 sums add N u (|mean| / den + |out|)
    (recursive-summation bound) to the kernel's bound, whose moments are float64."""
    g = load_golden("rtg_adv.npz")
    tag = f"g{gamma}"
    rew, mask = tn(g["rew"]), tn(g["mask"]).astype(np.uint8)
    val = tn(g[f"{tag}_values"])
    F.check_rtg(tn(g[f"{tag}_rtg"]), rew, mask, gamma)
    F.check_rtg(tn(g[f"{tag}_ppo_mc_group_rtgs"]), rew, mask, gamma)
    F.check_mc_adv(tn(g[f"{tag}_ppo_mc_group_adv"]), rew, val, mask, gamma)
    F.check_gae(tn(g[f"{tag}_ppo_gae_group_adv"]), tn(g[f"{tag}_ppo_gae_group_rtgs"]), rew, val, mask, gamma, 0.95)
    w = mask.astype(bool)

    def held(rec, x, group_size, mode, cols):
        truth, bound, cnt, _ = F.normalize_fp64(x, mask, group_size, mode)
        t, b, c = truth[:, cols].T[w[:, cols].T], bound[:, cols].T[w[:, cols].T], cnt[:, cols].T[w[:, cols].T]
        xs = x[:, cols].T[w[:, cols].T].astype(np.float64)
        den = np.median(np.abs(xs - xs.mean())[t != 0] / np.abs(t[t != 0]))
        extra = c * F.U * (np.abs(xs).mean() / den + np.abs(t))
        assert (np.abs(rec.astype(np.float64) - t) <= b + extra).all(), float((np.abs(rec - t) / (b + extra)).max())

    rtg = tn(g[f"{tag}_rtg"])
    for i in range(3):                                                    # GRPO: per group of 4 envs, mode 0
        held(g[f"{tag}_grpo_adv_{i}"], rtg, 4, 0, slice(4 * i, 4 * i + 4))
    for kind in ("mc", "gae"):                                            # PPO: the whole batch, mode 1
        held(g[f"{tag}_ppo_{kind}_adv"], tn(g[f"{tag}_ppo_{kind}_group_adv"]), 12, 1, slice(0, 12))
        held(g[f"{tag}_ppo_{kind}_ret"], tn(g[f"{tag}_ppo_{kind}_group_rtgs"]), 12, 1, slice(0, 12))


@pytest.mark.parametrize("kind", ["actor", "actorcritic"])
def test_logp_reproduces_the_recorded_reference(kind):
    """logp_eval is MultivariateNormal.log_prob's float32 result: a triangular solve, a squared norm and a half log-determinant,
    each term rounded as often as the kernel's (the solve's division for the kernel's two multiplications) -- the kernel's bound
    holds it."""
    g = load_golden(f"policy_{kind}.npz")
    r = F.check_logp(g["logp_eval"], g["mean"], g["action"], g["cov"])
    print(f"\n[fp64] recorded logp_eval ({kind}): max err / bound {r:.3f}")


def _torch64_loss(inp):
    """float64 torch autograd of the reference's formulae (oracle.learner.grpo_objective :296-301, ppo_loss :323-329; sums with the
    kernel's coefficients instead of means) on the valid rows."""
    c, valid = F._clean(inp)
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))
    sel = torch.from_numpy(valid)
    mean = t(c["mean"]).requires_grad_(True)
    act, lpo, adv = t(c["act"]), t(c["logp_old"]), t(c["adv"])
    ls = None
    if c.get("log_std") is not None:
        ls = t(c["log_std"]).requires_grad_(True)
        lp = (-0.5 * ((act - mean) ** 2 * torch.exp(-2 * ls)).sum(1) - 0.5 * mean.shape[1] * math.log(2 * math.pi) - ls.sum())
    else:
        lp = L.gaussian_log_prob(mean, act, t(c["var"]))
    sc, cc, kc = (float(v) for v in c["coefs"])
    eps = float(c["epsilon"])
    if c.get("norm") is not None:
        am, ai, rm, ri = (float(v) for v in c["norm"])
        adv = (adv - am) * ai
    ratio = torch.exp(lp - lpo)
    surr = torch.min(ratio * adv, torch.clamp(ratio, 1 - eps, 1 + eps) * adv)[sel].sum()
    total, crit, kl = sc * surr, torch.zeros(()), torch.zeros(())
    value = None
    if c.get("value") is not None:
        value = t(c["value"]).requires_grad_(True)
        crit = ((value - (t(c["ret"]) - rm) * ri) ** 2)[sel].sum()
        total = total + cc * crit
    if kc != 0.0:
        kl = (torch.exp(lpo) * (lpo - lp))[sel].sum()
        total = total + kc * kl
    if c.get("logp_ref") is not None:
        x = t(c["logp_ref"]) - lp
        kl = (torch.exp(x) - x - 1)[sel].sum()
        total = total - float(c["ref_coef"]) * kl
    total.backward()
    return dict(sums=[float(surr.detach()), float(crit.detach()), float(kl.detach()), float(valid.sum())], grad_mean=mean.grad.numpy(),
                grad_value=None if value is None else value.grad.numpy(), grad_log_std=None if ls is None else ls.grad.numpy())


@pytest.mark.parametrize("variant", list(F.LOSS_VARIANTS))
def test_loss_restatement_is_float64_autograd_of_the_reference_formulae(variant):
    """The closed form against autograd, both float64: 1e-12 relative (a few hundred float64 roundings over 255 rows)."""
    A = 3
    inp = F.loss_inputs(variant, A, 255)
    ref, want = F.loss_fp64(inp), _torch64_loss(inp)
    tol = lambda a: 1e-12 * max(1.0, float(np.abs(a).max()))
    assert np.abs(ref["sums"] - np.array(want["sums"])).max() <= 1e-12 * max(1.0, np.abs(want["sums"]).max())
    assert np.abs(ref["grad_mean"] - want["grad_mean"]).max() <= tol(want["grad_mean"])
    assert np.abs(ref["grad_mean"]).max() > 0 and not ref["grad_mean"][~ref["valid"]].any()
    if want["grad_value"] is not None:
        assert np.abs(ref["grad_value"] - want["grad_value"]).max() <= tol(want["grad_value"])
    if want["grad_log_std"] is not None:
        assert np.abs(ref["std_rows"][:, :A].sum(0) - want["grad_log_std"]).max() <= tol(want["grad_log_std"]) * 255
        assert not ref["std_rows"][:, A:].any()


# ------------------------------------------------------------------------------------------------------------------------------
# 2. the float32 oracle alone stays inside every bound, on the GPU tests' inputs
# ------------------------------------------------------------------------------------------------------------------------------
def test_gae_coefficients_differ_at_the_odd_pair_only():
    for g, l in F.GAE_PAIRS:
        same = F.coef_kernel(g, l) == F.coef_reference(g, l)
        assert same == ((g, l) != F.ODD_PAIR), (g, l)
    ck, cr = F.coef_kernel(*F.ODD_PAIR), F.coef_reference(*F.ODD_PAIR)
    assert abs(float(ck) - float(cr)) == float(np.spacing(min(ck, cr)))            # one float32 ulp: 0.96515006 against 0.96515


@pytest.mark.parametrize("T,n", F.SCAN_SHAPES)
def test_oracle_scans_stay_inside_the_propagated_bounds(T, n):
    rew, val, mask, lens = F.scan_inputs(T, n)
    assert lens.min() >= 1 and lens.max() <= T and (n < 2 or (lens[0] == 1 and lens[1] == T))
    worst = 0.0
    for gamma in F.GAMMAS + [F.ODD_PAIR[0]]:
        rtg = oracle_rtg(rew, mask, gamma)
        assert np.array_equal(rtg, F.rtg_scan_f32(rew, mask, gamma))
        worst = max(worst, F.check_rtg(rtg, rew, mask, gamma), F.check_mc_adv(rtg - val, rew, val, mask, gamma))
    for gamma, lam in F.GAE_PAIRS:
        adv, ret = oracle_gae(rew, val, mask, gamma, lam)
        emu = F.gae_scan_f32(rew, val, mask, gamma, F.coef_reference(gamma, lam))
        assert np.array_equal(adv, emu[0]) and np.array_equal(ret, emu[1]), (gamma, lam)
        worst = max(worst, F.check_gae(adv, ret, rew, val, mask, gamma, lam))
        if (gamma, lam) == F.ODD_PAIR:                         # the kernel's coefficient: other bits, same bound
            k_adv, k_ret = F.gae_scan_f32(rew, val, mask, gamma, F.coef_kernel(gamma, lam))
            assert T < 3 or n < 3 or not np.array_equal(k_adv, adv)
            worst = max(worst, F.check_gae(k_adv, k_ret, rew, val, mask, gamma, lam))
    print(f"\n[fp64] oracle scans T={T} n={n}: max err / bound {worst:.3f}")
    assert n == 1 or worst > 0.01, "a bound a hundred times the oracle's own error would check little"


@pytest.mark.parametrize("T", F.MOMENT_HORIZONS)
@pytest.mark.parametrize("group_size", F.GROUP_SIZES)
def test_oracle_moments_and_normalisation_stay_inside_the_bounds(group_size, T):
    x, mask = F.moments_inputs(group_size, T)
    r = F.check_moments(F.moments_plain(x, mask, group_size), x, mask, group_size)
    for mode in (0, 1):
        r = max(r, F.check_normalize(F.normalize_oracle32(x, mask, group_size, mode), x, mask, group_size, mode))
    print(f"\n[fp64] oracle moments / normalisation group {group_size} T={T}: max err / bound {r:.3f}")


def test_oracle_one_entry_and_empty_groups():
    x, mask = F.moments_inputs(65, 33, special=True)
    cnt = F.moments_fp64(x, mask, 65)[0]
    assert cnt[1] == 1 and cnt[2] == 0 and cnt[0] >= 2
    for mode in (0, 1):
        out = F.normalize_oracle32(x, mask, 65, mode)
        F.check_normalize(out, x, mask, 65, mode)
        assert np.isnan(out[:, 65:130][mask[:, 65:130] == 1]).all() and not out[:, 130:].any()
        with pytest.raises(AssertionError, match="NaN"):
            F.check_normalize(np.where(np.isnan(out), np.float32(0), out), x, mask, 65, mode)


@pytest.mark.parametrize("A,M", F.LOGP_CASES)
def test_oracle_logp_stays_inside_the_bound(A, M):
    """torch's float32 row rounds more often than the kernel's: its constant is two float32 subtractions of float32 terms (u |lp|,
    u A log(2 pi) / 2) from float32 logarithms (2 u sum |log var_k|: one ulp each, then their sum) -- that much is allowed on top."""
    mean, act, var = F.logp_inputs(A, M)
    assert var.min() >= 1e-2 * (1 - 1e-6) and var.max() <= 10 * (1 + 1e-6) and (A < 2 or var.max() / var.min() > 900)
    extra = F.U * (np.abs(F.logp_fp64(mean, act, var)[0]) + 0.5 * A * F.LOG_2PI + 2 * np.abs(np.log(var.astype(np.float64))).sum())
    r = F.check_logp(F.logp_oracle32(mean, act, var), mean, act, var, extra=extra)
    print(f"\n[fp64] oracle logp A={A} M={M}: max err / bound {r:.3f}")


_REFS = {}


def reference(tag, inp):
    if tag not in _REFS:
        _REFS[tag] = F.loss_reference(inp)
    return _REFS[tag]


@pytest.mark.parametrize("variant,A", F.LOSS_PARAMS)
def test_oracle_loss_stays_inside_the_bar_and_the_edge_cap(variant, A):
    """torch's float32 rows are inside 4 x their own error by construction; the numpy float32 evaluation of the closed form in the
    kernel's operation order (different roundings from torch's) must be inside too.  The six clip cells are populated and the edge
    band holds < 0.1 % of the rows on the reference alone."""
    worst, edges, rows = {}, 0, 0
    for tag, inp in F.loss_cases(variant, A):
        R = reference(tag, inp)
        edges, rows = edges + int(R["edge"].sum()), rows + int(R["ref"]["valid"].sum())
        for got in (R["t32"], F.loss_fp64(inp, dtype=np.float32)):
            for k, v in F.check_loss(got, R, tag).items():
                worst[k] = max(worst.get(k, 0.0), v)
        if inp["mean"].shape[0] == 255:                                   # the M = 1 cases: one row of each stratum
            rows1 = F.single_rows(inp)
            assert len(rows1) == 7 and sorted(j % 7 for j in rows1) == list(range(7))
            for j in rows1:
                for k, v in F.check_loss_row(F.loss_fp64(F.loss_row(inp, j), dtype=np.float32), R, j, tag).items():
                    worst[k] = max(worst.get(k, 0.0), v)
    print(f"\n[fp64] oracle loss {variant} A={A}: err / bar {({k: round(v, 3) for k, v in worst.items()})}; {edges} of {rows} rows in the edge band")
    assert edges <= F.EDGE_CAP * rows


# ------------------------------------------------------------------------------------------------------------------------------
# 3. wrong kernels are rejected
# ------------------------------------------------------------------------------------------------------------------------------
def test_a_scan_that_loses_its_carry_at_a_chunk_boundary_is_rejected():
    rew, val, mask, _ = F.scan_inputs(97, 300)
    gamma, lam = 0.999, 0.95

    def chunked(fn):
        """fn run on 32-step chunks cut from the end, each chunk starting from a zero carry: [T - 32, T), [T - 64, T - 32), ..."""
        outs, T = [], rew.shape[0]
        for hi in range(T, 0, -32):
            lo = max(hi - 32, 0)
            outs.insert(0, fn(slice(lo, hi)))
        return outs

    rtg = np.concatenate(chunked(lambda s: F.rtg_scan_f32(rew[s], mask[s], gamma)))
    with pytest.raises(AssertionError, match="out of bound"):
        F.check_rtg(rtg, rew, mask, gamma)
    # GAE: the carry of A zeroed where t + 1 is a chunk's first step (V_{t+1} m_{t+1} kept: only next_a_m is lost)
    A, _ = F.gae_scan_f32(rew, val, mask, gamma, F.coef_reference(gamma, lam))
    T = rew.shape[0]
    bad = A.copy()
    c, g = F.coef_reference(gamma, lam), np.float32(gamma)
    for t in range(T - 2, -1, -1):
        nam = np.float32(0) if (T - 1 - t) % 32 == 0 else (c * bad[t + 1]) * mask[t + 1].astype(np.float32)
        bad[t] = ((rew[t] + g * (val[t + 1] * mask[t + 1].astype(np.float32))) - val[t]) + nam
    assert not np.array_equal(bad, A)
    with pytest.raises(AssertionError, match="out of bound"):
        F.check_gae(bad, val + bad, rew, val, mask, gamma, lam)
    F.check_gae(A, val + A, rew, val, mask, gamma, lam)


def test_a_gae_delta_from_the_masked_reward_and_a_return_without_the_value_are_rejected():
    """r_t m_t differs from r_t only where m_t = 0, and A_t there reaches no valid step (the carry is cut by the same m_t): the
    two deltas can be told apart only beyond an episode's end, where the inputs hold garbage rewards and check_gae() looks too."""
    rew, val, mask, lens = F.scan_inputs(33, 63)
    gamma, lam = 0.999, 0.95
    A, ret, _, _ = F.gae_fp64(rew, val, mask, gamma, lam, masked_reward=True)
    w = mask.astype(bool)
    assert np.array_equal(A[w], F.gae_fp64(rew, val, mask, gamma, lam)[0][w])
    with pytest.raises(AssertionError, match="adv.*out of bound"):
        F.check_gae(A.astype(np.float32), ret.astype(np.float32), rew, val, mask, gamma, lam)
    good = F.gae_scan_f32(rew, val, mask, gamma, F.coef_reference(gamma, lam))
    F.check_gae(good[0], good[1], rew, val, mask, gamma, lam)
    with pytest.raises(AssertionError, match="ret.*out of bound"):
        F.check_gae(good[0], good[0], rew, val, mask, gamma, lam)                                   # ret without + V


@pytest.mark.parametrize("group_size", [257, 1000])
def test_moments_from_a_wrong_base_or_without_the_strided_tail_are_rejected(group_size):
    x, mask = F.moments_inputs(group_size, 33)
    F.check_moments(F.moments_plain(x, mask, group_size), x, mask, group_size)
    with pytest.raises(AssertionError):
        F.check_moments(F.moments_plain(x, mask, group_size, base_stride=256), x, mask, group_size)
    with pytest.raises(AssertionError):
        F.check_moments(F.moments_plain(x, mask, group_size, max_e=256), x, mask, group_size)


@pytest.mark.parametrize("group_size,T", [(g, T) for g in F.GROUP_SIZES for T in F.MOMENT_HORIZONS if g * T >= 2])
def test_a_biased_variance_and_a_missing_epsilon_are_rejected(group_size, T):
    x, mask = F.moments_inputs(group_size, T)
    for mode in (0, 1):
        with pytest.raises(AssertionError, match="out of bound"):
            F.check_normalize(F.normalize_oracle32(x, mask, group_size, mode, biased=True), x, mask, group_size, mode)
    with pytest.raises(AssertionError, match="out of bound"):
        F.check_normalize(F.normalize_oracle32(x, mask, group_size, 1, no_eps=True), x, mask, group_size, 1)


def test_a_logp_that_drops_an_action_column_is_rejected():
    for M in (1, 255, 1000):
        mean, act, var = F.logp_inputs(5, M)
        for k in range(5):
            with pytest.raises(AssertionError, match="out of bound"):
                F.check_logp(F.logp_oracle32(mean, act, var, drop_column=k), mean, act, var)


@pytest.mark.parametrize("variant", list(F.LOSS_VARIANTS))
def test_wrong_clip_branches_and_a_leaking_mask_are_rejected(variant):
    A, M = 3, 255
    inp = F.loss_inputs(variant, A, M)
    R = reference(f"{variant} A={A} M={M}", inp)
    F.check_loss(F.loss_fp64(inp, dtype=np.float32), R)
    for mutate in ("keep_neg_below", "drop_neg_above"):
        with pytest.raises(AssertionError, match="grad_mean"):
            F.check_loss(F.loss_fp64(inp, dtype=np.float32, mutate=mutate), R)
    # a hidden row that is read: NaN into the sums ...
    leak = F.loss_fp64(inp, dtype=np.float32)
    leak["sums"] = leak["sums"] + np.array([np.nan, 0, 0, 0])
    with pytest.raises(AssertionError, match="not finite"):
        F.check_loss(leak, R)
    # ... and, had the hidden rows held ordinary numbers, a wrong count, wrong sums and non-zero gradients
    finite = F.loss_inputs(variant, A, M)
    for i, k in enumerate(("mean", "act", "logp_old", "adv", "value", "ret", "logp_ref")):
        if finite[k] is not None:
            finite[k] = np.where(np.isnan(finite[k]), np.float32(0.37 + 0.2 * i), finite[k]).astype(np.float32)
    leak = F.loss_fp64(finite, dtype=np.float32, mutate="ignore_mask")
    with pytest.raises(AssertionError, match="valid count"):
        F.check_loss(leak, R)
    leak["sums"][3] = R["ref"]["sums"][3]
    with pytest.raises(AssertionError, match="hidden row"):
        F.check_loss(leak, R)
    for k in ("grad_mean", "grad_value", "std_rows"):
        if leak[k] is not None:
            leak[k][~R["ref"]["valid"]] = 0
    with pytest.raises(AssertionError, match="sum_"):
        F.check_loss(leak, R)
