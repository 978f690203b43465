"""The scalar side of learn() on the GPU -- tg_rtg_scan, tg_gae_scan, tg_returns_moments, tg_ppo_returns, tg_masked_moments,
tg_group_normalize, tg_gaussian_logp, tg_surrogate_loss{,_ref,_std} -- against the float64 restatements and bounds of
tests/returns_loss_fp64.py (every bound is derived in that module's docstring; tests/test_returns_loss_fp64.py shows on the CPU
that the float32 oracle passes the same checkers on the same inputs and that wrong kernels do not).

What the shapes are for: the 32-step chunk boundary of the scans (T = 31, 32, 33, 64, 97), the 256-thread launch shape of
n > 2^18, the strided loop of group_moments_kernel (group > 256), groups that are no multiple of the wavefront and their base
g * group_size, blockIdx.y > 0 of tg_group_normalize (T > 32), every act_dim of the log-prob and loss switches, both grid-stride
loops (M > 4096 x 256 resp. 1024 x 256), strided operands, all six clip cells, and hidden rows that hold NaN.

Zero-variance groups are out of scope: the one-pass variance need not round to exactly 0 there (returns_loss_fp64's docstring).

Every test prints the largest observed error over its bound."""
import numpy as np
import pytest
import torch

import returns_loss_fp64 as F
from oracle import learner as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tg():
    import trajopt_grpo_amd as tg
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return tg


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def host(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------------------------------------------------------------------
# the scans, alone and fused
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,n", F.SCAN_SHAPES)
def test_scans_against_fp64_and_bit_for_bit_against_the_oracle(tg, dev, T, n):
    """tg_rtg_scan / tg_returns_moments / tg_ppo_returns (Monte Carlo) at every gamma, tg_gae_scan / tg_ppo_returns (GAE) at every
    (gamma, lam): inside the propagated float64 bound; reward-to-go bit for bit the oracle's; GAE bit for bit the oracle's wherever
    rn_mul(fl32(gamma), fl32(lam)) == fl32(gamma * lam), and at (0.995, 0.97), where the kernel's coefficient is one ulp off the
    reference's, bit for bit the oracle recurrence run with the kernel's coefficient and still inside the bound of the
    reference's.  The fused forms' moments (one group of n) are held to the moments bound on the kernel's own output."""
    K = tg.hip_ops
    rew, val, mask, lens = F.scan_inputs(T, n)
    d = lambda a: torch.from_numpy(a).to(dev)
    rew_d, val_d, mask_d = d(rew), d(val), d(mask)
    tr = lambda a: torch.from_numpy(np.ascontiguousarray(a.T))
    rew_o, val_o, mask_o = tr(rew), tr(val), tr(mask.astype(np.float32))
    worst = 0.0
    for gamma in F.GAMMAS + [F.ODD_PAIR[0]]:
        rtg = host(K.rtg_scan(rew_d, mask_d, gamma))
        want = L.rtg_scan(rew_o, mask_o, gamma).numpy().T
        assert np.array_equal(rtg, want), f"reward-to-go not bit-exact at gamma={gamma}"
        worst = max(worst, F.check_rtg(rtg, rew, mask, gamma, f"tg_rtg_scan gamma={gamma}"))
        rtg2, mom = K.returns_moments(rew_d, mask_d, gamma, n)
        assert np.array_equal(host(rtg2), rtg), f"tg_returns_moments' returns differ from tg_rtg_scan's at gamma={gamma}"
        worst = max(worst, F.check_moments(host(mom), rtg, mask, n, f"tg_returns_moments gamma={gamma}"))
        adv_d, ret_d = torch.empty_like(rew_d), torch.empty_like(rew_d)
        mom = host(K.ppo_returns(rew_d, val_d, mask_d, gamma, 0.95, True, adv_d, ret_d))
        adv, ret = host(adv_d), host(ret_d)
        assert np.array_equal(ret, rtg) and np.array_equal(adv, (L.rtg_scan(rew_o, mask_o, gamma) - val_o).numpy().T)
        worst = max(worst, F.check_mc_adv(adv, rew, val, mask, gamma, f"tg_ppo_returns mc gamma={gamma}"),
                    F.check_moments(mom[:1], adv, mask, n, "tg_ppo_returns mc adv moments"),
                    F.check_moments(mom[1:], ret, mask, n, "tg_ppo_returns mc ret moments"))
    for gamma, lam in F.GAE_PAIRS:
        tag = f"gamma={gamma} lam={lam}"
        a_d, r_d = K.gae_scan(rew_d, val_d, mask_d, gamma, lam)
        adv, ret = host(a_d), host(r_d)
        if F.coef_kernel(gamma, lam) == F.coef_reference(gamma, lam):
            oa, oret = L.gae_scan(rew_o, val_o, mask_o, gamma, lam)
            assert np.array_equal(adv, oa.numpy().T) and np.array_equal(ret, oret.numpy().T), f"GAE not bit-exact at {tag}"
        else:
            assert (gamma, lam) == F.ODD_PAIR
            ka, kret = F.gae_scan_f32(rew, val, mask, gamma, F.coef_kernel(gamma, lam))
            assert np.array_equal(adv, ka) and np.array_equal(ret, kret), f"GAE is not the recurrence with rn_mul(gamma, lam) at {tag}"
        worst = max(worst, F.check_gae(adv, ret, rew, val, mask, gamma, lam, f"tg_gae_scan {tag}"))
        adv_d, ret_d = torch.empty_like(rew_d), torch.empty_like(rew_d)
        mom = host(K.ppo_returns(rew_d, val_d, mask_d, gamma, lam, False, adv_d, ret_d))
        assert np.array_equal(host(adv_d), adv) and np.array_equal(host(ret_d), ret), f"tg_ppo_returns differs from tg_gae_scan at {tag}"
        worst = max(worst, F.check_moments(mom[:1], adv, mask, n, "tg_ppo_returns gae adv moments"),
                    F.check_moments(mom[1:], ret, mask, n, "tg_ppo_returns gae ret moments"))
    print(f"\n[fp64] scans T={T} n={n}: max err / bound {worst:.3f}")


# ------------------------------------------------------------------------------------------------------------------------------
# masked moments and group normalisation
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", F.MOMENT_HORIZONS)
@pytest.mark.parametrize("group_size", F.GROUP_SIZES)
def test_moments_and_normalisation_against_fp64(tg, dev, group_size, T):
    """Three groups (n = 3 group_size) of scale 1e-3 / 1 / 30 and |mean| / std ~ 0 / 10 / 100 under an arbitrary mask with garbage
    behind it: exact counts, float64 sums inside the summation bound, both normalisation modes inside their bound, hidden entries
    exactly 0.  At group_size = T = 1 every group has one entry: NaN there, as torch.std makes it."""
    K = tg.hip_ops
    x, mask = F.moments_inputs(group_size, T)
    x_d, mask_d = torch.from_numpy(x).to(dev), torch.from_numpy(mask).to(dev)
    mom_d = K.masked_moments(x_d, mask_d, group_size)
    worst = F.check_moments(host(mom_d), x, mask, group_size, "tg_masked_moments")
    for mode in (0, 1):
        out = host(K.group_normalize(x_d, mask_d, mom_d, mode, group_size))
        worst = max(worst, F.check_normalize(out, x, mask, group_size, mode, "tg_group_normalize"))
    print(f"\n[fp64] moments / normalisation group {group_size} T={T}: max err / bound {worst:.3f}")


def test_one_entry_groups_give_nan_and_empty_groups_zeros(tg, dev):
    K = tg.hip_ops
    x, mask = F.moments_inputs(65, 33, special=True)
    x_d, mask_d = torch.from_numpy(x).to(dev), torch.from_numpy(mask).to(dev)
    mom_d = K.masked_moments(x_d, mask_d, 65)
    F.check_moments(host(mom_d), x, mask, 65)
    assert host(mom_d)[:, 0].tolist()[1:] == [1.0, 0.0]
    for mode in (0, 1):
        out = host(K.group_normalize(x_d, mask_d, mom_d, mode, 65))
        F.check_normalize(out, x, mask, 65, mode)                          # (asserts the NaN and the exact zeros)
        assert np.isnan(out[:, 65:130][mask[:, 65:130] == 1]).all() and int(np.isnan(out).sum()) == 1
        assert not out[:, 130:].any()


# ------------------------------------------------------------------------------------------------------------------------------
# Gaussian log-probability
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A,M", F.LOGP_CASES)
def test_gaussian_logp_against_fp64(tg, dev, A, M):
    """Contiguous and column-major actions and a mean with a row stride of A + 3: the same bits, inside the bound."""
    K = tg.hip_ops
    mean, act, var = F.logp_inputs(A, M)
    mean_d, act_d = torch.from_numpy(mean).to(dev), torch.from_numpy(act).to(dev)
    lp = K.gaussian_logp(mean_d, act_d, var)
    act_cm = act_d.t().contiguous().t()
    wide = torch.full((M, A + 3), float("nan"), device=dev)
    wide[:, :A] = mean_d
    assert (A == 1 or M == 1 or act_cm.stride() == (1, M)) and wide[:, :A].stride(0) == A + 3
    assert torch.equal(K.gaussian_logp(mean_d, act_cm, var), lp) and torch.equal(K.gaussian_logp(wide[:, :A], act_cm, var), lp)
    r = F.check_logp(host(lp), mean, act, var, f"tg_gaussian_logp A={A} M={M}")
    print(f"\n[fp64] logp A={A} M={M}: max err / bound {r:.3f}")


# ------------------------------------------------------------------------------------------------------------------------------
# the loss head
# ------------------------------------------------------------------------------------------------------------------------------
def run_loss(K, dev, inp, strided):
    """One launch of tg_surrogate_loss / _ref / _std on `inp` (returns_loss_fp64.loss_inputs): -> the checkers' dict.
    strided: column-major actions and a mean of row stride A + 3 whose padding holds NaN."""
    d = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    M, A = inp["mean"].shape
    mean, act = d(inp["mean"]), d(inp["act"])
    if strided:
        wide = torch.full((M, A + 3), float("nan"), device=dev)
        wide[:, :A] = mean
        mean, act = wide[:, :A], act.t().contiguous().t()
    ppo = inp["value"] is not None
    coef = d(np.array(inp["coefs"], dtype=np.float32)) if ppo else None
    host_coefs = (0.0, 0.0, 0.0) if ppo else tuple(float(v) for v in inp["coefs"])
    std_out = torch.full((M, 4), float("nan"), device=dev) if inp.get("log_std") is not None else None
    _, sums, g_mean, g_val = K.surrogate_loss(mean, d(inp["value"]), act, d(inp["logp_old"]), d(inp["adv"]), d(inp["ret"]), d(inp["mask"]),
                                              d(inp["norm"]), None if inp["var"] is None else [float(v) for v in inp["var"]],
                                              float(inp["epsilon"]), *host_coefs, want_total=False, coef=coef, logp_ref=d(inp["logp_ref"]),
                                              ref_coef=float(inp["ref_coef"]), log_std=d(inp.get("log_std")), std_out=std_out)
    return dict(sums=host(sums), grad_mean=host(g_mean), grad_value=None if g_val is None else host(g_val),
                std_rows=None if std_out is None else host(std_out))


@pytest.mark.parametrize("variant,A", F.LOSS_PARAMS)
def test_loss_head_against_fp64(tg, dev, variant, A):
    """GRPO form (no value, host coefficients), PPO form (value / return, norm and coefficients read from the device), each plain,
    with the reference-policy penalty (GRPO) and with the learned std (A <= 4): M = 255 and 10007 (A = 8: also 1024 x 256 + 257),
    and M = 1 as single rows of the M = 255 case, one per stratum.  The six clip cells are populated (asserted), 20 % of the rows
    are hidden and hold NaN: exact zeros there, finite sums, sums[3] the valid count.  Gradients, std rows and sums inside 4 x torch's
    float32 error (returns_loss_fp64's docstring); rows in the clip-edge band may take either branch."""
    K = tg.hip_ops
    worst = {}
    for i, (tag, inp) in enumerate(F.loss_cases(variant, A)):
        R = F.loss_reference(inp)
        for strided in ((False, True) if i == 0 else (bool(i % 2),)):
            got = run_loss(K, dev, inp, strided)
            for k, v in F.check_loss(got, R, f"{tag} strided={strided}").items():
                worst[k] = max(worst.get(k, 0.0), v)
        if i == 0:
            for j in F.single_rows(inp):
                got = run_loss(K, dev, F.loss_row(inp, j), strided=bool(j % 2))
                for k, v in F.check_loss_row(got, R, j, f"{tag} M=1").items():
                    worst[k] = max(worst.get(k, 0.0), v)
    print(f"\n[fp64] loss {variant} A={A}: max err / bar {({k: round(v, 3) for k, v in worst.items()})}")
