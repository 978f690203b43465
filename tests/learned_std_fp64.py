"""fp64 restatement of one PPO / GRPO optimizer step with a LEARNED diagonal covariance, for tests/test_learned_std_cpu.py and
tests/test_learned_std_gpu.py.  Nothing here touches the GPU or the package under test: torch-CPU only.

Written from algorithms/ppo.py:159-183 and algorithms/grpo.py:122-145 with
    dist = MultivariateNormal(actor(s), diag(exp(2 log_std)))
in place of the fixed `self.cov`: log-probability and entropy come from torch.distributions, the gradient of log_std from torch
autograd of that very loss.  `analytic_log_std_grad` is the closed form the kernels implement,
    d loss / d log_std[k] = sum_rows dlp (dmu_k^2 exp(-2 log_std[k]) - 1) - entropy_coef,
and tests/test_learned_std_cpu.py holds it against the autograd gradient.  Every function takes a `dtype`: float64 is the
yardstick, float32 (optionally with bf16 autocast of the nets) is "torch's own autograd of the same step", whose distance from the
yardstick sets the tolerance of the native path.

Rows are in the device trajectory's order (time-major over the valid (t, env) pairs): `valid_rows` converts the reference layout."""
import math

import torch
from torch.distributions import MultivariateNormal


def mlp(sd, x, activation="ReLU", autocast=False):
    """Sequential(Linear, act, ..., Linear) from a `network.{0,2,..}.{weight,bias}` dict of leaf tensors."""
    n = len(sd) // 2
    fn = {"ReLU": torch.relu, "Tanh": torch.tanh, "Sigmoid": torch.sigmoid}[activation]
    with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
        h = x
        for i in range(n):
            h = torch.nn.functional.linear(h, sd[f"network.{2 * i}.weight"], sd[f"network.{2 * i}.bias"])
            if i < n - 1:
                h = fn(h)
    return h.to(x.dtype)


def leaves(sd, dtype):
    return {k: v.detach().cpu().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}


def valid_rows(obs, act, rew, mask, dtype):
    """Reference layout [G][E][T][..] -> time-major [T][n] tensors and the flat index of the valid rows in that order."""
    G, E, T, S = obs.shape
    n = G * E
    o = obs.reshape(n, T, S).permute(1, 0, 2).to(dtype)
    a = act.reshape(n, T, -1).permute(1, 0, 2).to(dtype)
    r = rew.reshape(n, T).t().to(dtype)
    m = mask.reshape(n, T).t().bool()
    return o, a, r, m


def rtg(r, m, gamma):
    """grpo.py:66-74 == ppo.py:100-111 on [T][n]."""
    T = r.shape[0]
    mf = m.to(r.dtype)
    out = torch.zeros_like(r)
    for t in reversed(range(T)):
        out[t] = r[t] * mf[t] + (gamma * out[t + 1] * mf[t + 1] if t < T - 1 else 0.0)
    return out


def gaussian(mean, log_std):
    return MultivariateNormal(mean, torch.diag(torch.exp(2.0 * log_std)))


def actor_loss(mean, act, log_std, old_lp, adv, *, epsilon, surr_coef, kl_coef=0.0, entropy_coef=0.0, lp_ref=None, ref_coef=0.0):
    """surr_coef sum min(rho A, clip(rho) A) + kl_coef sum exp(lp_old)(lp_old - lp) - ref_coef sum D - entropy_coef mean(H):
    PPO (ppo.py:159-179): surr_coef = -1/n, kl_coef = kl_coeff/n; GRPO (grpo.py:122-140): surr_coef = 1/G, ref_coef = beta/G."""
    dist = gaussian(mean, log_std)
    lp = dist.log_prob(act)
    rho = torch.exp(lp - old_lp)
    loss = surr_coef * torch.min(rho * adv, torch.clamp(rho, 1 - epsilon, 1 + epsilon) * adv).sum()
    if kl_coef:
        loss = loss + kl_coef * (torch.exp(old_lp) * (old_lp - lp)).sum()
    if lp_ref is not None and ref_coef:
        x = lp_ref - lp
        loss = loss - ref_coef * (torch.exp(x) - x - 1).sum()
    if entropy_coef:
        loss = loss - entropy_coef * dist.entropy().mean()
    return loss


def analytic_log_std_grad(mean, act, log_std, old_lp, adv, *, epsilon, surr_coef, kl_coef=0.0, entropy_coef=0.0, lp_ref=None, ref_coef=0.0):
    """The closed form of d actor_loss / d log_std (what the loss heads + tg_log_std_grad compute)."""
    A = act.shape[1]
    inv_var = torch.exp(-2.0 * log_std)
    dmu = act - mean
    lp = -0.5 * (dmu * dmu * inv_var).sum(1) - 0.5 * A * math.log(2 * math.pi) - log_std.sum()
    rho = torch.exp(lp - old_lp)
    lo, hi = 1 - epsilon, 1 + epsilon
    s1, s2 = rho * adv, torch.clamp(rho, lo, hi) * adv
    inside = (rho >= lo) & (rho <= hi)
    w = torch.where(inside, torch.ones_like(rho), (s1 < s2).to(rho.dtype))
    dlp = surr_coef * adv * rho * w
    if kl_coef:
        dlp = dlp - kl_coef * torch.exp(old_lp)
    if lp_ref is not None and ref_coef:
        dlp = dlp + ref_coef * (torch.exp(lp_ref - lp) - 1)
    return (dlp[:, None] * (dmu * dmu * inv_var - 1)).sum(0) - entropy_coef


def _adam(params, lr):
    return torch.optim.Adam(params, lr=lr)


def ppo_steps(actor_sd, critic_sd, log_std, obs, act, rew, mask, *, activation="ReLU", epsilon=0.2, gamma=0.99, c1=0.5, kl_coeff=0.5,
              entropy=0.01, lr=3e-4, updates=1, batches=None, max_grad_norm=None, dtype=torch.float64, autocast=False):
    """PPO.learn (ppo.py:64-186, Monte-Carlo returns) on a trajectory in the reference layout.  batches: per optimizer step an index
    vector into the valid rows (device order), or None = full batch, `updates` steps.  Returns log_std's gradient and value after
    every step, the pre-clip gradient norms and the final net parameters."""
    a_sd, c_sd = leaves(actor_sd, dtype), leaves(critic_sd, dtype)
    ls = log_std.detach().cpu().to(dtype).clone().requires_grad_(True)
    o, a, r, m = valid_rows(obs, act, rew, mask, dtype)
    with torch.no_grad():
        V = mlp(c_sd, o, activation, autocast).squeeze(-1) * m
        R = rtg(r, m, gamma)
        adv, ret = (R - V)[m], R[m]
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
        ret = (ret - ret.mean()) / (ret.std() + 1e-8)
        O, Aa = o[m], a[m]
        old_lp = gaussian(mlp(a_sd, O, activation, autocast), ls).log_prob(Aa)
    params = list(a_sd.values()) + list(c_sd.values()) + [ls]
    opt = _adam(params, lr)
    steps = batches if batches is not None else [None] * updates
    out = {"grad": [], "log_std": [], "norm": [], "entropy": []}
    for b in steps:
        sl = slice(None) if b is None else b
        n = O[sl].shape[0]
        out["entropy"].append(float(gaussian(torch.zeros(1, ls.numel(), dtype=dtype), ls.detach()).entropy()))
        loss = actor_loss(mlp(a_sd, O[sl], activation, autocast), Aa[sl], ls, old_lp[sl], adv[sl], epsilon=epsilon, surr_coef=-1.0 / n,
                          kl_coef=kl_coeff / n, entropy_coef=entropy)
        loss = loss + c1 * torch.nn.functional.mse_loss(mlp(c_sd, O[sl], activation, autocast).squeeze(-1), ret[sl])
        opt.zero_grad()
        loss.backward()
        out["norm"].append(float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in params))))
        out["grad"].append(ls.grad.detach().clone())             # (pre-clip)
        if max_grad_norm is not None:
            torch.nn.utils.clip_grad_norm_(params, max_grad_norm)
        opt.step()
        out["log_std"].append(ls.detach().clone())
    out["params"] = [p.detach() for p in params[:-1]]
    return out


def grpo_steps(actor_sd, log_std, obs, act, rew, mask, *, activation="ReLU", epsilon=0.2, gamma=0.99, beta=0.0, ref_sd=None, ref_var=None,
               ref_activation="ReLU", lr=3e-4, updates=1, dtype=torch.float64, autocast=False):
    """GRPO.learn (grpo.py:50-148; descent on J as written; the old policy is the current one at entry).  ref_sd / ref_var: the frozen
    reference policy's actor and diag(cov), with beta != 0: J = (sum min(..) - beta sum D) / G, D = exp(x) - x - 1, x = lp_ref - lp."""
    a_sd = leaves(actor_sd, dtype)
    ls = log_std.detach().cpu().to(dtype).clone().requires_grad_(True)
    G, E = obs.shape[0], obs.shape[1]
    o, a, r, m = valid_rows(obs, act, rew, mask, dtype)
    with torch.no_grad():
        R = rtg(r, m, gamma)
        adv = torch.zeros_like(R)
        for g in range(G):
            cols = slice(g * E, (g + 1) * E)
            v = R[:, cols][m[:, cols]]
            adv[:, cols] = (R[:, cols] - v.mean()) / torch.std(v + 1e-8)
        O, Aa, adv = o[m], a[m], adv[m]
        old_lp = gaussian(mlp(a_sd, O, activation, autocast), ls).log_prob(Aa)
        lp_ref = None
        if ref_sd is not None and beta:
            rs = {k: v.detach().cpu().to(dtype) for k, v in ref_sd.items()}
            lp_ref = MultivariateNormal(mlp(rs, O, ref_activation, autocast), torch.diag(torch.as_tensor(ref_var).to(dtype))).log_prob(Aa)
    params = list(a_sd.values()) + [ls]
    opt = _adam(params, lr)
    out = {"grad": [], "log_std": []}
    for _ in range(updates):
        J = actor_loss(mlp(a_sd, O, activation, autocast), Aa, ls, old_lp, adv, epsilon=epsilon, surr_coef=1.0 / G, lp_ref=lp_ref,
                       ref_coef=beta / G)
        opt.zero_grad()
        J.backward()
        out["grad"].append(ls.grad.detach().clone())
        opt.step()
        out["log_std"].append(ls.detach().clone())
    out["params"] = [p.detach() for p in params[:-1]]
    return out


def bar(ref64, torch32):
    """The native path's allowance: 4x the distance of torch's own float32 autograd from the fp64 yardstick (a different summation
    order over the rows), and never below 4 roundings of the result to float32 (the distance can be exactly zero)."""
    ref64 = torch.as_tensor(ref64, dtype=torch.float64)
    err = float((torch.as_tensor(torch32).double() - ref64).abs().max())
    return 4.0 * max(err, 2.0 ** -23 * float(ref64.abs().max())), err
