"""GRPO's KL penalty to a frozen reference policy (GRPO(ref_model=..., beta=...); DeepSeekMath's GRPO as algorithms/grpo.py:127-134
means it) through every layer: the `_ref` entry points of the C ABI (argument checks on the CPU), the five training heads against
torch fp64 autograd of the penalised loss, and GRPO.learn() against an fp64 restatement of the whole iteration (masked rows, Adam).

Per valid row: x = log pi_ref(a|s) - log pi(a|s), D = exp(x) - x - 1, J = (sum min(rho A, clip(rho) A) - beta sum D) / G."""
import copy
import ctypes as C
import math

import pytest
import torch

import trajopt_grpo_amd as tg

N = tg._native
REF_ENTRIES = ["tg_surrogate_loss_ref", "tg_mlp_forward_chain_loss_ref", "tg_mlp_f32_forward_backward_ref",
               "tg_mlp_f32w_forward_backward_ref", "tg_mlp_f32r_forward_backward_ref"]


# ---------------------------------------------------------------------------------------------------------------------------
# CPU: the C ABI
# ---------------------------------------------------------------------------------------------------------------------------
def test_ref_entry_points_are_exported_and_the_abi_is_13():
    lib = N.load()
    for name in REF_ENTRIES:
        assert name in N.SIGNATURES and hasattr(lib, name), name
    assert lib.tg_abi_version() == N.ABI_VERSION == 13


def test_ref_penalty_struct_layout():
    assert C.sizeof(N.RefPenalty) == 16
    assert (N.RefPenalty.d_logp_ref.offset, N.RefPenalty.coef.offset, N.RefPenalty.reserved.offset) == (0, 8, 12)


def _call(name, loss, ref):
    """One `_ref` call whose arguments are refused before anything is launched (the pointers are never dereferenced)."""
    lib, fake = N.load(), 256
    arr = (C.c_void_p * 8)(*([fake] * 8))
    if name == "tg_surrogate_loss_ref":
        return lib.tg_surrogate_loss_ref(C.byref(loss), C.byref(ref), None)
    if name == "tg_mlp_forward_chain_loss_ref":
        return lib.tg_mlp_forward_chain_loss_ref(fake, fake, fake, 128, 3, 100, arr, arr, C.byref(loss), C.byref(ref), None)
    if name == "tg_mlp_f32_forward_backward_ref":
        return lib.tg_mlp_f32_forward_backward_ref(fake, 8, fake, 128, 3, 100, arr, arr, None, C.byref(loss), C.byref(ref), None)
    if name == "tg_mlp_f32w_forward_backward_ref":
        return lib.tg_mlp_f32w_forward_backward_ref(fake, 8, fake, fake, 3, 100, arr, arr, C.byref(loss), C.byref(ref), None)
    return lib.tg_mlp_f32r_forward_backward_ref(fake, 8, fake, fake, fake, 128, 2, 100, arr, arr, None, C.byref(loss), C.byref(ref), None)


@pytest.mark.parametrize("name", REF_ENTRIES)
def test_ref_entry_points_refuse_a_critic_a_missing_reference_and_a_kl_coef(name):
    lib = N.load()
    if name == "tg_surrogate_loss_ref":
        critic, actor = N.LossArgs(), N.LossArgs()
        critic.d_value = 256                                       # (a value head: PPO's critic term)
    else:
        critic, actor = N.ChainLoss(), N.ChainLoss()
        critic.kind = 1
    ref = N.RefPenalty()
    ref.d_logp_ref, ref.coef = 256, 0.5
    assert _call(name, critic, ref) != 0 and b"actor term" in lib.tg_last_error()
    missing = N.RefPenalty()
    missing.coef = 0.5
    assert _call(name, actor, missing) != 0 and b"d_logp_ref is null" in lib.tg_last_error()
    actor.kl_coef = 0.1
    assert _call(name, actor, ref) != 0 and b"kl_coef" in lib.tg_last_error()


def test_grpo_checks_its_reference_policy():
    pol = tg.GaussianActor_NeuralNetwork(5, 1, (16,), cov=0.5, device="cpu")
    opt = torch.optim.Adam(pol.parameters(), lr=1e-3)
    with pytest.raises(ValueError, match="GaussianActor"):
        tg.GRPO(0.2, 0.5, 0.9, pol, opt, ref_model=pol.actor)
    with pytest.raises(ValueError, match="widths"):
        tg.GRPO(0.2, 0.5, 0.9, pol, opt, ref_model=tg.GaussianActor_NeuralNetwork(4, 1, (16,), device="cpu"))
    with pytest.raises(ValueError, match="widths"):
        tg.GRPO(0.2, 0.5, 0.9, pol, opt, ref_model=tg.GaussianActor_NeuralNetwork(5, 2, (16,), device="cpu"))
    ok = tg.GRPO(0.2, 0.5, 0.9, pol, opt, ref_model=tg.GaussianActorCritic_NeuralNetwork(5, 1, (32, 32), device="cpu"))
    assert ok.ref_model is not None and ok.metadata()["beta"] == 0.5


# ---------------------------------------------------------------------------------------------------------------------------
# GPU: the five heads against torch fp64 autograd
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda", 0)


def _fp64_loss(net, X, masks, act, lpo, adv, lref, var, eps, sc, rc):
    """The penalised clipped surrogate in fp64 through torch autograd, with the kernel's own ReLU masks (a pre-activation within
    fp32 rounding of zero may fall on the other side in fp64): sums {0: surrogate, 2: D, 3: count}, d loss / d output, grads."""
    lin = [m for m in net.network if isinstance(m, torch.nn.Linear)]
    params = []
    for l in lin:
        params += [l.weight.detach().double().requires_grad_(), l.bias.detach().double().requires_grad_()]
    h = X.double()
    for i in range(len(lin) - 1):
        h = (h @ params[2 * i].t() + params[2 * i + 1]) * masks[i]
    out = h @ params[-2].t() + params[-1]
    out.retain_grad()
    A = out.shape[1]
    v = var.double().to(out.device)
    logp = -0.5 * (((act.double() - out) ** 2) / v).sum(1) - 0.5 * A * math.log(2 * math.pi) - 0.5 * float(torch.log(v).sum())
    rho = torch.exp(logp - lpo.double())
    surr = torch.minimum(rho * adv.double(), torch.clamp(rho, 1 - eps, 1 + eps) * adv.double())
    x = lref.double() - logp
    D = torch.exp(x) - x - 1
    (sc * surr.sum() - rc * D.sum()).backward()
    return {0: float(surr.sum()), 2: float(D.sum()), 3: float(X.shape[0])}, out.grad, [p.grad for p in params]


def _head_inputs(net, X, A, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    rows = X.shape[0]
    act = torch.randn(rows, A, device=dev, generator=g)
    lpo = (-0.5 * torch.rand(rows, device=dev, generator=g) - 1.0).contiguous()
    adv = torch.randn(rows, device=dev, generator=g)
    var = torch.full((A,), 0.3)
    with torch.no_grad():                                          # |lp_ref - lp| up to 3: exp on both sides of 1
        mean = copy.deepcopy(net).double()(X.double())
        lp = -0.5 * (((act.double() - mean) ** 2) / 0.3).sum(1) - 0.5 * A * math.log(2 * math.pi * 0.3)
    lref = (lp + 6.0 * torch.rand(rows, device=dev, dtype=torch.float64, generator=g) - 3.0).float().contiguous()
    return act, lpo, adv, var, lref


F32_HEADS = {"resident": (5, 1, (128, 128)), "chain64": (5, 1, (64, 64, 64)), "chain128": (20, 4, (128,) * 4),
             "wide": (20, 4, (256,) * 5), "library": (6, 2, (96, 96))}


@pytest.mark.gpu
@pytest.mark.parametrize("head", list(F32_HEADS))
@pytest.mark.parametrize("rows", [1, 255, 70001])
def test_f32_heads_with_the_reference_penalty_match_fp64(dev, head, rows):
    """tg_mlp_f32{r,,w}_forward_backward_ref and (a shape outside the chain gates) tg_surrogate_loss_ref: loss sums incl. the KL slot,
    d loss / d output and every parameter gradient against fp64 at test_f32_chain_update_matches_fp64_autograd's bounds;
    bit-identical run to run."""
    from trajopt_grpo_amd import mlp as M, hip_ops as K
    S, A, hidden = F32_HEADS[head]
    torch.manual_seed(rows + S)
    net = tg.NeuralNetwork(S, A, hidden, "ReLU").to(dev)
    X = torch.randn(rows, S, device=dev)
    act, lpo, adv, var, lref = _head_inputs(net, X, A, dev, rows + 1)
    eps, sc = 0.2, -1.0 / rows
    rc = 0.5 * sc

    def run():
        m = M.GemmMLP(net, torch.float32)
        m.f32_store_all = True
        for p in net.parameters():
            p.grad = torch.zeros_like(p)
        xp = m.prepare_input(X)
        if head == "library":
            assert m._f32 is None and not m.can_fuse_head()
            mean = m.forward(xp, keep=True)
            masks = [a.clone() > 0 for a in m._acts[1:]]
            _, s, g, _ = K.surrogate_loss(mean, None, act, lpo, adv, None, None, None, var, eps, sc, 0.0, 0.0, want_total=False,
                                          logp_ref=lref, ref_coef=rc)
            dout = g.clone()
            m.backward(g)
        else:
            assert m._f32 is not None and m.can_fuse_head()
            assert (head == "resident") == bool(m._f32.res) and (head == "wide") == bool(m._f32.wide)
            s = m.forward_loss(xp, 0, act=act, logp_old=lpo, adv=adv, var=var, epsilon=eps, surr_coef=sc, logp_ref=lref, ref_coef=rc)
            masks = [a.clone() > 0 for a in m._acts[1:]]
            dout = m._dz_head[:, :A].clone()
            m.backward_fused()
        torch.cuda.synchronize()
        return s.clone(), dout, [p.grad.clone() for p in net.parameters()], masks

    s, dout, got, masks = run()
    s2, dout2, got2, _ = run()
    assert torch.equal(s, s2) and torch.equal(dout, dout2) and all(torch.equal(a, b) for a, b in zip(got, got2))
    want, g, ref = _fp64_loss(net, X, masks, act, lpo, adv, lref, var, eps, sc, rc)
    for k, v in want.items():
        assert abs(float(s[k]) - v) <= 2e-6 * (abs(v) + 1.0), (k, float(s[k]), v)
    assert float(s[2]) > 0.1 * rows                                # (the penalty is really there)
    assert float((dout.double() - g).abs().max()) <= 2e-5 * (float(g.abs().max()) + 1e-30)
    for i, (gg, r) in enumerate(zip(got, ref)):
        assert float((gg.double() - r).abs().max()) <= 2e-5 * max(1.0, (rows / 1000) ** 0.5) * (float(r.abs().max()) + 1e-12), (i, rows)


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [1, 255, 70001])
def test_bf16_chain_head_with_the_reference_penalty(dev, rows):
    """tg_mlp_forward_chain_loss_ref (bf16 20-256x5-4): against the unfused bf16 path (tg_mlp_forward_chain + tg_surrogate_loss_ref +
    the backward chain) at test_forward_chain_with_the_loss_head_inside's bounds, and its loss sums (KL slot included) against fp64
    of the kernel's own head output; bit-identical run to run."""
    from trajopt_grpo_amd import mlp as M, hip_ops as K
    S, A, H = 20, 4, 256
    torch.manual_seed(rows)
    net = tg.NeuralNetwork(S, A, (H,) * 5, "ReLU").to(dev)
    X = torch.randn(rows, S, device=dev)
    act, lpo, adv, var, lref = _head_inputs(net, X, A, dev, rows + 2)
    eps, sc = 0.2, -1.0 / rows
    rc = 0.5 * sc
    mlp = M.GemmMLP(net, torch.bfloat16)
    for p in net.parameters():
        p.grad = torch.zeros_like(p)
    xp = mlp.prepare_input(X)
    out = mlp.forward(xp, keep=True)
    _, s_ref, g_mean, _ = K.surrogate_loss(out, None, act, lpo, adv, None, None, None, var, eps, sc, 0.0, 0.0, want_total=False,
                                           logp_ref=lref, ref_coef=rc)
    mlp.backward(g_mean)
    dz_ref = mlp._ws.get("z_head", rows, mlp.out_pad, torch.bfloat16, dev).clone()
    torch.cuda.synchronize()
    ref = [p.grad.clone() for p in net.parameters()]
    # fp64 of the loss sums from the same head output
    v = var.double().to(dev)
    lp = -0.5 * (((act.double() - out.double()) ** 2) / v).sum(1) - 0.5 * A * math.log(2 * math.pi) - 0.5 * float(torch.log(v).sum())
    x = lref.double() - lp
    d64 = float((torch.exp(x) - x - 1).sum())

    def run():
        m2 = M.GemmMLP(net, torch.bfloat16)
        assert m2.can_fuse_head()
        for p in net.parameters():
            p.grad = torch.zeros_like(p)
        s = m2.forward_loss(xp, 0, act=act, logp_old=lpo, adv=adv, var=var, epsilon=eps, surr_coef=sc, logp_ref=lref, ref_coef=rc)
        dz = m2._dz_head.clone()
        m2.backward_fused()
        torch.cuda.synchronize()
        return s.clone(), dz, [p.grad.clone() for p in net.parameters()]

    s, dz, got = run()
    s2, dz2, got2 = run()
    assert torch.equal(s, s2) and torch.equal(dz, dz2) and all(torch.equal(a, b) for a, b in zip(got, got2))
    ddz = (dz.float() - dz_ref.float()).abs()
    assert float((ddz > 2.0 ** -7 * dz_ref.float().abs() + 1e-30).float().mean()) < 1e-3 and float(ddz.max()) <= 2.0 ** -6 * float(dz_ref.float().abs().max())
    for j in (0, 2, 3):
        assert abs(float(s[j]) - float(s_ref[j])) <= 1e-6 * (abs(float(s_ref[j])) + 1.0), (j, float(s[j]), float(s_ref[j]))
    assert abs(float(s[2]) - d64) <= 1e-5 * (abs(d64) + 1.0) and d64 > 0.1 * rows
    for (n, _), a, b in zip(net.named_parameters(), ref, got):
        # (2x the plain head's bound: the penalty's d loss / d output spans exp(+-3), and the fused and unfused weight gradients
        # sum those rows in different orders)
        assert float((a - b).abs().max()) <= 4e-5 * (float(a.abs().max()) + 1e-9) * max(1.0, (rows / 1000) ** 0.5), n


# ---------------------------------------------------------------------------------------------------------------------------
# GPU: GRPO.learn() end to end
# ---------------------------------------------------------------------------------------------------------------------------
def _fp64_grpo(pol, ref, buf, *, epsilon, beta, gamma, updates, maximize, lr):
    """GRPO's iteration in fp64 from the buffer's reference-layout tensors: reward-to-go (grpo.py:66-74), group advantages
    (:110-115), ratios against the pre-update policy, the reference penalty on the valid rows, torch Adam on fp64 copies."""
    obs, act = buf.group_observations.double().cpu(), buf.group_actions.double().cpu()
    rew, mask = buf.group_rewards.double().cpu(), buf.group_masks.double().cpu()
    G, E, T, S = obs.shape
    A = act.shape[-1]
    rtg = torch.zeros_like(rew)
    for t in reversed(range(T)):
        rtg[..., t] = rew[..., t] * mask[..., t] + (gamma * rtg[..., t + 1] * mask[..., t + 1] if t < T - 1 else 0.0)
    m = mask.reshape(G, -1).bool()
    o, a, r = obs.reshape(G, -1, S), act.reshape(G, -1, A), rtg.reshape(G, -1)
    rows = [(o[g][m[g]], a[g][m[g]], (r[g][m[g]] - r[g][m[g]].mean()) / torch.std(r[g][m[g]] + 1e-8)) for g in range(G)]
    net = copy.deepcopy(pol.actor).cpu().double()
    rnet = copy.deepcopy(ref.actor).cpu().double()
    var, rvar = pol.var.double(), ref.var.double()

    def logp(n, v, x, y):
        mu = n(x)
        return -0.5 * (((y - mu) ** 2) / v).sum(-1) - 0.5 * A * math.log(2 * math.pi) - 0.5 * float(torch.log(v).sum())

    with torch.no_grad():
        old = [logp(net, var, x, y) for x, y, _ in rows]
        lref = [logp(rnet, rvar, x, y) for x, y, _ in rows]
    opt = torch.optim.Adam(net.parameters(), lr=lr)
    Js, kls = [], []
    n_valid = sum(x.shape[0] for x, _, _ in rows)
    for _ in range(updates):
        J, Dsum = 0.0, 0.0
        for (x, y, adv), lo, lr_ in zip(rows, old, lref):
            lp = logp(net, var, x, y)
            rho = torch.exp(lp - lo)
            d = lr_ - lp
            D = torch.exp(d) - d - 1
            J = J + torch.minimum(rho * adv, torch.clamp(rho, 1 - epsilon, 1 + epsilon) * adv).sum() - beta * D.sum()
            Dsum += float(D.sum())
        J = J / G
        opt.zero_grad()
        (-J if maximize else J).backward()
        opt.step()
        Js.append(float(J))
        kls.append(Dsum / n_valid)
    return net, Js, kls


E2E = {"cartpole_res": dict(env="CartPole", S=5, A=1, hidden=(128, 128), G=64, E=64, T=32, cd=None),
       "quadpole_wide": dict(env="QuadPole", S=20, A=4, hidden=(256,) * 3, G=8, E=32, T=48, cd=None),
       "quadpole_bf16": dict(env="QuadPole", S=20, A=4, hidden=(256,) * 5, G=8, E=64, T=48, cd=torch.bfloat16)}


def _setup(case, dev, seed=0, ref_scale=0.05, beta=0.5, maximize=False, ref=True, updates=2):
    c = E2E[case]
    torch.manual_seed(seed)
    pol = tg.GaussianActor_NeuralNetwork(c["S"], c["A"], c["hidden"], cov=0.5, device=dev)
    refm = copy.deepcopy(pol)
    with torch.no_grad():                                          # a perturbed copy of the policy
        for p in refm.actor.parameters():
            p.add_(ref_scale * torch.randn_like(p) * (p.abs().mean() + 1e-3))
    env_cls = getattr(tg, c["env"])
    mgr = tg.RolloutManager(lambda: env_cls(max_steps=c["T"]), pol, num_workers=c["G"], num_episodes_per_worker=c["E"], seed=seed + 11,
                            **({"compute_dtype": c["cd"]} if c["cd"] is not None else {}))
    buf = tg.Rollout_Buffer(mgr)
    buf.sample()
    algo = tg.GRPO(epsilon=0.2, beta=beta, gamma=0.99, policy=pol, optimizer=torch.optim.Adam(pol.parameters(), lr=3e-4),
                   ref_model=refm if ref else None, updates_per_iter=updates, maximize=maximize, autocast_dtype=c["cd"])
    return pol, refm, buf, algo


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(E2E))
@pytest.mark.parametrize("maximize", [False, True])
def test_grpo_learn_with_a_reference_policy_matches_fp64(dev, case, maximize):
    """GRPO(ref_model=perturbed copy, beta=0.5).learn() with two updates: J and kl_ref of each update and the post-update weights
    against the fp64 restatement (masked rows, Adam).  C2's shape (4,096 CartPole envs, fp32 5-128-128-1: the resident kernel),
    QuadPole fp32 H = 256 (the wide kernel), QuadPole bf16 20-256x5-4 (the bf16 chain)."""
    pol, refm, buf, algo = _setup(case, dev, maximize=maximize)
    before = copy.deepcopy(pol.actor)
    want_net, Js, kls = _fp64_grpo(pol, refm, buf, epsilon=0.2, beta=0.5, gamma=0.99, updates=2, maximize=maximize, lr=3e-4)
    m = algo._mlp(pol.actor)
    algo.learn(buf)
    st = algo.last_stats
    assert m is not None and m.can_fuse_head()
    bf16 = E2E[case]["cd"] is not None
    tol = 5e-3 if bf16 else 1e-4
    assert len(st["J"]) == 2 and len(st["kl_ref"]) == 2
    for j_gpu, j_cpu in zip(st["J"], Js):
        assert abs(j_gpu - j_cpu) <= tol * max(1.0, abs(j_cpu)), (st["J"], Js)
    for k_gpu, k_cpu in zip(st["kl_ref"], kls):
        assert abs(k_gpu - k_cpu) <= tol * max(1e-3, abs(k_cpu)), (st["kl_ref"], kls)
    assert kls[0] > 0
    for (n, p_gpu), p_cpu, p0 in zip(pol.actor.named_parameters(), want_net.parameters(), before.parameters()):
        got, want, start = p_gpu.detach().double().cpu(), p_cpu.detach(), p0.detach().double().cpu()
        # (Adam's normalised step: an entry whose gradient sits at rounding level may move by up to 2 lr in either direction)
        assert float((got - want).abs().max()) <= 2 * 2 * 3e-4 + 1e-6, n
        if bf16:
            dg, dw = (got - start).reshape(-1), (want - start).reshape(-1)
            assert float(torch.dot(dg, dw) / (dg.norm() * dw.norm() + 1e-30)) > 0.9, n
        else:
            assert float((got - want).norm() / (want.norm() + 1e-12)) < 2e-4, n


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["cartpole_res", "quadpole_bf16"])
def test_no_reference_and_beta_zero_are_the_plain_path(dev, case, monkeypatch):
    """ref_model=None and (ref_model, beta=0) give bit-identical weights and statistics, and neither launches a `_ref` entry point
    (no reference pass either); with beta != 0 the `_ref` entry runs."""
    lib = N.load()
    calls = {n: 0 for n in REF_ENTRIES}
    for name in REF_ENTRIES:
        fn = getattr(lib, name)

        def counted(*args, _fn=fn, _n=name):
            calls[_n] += 1
            return _fn(*args)
        monkeypatch.setattr(lib, name, counted)
    out = []
    for ref, beta in ((False, 0.5), (True, 0.0)):
        pol, _, buf, algo = _setup(case, dev, beta=beta, ref=ref)
        algo.learn(buf)
        torch.cuda.synchronize()
        out.append(([p.detach().clone() for p in pol.actor.parameters()], dict(algo.last_stats)))
    assert sum(calls.values()) == 0, calls
    (w0, s0), (w1, s1) = out
    assert all(torch.equal(a, b) for a, b in zip(w0, w1)) and s0 == s1 and "kl_ref" not in s0
    pol, _, buf, algo = _setup(case, dev, beta=0.5, ref=True)
    algo.learn(buf)
    torch.cuda.synchronize()
    assert sum(calls.values()) == 2 and "kl_ref" in algo.last_stats
    assert not all(torch.equal(a, b) for a, b in zip(w0, pol.actor.parameters()))


@pytest.mark.gpu
def test_maximize_with_a_large_beta_pulls_the_policy_to_the_reference(dev):
    """maximize=True, beta = 20 and a reference policy far from the policy: the mean D of a fixed buffer decreases monotonically over
    a few learn() calls (the penalty keeps the policy close to the reference, as DeepSeekMath's GRPO intends)."""
    pol, refm, buf, algo = _setup("cartpole_res", dev, ref_scale=2.0, beta=20.0, maximize=True, updates=2)
    kl = []
    for _ in range(4):
        algo.learn(buf)
        kl += algo.last_stats["kl_ref"]
    assert kl[0] > 1e-3 and all(b < a for a, b in zip(kl, kl[1:])), kl


@pytest.mark.gpu
def test_writes_to_the_reference_policy_between_learn_calls_are_seen(dev):
    """A caller refreshing the reference policy through `.data` between learn() calls: the next reference pass reads the new weights
    (the entry refresh of its weight layouts), so setting it to the policy itself gives D = 0 up to rounding."""
    pol, refm, buf, algo = _setup("cartpole_res", dev, updates=1)
    algo.learn(buf)
    assert algo.last_stats["kl_ref"][0] > 1e-6
    for p, q in zip(refm.actor.parameters(), pol.actor.parameters()):
        p.data.copy_(q.data)
    algo.learn(buf)
    assert abs(algo.last_stats["kl_ref"][0]) < 1e-6, algo.last_stats["kl_ref"]
