"""Tanh hidden activations on the fp32 hot path, on the MI355X: the kernels' tanh against fp64, the fused fp32 rollout with a Tanh
actor against fp64 at every recorded step and across rank shards, the `_act` entries with TG_ACT_RELU against the plain ones (bits),
the chain learner's forward + loss + backward with Tanh against fp64 autograd for every head, learn() end to end, and the path
choice of the Tanh configurations that stay on torch.

The kernels' tanh is the device library's tanhf; the bound relied on is |tanhf(z) - tanh(z)| <= C_TANH u, u = 2^-24 (every
|tanh| < 1, so that is at most C_TANH ulps of a result in [0.5, 1) and more ulps below)."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from test_fused_rollout_fp64 import (DIMS, ENVS, U, _assert_shards_equal_whole, _cus, actor_layers, check_actions, gamma, make_env,
                                     philox_draws, sigmas)
from test_grpo_ref_kl import _fp64_grpo, _head_inputs

pytestmark = pytest.mark.gpu

C_TANH = 4.0


@pytest.fixture(scope="module")
def tg():
    import trajopt_grpo_amd as tg
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return tg


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def tanh_policy(tg, S, A, hidden, dev, seed, critic=False):
    torch.manual_seed(seed)
    cls = tg.GaussianActorCritic_NeuralNetwork if critic else tg.GaussianActor_NeuralNetwork
    return cls(S, A, hidden, activation="Tanh", cov=0.3, device=dev)


# ------------------------------------------------------------------------------------------------------------------------------
# (a) the kernels' tanh against fp64
# ------------------------------------------------------------------------------------------------------------------------------
def test_kernel_tanh_is_within_its_stated_bound_of_fp64(tg, dev):
    """Linear(4, 64) Tanh Linear(64, 4) with a one-hot first layer (z = x exactly) and a one-hot head on features 0..3: the chain
    kernel's forward (tg_mlp_f32_forward_act) returns fl(tanh(x)) itself.  A dense sweep of [-20, 20] plus +-0, tiny, subnormal and
    large values: |got - tanh(x)| <= C_TANH u and odd symmetry exact.  (The fused rollout kernel calls the same act_f32<Tanh>: its
    actions are held to this bound in the fp64 rollout tests below.)"""
    from trajopt_grpo_amd import mlp as M
    net = tg.NeuralNetwork(4, 4, (64,), "Tanh").to(dev)
    with torch.no_grad():
        for p in net.parameters():
            p.zero_()
        lin = [m for m in net.network if isinstance(m, torch.nn.Linear)]
        lin[0].weight[:4, :4] = torch.eye(4)
        lin[1].weight[:4, :4] = torch.eye(4)
    m = M.GemmMLP(net, torch.float32)
    assert m._f32 is not None and m._f32.act == tg._native.TG_ACT_TANH
    sweep = torch.linspace(-20.0, 20.0, 4_000_001, dtype=torch.float32)
    special = torch.tensor([0.0, -0.0, 1e-45, -1e-45, 1e-38, -1e-38, 1e-30, 1e-10, -1e-10, 1e-4, 0.625, -0.625, 0.6249999, 0.6250001,
                            9.0, 9.1, 40.0, -40.0, 88.0, 1e30, -1e30, 3.4e38, -3.4e38], dtype=torch.float32)
    x = torch.cat([sweep, special, -sweep[:1000] * 1e-6])
    x = torch.cat([x, x.new_zeros((-x.numel()) % 4)])
    X = x.view(-1, 4).to(dev)
    out = m.forward(m.prepare_input(X), keep=False)
    torch.cuda.synchronize()
    got = out.double().reshape(-1).cpu()
    want = torch.tanh(x.double())
    err = (got - want).abs()
    assert float(err.max()) <= C_TANH * U, (float(err.max()) / U, float(x[err.argmax()]))
    neg = out.reshape(-1).cpu()
    outn = m.forward(m.prepare_input(-X), keep=False).reshape(-1).cpu()
    assert torch.equal(outn, -neg)                                     # odd: the sign is copied back onto tanh(|x|)
    assert float(got.abs().max()) <= 1.0


# ------------------------------------------------------------------------------------------------------------------------------
# (b) the fused fp32 rollout with a Tanh actor against fp64 at every recorded step
# ------------------------------------------------------------------------------------------------------------------------------
def f32_tanh_mean_and_bound(layers, x, k1):
    """test_fused_rollout_fp64.f32_mean_and_bound with tanh in place of relu: tanh is 1-Lipschitz, so an activation's error is its
    input's error plus the kernel's tanhf error (<= C_TANH u)."""
    h, e = x, torch.zeros_like(x)
    for li, (W, b) in enumerate(layers):
        K = k1 if li == 0 else W.shape[1]
        Wa = W.abs()
        z = h @ W.t() + b
        e = e @ Wa.t() + gamma(K + 1) * ((h.abs() + e) @ Wa.t() + b.abs())
        if li + 1 < len(layers):
            h, e = torch.tanh(z), e + C_TANH * U
        else:
            h = z
    return h, e


F32_SHAPES = [(H,) * L for H in (64, 128) for L in (1, 2, 3, 4)]


@pytest.mark.parametrize("block_envs", [16, 32])
@pytest.mark.parametrize("hidden", F32_SHAPES, ids=lambda h: f"{h[0]}x{len(h)}")
@pytest.mark.parametrize("name", ENVS)
def test_fused_f32_tanh_actor_matches_fp64_at_every_step(tg, dev, name, hidden, block_envs):
    S, A = DIMS[name]
    T, G, Eps = 24, 3, 43
    pol = tanh_policy(tg, S, A, hidden, dev, seed=300 + len(hidden) + hidden[0])
    eng = tg.DeviceRollout(make_env(tg, name, T), pol, G, Eps, seed=41)
    eng.f32_block_envs = block_envs
    assert eng.fused and eng._fused_f32 and eng._f32_act == tg._native.TG_ACT_TANH
    tr = eng.run()
    assert eng._frag.block_envs == block_envs
    eps = philox_draws(tg, make_env(tg, name, T), pol, G, Eps, 41, dev)
    layers = actor_layers(pol)
    k1 = (S + 7) // 8 * 8
    check_actions(tr, eps, sigmas(eng), lambda x: f32_tanh_mean_and_bound(layers, x, k1), k_alive_min=G * Eps * 2)


@pytest.mark.parametrize("block_envs", [16, 32])
def test_fused_f32_tanh_split_launch_matches_fp64(tg, dev, block_envs):
    name, hidden = "QuadPole", (128, 128, 128)
    S, A = DIMS[name]
    T, G, Eps = 24, 3, 43
    pol = tanh_policy(tg, S, A, hidden, dev, seed=7)
    whole = tg.DeviceRollout(make_env(tg, name, T), pol, G, Eps, seed=42)
    whole.f32_block_envs = block_envs
    ref = [x.clone() for x in (lambda t: (t.obs, t.act, t.rew, t.mask, t.len))(whole.run())]
    split = tg.DeviceRollout(make_env(tg, name, T), pol, G, Eps, seed=42)
    split.f32_block_envs = block_envs
    split._seed_host, split._stream_host = 42, 0
    with torch.cuda.device(dev):
        split._enqueue_prepare(None)
        split._enqueue_fused(0, 13)
        split.rng[1] -= 1
        split._enqueue_fused(13, T)
    torch.cuda.synchronize()
    tr = split.traj
    assert bool(tr.mask[13:].any())
    eps = philox_draws(tg, make_env(tg, name, T), pol, G, Eps, 42, dev)
    layers = actor_layers(pol)
    check_actions(tr, eps, sigmas(split), lambda x: f32_tanh_mean_and_bound(layers, x, 24))
    for a, b in zip((tr.obs, tr.act, tr.rew, tr.mask, tr.len), ref):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------------------------------
# (c) rank shards
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_cu", [1, 2], ids=["block16", "block32"])
def test_fused_f32_tanh_shards_equal_the_whole_rollout(tg, dev, per_cu):
    """G E = 16 x CUs (every engine takes 16 envs per workgroup) and 2 x 16 x CUs (the whole rollout takes 32; its halves and
    quarters alone would take 16): every shard reproduces the whole rollout bit for bit."""
    lib = tg._native.load()
    n_total = per_cu * 16 * _cus(dev)
    G, T = 8, 16
    Eps = n_total // G
    pol = tanh_policy(tg, 5, 1, (128, 128), dev, seed=3)
    engines = _assert_shards_equal_whole(tg, lambda: tg.CartPole(max_steps=T), pol, G, Eps, (2, 4), dev)
    assert all(e.fused and e._fused_f32 and e._f32_act == tg._native.TG_ACT_TANH for e in engines)
    assert {e._f32_block_envs for e in engines} == {16 * per_cu}
    assert lib.tg_fused_rollout_f32_block_envs(n_total, 1) == 16 * per_cu


# ------------------------------------------------------------------------------------------------------------------------------
# (d) the `_act` entries with TG_ACT_RELU are the plain entries
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hidden", [(64,), (128, 128, 128)])
@pytest.mark.parametrize("with_ref", [False, True])
def test_act_entries_with_relu_are_bit_identical_to_the_plain_ones(tg, dev, hidden, with_ref):
    from trajopt_grpo_amd import mlp as M
    Nn = tg._native
    lib = Nn.load()
    S, A, rows = 5, 2, 3001
    torch.manual_seed(11)
    net = tg.NeuralNetwork(S, A, hidden, "ReLU").to(dev)
    f = M.F32ChainStream(net, hidden[0])
    X = torch.randn(rows, S, device=dev)
    xp = torch.zeros(rows, f.in_pad, device=dev)
    xp[:, :S] = X
    st = Nn.stream_ptr(dev)
    o1, o2 = torch.zeros(rows, 4, device=dev), torch.ones(rows, 4, device=dev)
    Nn.check(lib.tg_mlp_f32_forward(xp.data_ptr(), f.in_pad, f.stream.data_ptr(), f.H, f.n_hidden, rows, o1.data_ptr(), st), "fwd")
    Nn.check(lib.tg_mlp_f32_forward_act(xp.data_ptr(), f.in_pad, f.stream.data_ptr(), f.H, f.n_hidden, rows, o2.data_ptr(),
                                        Nn.TG_ACT_RELU, st), "fwd_act")
    torch.cuda.synchronize()
    assert torch.equal(o1, o2)
    act, lpo, adv, var, lref = _head_inputs(net, X, A, dev, 5)
    nh, H = f.n_hidden, f.H
    blocks = lib.tg_mlp_f32_blocks()

    def train(entry):
        acts = [torch.full((rows, H), float("nan"), device=dev) for _ in range(nh)]
        dzs = [torch.full((rows, H), float("nan"), device=dev) for _ in range(nh)]
        dout = torch.zeros(rows, 4, device=dev)
        work = torch.zeros(blocks * 4, dtype=torch.float64, device=dev)
        a = Nn.ChainLoss()
        a.kind, a.act_dim = 0, A
        a.d_act, a.act_row_stride, a.act_col_stride = act.data_ptr(), A, 1
        a.d_logp_old, a.d_adv, a.d_dout8, a.d_work = lpo.data_ptr(), adv.data_ptr(), dout.data_ptr(), work.data_ptr()
        for k in range(A):
            a.var[k] = 0.3
        a.norm_mean, a.norm_inv, a.epsilon, a.surr_coef = 0.1, 1.3, 0.2, -1.0 / rows
        a.kl_coef = 0.0 if with_ref else 0.5 / rows
        ref = None
        if with_ref:
            ref = Nn.RefPenalty()
            ref.d_logp_ref, ref.coef = lref.data_ptr(), -0.5 / rows
        pa = (C.c_void_p * nh)(*[t.data_ptr() for t in acts])
        pz = (C.c_void_p * nh)(*[t.data_ptr() for t in dzs])
        if entry == "plain" and ref is None:
            rc = lib.tg_mlp_f32_forward_backward(xp.data_ptr(), f.in_pad, f.stream.data_ptr(), H, nh, rows, pa, pz, None, C.byref(a), st)
        elif entry == "plain":
            rc = lib.tg_mlp_f32_forward_backward_ref(xp.data_ptr(), f.in_pad, f.stream.data_ptr(), H, nh, rows, pa, pz, None, C.byref(a),
                                                     C.byref(ref), st)
        else:
            rc = lib.tg_mlp_f32_forward_backward_act(xp.data_ptr(), f.in_pad, f.stream.data_ptr(), H, nh, rows, pa, pz, None, C.byref(a),
                                                     C.byref(ref) if ref is not None else None, Nn.TG_ACT_RELU, st)
        Nn.check(rc, entry)
        torch.cuda.synchronize()
        return acts + dzs + [dout, work]

    for x, y in zip(train("plain"), train("act")):
        assert torch.equal(x, y)


class _ActLib:
    """The library with tg_fused_rollout_f32 answered by tg_fused_rollout_f32_act(..., TG_ACT_RELU, stream)."""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def tg_fused_rollout_f32(self, *args):
        return self._lib.tg_fused_rollout_f32_act(*args[:-1], 0, args[-1])


@pytest.mark.parametrize("block_envs", [16, 32])
def test_fused_rollout_act_with_relu_is_bit_identical(tg, dev, block_envs):
    torch.manual_seed(12)
    pol = tg.GaussianActor_NeuralNetwork(10, 2, (128, 128, 128), cov=0.3, device=dev)
    runs = []
    for via_act in (False, True):
        eng = tg.DeviceRollout(tg.QuadPole2D(max_steps=32), pol, 4, 37, seed=5)
        eng.f32_block_envs = block_envs
        assert eng._fused_f32 and eng._f32_act == tg._native.TG_ACT_RELU
        if via_act:
            eng.lib = _ActLib(eng.lib)
        tr = eng.run()
        torch.cuda.synchronize()
        runs.append([x.clone() for x in (tr.obs, tr.act, tr.rew, tr.mask, tr.len)])
    assert all(torch.equal(a, b) for a, b in zip(*runs))


# ------------------------------------------------------------------------------------------------------------------------------
# (e) the chain learner with Tanh against fp64 autograd, every head kind
# ------------------------------------------------------------------------------------------------------------------------------
HEADS = ["grpo", "grpo_ref", "ppo_actor", "ppo_critic"]
LEARN_SHAPES = [(5, 1, (64,)), (10, 2, (64, 64)), (20, 4, (64,) * 3), (7, 3, (64,) * 4),
                (5, 1, (128,)), (5, 1, (128, 128)), (32, 4, (128,) * 3), (20, 4, (128,) * 4)]


@pytest.mark.parametrize("head", HEADS)
@pytest.mark.parametrize("dims", LEARN_SHAPES, ids=lambda d: f"{d[0]}-{d[2][0]}x{len(d[2])}-{d[1]}")
@pytest.mark.parametrize("rows", [1, 255, 70001])
def test_f32_tanh_chain_update_matches_fp64_autograd(tg, dev, head, dims, rows):
    """forward_loss() + backward_fused() of a Tanh net (tg_mlp_f32_forward_backward_act + tg_mlp_f32_weight_grad): loss sums, every
    stored activation and dZ, d loss / d output and every parameter gradient against fp64 autograd, at
    test_f32_chain_update_matches_fp64_autograd's tolerances; gradients accumulate; bit-identical run to run."""
    from trajopt_grpo_amd import mlp as M
    S, A, hidden = dims
    kind = 1 if head == "ppo_critic" else 0
    if kind == 1:
        A = 1
    torch.manual_seed(rows + S + HEADS.index(head))
    net = tg.NeuralNetwork(S, A, hidden, "Tanh").to(dev)
    X = torch.randn(rows, S, device=dev)
    act, lpo, adv, var, lref = _head_inputs(net, X, A, dev, rows + 3)
    ret = torch.randn(rows, device=dev)
    eps, sc, cc = 0.2, -1.0 / rows, 0.5 / rows
    kc = 0.5 / rows if head == "ppo_actor" else 0.0
    rc = 0.5 * sc if head == "grpo_ref" else 0.0
    norm = [0.1, 1.3, -0.2, 0.7] if head.startswith("ppo") else None

    def run():
        m = M.GemmMLP(net, torch.float32)
        for i, p in enumerate(net.parameters()):
            p.grad = torch.full_like(p, 0.25 * (i + 1))               # the kernels must ADD to what is there
        assert m._f32 is not None and m._f32.act == tg._native.TG_ACT_TANH and m.f32_store_all and m.can_fuse_head()
        xp = m.prepare_input(X)
        if kind == 0:
            s = m.forward_loss(xp, 0, act=act, logp_old=lpo, adv=adv, norm=None if norm is None else norm[0:2], var=var, epsilon=eps,
                               surr_coef=sc, kl_coef=kc, logp_ref=lref if rc else None, ref_coef=rc)
        else:
            s = m.forward_loss(xp, 1, ret=ret, norm=norm[2:4], critic_coef=cc)
        stored = [t.clone() for t in m._acts[1:]], [t.clone() for t in m._bits], m._dz_head.clone(), m._tmask
        m.backward_fused()
        torch.cuda.synchronize()
        return s.clone(), [p.grad.clone() for p in net.parameters()], stored

    s, got, (acts, dzs, dout, tmask) = run()
    s2, got2, _ = run()
    assert tmask is None
    assert torch.equal(s, s2) and all(torch.equal(a, b) for a, b in zip(got, got2))
    lin = [mod for mod in copy.deepcopy(net).double().network if isinstance(mod, torch.nn.Linear)]
    params = []
    for l in lin:
        params += [l.weight.detach().clone().requires_grad_(), l.bias.detach().clone().requires_grad_()]
    hs, h = [], X.double()
    for l in range(len(hidden)):
        h = torch.tanh(h @ params[2 * l].t() + params[2 * l + 1])
        h.retain_grad()
        hs.append(h)
    out = h @ params[-2].t() + params[-1]
    out.retain_grad()
    if kind == 0:
        v = var.double().to(dev)
        logp = -0.5 * (((act.double() - out) ** 2) / v).sum(1) - 0.5 * A * np.log(2 * np.pi) - 0.5 * float(torch.log(v).sum())
        rho = torch.exp(logp - lpo.double())
        an = adv.double() if norm is None else (adv.double() - norm[0]) * norm[1]
        surr = torch.minimum(rho * an, torch.clamp(rho, 1 - eps, 1 + eps) * an)
        if rc:
            x = lref.double() - logp
            D = torch.exp(x) - x - 1
            total = sc * surr.sum() - rc * D.sum()
            want = {0: float(surr.sum()), 2: float(D.sum()), 3: float(rows)}
        else:
            kl = torch.exp(lpo.double()) * (lpo.double() - logp)
            total = sc * surr.sum() + kc * kl.sum()
            want = {0: float(surr.sum()), 2: float(kl.sum()) if kc else None, 3: float(rows)}
    else:
        d = out[:, 0] - (ret.double() - norm[2]) * norm[3]
        total = cc * (d * d).sum()
        want = {1: float((d * d).sum()), 3: float(rows)}
    total.backward()
    g = out.grad
    for k, val in want.items():
        if val is not None:
            assert abs(float(s[k]) - val) <= 2e-6 * (abs(val) + 1.0), (k, float(s[k]), val)
    for i, (a, hh) in enumerate(zip(acts, hs)):
        assert float((a.double() - hh.detach()).abs().max()) <= 1e-5 * (float(hh.abs().max()) + 1e-6), i
    assert float((dout[:, :A].double() - g).abs().max()) <= 2e-5 * (float(g.abs().max()) + 1e-30) and torch.all(dout[:, A:] == 0)
    for l, hh in enumerate(hs):                 # d loss / d pre-activation: the gradient at h times (1 - h^2), as tanh_backward forms it
        dz = hh.grad * (1 - hh.detach() ** 2)
        assert float((dzs[l].double() - dz).abs().max()) <= 2e-5 * (float(dz.abs().max()) + 1e-30), l
    for i, (gg, p) in enumerate(zip(got, params)):
        r, base = p.grad, 0.25 * (i + 1)
        scale = float(r.abs().max()) + 1e-12
        assert float((gg.double() - base - r).abs().max()) <= (2e-5 * max(1.0, (rows / 1000) ** 0.5)) * scale + 4e-7 * base, (i, rows)


# ------------------------------------------------------------------------------------------------------------------------------
# (f) learn() end to end on Tanh policies
# ------------------------------------------------------------------------------------------------------------------------------
def _assert_native(tg, algo, pol, mgr):
    m = algo._mlp(pol.actor)
    assert m is not None and m.act == "Tanh" and m._f32 is not None and m._f32.act == tg._native.TG_ACT_TANH
    assert mgr.engine.fused and mgr.engine._fused_f32 and mgr.engine._f32_act == tg._native.TG_ACT_TANH


@pytest.mark.parametrize("hidden", [(128, 128), (128,) * 4], ids=["5-128x2-1", "5-128x4-1"])
@pytest.mark.parametrize("with_ref", [False, True])
@pytest.mark.parametrize("maximize", [False, True])
def test_grpo_learn_on_a_tanh_policy_matches_fp64(tg, dev, hidden, with_ref, maximize):
    """GRPO on C2's setup shape (CartPole, fp32) with a Tanh actor, two updates: J (and kl_ref) of each update and the post-update
    weights against test_grpo_ref_kl's fp64 restatement, at that test's fp32 tolerances."""
    torch.manual_seed(21)
    pol = tg.GaussianActor_NeuralNetwork(5, 1, hidden, activation="Tanh", cov=0.5, device=dev)
    refm = copy.deepcopy(pol)
    with torch.no_grad():
        for p in refm.actor.parameters():
            p.add_(0.05 * torch.randn_like(p) * (p.abs().mean() + 1e-3))
    mgr = tg.RolloutManager(lambda: tg.CartPole(max_steps=32), pol, num_workers=64, num_episodes_per_worker=64, seed=11)
    buf = tg.Rollout_Buffer(mgr)
    buf.sample()
    beta = 0.5 if with_ref else 0.0
    algo = tg.GRPO(epsilon=0.2, beta=beta, gamma=0.99, policy=pol, optimizer=torch.optim.Adam(pol.parameters(), lr=3e-4),
                   ref_model=refm if with_ref else None, updates_per_iter=2, maximize=maximize)
    _assert_native(tg, algo, pol, mgr)
    before = copy.deepcopy(pol.actor)
    want_net, Js, kls = _fp64_grpo(pol, refm, buf, epsilon=0.2, beta=beta, gamma=0.99, updates=2, maximize=maximize, lr=3e-4)
    algo.learn(buf)
    st = algo.last_stats
    assert len(st["J"]) == 2
    for j_gpu, j_cpu in zip(st["J"], Js):
        assert abs(j_gpu - j_cpu) <= 1e-4 * max(1.0, abs(j_cpu)), (st["J"], Js)
    if with_ref:
        assert kls[0] > 0
        for k_gpu, k_cpu in zip(st["kl_ref"], kls):
            assert abs(k_gpu - k_cpu) <= 1e-4 * max(1e-3, abs(k_cpu)), (st["kl_ref"], kls)
    for (n, p_gpu), p_cpu, p0 in zip(pol.actor.named_parameters(), want_net.parameters(), before.parameters()):
        got, want = p_gpu.detach().double().cpu(), p_cpu.detach()
        assert float((got - want).abs().max()) <= 2 * 2 * 3e-4 + 1e-6, n
        assert float((got - want).norm() / (want.norm() + 1e-12)) < 2e-4, n
        assert not torch.equal(got, p0.detach().double().cpu()), n


@pytest.mark.parametrize("batch_size", [None, 1024], ids=["full", "minibatch"])
def test_ppo_learn_on_a_tanh_policy_matches_the_torch_path(tg, dev, batch_size):
    """PPO on a Tanh actor-critic (5-128x3-1, CartPole), two learn() calls: the native path (fp32 fused rollout, chain learner) and
    the fallback (fused_mlp=False: torch autograd) on the same buffers from the same weights: weights and last_stats agree."""
    pol = tanh_policy(tg, 5, 1, (128,) * 3, dev, seed=31, critic=True)
    pol_t = copy.deepcopy(pol)
    mgr = tg.RolloutManager(lambda: tg.CartPole(max_steps=32), pol, num_workers=32, num_episodes_per_worker=64, seed=12)
    buf = tg.Rollout_Buffer(mgr)
    mk = lambda p, fused: tg.PPO(epsilon=0.2, policy=p, optimizer=torch.optim.Adam(p.parameters(), lr=3e-4), ref_model=None,
                                 updates_per_iter=2, gamma=0.99, batch_size=batch_size, fused_mlp=fused)
    algo, algo_t = mk(pol, True), mk(pol_t, False)
    for it in range(2):
        buf.sample()
        if it == 0:
            _assert_native(tg, algo, pol, mgr)
            assert algo._mlp(pol.critic) is not None and algo_t._mlp(pol_t.actor) is None and algo_t._mlp(pol_t.critic) is None
        with torch.no_grad():                                  # (the fallback learns from the native run's weights of this iteration)
            for p, q in zip(pol_t.parameters(), pol.parameters()):
                p.copy_(q)
        algo.learn(buf)
        algo_t.learn(buf)
        torch.cuda.synchronize()
        for key in ("total_loss",):
            a, b = np.asarray(algo.last_stats[key], dtype=np.float64), np.asarray(algo_t.last_stats[key], dtype=np.float64)
            assert a.shape == b.shape and np.allclose(a, b, rtol=1e-4, atol=1e-6), (key, a, b)
        for (n, p), q in zip(pol.actor.named_parameters(), pol_t.actor.parameters()):
            d = (p.detach() - q.detach()).double()
            assert float(d.abs().max()) <= 2 * 2 * 3e-4 + 1e-6 and float(d.norm() / q.detach().double().norm()) < 2e-4, (it, n)


# ------------------------------------------------------------------------------------------------------------------------------
# (g) uncovered Tanh configurations keep today's path
# ------------------------------------------------------------------------------------------------------------------------------
def test_uncovered_tanh_configurations_keep_the_torch_path(tg, dev):
    opt = lambda p: torch.optim.Adam(p.parameters(), lr=1e-3)
    covered = tanh_policy(tg, 5, 1, (128, 128), dev, seed=1)
    wide = tanh_policy(tg, 5, 1, (256, 256), dev, seed=2)
    mixed = tg.GaussianActor_NeuralNetwork(5, 1, (128, 128), activation=["Tanh", "ReLU"], cov=0.3, device=dev)
    sig = tg.GaussianActor_NeuralNetwork(5, 1, (128, 128), activation="Sigmoid", cov=0.3, device=dev)
    g = lambda p, **kw: tg.GRPO(0.2, 0.0, 0.99, p, opt(p), **kw)
    assert g(covered)._mlp(covered.actor) is not None
    assert g(covered, autocast_dtype=torch.bfloat16)._mlp(covered.actor) is None
    assert g(covered, fused_mlp=False)._mlp(covered.actor) is None
    for p in (wide, mixed, sig):
        assert g(p)._mlp(p.actor) is None
    env = lambda: tg.CartPole(max_steps=16)
    assert tg.DeviceRollout(env(), covered, 2, 16).fused
    for p, kw in ((covered, {"compute_dtype": torch.bfloat16}), (wide, {}), (mixed, {}), (sig, {}), (covered, {"fused": False})):
        eng = tg.DeviceRollout(env(), p, 2, 16, **kw)
        assert not eng.fused and eng._mlp is None and (eng._fused_f32 == (kw == {"fused": False}))
    with pytest.raises(ValueError, match="Tanh"):
        tg.DeviceRollout(env(), wide, 2, 16, fused=True)
    # ... and still learns there (torch autograd), as before
    mgr = tg.RolloutManager(env, wide, num_workers=2, num_episodes_per_worker=32)
    buf = tg.Rollout_Buffer(mgr)
    buf.sample()
    algo = g(wide)
    before = [p.detach().clone() for p in wide.parameters()]
    algo.learn(buf)
    assert not mgr.engine.fused and algo._mlp(wide.actor) is None
    assert any(not torch.equal(a, b) for a, b in zip(before, wide.parameters()))
