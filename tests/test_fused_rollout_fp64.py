"""The fused rollout kernels' actor against fp64, at every recorded step, and their trajectories across rank shards.

tg_fused_rollout_f32 (fp32 products, C2) and tg_fused_rollout (bf16 products, C3) run the actor MLP, the Philox sample and the
dynamics of a whole rollout in one launch.  The dynamics are pinned elsewhere (a teacher-forced replay reproduces every recorded
trajectory bit for bit); here the ACTOR is: for every alive (t, env, a) the recorded action must equal

    mean_ref(obs[:, t]) + sigma * eps[t, env]

within a bound derived from the kernel's arithmetic, where obs[:, t] is the observation the kernel itself recorded, eps is the
Philox draw of (env, t) read back from the per-step kernel, and mean_ref is computed in fp64.  The bounds are rigorous (forward
error analysis with gamma_k = k u / (1 - k u), u = 2^-24), not tuned: a wrong bias, a k-column slip, a lost head partial or an
env's activations swapped with another env's exceed them by orders of magnitude.

The second half pins that a rollout split into rank shards (group_offset + global_groups) reproduces the one-engine rollout bit
for bit on both sides of every size threshold that selects a kernel variant."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

DIMS = {"CartPole": (5, 1), "QuadPole2D": (10, 2), "QuadPole": (20, 4), "Pendulum": (3, 1)}
ENVS = list(DIMS)
U = 2.0 ** -24                                      # unit roundoff of fp32 (round to nearest)


@pytest.fixture(scope="module")
def tg():
    import trajopt_grpo_amd as tg
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return tg


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def gamma(k):
    return k * U / (1.0 - k * U)


# ------------------------------------------------------------------------------------------------------------------------------
# shared helpers
# ------------------------------------------------------------------------------------------------------------------------------
def make_env(tg, name, T):
    return tg.environments.ENV_CLASSES[name](max_steps=T)


def philox_draws(tg, env, pol, G, Eps, seed, dev, group_offset=0):
    """eps [A][T][n] fp32: the standard normal draw of every (env, t) of the first rollout of an engine seeded `seed`, read back
    from the per-step kernel (tg_rollout_step with mean 0 and sigma 1 records rn_add(0, rn_mul(1, eps)) == eps).  Every env is
    made alive again in front of each step (len = 0), so the draw of every (env, t) is recorded whatever the dynamics do."""
    Nn = tg._native
    eng = tg.DeviceRollout(env, pol, G, Eps, seed=seed, fused=False, use_graph=False, group_offset=group_offset)
    eng._seed_host, eng._stream_host = seed, 0
    A, T, n = eng.A, eng.T, eng.n
    zeros, ones = torch.zeros(n, A, device=dev), (C.c_float * A)(*([1.0] * A))
    lib, st = Nn.load(), Nn.stream_ptr(dev)
    with torch.cuda.device(dev):
        eng._enqueue_prepare(None)
        tr = eng.traj.native()
        for t in range(T):
            eng.traj.len.zero_()
            Nn.check(lib.tg_rollout_step(C.byref(eng.params), C.byref(tr), t, zeros.data_ptr(), A, ones, eng.rng.data_ptr(),
                                         group_offset * eng.E, st), "tg_rollout_step")
    torch.cuda.synchronize()
    return eng.traj.act.clone()


def actor_layers(pol):
    return [(l.weight.detach().double(), l.bias.detach().double()) for l in pol.actor.network if isinstance(l, torch.nn.Linear)]


def f32_mean_and_bound(layers, x, k1):
    """fp64 actor mean and a rigorous bound on the fp32 kernel's error.  Layer l of the kernel sums K products and its bias in
    fp32 in some order (MFMA chain, then the head's per-lane partials and their fixed-order reduction): whatever the order,
    |fl(W h + b) - (W h + b)| <= gamma_{K+1} (|W| |h| + |b|) (Higham, Accuracy and Stability, 3.1).  With h off by e from the
    exact activation, the exact product is off by |W| e more; ReLU is 1-Lipschitz.  So
        e_1 = gamma_{K1+1} (|W_1| |x| + |b_1|)                         (x: the recorded fp32 observation, exact; K1 = S padded to 8)
        e_{l+1} = |W_{l+1}| e_l + gamma_{H+1} (|W_{l+1}| (|h_l| + e_l) + |b_{l+1}|)     (the head the same way)."""
    h, e = x, torch.zeros_like(x)
    for li, (W, b) in enumerate(layers):
        K = k1 if li == 0 else W.shape[1]
        Wa = W.abs()
        z = h @ W.t() + b
        e = e @ Wa.t() + gamma(K + 1) * ((h.abs() + e) @ Wa.t() + b.abs())
        h = torch.relu(z) if li + 1 < len(layers) else z
    return h, e


def bf16_rne(z):
    """Round fp64 values to bf16 (8 significant bits), nearest-even, in one step (z = m 2^e, 0.5 <= |m| < 1: m * 256 is exact)."""
    m, e = torch.frexp(z)
    return torch.ldexp(torch.round(m * 256.0), (e - 8).to(z.dtype))


def bf16_ulp(v):
    """Twice the spacing of bf16 values at magnitude v >= 0 (v = m 2^e, 0.5 <= m < 1: spacing 2^(e-8)); the factor two covers the
    larger spacing above a power of two."""
    _, e = torch.frexp(v.clamp_min(2.0 ** -120))
    return torch.ldexp(torch.ones_like(v), (e - 7).to(v.dtype))


def bf16_mean_and_bound(layers, x):
    """fp64 forward with the bf16 kernel's own roundings, and a rigorous bound on the kernel's error.
    The kernel: input and weights rounded to bf16 (nearest-even; FragmentStream converts the fp32 masters, the state is cast with
    (__bf16)), biases fp32 in the accumulators, v_mfma_f32_32x32x16_bf16 (bf16 x bf16 products are exact in fp32) summing
    K = 32 (the padded first layer) or H terms plus the bias in fp32, then relu_pack_bf16: ONE v_cvt_pk_bf16_f32 (nearest-even)
    and a clamp of the packed halves, i.e. h = relu(bf16_rne(acc)).  The head is summed in fp32 and never rounded to bf16.
    Reference: the same, every sum exact.  Error: the accumulation term E_l = |W_l| d_{l-1} + gamma_{K+1} (|W_l| (|h_{l-1}| +
    d_{l-1}) + |b_l|) bounds |acc_kernel - z_ref|.  Rounding is monotone, so where bf16_rne(z - E) == bf16_rne(z + E) the kernel
    rounds to the reference's bf16 value exactly (d_l = 0: no flip possible, none allowed); elsewhere the two roundings may
    differ, by at most E + one bf16 ulp of |z| + E (d_l).  The head: e = |W| d_L + gamma_{H+1} (|W| (|h_L| + d_L) + |b|)."""
    h = bf16_rne(x)
    d = torch.zeros_like(h)
    flips = 0
    for li, (W, b) in enumerate(layers):
        Wb = W.float().to(torch.bfloat16).double()
        K = 32 if li == 0 else W.shape[1]
        Wa = Wb.abs()
        z = h @ Wb.t() + b
        E = d @ Wa.t() + gamma(K + 1) * ((h.abs() + d) @ Wa.t() + b.abs())
        if li + 1 == len(layers):
            return z, E, flips
        E = E * (1.0 + 1e-12)                                          # (fp64 evaluation of z and E)
        near = bf16_rne(z - E) != bf16_rne(z + E)
        flips += int(near.sum())
        h = torch.relu(bf16_rne(z))
        d = torch.where(near, E + bf16_ulp(z.abs() + E), torch.zeros_like(E))


def check_actions(traj, eps, sigma, mean_fn, k_alive_min=1):
    """Every alive (t, env, a): |act - (mean_ref + sigma eps)| <= bound + the two fp32 roundings of `mean + sigma * eps`
    (rn_mul, rn_add: u (|mean| + e + |sigma eps|) each, with margin)."""
    mask = traj.mask.bool()                                            # [T][n]
    tt, nn = mask.nonzero(as_tuple=True)
    assert tt.numel() >= k_alive_min
    x = traj.obs[:, tt, nn].t().double()                              # [rows][S]: the observation before action t
    out = mean_fn(x)
    mean, e = out[0], out[1]
    A = mean.shape[1]
    se = torch.stack([sigma[k] * eps[k, tt, nn].double() for k in range(A)], dim=1)
    got = traj.act[:, tt, nn].t().double()
    want = mean + se
    bound = e + 2.0 * U * (mean.abs() + e + se.abs()) * (1.0 + 1e-6)
    err = (got - want).abs()
    bad = err > bound
    assert not bool(bad.any()), (f"{int(bad.sum())} of {bad.numel()} actions out of bound; worst err {float(err.max()):.3e} "
                                 f"at bound {float(bound[err.argmax() // A, err.argmax() % A]):.3e}; "
                                 f"first bad (t, env) = {(int(tt[bad.nonzero()[0, 0]]), int(nn[bad.nonzero()[0, 0]]))}")
    return out


def sigmas(eng):
    return [float(v) for v in eng._sigma]


def f32_policy(tg, S, A, hidden, dev, seed):
    torch.manual_seed(seed)
    return tg.GaussianActor_NeuralNetwork(S, A, hidden, cov=0.3, device=dev)


# ------------------------------------------------------------------------------------------------------------------------------
# the draw helper itself
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["f32x16", "f32x32", "bf16"])
def test_recovered_draws_are_the_fused_kernels_draws(tg, dev, kernel):
    """With every actor weight and bias zero the mean is exactly 0, and with cov = 1 sigma is exactly 1: the fused kernels record
    rn_add(0, rn_mul(1, eps)) == eps itself, at every alive (t, env).  The helper must reproduce those bits (step 0 included)."""
    name, T, G, Eps = "QuadPole", 24, 3, 43
    S, A = DIMS[name]
    hidden = (128, 128) if kernel != "bf16" else (256, 256)
    torch.manual_seed(0)
    pol = tg.GaussianActor_NeuralNetwork(S, A, hidden, cov=1.0, device=dev)
    with torch.no_grad():
        for p in pol.actor.parameters():
            p.zero_()
    cdt = torch.bfloat16 if kernel == "bf16" else None
    eng = tg.DeviceRollout(make_env(tg, name, T), pol, G, Eps, seed=31, compute_dtype=cdt, fused=True)
    if kernel != "bf16":
        eng.f32_block_envs = 16 if kernel == "f32x16" else 32
    assert eng.fused and eng._fused_f32 == (kernel != "bf16") and sigmas(eng) == [1.0] * A
    tr = eng.run()
    eps = philox_draws(tg, make_env(tg, name, T), pol, G, Eps, 31, dev)
    m = tr.mask.bool()
    assert bool(m[0].all())
    assert torch.equal(tr.act[:, 0, :], eps[:, 0, :])                  # the step-0 draw of a real rollout
    assert torch.equal(tr.act[:, m], eps[:, m])                        # ... and every later one
    assert float(eps[:, m].std()) > 0.9


# ------------------------------------------------------------------------------------------------------------------------------
# fp32 kernel: all 64 instantiations against fp64
# ------------------------------------------------------------------------------------------------------------------------------
F32_SHAPES = [(H,) * L for H in (64, 128) for L in (1, 2, 3, 4)]


@pytest.mark.parametrize("block_envs", [16, 32])
@pytest.mark.parametrize("hidden", F32_SHAPES, ids=lambda h: f"{h[0]}x{len(h)}")
@pytest.mark.parametrize("name", ENVS)
def test_fused_f32_actor_matches_fp64_at_every_step(tg, dev, name, hidden, block_envs):
    """tg_fused_rollout_f32, every (env, width, depth, block size) it instantiates, 129 envs (a ragged last workgroup for both
    block sizes), T = 24: each recorded action within the fp32 forward-error bound of the fp64 actor on the recorded state."""
    S, A = DIMS[name]
    T, G, Eps = 24, 3, 43
    pol = f32_policy(tg, S, A, hidden, dev, seed=100 + len(hidden) + hidden[0])
    eng = tg.DeviceRollout(make_env(tg, name, T), pol, G, Eps, seed=41)
    eng.f32_block_envs = block_envs
    assert eng.fused and eng._fused_f32
    tr = eng.run()
    assert eng._frag.block_envs == block_envs
    eps = philox_draws(tg, make_env(tg, name, T), pol, G, Eps, 41, dev)
    layers = actor_layers(pol)
    k1 = (S + 7) // 8 * 8
    check_actions(tr, eps, sigmas(eng), lambda x: f32_mean_and_bound(layers, x, k1), k_alive_min=G * Eps * 2)


@pytest.mark.parametrize("block_envs", [16, 32])
def test_fused_f32_split_launch_matches_fp64(tg, dev, block_envs):
    """[0, 13) then [13, T) in two launches: the second launch picks its states up from the recorded observations; its actions
    are held to the fp64 bound, and the whole trajectory equals one launch."""
    name, hidden = "QuadPole", (128, 128, 128)
    S, A = DIMS[name]
    T, G, Eps = 24, 3, 43
    pol = f32_policy(tg, S, A, hidden, dev, seed=7)
    whole = tg.DeviceRollout(make_env(tg, name, T), pol, G, Eps, seed=42)
    whole.f32_block_envs = block_envs
    ref = [x.clone() for x in (lambda t: (t.obs, t.act, t.rew, t.mask, t.len))(whole.run())]
    split = tg.DeviceRollout(make_env(tg, name, T), pol, G, Eps, seed=42)
    split.f32_block_envs = block_envs
    split._seed_host, split._stream_host = 42, 0
    with torch.cuda.device(dev):
        split._enqueue_prepare(None)
        split._enqueue_fused(0, 13)
        split.rng[1] -= 1                                  # _enqueue_fused advanced the stream id; the same rollout continues
        split._enqueue_fused(13, T)
    torch.cuda.synchronize()
    tr = split.traj
    assert bool(tr.mask[13:].any())
    eps = philox_draws(tg, make_env(tg, name, T), pol, G, Eps, 42, dev)
    layers = actor_layers(pol)
    check_actions(tr, eps, sigmas(split), lambda x: f32_mean_and_bound(layers, x, 24))
    for a, b in zip((tr.obs, tr.act, tr.rew, tr.mask, tr.len), ref):
        assert torch.equal(a, b)


@pytest.mark.parametrize("agents,block_envs,G,Eps", [(2, 16, 3, 7), (16, 16, 2, 3), (32, 32, 3, 1)])
def test_fused_f32_swarm_actor_matches_fp64(tg, dev, agents, block_envs, G, Eps):
    """QuadPoleSwarm on the fp32 kernel: a swarm's bodies are consecutive env slots of the workgroup; each body's actor is the
    fp64 actor of its own recorded state."""
    T, S, A = 24, 20, 4
    pol = f32_policy(tg, S, A, (128, 128), dev, seed=9)
    mk = lambda: tg.QuadPoleSwarm(n_agents=agents, max_steps=T)
    eng = tg.DeviceRollout(mk(), pol, G, Eps, seed=43)
    eng.f32_block_envs = block_envs
    tr = eng.run()
    assert eng._fused_f32 and eng._frag.block_envs == block_envs and tr.n == G * Eps * agents
    eps = philox_draws(tg, mk(), pol, G, Eps, 43, dev)
    layers = actor_layers(pol)
    check_actions(tr, eps, sigmas(eng), lambda x: f32_mean_and_bound(layers, x, 24))
    per_env = tr.len.view(-1, agents)
    assert torch.equal(per_env, per_env[:, :1].expand_as(per_env))


def test_fused_f32_refuses_a_swarm_wider_than_its_block(tg, dev):
    """32 bodies do not fit a 16-env workgroup: the launch is refused by the library (set_error -> _native.check), nothing runs."""
    T = 16
    pol = f32_policy(tg, 20, 4, (128, 128), dev, seed=9)
    eng = tg.DeviceRollout(tg.QuadPoleSwarm(n_agents=32, max_steps=T), pol, 2, 1, seed=44)
    eng.f32_block_envs = 16
    with pytest.raises(RuntimeError, match="tg_fused_rollout_f32.*agents=32"):
        eng.run()
    torch.cuda.synchronize()
    assert not bool(eng.traj.mask.any()) and not bool(eng.traj.act.any())


# ------------------------------------------------------------------------------------------------------------------------------
# bf16 kernel against the fp64 forward with the kernel's own roundings
# ------------------------------------------------------------------------------------------------------------------------------
def staggered_initial_states(tg, name, T, G, Eps, dev, seed):
    """Initial states drawn by the env's own reset, then pushed out along x at speeds spread from 0 to 12 (CartPole) / 16
    (QuadPole) m/s, shuffled over the envs: episodes end at every step from ~5 on, and some run to the horizon."""
    eng = tg.DeviceRollout(make_env(tg, name, T), f32_policy(tg, *DIMS[name], (64,), dev, seed=1), G, Eps, seed=seed,
                           fused=False, use_graph=False)
    eng._seed_host, eng._stream_host = seed, 0
    with torch.cuda.device(dev):
        eng._enqueue_prepare(None)
    init = eng.traj.obs[:, 0, :].t().clone()                            # [n][S]
    n = init.shape[0]
    g = torch.Generator().manual_seed(seed)
    v = torch.linspace(0.0, 12.0 if name == "CartPole" else 16.0, n)[torch.randperm(n, generator=g)]
    vi = 1 if name == "CartPole" else 3
    init[:, 0] = 0.0
    init[:, vi] = v.to(dev)
    return init.cpu().numpy()


BF16_CASES = [(name, H, L) for name in ENVS for H in (128, 256) for L in (1, 2, 3, 5)]


def _bf16_case(tg, dev, name, H, L, G, Eps, T, seed, late):
    """One tg_fused_rollout run of an (H,) * L bf16 policy; CartPole and QuadPole start from staggered states, and the test asserts
    its own premise: some episodes end before the first compaction (t = 8), some are still running after t = `late`."""
    S, A = DIMS[name]
    torch.manual_seed(200 + H + L)
    pol = tg.GaussianActor_NeuralNetwork(S, A, (H,) * L, cov=0.3, device=dev)
    eng = tg.DeviceRollout(make_env(tg, name, T), pol, G, Eps, seed=seed, compute_dtype=torch.bfloat16, fused=True)
    assert eng.fused and not eng._fused_f32
    staggered = name in ("CartPole", "QuadPole")
    tr = eng.run(initial_states=staggered_initial_states(tg, name, T, G, Eps, dev, seed) if staggered else None)
    if staggered:
        assert int((tr.len < 8).sum()) > 0 and int((tr.len > late).sum()) > 0, tr.len.bincount()
    eps = philox_draws(tg, make_env(tg, name, T), pol, G, Eps, seed, dev)
    layers = actor_layers(pol)
    check_actions(tr, eps, sigmas(eng), lambda x: bf16_mean_and_bound(layers, x))
    # every env's record is its own across the compactions: lengths match the masks, and the teacher-forced replay of the recorded
    # initial states and actions (same fp32 dynamics code) reproduces every observation, reward and mask
    fo, fa, fr, fm, fl = (x.clone() for x in (tr.obs, tr.act, tr.rew, tr.mask, tr.len))
    assert torch.equal(fm.sum(0, dtype=torch.int32), fl) and bool((fl > 0).all())
    plain = tg.DeviceRollout(make_env(tg, name, T), pol, G, Eps, seed=seed, fused=False, use_graph=False)
    replay = plain.run(initial_states=fo[:, 0, :].t().cpu().numpy(), forced_actions=fa.permute(2, 1, 0).cpu().numpy())
    assert torch.equal(replay.len, fl) and torch.equal(replay.mask, fm)
    assert torch.equal(replay.obs, fo) and torch.equal(replay.rew, fr)
    return tr


@pytest.mark.parametrize("name,H,L", BF16_CASES, ids=[f"{n}-{h}x{l}" for n, h, l in BF16_CASES])
def test_fused_bf16_actor_matches_fp64_at_every_step(tg, dev, name, H, L):
    """tg_fused_rollout at 600 envs (4-wave variant, 128 envs per workgroup: four full workgroups and a ragged one), T = 48."""
    tr = _bf16_case(tg, dev, name, H, L, G=3, Eps=200, T=48, seed=51, late=24)
    assert tr.n < 32768 and tr.n % 128 != 0


@pytest.mark.parametrize("name,H,L", [("CartPole", 256, 2), ("QuadPole", 128, 3)])
def test_fused_bf16_actor_matches_fp64_in_the_8_wave_variant(tg, dev, name, H, L):
    """32,968 envs: the 8-wave variant (256 envs per workgroup, the last one ragged), T = 16: one compaction."""
    tr = _bf16_case(tg, dev, name, H, L, G=8, Eps=4121, T=16, seed=52, late=12)
    assert tr.n >= 32768 and tr.n % 256 != 0


# ------------------------------------------------------------------------------------------------------------------------------
# shard invariance across the variant thresholds
# ------------------------------------------------------------------------------------------------------------------------------
def _cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def _assert_shards_equal_whole(tg, mk, pol, G, Eps, splits, dev, **kw):
    whole = tg.DeviceRollout(mk(), pol, G, Eps, seed=61, **kw)
    wt = whole.run()
    ref = [x.clone() for x in (wt.obs, wt.act, wt.rew, wt.mask, wt.len)]
    engines = [whole]
    for k in splits:
        per = G // k
        for r in range(k):
            part = tg.DeviceRollout(mk(), pol, per, Eps, seed=61, group_offset=r * per, global_groups=G, **kw)
            pt = part.run()
            sl = slice(r * per * part.E, (r + 1) * per * part.E)
            assert torch.equal(pt.len, ref[4][sl]) and torch.equal(pt.mask, ref[3][:, sl]), (k, r)
            assert torch.equal(pt.obs, ref[0][:, :, sl]) and torch.equal(pt.act, ref[1][:, :, sl]), (k, r)
            assert torch.equal(pt.rew, ref[2][:, sl]), (k, r)
            engines.append(part)
            del part, pt
    return engines


def test_fused_f32_shards_equal_the_whole_rollout_across_the_block_threshold(tg, dev):
    """G E = 2 x 16 x CUs fp32 envs: one engine takes 32 envs per workgroup; a half or a quarter of them alone would take 16.  The
    shards (group_offset, global_groups) must use the whole rollout's kernel and reproduce its trajectory bit for bit."""
    lib = tg._native.load()
    n_total = 2 * 16 * _cus(dev)
    assert lib.tg_fused_rollout_f32_block_envs(n_total // 2, 1) == 16 and lib.tg_fused_rollout_f32_block_envs(n_total, 1) == 32
    G, T = 8, 16
    Eps = n_total // G
    pol = f32_policy(tg, 5, 1, (128, 128), dev, seed=3)
    engines = _assert_shards_equal_whole(tg, lambda: tg.CartPole(max_steps=T), pol, G, Eps, (2, 4), dev)
    assert all(e.fused and e._fused_f32 for e in engines)
    assert {e._f32_block_envs for e in engines} == {32}


def test_fused_bf16_shards_equal_the_whole_rollout_across_the_wave_threshold(tg, dev):
    """65,536 bf16 envs: one engine takes the 8-wave variant (n >= 32,768), a quarter or an eighth of them the 4-wave one.  The two
    variants compute an env's column with the same products in the same order (only the env -> workgroup map differs), so the
    shards must reproduce the whole rollout bit for bit."""
    n_total, G, T = 65536, 8, 24
    Eps = n_total // G
    assert n_total >= 32768 and n_total // 4 < 32768
    torch.manual_seed(4)
    pol = tg.GaussianActor_NeuralNetwork(20, 4, (128, 128), cov=0.3, device=dev)
    engines = _assert_shards_equal_whole(tg, lambda: tg.QuadPole(max_steps=T), pol, G, Eps, (4, 8), dev,
                                         compute_dtype=torch.bfloat16)
    assert all(e.fused and not e._fused_f32 for e in engines)


@pytest.mark.parametrize("cdt", [None, torch.bfloat16], ids=["f32", "bf16"])
def test_gemm_path_shards_equal_the_whole_rollout(tg, dev, cdt):
    """The per-step path (GEMM chain + tg_rollout_step) at the fp32 straddle size, split in 2 and 4."""
    n_total, G, T = 2 * 16 * _cus(dev), 8, 8
    Eps = n_total // G
    pol = f32_policy(tg, 20, 4, (128, 128), dev, seed=5)
    engines = _assert_shards_equal_whole(tg, lambda: tg.QuadPole(max_steps=T), pol, G, Eps, (2, 4), dev,
                                         compute_dtype=cdt, fused=False, use_graph=False)
    assert not any(e.fused for e in engines)
