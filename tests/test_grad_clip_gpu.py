"""Global gradient-norm clipping on the GPU (GRPO / PPO `max_grad_norm`): the norm launch against float64, the clipped optimizer
step against `g.mul_(coef); torch.optim.Adam.step()` bit for bit, learn() with a clip that bites at every update against the CPU
oracle stepping an Adam whose step() calls clip_grad_norm_ first, a clip that never bites against no clip bit for bit, the choice of
path, and two ranks against one.  Every case runs once."""
import copy
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import learner as L

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def tg():
    import trajopt_grpo_amd as tg
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return tg


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def n_params(S, A, hidden):
    dims = [S] + list(hidden) + [A]
    return sum(a * b + b for a, b in zip(dims, dims[1:]))


# ------------------------------------------------------------------------------------------------------------------------------
# 1. tg_grad_clip_coef against float64
# ------------------------------------------------------------------------------------------------------------------------------
def _clip_coef(tg, flat, max_norm):
    N = tg._native
    lib, n = N.load(), flat.numel()
    out = torch.full((2,), -7.0, dtype=torch.float32, device=flat.device)
    work = torch.empty(max(int(lib.tg_grad_clip_workspace(n)) // 8, 1), dtype=torch.float64, device=flat.device)
    N.check(lib.tg_grad_clip_coef(flat.data_ptr() if n else None, n, max_norm, out.data_ptr(), work.data_ptr(), N.stream_ptr(flat.device)),
            "tg_grad_clip_coef")
    torch.cuda.synchronize()
    return out.cpu()


SIZES = [1, 63, 64, 255, 256, 257, (1 << 20) + 3, n_params(5, 1, (128, 128)), n_params(20, 4, (256,) * 5) + n_params(20, 1, (256,) * 5)]
FILLS = ["1e-6", "1", "1e6", "one_3e38", "zero"]


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("n", SIZES)
def test_norm_and_coefficient_against_float64(tg, dev, n, fill):
    """Bounds derived, not tuned.  The float64 sum of n squares of float32 values (each product exact) is within n 2^-53 relative;
    sqrt, the rounding of the norm to float32, of max_norm to float32, `+ 1e-6` and the divide each add at most 2^-24 relative:
    |norm - norm64| <= 1 ulp32(norm64), |coef - coef64| <= 4 2^-24 coef64 below the clamp, coef == 1 exactly whenever
    norm64 + 1e-6 <= max_norm (1 - 2^-21).  A clipping and a non-clipping max_norm per buffer; the same bytes give the same bits."""
    g = torch.Generator(device=dev).manual_seed(n + len(fill))
    if fill == "zero":
        x = torch.zeros(n, device=dev)
    elif fill == "one_3e38":                        # (its float32 square overflows; the float64 sum must not)
        x = torch.randn(n, device=dev, generator=g) * 1e-3
        x[n // 2] = 3e38
    else:
        x = torch.randn(n, device=dev, generator=g) * float(fill)
    norm64 = float(np.sqrt(np.sum(x.cpu().numpy().astype(np.float64) ** 2)))
    for max_norm in ((1.0,) if fill == "zero" else (norm64 / 3.7, norm64 * 2.0 + 1e-5)):
        a, b = _clip_coef(tg, x, max_norm), _clip_coef(tg, x, max_norm)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        norm, coef = float(a[0]), float(a[1])
        print(f"n={n} fill={fill} max_norm={max_norm:.9g} norm={norm:.9g} norm64={norm64:.17g} coef={coef:.9g}")
        if fill == "zero":
            assert (norm, coef) == (0.0, 1.0)
            continue
        assert abs(norm - norm64) <= float(np.spacing(np.float32(norm64))), (norm, norm64)
        coef64 = max_norm / (norm64 + 1e-6)
        if norm64 + 1e-6 <= max_norm * (1.0 - 2.0 ** -21):
            assert coef == 1.0
        if coef64 < 1.0:
            assert abs(coef - coef64) <= 4 * 2.0 ** -24 * coef64 and coef <= 1.0, (coef, coef64)


def test_empty_buffer_gives_norm_zero_and_coefficient_one(tg, dev):
    out = _clip_coef(tg, torch.empty(0, device=dev), 2.5)
    assert (float(out[0]), float(out[1])) == (0.0, 1.0)


# ------------------------------------------------------------------------------------------------------------------------------
# 2. the clipped step against torch, bit for bit
# ------------------------------------------------------------------------------------------------------------------------------
def _state(opt, params):
    return [(p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone(), p.grad.clone()) for p in params]


def _assert_same(a, b, what):
    for i, (x, y) in enumerate(zip(a, b)):
        for j, name in enumerate(("param", "exp_avg", "exp_avg_sq", "grad")):
            assert torch.equal(x[j], y[j]), (what, i, name)


@pytest.mark.parametrize("coef", [1.0, 0.37, 1e-4])
def test_clipped_step_is_bit_identical_to_mul_then_torch_adam(tg, dev, coef):
    """tg_adam_step_clip over tensors of mixed sizes, three consecutive steps: parameters, both moments and the gradients left
    behind (zero_grads = 0: g * coef; the middle step zeroes them instead) equal `g.mul_(coef); torch.optim.Adam.step()`; with
    coef == 1 it also equals tg_adam_step."""
    from trajopt_grpo_amd import optim as O
    gen = torch.Generator(device=dev).manual_seed(17)
    shapes = [(1,), (63,), (257,), (128, 128), (70001,), (64, 5)]
    base = [torch.randn(s, device=dev, generator=gen) for s in shapes]
    sets = [[torch.nn.Parameter(t.clone()) for t in base] for _ in range(3)]
    opts = [torch.optim.Adam(ps, lr=3e-4) for ps in sets]
    fused_clip, fused_plain = O.FusedAdam(opts[0]), O.FusedAdam(opts[2])
    c = torch.tensor([coef], dtype=torch.float32, device=dev)
    for it in range(3):
        zero = it == 1
        for k in range(len(shapes)):
            g = torch.randn(shapes[k], device=dev, generator=gen) * (10.0 ** (k - 3))
            for ps in sets:
                ps[k].grad = g.clone()
        assert fused_clip.step(zero_grads=zero, clip_coef=c) and fused_clip.grads_zeroed == zero
        for p in sets[1]:
            p.grad.mul_(c)                              # clip_grad_norm_'s own scaling (a device tensor, float32 product)
        opts[1].step()
        if zero:
            for p in sets[1]:
                p.grad.zero_()
        torch.cuda.synchronize()
        _assert_same(_state(opts[0], sets[0]), _state(opts[1], sets[1]), ("clip vs torch", it))
        if coef == 1.0:
            assert fused_plain.step(zero_grads=zero)
            _assert_same(_state(opts[0], sets[0]), _state(opts[2], sets[2]), ("clip vs tg_adam_step", it))


@pytest.mark.parametrize("coef", [1.0, 0.37, 1e-4])
def test_clipped_step_with_push_keeps_every_layout_current(tg, dev, coef):
    """tg_adam_step_push_clip on an actor-critic (fp32 chain streams): the same bits as mul + torch's step, and every derived
    layout equal to a tg_gather_streams of the stepped weights, over three consecutive steps."""
    from trajopt_grpo_amd import mlp as M, optim as O
    torch.manual_seed(13)
    pol = tg.GaussianActorCritic_NeuralNetwork(5, 1, (128, 128), cov=0.3, device=dev)
    pol_t = copy.deepcopy(pol)
    opt, opt_t = torch.optim.Adam(pol.parameters(), lr=3e-4), torch.optim.Adam(pol_t.parameters(), lr=3e-4)
    gen = torch.Generator(device=dev).manual_seed(5)
    for p, q in zip(pol.parameters(), pol_t.parameters()):
        p.grad = torch.randn(p.shape, device=dev, generator=gen) * 1e-2
        q.grad = p.grad.clone()
    mlps = [M.GemmMLP(pol.actor, torch.float32), M.GemmMLP(pol.critic, torch.float32)]
    fused = O.FusedAdam(opt)
    assert fused.step()
    opt_t.step()
    ref = O.StreamRefresher(fused, mlps)
    for m in mlps:
        m.refresh()
    assert ref.run()
    streams = [m._f32.stream for m in mlps]
    c = torch.tensor([coef], dtype=torch.float32, device=dev)
    for it in range(3):
        # (fresh gradient VALUES in the tensors the optimizer's table already points at: a new tensor would rebuild the tables)
        for p, q in zip(pol.parameters(), pol_t.parameters()):
            p.grad.copy_(torch.randn(p.shape, device=dev, generator=gen) * 1e-2)
            q.grad.copy_(p.grad)
        assert fused.step(zero_grads=False, refresher=ref, clip_coef=c) and fused.pushed
        for q in pol_t.parameters():
            q.grad.mul_(c)
        opt_t.step()
        torch.cuda.synchronize()
        _assert_same(_state(opt, list(pol.parameters())), _state(opt_t, list(pol_t.parameters())), ("push clip vs torch", it))
        pushed = [s.clone() for s in streams]
        assert ref.run()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(pushed, streams)), it


# ------------------------------------------------------------------------------------------------------------------------------
# 3. learn() with a clip that bites at every update, against the oracle
# ------------------------------------------------------------------------------------------------------------------------------
class ClipAdam(torch.optim.Adam):
    """The reference's two-line edit: clip_grad_norm_ between backward() and step().  `norms`: the float64 pre-clip norm of
    every step."""

    def __init__(self, params, max_norm, **kw):
        super().__init__(params, **kw)
        self.max_norm, self.norms = max_norm, []

    def step(self, closure=None):
        ps = [p for g in self.param_groups for p in g["params"]]
        self.norms.append(float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in ps))))
        if self.max_norm is not None:
            torch.nn.utils.clip_grad_norm_(ps, self.max_norm)
        return super().step(closure)


LR = 3e-4
# name -> (algorithm, env, S, A, hidden, activation, compute dtype, G, E, T, batch_size)
LEARN = {
    "grpo_f32_resident": ("grpo", "CartPole", 5, 1, (128, 128), "ReLU", None, 32, 64, 32, None),        # (today's rider path)
    "grpo_f32_chain": ("grpo", "CartPole", 5, 1, (128,) * 4, "ReLU", None, 32, 64, 32, None),
    "ppo_f32_full": ("ppo", "CartPole", 5, 1, (128,) * 3, "ReLU", None, 8, 32, 32, None),
    "ppo_f32_minibatch": ("ppo", "CartPole", 5, 1, (128,) * 3, "ReLU", None, 8, 32, 32, 1024),
    "grpo_bf16_chain": ("grpo", "QuadPole", 20, 4, (256,) * 5, "ReLU", torch.bfloat16, 8, 64, 48, None),
    "grpo_torch_sigmoid": ("grpo", "CartPole", 5, 1, (128, 128), "Sigmoid", None, 32, 64, 32, None),     # (torch autograd fallback)
}


def _oracle_copy(pol, S, A, hidden, act, critic):
    ora = L.OraclePolicy(S, A, hidden, activation=act, cov=0.5, critic=critic)
    sd = pol.state_dict()
    cp = lambda d: {n: v.detach().cpu().clone() for n, v in d.items()}
    ora.load_state_dict({k: cp(v) for k, v in sd.items()} if critic else cp(sd))
    return ora


def _device_order(mask):
    """Row of the device trajectory's valid-row order (time-major) for every row of the reference's order (env-major), as
    test_ppo_minibatch_learn_matches_reference maps them."""
    G, E, T = mask.shape
    m = mask.bool()
    n = int(m.sum())
    ref_pos = torch.full((G * E, T), -1, dtype=torch.long)
    ref_pos[m.reshape(G * E, T)] = torch.arange(n)
    ours = torch.full((n,), -1, dtype=torch.long)
    ours[ref_pos.t()[m.reshape(G * E, T).t()]] = torch.arange(n)
    return ours


def _reference_round(case, ora, old, buf, max_norm, opt=None):
    """One learn() of the reference on `buf`, stepping a ClipAdam (`opt`: the one of the previous round, its moments and step
    counts carried on as the learner's optimizer carries them): (J / total loss of every step, the optimizer with the norms this
    round recorded, the minibatch permutations in the reference's row order)."""
    algo_name, bs = LEARN[case][0], LEARN[case][10]
    perms = None
    if bs is not None:
        n = int(buf.group_masks.sum())
        gen = torch.Generator().manual_seed(n)
        perms = [torch.randperm(n, generator=gen) for _ in range(2)]
    if opt is None:
        opt = ClipAdam(ora.parameters(), max_norm, lr=LR)
    opt.norms = []
    args = (buf.group_observations, buf.group_actions, buf.group_rewards, buf.group_masks)
    if algo_name == "grpo":
        stats = L.grpo_learn(ora, old, opt, *args, epsilon=0.2, gamma=0.99, updates_per_iter=2)
    else:
        logs = L.ppo_learn(ora, opt, *args, epsilon=0.2, gamma=0.99, updates_per_iter=2, batch_size=bs, permutations=perms)
        stats = [l["total"] for l in logs]
    return stats, opt, perms


def _setup_case(tg, dev, case, seed):
    algo_name, env_name, S, A, hidden, act, cdt, G, E, T, bs = LEARN[case]
    torch.manual_seed(seed)
    cls = tg.GaussianActorCritic_NeuralNetwork if algo_name == "ppo" else tg.GaussianActor_NeuralNetwork
    pol = cls(S, A, hidden, activation=act, cov=0.5, device=dev)
    env_cls = getattr(tg, env_name)
    mgr = tg.RolloutManager(lambda: env_cls(max_steps=T), pol, num_workers=G, num_episodes_per_worker=E, seed=seed + 11,
                            **({"compute_dtype": cdt} if cdt is not None else {}))
    buf = tg.Rollout_Buffer(mgr)
    buf.sample()
    return pol, mgr, buf


def _make_algo(tg, case, pol, max_grad_norm):
    algo_name, _, _, _, _, _, cdt, _, _, _, bs = LEARN[case]
    opt = torch.optim.Adam(pol.parameters(), lr=LR)
    if algo_name == "grpo":
        return tg.GRPO(epsilon=0.2, beta=0.0, gamma=0.99, policy=pol, optimizer=opt, updates_per_iter=2, autocast_dtype=cdt,
                       max_grad_norm=max_grad_norm)
    return tg.PPO(epsilon=0.2, policy=pol, optimizer=opt, ref_model=None, updates_per_iter=2, gamma=0.99, batch_size=bs,
                  autocast_dtype=cdt, max_grad_norm=max_grad_norm)


def _check_against_reference(case, pol, ora, algo, ref_stats, ref_opt, before, steps_so_far, max_norm):
    """Tolerances: those of the existing test of the same path against the same kind of reference.
      fp32 GRPO (resident / chain kernels, torch fallback) -- test_c2_size_grpo_learn_matches_the_oracle: J 2e-4, weights 3e-4 in
        relative L2 and 2 lr per step in the maximum; gradients (norm, final .grad) test_grpo_learn_matches_reference's rtol 2e-3;
      fp32 PPO -- test_learn_at_chain_kernel_shapes_matches_reference (fp32): weights 1e-5 with <= 10 % Adam-amplified outliers of
        at most 2 lr per step, last gradient 5e-2 in L2; losses 1e-4 (test_ppo_learn_on_a_tanh_policy_matches_the_torch_path);
      bf16 chain -- test_grpo_learn_with_a_reference_policy_matches_fp64 (bf16): J 5e-3, weights 2 lr per step in the maximum and
        update cosine > 0.9; gradients test_learn_at_chain_kernel_shapes_matches_reference's bf16 bounds (first 0.2, later 0.35)."""
    algo_name, cdt = LEARN[case][0], LEARN[case][6]
    st = algo.last_stats
    got_stats = st["J"] if algo_name == "grpo" else st["total_loss"]
    norms = st["grad_norm"]
    print(case, "stats", got_stats, ref_stats, "grad_norm", norms, ref_opt.norms, "max_norm", max_norm)
    assert len(norms) == len(ref_opt.norms) == len(got_stats)
    assert all(n > max_norm for n in norms) and all(n > max_norm for n in ref_opt.norms), "every update is meant to be clipped"
    bf16 = cdt is not None
    s_tol = 5e-3 if bf16 else (2e-4 if algo_name == "grpo" else 1e-4)
    for a, b in zip(got_stats, ref_stats):
        assert abs(a - b) <= s_tol * max(1.0, abs(b)), (got_stats, ref_stats)
    later = 0.35 if bf16 else (2e-3 if algo_name == "grpo" else 5e-2)
    for i, (a, b) in enumerate(zip(norms, ref_opt.norms)):
        g_tol = 0.2 if (bf16 and i == 0 and steps_so_far == len(norms)) else later
        assert abs(a - b) <= g_tol * b, (i, a, b)
    ref_params, gpu_params = ora.parameters(), list(pol.parameters())
    assert len(ref_params) == len(gpu_params)
    # the gradients left behind are the CLIPPED ones of the last step
    got_g = torch.cat([p.grad.reshape(-1) for p in gpu_params]).double().cpu()
    ref_g = torch.cat([p.grad.reshape(-1) for p in ref_params]).double()
    print(case, "final grad norm", float(got_g.norm()), float(ref_g.norm()), "rel diff", float((got_g - ref_g).norm() / ref_g.norm()))
    assert float(got_g.norm()) <= max_norm * (1 + 1e-5)
    assert float((got_g - ref_g).norm()) <= later * float(ref_g.norm())
    for i, (p, q, p0) in enumerate(zip(gpu_params, ref_params, before)):
        got, want = p.detach().double().cpu(), q.detach().double()
        d = (got - want).abs()
        print(case, "tensor", i, "max", float(d.max()), "rel", float((got - want).norm() / (want.norm() + 1e-12)),
              "frac>1e-5", float((d > 1e-5).double().mean()))
        assert float(d.max()) <= 2 * steps_so_far * LR + 1e-6, (i, float(d.max()))
        if bf16:
            dg, dw = (got - p0).reshape(-1), (want - p0).reshape(-1)
            assert float(torch.dot(dg, dw) / (dg.norm() * dw.norm() + 1e-30)) > 0.9, i
        elif algo_name == "grpo":
            assert float((got - want).norm() / (want.norm() + 1e-12)) < 3e-4, i
        else:
            assert float((d > 1e-5).double().mean()) <= 0.10, i
        assert not torch.equal(got, p0), i


@pytest.mark.parametrize("case", list(LEARN))
def test_learn_with_a_biting_clip_matches_the_clipping_reference(tg, dev, case):
    """max_grad_norm = a quarter of the smallest pre-clip norm an UNCLIPPED reference run sees; then the reference (oracle.learner
    on the CPU, stepping ClipAdam) and GRPO / PPO(max_grad_norm=...) learn from the same buffer and the same weights.  A second
    rollout + learn() round follows on the fp32 GRPO resident case: the rollout and the learner read layouts that the clipped
    step's own launch wrote."""
    algo_name, _, S, A, hidden, act, cdt, _, _, _, bs = LEARN[case]
    critic = algo_name == "ppo"
    pol, mgr, buf = _setup_case(tg, dev, case, seed=3)
    torch.set_num_threads(8)
    probe = _oracle_copy(pol, S, A, hidden, act, critic)
    _, probe_opt, _ = _reference_round(case, probe, copy.deepcopy(probe), buf, None)
    max_norm = min(probe_opt.norms) / 4.0
    ora = _oracle_copy(pol, S, A, hidden, act, critic)
    old = copy.deepcopy(ora)
    before = [p.detach().double().cpu().clone() for p in pol.parameters()]
    algo = _make_algo(tg, case, pol, max_norm)
    steps, ref_opt = 0, None
    for r in range(2 if case == "grpo_f32_resident" else 1):
        if r > 0:
            buf.sample()
        ref_stats, ref_opt, perms = _reference_round(case, ora, old, buf, max_norm, ref_opt)
        if perms is not None:
            order = _device_order(buf.group_masks)
            it = iter([order[p] for p in perms])
            algo.permutation_fn = lambda n, device: next(it).to(device)
        algo.learn(buf)
        torch.cuda.synchronize()
        steps += len(ref_opt.norms)
        m = algo._mlp(pol.actor)
        if act == "Sigmoid":
            assert m is None
        elif cdt is not None:
            assert m._chain is not None and m._bchain is not None
        else:
            assert m._f32 is not None and algo._fused_adam.pushed
        _check_against_reference(case, pol, ora, algo, ref_stats, ref_opt, before, steps, max_norm)


# ------------------------------------------------------------------------------------------------------------------------------
# 4. a clip that never bites is the unclipped run, bit for bit
# ------------------------------------------------------------------------------------------------------------------------------
NEVER = {"grpo_5-128-128-1": ("grpo", "CartPole", 5, 1, (128, 128), 16, 32, 60), "ppo_20-256x5": ("ppo", "QuadPole", 20, 4, (256,) * 5, 4, 32, 48)}


@pytest.mark.parametrize("case", list(NEVER))
def test_a_clip_that_never_bites_is_the_unclipped_run_bit_for_bit(tg, dev, case):
    """max_grad_norm = 1e30 against None, same seed, same buffer, two learn() calls: the coefficient is exactly 1 and g * 1.0f == g,
    so every parameter, both Adam moments and the final .grad are identical (GRPO's unclipped run takes the rider launch, which is
    bit-identical to the separate step)."""
    algo_name, env_name, S, A, hidden, G, E, T = NEVER[case]

    def run(max_grad_norm):
        torch.manual_seed(33)
        cls = tg.GaussianActorCritic_NeuralNetwork if algo_name == "ppo" else tg.GaussianActor_NeuralNetwork
        pol = cls(S, A, hidden, cov=0.5, device=dev)
        env_cls = getattr(tg, env_name)
        mgr = tg.RolloutManager(lambda: env_cls(max_steps=T), pol, num_workers=G, num_episodes_per_worker=E, seed=5)
        buf = tg.Rollout_Buffer(mgr)
        opt = torch.optim.Adam(pol.parameters(), lr=1e-3)
        if algo_name == "grpo":
            algo = tg.GRPO(epsilon=0.15, beta=0.0, gamma=0.9, policy=pol, optimizer=opt, updates_per_iter=3, max_grad_norm=max_grad_norm)
        else:
            algo = tg.PPO(epsilon=0.2, policy=pol, optimizer=opt, ref_model=None, updates_per_iter=3, gamma=0.99, batch_size=None,
                          max_grad_norm=max_grad_norm)
        for _ in range(2):
            buf.sample()
            algo.learn(buf)
        torch.cuda.synchronize()
        out = {}
        for i, p in enumerate(pol.parameters()):
            st = opt.state[p]
            out[f"p{i}"], out[f"g{i}"], out[f"m{i}"], out[f"v{i}"] = p.detach().clone(), p.grad.clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone()
        return out, dict(algo.last_stats)

    (a, sa), (b, sb) = run(None), run(1e30)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert "grad_norm" not in sa and len(sb.pop("grad_norm")) == 3 and sa == sb


# ------------------------------------------------------------------------------------------------------------------------------
# 5. path choice
# ------------------------------------------------------------------------------------------------------------------------------
def test_rider_only_without_a_clip_and_fused_step_with_one(tg, dev, monkeypatch):
    """One rank, GRPO 5-128-128-1 fp32.  Without max_grad_norm the optimizer step still rides on the gradient reduction and
    last_stats has no "grad_norm"; with one no rider is asked for, the fused step (tg_adam_step_push_clip) runs and keeps the
    layouts current, and the statistics carry one norm per update."""
    from trajopt_grpo_amd import optim as O
    lib = tg._native.load()
    names = ["tg_adam_step", "tg_adam_step_push", "tg_adam_step_clip", "tg_adam_step_push_clip", "tg_grad_clip_coef"]
    calls, rides = [], []
    for n in names:
        monkeypatch.setattr(lib, n, (lambda *a, _f=getattr(lib, n), _n=n: (calls.append(_n), _f(*a))[1]))
    orig_rider = O.FusedAdam.rider

    def counting(self, *a, **k):
        r = orig_rider(self, *a, **k)
        rides.append(r is not None)
        return r

    monkeypatch.setattr(O.FusedAdam, "rider", counting)
    for max_grad_norm in (None, 0.5):
        torch.manual_seed(2)
        pol = tg.GaussianActor_NeuralNetwork(5, 1, (128, 128), cov=0.5, device=dev)
        mgr = tg.RolloutManager(lambda: tg.CartPole(max_steps=32), pol, num_workers=4, num_episodes_per_worker=16, seed=6)
        buf = tg.Rollout_Buffer(mgr)
        buf.sample()
        algo = tg.GRPO(epsilon=0.15, beta=0.0, gamma=0.9, policy=pol, optimizer=torch.optim.Adam(pol.parameters(), lr=3e-4),
                       updates_per_iter=3, max_grad_norm=max_grad_norm)
        calls.clear()
        rides.clear()
        algo.learn(buf)
        torch.cuda.synchronize()
        m = algo._mlp(pol.actor)
        assert m._f32 is not None and "f32" not in m._stale
        if max_grad_norm is None:
            assert calls == ["tg_adam_step"] and rides == [False, True, True], (calls, rides)
            assert isinstance(algo._adam_rider(pol.actor, last=False, whole_update=True), tg._native.AdamRider)
            assert "grad_norm" not in algo.last_stats
        else:
            assert rides == [] and algo._adam_rider(pol.actor, last=False, whole_update=True) is None
            assert calls == ["tg_grad_clip_coef", "tg_adam_step_clip", "tg_grad_clip_coef", "tg_adam_step_push_clip",
                             "tg_grad_clip_coef", "tg_adam_step_push_clip"], calls
            assert algo._fused_adam.pushed and len(algo.last_stats["grad_norm"]) == 3
            assert all(n > 0.5 for n in algo.last_stats["grad_norm"])


def test_an_optimizer_the_fused_step_does_not_take_is_clipped_through_the_bucket(tg, dev):
    """AdamW keeps torch's own step(): the flat bucket is scaled by the device-side coefficient first.  Against the same learner
    without max_grad_norm stepping an AdamW whose step() calls clip_grad_norm_ itself."""
    class ClipAdamW(torch.optim.AdamW):
        def step(self, closure=None):
            torch.nn.utils.clip_grad_norm_([p for g in self.param_groups for p in g["params"]], 0.05)
            return super().step(closure)

    out = []
    for own in (True, False):
        torch.manual_seed(4)
        pol = tg.GaussianActor_NeuralNetwork(5, 1, (128, 128), cov=0.5, device=dev)
        mgr = tg.RolloutManager(lambda: tg.CartPole(max_steps=32), pol, num_workers=4, num_episodes_per_worker=16, seed=6)
        buf = tg.Rollout_Buffer(mgr)
        buf.sample()
        opt = torch.optim.AdamW(pol.parameters(), lr=3e-4) if own else ClipAdamW(pol.parameters(), lr=3e-4)
        algo = tg.GRPO(epsilon=0.15, beta=0.0, gamma=0.9, policy=pol, optimizer=opt, updates_per_iter=3,
                       max_grad_norm=0.05 if own else None)
        algo.learn(buf)
        torch.cuda.synchronize()
        if own:
            assert all(n > 0.05 for n in algo.last_stats["grad_norm"])
        out.append(([p.detach().clone() for p in pol.parameters()], [p.grad.clone() for p in pol.parameters()]))
    # torch's clip_grad_norm_ takes its norm in float32 and multiplies by reciprocal * max_norm: the two coefficients agree to a
    # few float32 roundings (1e-6), and so do the clipped gradients; AdamW's normalised step moves a weight by at most lr per step
    for a, b in zip(out[0][1], out[1][1]):
        assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max())
    for a, b in zip(out[0][0], out[1][0]):
        assert float((a - b).abs().max()) <= 2 * 3 * 3e-4 + 1e-6


# ------------------------------------------------------------------------------------------------------------------------------
# 6. ranks
# ------------------------------------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_ranks_with_a_clip_equal_one_rank_with_the_same_clip(tmp_path):
    """tests/grad_clip_dist_worker.py as fresh child processes (the harness of test_distributed_gpu.py: gloo, both ranks on cuda:0,
    half the groups each): the norm is taken after the all-reduce, so both ranks report bit-identical norms and weights, every
    update is clipped, and the weights equal the one-rank run's to that harness's 1e-6 (relative L2)."""
    worker = os.path.join(HERE, "grad_clip_dist_worker.py")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="2")
    procs, outs = [], {}
    for world in (1, 2):
        port = _free_port()
        outs[world] = [str(tmp_path / f"w{world}_r{r}.pt") for r in range(world)]
        for r in range(world):
            procs.append(subprocess.Popen([sys.executable, worker, str(r), str(world), str(port), outs[world][r]],
                                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env))
    for p in procs:
        try:
            log, _ = p.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            pytest.fail("a rank did not finish in 300 s")
        assert p.returncode == 0, log.decode("utf-8", "replace")[-3000:]
    one = torch.load(outs[1][0], weights_only=False)
    two = [torch.load(f, weights_only=False) for f in outs[2]]
    for case, rec in one.items():
        a, b = two[0][case], two[1][case]
        print(case, "grad_norm", rec["grad_norm"], a["grad_norm"], "max_norm", rec["max_grad_norm"])
        assert a["grad_norm_bits"] == b["grad_norm_bits"] and all(torch.equal(x, y) for x, y in zip(a["weights"], b["weights"]))
        assert len(rec["grad_norm"]) == len(a["grad_norm"]) > 0
        for r_ in (rec, a):
            assert all(n > r_["max_grad_norm"] for n in r_["grad_norm"]), "every update is meant to be clipped"
        for x, y in zip(a["grad_norm"], rec["grad_norm"]):
            assert abs(x - y) <= 1e-4 * y, (x, y)             # (the harness's bound on the update of an fp32 learner)
        for x, y in zip(a["weights"], rec["weights"]):
            assert float((x.double() - y.double()).norm()) <= 1e-6 * float(y.double().norm()), case
