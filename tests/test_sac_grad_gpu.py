"""DeviceActor.rsample / .q_evaluate (csrc/policy_sac_grad.hip) against act() / q_values() bit for bit and against float64 autograd of the
same nets.

Bars (derived, not tuned): every gradient tensor is held to learned_std_fp64.bar: 4x the distance of torch's float32 autograd from the
float64 one, floored at 4 x 2^-23 x max |ref grad|.  Every check prints its figures.  The derivatives of ReLU and of the log-std
clamp are discontinuous and 1 - a^2 cancels for large |u|, so a comparison means something only away from those points: conditions()
asserts that on the float64 reference (the draws of DRAW were chosen on the CPU from it alone, with policy_step_ref.eps), and every
test re-asserts it on the kernel's own eps."""
import copy

import pytest
import torch

import learned_std_fp64 as F
import policy_step_ref as R
from test_policy_step_gpu import DEV

pytestmark = pytest.mark.gpu

# (S, A, H, actor hidden layers, Q hidden layers, activation): tests/test_sac_target_cpu.py's
CASES = [(3, 1, 64, 1, 2, "ReLU"), (10, 2, 128, 3, 1, "Tanh"), (20, 4, 256, 2, 2, "ReLU"), (28, 4, 64, 2, 2, "Tanh")]
ROWS = [1, 64, 70, 130]
CLAMPED = (CASES[1], 17, 8.0)             # the head scaled so that log-std entries leave [-5, 2] while max |u| stays <= 4
BOUNDS = (-5.0, 2.0)
# the draw (rows, loss weights and the actor's seed) per (path, case index, m, head scale) where draw 0 misses conditions(); path "q":
# the critics at a plain action, "pi": the actor path
DRAW = {("q", 0, 64, 1.0): 3, ("q", 0, 70, 1.0): 1, ("q", 0, 130, 1.0): 13, ("q", 2, 64, 1.0): 8, ("q", 2, 70, 1.0): 47, ("q", 2, 130, 1.0): 1913,
        ("pi", 0, 64, 1.0): 3, ("pi", 0, 70, 1.0): 5, ("pi", 0, 130, 1.0): 37, ("pi", 1, 130, 1.0): 1, ("pi", 2, 64, 1.0): 374,
        ("pi", 2, 70, 1.0): 516, ("pi", 2, 130, 1.0): 13919, ("pi", 1, 17, 8.0): 15}


@pytest.fixture(scope="module")
def tg():
    import trajopt_grpo_amd as tg
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return tg


def problem(case, m, scale=1.0, path="pi", draw=None):
    """The nets, rows, loss weights and the actor's seed of a case at m rows, on the CPU in float32 (seeded: the same at every call)."""
    S, A, H, nh_a, nh_q, act = case
    k = CASES.index(case)
    draw = DRAW.get((path, k, m, scale), 0) if draw is None else draw
    nets = [R.make_net(S, H, nh_a, 2 * A, act, seed=31, scale=scale), R.make_net(S + A, H, nh_q, 1, act, seed=32),
            R.make_net(S + A, H, nh_q, 1, act, seed=33)]
    g = torch.Generator().manual_seed(100000 * draw + 1000 * k + m)
    obs, action = torch.randn(m, S, generator=g), torch.tanh(torch.randn(m, A, generator=g))
    return nets, obs, action, [torch.randn(m, generator=g) for _ in range(3)], draw


def q_of(q1, q2, obs, act):
    x = torch.cat([obs, act], dim=-1)
    return q1(x).squeeze(-1), q2(x).squeeze(-1)


def actor_of(actor, obs, eps):
    """tools/vec_env_sac.py's Actor.forward on a given draw -> action, logp, and (u, pre-clamp log-std) for conditions()."""
    mu, raw = actor(obs).split(eps.shape[1], dim=-1)
    ls = raw.clamp(*BOUNDS)
    u = mu + ls.exp() * eps
    a = torch.tanh(u)
    logp = (-0.5 * ((u - mu) / ls.exp()).pow(2) - ls - R.HALF_LOG_2PI).sum(-1)
    return a, logp - torch.log(1.0 - a.pow(2) + 1e-6).sum(-1), u, raw


def relu_margin(net, x):
    """Smallest |hidden pre-activation| / the layer's largest over the hidden layers of a ReLU net (inf for a Tanh net)."""
    h, worst = x, float("inf")
    for mod in net:
        if isinstance(mod, torch.nn.ReLU):
            worst = min(worst, float(h.abs().min() / h.abs().max()))
        h = mod(h)
    return worst


def conditions(nets, obs, action, eps=None):
    """The kink conditions in float64: with `eps` on the actor path and the critics on [obs, a], else on the critics at `action`."""
    nets = [copy.deepcopy(n).double() for n in nets]
    with torch.no_grad():
        margin = float("inf")
        if eps is not None:
            action, _, u, raw = actor_of(nets[0], obs.double(), eps.double())
            assert float(u.abs().max()) <= 4.0, "1 - a^2 would cancel in float32"
            assert float(torch.min((raw - BOUNDS[0]).abs(), (raw - BOUNDS[1]).abs()).min()) > 1e-3, "a log-std on a clamp bound"
            margin = relu_margin(nets[0], obs.double())
        x = torch.cat([obs.double(), action.double()], dim=-1)
        assert min(margin, relu_margin(nets[1], x), relu_margin(nets[2], x)) > 2.0 ** -16, "a ReLU pre-activation on its kink"
    return raw if eps is not None else None


def reference(nets, obs, action, w, eps, dtype, device):
    """torch autograd in `dtype` on `device` of sum(c logp) + sum(d1 q1) + sum(d2 q2) with a = the actor's draw on `eps`, or -- eps None
    -- of sum(c q1) + sum(d1 q2) at the leaf `action` -> (parameter gradients [actor's (actor path only), Q1's, Q2's], action.grad)."""
    nets = [copy.deepcopy(n).to(device=device, dtype=dtype) for n in nets]
    obs, *w = (t.to(device=device, dtype=dtype) for t in (obs, *w))
    if eps is None:
        action = action.to(device=device, dtype=dtype).requires_grad_(True)
        q1, q2 = q_of(nets[1], nets[2], obs, action)
        ((w[0] * q1).sum() + (w[1] * q2).sum()).backward()
    else:
        a, logp, _, _ = actor_of(nets[0], obs, eps.to(device=device, dtype=dtype))
        q1, q2 = q_of(nets[1], nets[2], obs, a)
        ((w[0] * logp).sum() + (w[1] * q1).sum() + (w[2] * q2).sum()).backward()
    grads = [p.grad for n in nets[0 if eps is not None else 1:] for p in n.parameters()]
    return [g.detach().double().cpu() for g in grads], (action.grad.double().cpu() if eps is None else None)


def device_actor(tg, nets, m, seed, grid_limit=0):
    nets = [n.to(DEV) for n in nets]
    da = tg.DeviceActor(nets[0], q_nets=nets[1:], num_envs=m, head="squashed", log_std_bounds=BOUNDS, seed=seed, device=DEV)
    da._grid_limit = grid_limit
    return da, nets


def assert_grads(tag, got, ref64, ref32):
    for k, (g, r64, r32) in enumerate(zip(got, ref64, ref32)):
        b, err32 = F.bar(r64, r32)
        err = float((g.detach().double().cpu() - r64).abs().max())
        print(f"{tag} grad[{k}] {tuple(r64.shape)}: native err {err:.3e}  torch-fp32 err {err32:.3e}  bar {b:.3e}")
        assert err <= b, (tag, k, err, b)


every = pytest.mark.parametrize("case,m", [(c, m) for c in CASES for m in ROWS], ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))


@every
def test_forwards_are_act_and_q_values_bit_for_bit(tg, case, m):
    nets, obs, action, _, seed = problem(case, m)
    da, nets = device_actor(tg, nets, m, seed, 2 if m == 130 else 0)
    twin, _ = device_actor(tg, nets, m, seed, 2 if m == 130 else 0)
    obs, action = obs.to(DEV), action.to(DEV)
    for _ in range(2):                                                 # the second call draws the next counter
        a, logp = da.rsample(obs)
        ta, tlogp, _ = twin.act(obs)
        assert a.grad_fn is not None and logp.grad_fn is not None and a.shape == (m, case[1]) and logp.shape == (m,)
        assert torch.equal(a, ta) and torch.equal(logp, tlogp) and torch.equal(da.calls, twin.calls)
    assert not torch.equal(da.eps, torch.zeros_like(da.eps)) and int(da.calls[0]) == 2
    q1, q2 = da.q_evaluate(obs, action)
    r1, r2, _ = twin.q_values(obs, action)
    assert q1.grad_fn is not None and torch.equal(q1, r1) and torch.equal(q2, r2)


@every
def test_critic_and_action_gradients_against_fp64(tg, case, m):
    nets, obs, action, w, seed = problem(case, m, path="q")
    conditions(nets, obs, action)
    g64, a64 = reference(nets, obs, action, w, None, torch.float64, "cpu")
    g32, a32 = reference(nets, obs, action, w, None, torch.float32, DEV)
    da, nets = device_actor(tg, nets, m, seed, 2 if m == 130 else 0)
    obs, action, *w = (t.to(DEV) for t in (obs, action, *w))
    q1, q2 = da.q_evaluate(obs, action)                                # a plain action: the Q parameters alone
    ((w[0] * q1).sum() + (w[1] * q2).sum()).backward()
    assert_grads(f"{case} m={m} critics", [p.grad for n in nets[1:] for p in n.parameters()], g64, g32)
    for n in nets[1:]:
        n.zero_grad(set_to_none=True)
    action.requires_grad_(True)                                        # a leaf action, the parameters left out: the action alone
    q1, q2 = da.q_evaluate(obs, action, detach_params=True)
    ((w[0] * q1).sum() + (w[1] * q2).sum()).backward()
    assert_grads(f"{case} m={m} action", [action.grad], [a64], [a32])
    assert all(p.grad is None for n in nets[1:] for p in n.parameters())


@pytest.mark.parametrize("case,m,scale", [(c, m, 1.0) for c in CASES for m in ROWS] + [CLAMPED], ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_actor_path_gradients_against_fp64(tg, case, m, scale):
    nets, obs, _, w, seed = problem(case, m, scale)
    da, dev_nets = device_actor(tg, copy.deepcopy(nets), m, seed, 2 if m == 130 else 0)
    dobs, *dw = (t.to(DEV) for t in (obs, *w))
    a, logp = da.rsample(dobs)
    q1, q2 = da.q_evaluate(dobs, a)
    ((dw[0] * logp).sum() + (dw[1] * q1).sum() + (dw[2] * q2).sum()).backward()
    eps = da.eps.cpu()
    raw = conditions(nets, obs, None, eps)
    if scale != 1.0:                                                   # a clamped entry's head row gets its gradient through mu alone
        out = (raw < BOUNDS[0]) | (raw > BOUNDS[1])
        assert bool(out.any()) and not bool(out.all())
    g64, _ = reference(nets, obs, None, w, eps, torch.float64, "cpu")
    g32, _ = reference(nets, obs, None, w, eps, torch.float32, DEV)
    assert_grads(f"{case} m={m} scale={scale}", [p.grad for n in dev_nets for p in n.parameters()], g64, g32)


def one_round(tg, case, m, da=None, dev_nets=None):
    nets, obs, _, w, seed = problem(case, m)
    if da is None:
        da, dev_nets = device_actor(tg, nets, m, seed)
    dobs, *dw = (t.to(DEV) for t in (obs, *w))
    a, logp = da.rsample(dobs)
    q1, q2 = da.q_evaluate(dobs, a)
    ((dw[0] * logp).sum() + (dw[1] * q1).sum() + (dw[2] * q2).sum()).backward()
    return da, dev_nets, [p for n in dev_nets for p in n.parameters()], (a, logp, q1, q2)


def test_two_rounds_are_bit_identical_and_a_second_backward_accumulates(tg):
    case, m = CASES[1], 130
    rounds = [[p.grad.clone() for p in one_round(tg, case, m)[2]] for _ in range(2)]
    assert all(torch.equal(a, b) for a, b in zip(*rounds))
    da, dev_nets, params, _ = one_round(tg, case, m)
    da.load_state_dict({**da.state_dict(), "calls": torch.zeros_like(da._calls)})          # the same draw again
    one_round(tg, case, m, da, dev_nets)                               # into the existing .grad: g + g
    assert all(torch.equal(p.grad, r + r) for p, r in zip(params, rounds[0]))


def test_an_in_place_optimizer_step_is_seen_by_the_next_call(tg):
    case, m = CASES[0], 70
    da, dev_nets, params, old = one_round(tg, case, m)
    torch.optim.SGD(params, lr=0.05).step()
    da.load_state_dict({**da.state_dict(), "calls": torch.zeros_like(da._calls)})
    obs = problem(case, m)[1].to(DEV)
    a, logp = da.rsample(obs)
    q1, q2 = da.q_evaluate(obs, a)
    twin, _ = device_actor(tg, dev_nets, m, da.seed)
    ta, tlogp, _ = twin.act(obs)
    assert torch.equal(a, ta) and torch.equal(logp, tlogp) and torch.equal(q1, twin.q_values(obs, ta)[0])
    assert not any(torch.equal(new, was) for new, was in zip((a, logp, q1, q2), old))


def test_what_is_not_built_raises(tg):
    case, m = CASES[0], 64
    nets, obs, action, _, seed = problem(case, m)
    da, nets = device_actor(tg, nets, m, seed)
    obs, action = obs.to(DEV), action.to(DEV)
    with pytest.raises(ValueError, match="no gradient to obs"):
        da.rsample(obs.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="no gradient to obs"):
        da.q_evaluate(obs.clone().requires_grad_(True), action)
    a, logp = da.rsample(obs)
    logp.sum().backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="already backpropagated"):
        logp.sum().backward()
    gaussian = tg.DeviceActor(R.make_net(3, 64, 1, 1, "ReLU", seed=1).to(DEV), num_envs=m, log_std=torch.zeros(1, device=DEV), device=DEV)
    with pytest.raises(ValueError, match="rsample\\(\\) is built for the squashed head"):
        gaussian.rsample(obs)
    with pytest.raises(ValueError, match="q_evaluate\\(\\) needs q_nets"):
        tg.DeviceActor(nets[0], num_envs=m, head="squashed", device=DEV).q_evaluate(obs, action)
