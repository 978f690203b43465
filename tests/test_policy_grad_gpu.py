"""DeviceActor.evaluate (tg_policy_eval_forward / _backward / _weight_grad, csrc/policy_grad.hip) against float64 autograd of the same nets.

Bars (derived, not tuned): the forward is held to the policy step's bar (test_policy_step_gpu.bar: 4x torch's own float32 error,
floored at 4 x 2^-23 x max |ref|, plus 4u per Tanh carried to the outputs); every gradient tensor to learned_std_fp64.bar: 4x the
distance of torch's float32 autograd from the float64 one, floored at 4 x 2^-23 x max |ref grad|.  Every check prints its figures."""
import copy

import pytest
import torch

import learned_std_fp64 as F
from policy_step_ref import HALF_LOG_2PI, make_net
from test_policy_step_gpu import DEV, bar, tanh_term

pytestmark = pytest.mark.gpu

# (S, A, H, actor hidden layers, critic hidden layers, activation)
CASES = [(3, 1, 64, 1, 2, "ReLU"), (10, 2, 128, 3, 1, "Tanh"), (20, 4, 256, 2, 2, "ReLU"), (32, 4, 64, 5, 1, "Tanh")]
ROWS = [1, 64, 70, 130]
E_COEF = 0.37
# the draw of the rows per (case index, m) where the first one (0) leaves a ReLU pre-activation too close to zero (see the test): found on
# the CPU from the float64 reference alone
DRAW = {(0, 64): 3, (0, 130): 21, (2, 64): 1152, (2, 70): 1102, (2, 130): 1397}


@pytest.fixture(scope="module")
def tg():
    import trajopt_grpo_amd as tg
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return tg


def problem(case, m):
    """The nets, log_std, rows and loss weights of a case at m rows, on the CPU in float32 (seeded: the same at every call)."""
    S, A, H, nh_a, nh_c, act = case
    actor, critic = make_net(S, H, nh_a, A, act, seed=21), make_net(S, H, nh_c, 1, act, seed=22)
    g = torch.Generator().manual_seed(100000 * DRAW.get((CASES.index(case), m), 0) + 1000 * CASES.index(case) + m)
    obs, action = torch.randn(m, S, generator=g), torch.randn(m, A, generator=g)
    c, d = torch.randn(m, generator=g), torch.randn(m, generator=g)
    return actor, critic, torch.linspace(-0.7, 0.2, A), obs, action, c, d


def relu_margin(net, obs):
    """Smallest |hidden pre-activation| / the layer's largest, over the hidden layers of a ReLU net, in float64."""
    h, worst = obs.double(), float("inf")
    for mod in net:
        if isinstance(mod, torch.nn.Linear):
            h = torch.nn.functional.linear(h, mod.weight.detach().double().cpu(), mod.bias.detach().double().cpu())
        else:
            worst = min(worst, float(h.abs().min() / h.abs().max()))
            h = torch.relu(h)
    return worst


def torch_eval(actor, critic, log_std, obs, action):
    """The composition evaluate() replaces, in the dtype of its arguments."""
    mu = actor(obs)
    ls = log_std.expand_as(mu)
    logp = (-0.5 * ((action - mu) / ls.exp()).pow(2) - ls - HALF_LOG_2PI).sum(-1)
    return logp, (ls + 0.5 + HALF_LOG_2PI).sum(-1), critic(obs).squeeze(-1) if critic is not None else None


def loss_of(out, c, d):
    logp, ent, value = out
    return (c * logp).sum() + E_COEF * ent.sum() + ((d * value).sum() if value is not None else 0.0)


def autograd_ref(actor, critic, log_std, obs, action, c, d, dtype, device):
    """-> (outputs, gradients [actor's, critic's, log_std's]) of torch autograd on copies of the nets in `dtype` on `device`."""
    nets = [copy.deepcopy(n).to(device=device, dtype=dtype) if n is not None else None for n in (actor, critic)]
    ls = log_std.detach().to(device=device, dtype=dtype).clone().requires_grad_(True)
    t = [v.to(device=device, dtype=dtype) for v in (obs, action, c, d)]
    out = torch_eval(nets[0], nets[1], ls, t[0], t[1])
    loss_of(out, t[2], t[3]).backward()
    grads = [p.grad for n in nets if n is not None for p in n.parameters()] + [ls.grad]
    return [o.detach().double().cpu() if o is not None else None for o in out], [g.detach().double().cpu() for g in grads]


def native(tg, actor, critic, log_std, obs, action, c, d, grid_limit=0):
    """One evaluate() + backward() -> (the DeviceActor, the outputs, the parameters whose .grad it filled)."""
    da = tg.DeviceActor(actor, critic, num_envs=1, log_std=log_std, device=DEV)
    da._grid_limit = grid_limit
    out = da.evaluate(obs, action)
    loss_of(out, c, d).backward()
    return da, out, [p for n in (actor, critic) if n is not None for p in n.parameters()] + [log_std]


def on_device(case, m):
    actor, critic, log_std, obs, action, c, d = problem(case, m)
    return (actor.to(DEV), critic.to(DEV), log_std.to(DEV).requires_grad_(True), *(t.to(DEV) for t in (obs, action, c, d)))


def assert_grads(tag, got, ref64, ref32):
    for k, (g, r64, r32) in enumerate(zip(got, ref64, ref32)):
        b, err32 = F.bar(r64, r32)
        err = float((g.detach().double().cpu() - r64).abs().max())
        print(f"{tag} grad[{k}] {tuple(r64.shape)}: native err {err:.3e}  torch-fp32 err {err32:.3e}  bar {b:.3e}")
        assert err <= b, (tag, k, err, b)


@pytest.mark.parametrize("m", ROWS)
@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_forward_and_gradients_against_fp64(tg, case, m):
    cpu = problem(case, m)
    if case[5] == "ReLU":
        # the ReLU derivative is discontinuous: the comparison is meaningful only if no float32 evaluation can sit on the other side
        # of a kink, i.e. no fp64 pre-activation lies within 2^-16 of zero relative to its layer's largest (the seeds of problem()
        # were chosen on the CPU so that this holds at every case and row count)
        assert min(relu_margin(cpu[0], cpu[3]), relu_margin(cpu[1], cpu[3])) > 2.0 ** -16
    ref64, gref64 = autograd_ref(*cpu, torch.float64, "cpu")
    ref32, gref32 = autograd_ref(*cpu, torch.float32, DEV)
    actor, critic, log_std, obs, action, c, d = on_device(case, m)
    da, out, params = native(tg, actor, critic, log_std, obs, action, c, d, grid_limit=2 if m == 130 else 0)
    assert all(o.grad_fn is not None and o.shape == (m,) for o in out)
    for name, got, r64, r32, extra in (("logp", out[0], ref64[0], ref32[0], tanh_term(actor)), ("entropy", out[1], ref64[1], ref32[1], 0.0),
                                       ("value", out[2], ref64[2], ref32[2], tanh_term(critic))):
        b, err32 = bar(r64.numpy(), r32.numpy(), extra)
        err = float((got.detach().double().cpu() - r64).abs().max())
        print(f"{case} m={m} {name}: native err {err:.3e}  torch-fp32 err {err32:.3e}  bar {b:.3e}")
        assert err <= b, (name, err, b)
    assert_grads(f"{case} m={m}", [p.grad for p in params], gref64, gref32)


@pytest.mark.parametrize("m", [70, 130])
@pytest.mark.parametrize("case", CASES[:2], ids=lambda c: "-".join(map(str, c)))
def test_mean_and_value_are_the_policy_steps_bit_for_bit(tg, case, m):
    """The three entries run one definition of the tile forward (csrc/policy_tile.hpp): evaluate()'s mu is the mean of a
    deterministic act() on the same rows and its value is values()', bit for bit.  (logp divides by exp(log_std): no identity.)"""
    actor, critic, log_std, obs, action, _, _ = on_device(case, m)
    da = tg.DeviceActor(actor, critic, num_envs=m, log_std=log_std, device=DEV)
    da._grid_limit = 2 if m == 130 else 0
    da.act(obs, deterministic=True)
    logp, _, value = da.evaluate(obs, action)
    assert torch.equal(logp.grad_fn.ws.mu, da.mean)                   # (the node's workspace holds mu for its backward)
    assert torch.equal(value.detach(), da.values(obs))


def test_two_rounds_are_bit_identical_and_a_second_backward_accumulates(tg):
    case, m = CASES[1], 130
    rounds = []
    for _ in range(2):
        rounds.append([p.grad.clone() for p in native(tg, *on_device(case, m))[2]])
    assert all(torch.equal(a, b) for a, b in zip(*rounds))
    actor, critic, log_std, obs, action, c, d = on_device(case, m)
    da, out, params = native(tg, actor, critic, log_std, obs, action, c, d)
    loss_of(da.evaluate(obs, action), c, d).backward()                # into the existing .grad: g + g
    assert all(torch.equal(p.grad, r + r) for p, r in zip(params, rounds[0]))


def test_an_in_place_optimizer_step_is_seen_by_the_next_evaluate(tg):
    case, m = CASES[0], 70
    actor, critic, log_std, obs, action, c, d = on_device(case, m)
    da, out, _ = native(tg, actor, critic, log_std, obs, action, c, d)
    torch.optim.SGD([*actor.parameters(), *critic.parameters(), log_std], lr=0.05).step()
    moved = da.evaluate(obs, action)
    cpu = [copy.deepcopy(n).cpu() for n in (actor, critic)]
    ref64 = torch_eval(cpu[0].double(), cpu[1].double(), log_std.detach().double().cpu(), obs.double().cpu(), action.double().cpu())
    with torch.no_grad():
        ref32 = torch_eval(actor, critic, log_std, obs, action)
    for got, old, r64, r32 in zip(moved, out, ref64, ref32):
        b, _ = bar(r64.detach().numpy(), r32.double().cpu().numpy())
        assert float((got.detach().double().cpu() - r64.detach()).abs().max()) <= b and not torch.equal(got, old)


def test_without_a_critic_value_is_none_and_what_is_not_built_raises(tg):
    case, m = CASES[0], 64
    actor, critic, log_std, obs, action, c, d = on_device(case, m)
    da, out, params = native(tg, actor, None, log_std, obs, action, c, d)
    assert out[2] is None
    _, gref64 = autograd_ref(*(v.cpu() if v is not None else None for v in (actor, None, log_std, obs, action, c, d)), torch.float64, "cpu")
    _, gref32 = autograd_ref(actor, None, log_std, obs, action, c, d, torch.float32, DEV)
    assert_grads("no critic", [p.grad for p in params], gref64, gref32)
    with pytest.raises(ValueError, match="no gradient to obs"):
        da.evaluate(obs.clone().requires_grad_(True), action)
    squashed = tg.DeviceActor(make_net(3, 64, 1, 2, "ReLU", seed=1).to(DEV), num_envs=1, head="squashed", device=DEV)
    with pytest.raises(ValueError, match="evaluate\\(\\) is built for the gaussian head"):
        squashed.evaluate(obs, action)
