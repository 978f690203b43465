"""The learned per-dimension log-std without a GPU: the policy surface (parameters, cov / var, checkpoints, refusals, autograd),
the fp64 yardstick's closed-form gradient against torch autograd of the reference's loss, and the exported / bound symbols."""
import copy
import math
import os

import pytest
import torch

import learned_std_fp64 as Y

HERE = os.path.dirname(os.path.abspath(__file__))
PUBLISHED = os.path.join(HERE, "golden", "published")


@pytest.fixture(scope="module")
def tg():
    import trajopt_grpo_amd as tg
    return tg


def _policies(tg, learn_std):
    kw = {"learn_std": True} if learn_std else {}
    return (tg.GaussianActor_NeuralNetwork(5, 2, (16, 16), cov=[0.1, 0.4], device="cpu", **kw),
            tg.GaussianActorCritic_NeuralNetwork(5, 2, (16, 16), cov=[0.1, 0.4], device="cpu", **kw))


def test_constructing_a_learned_std_policy_and_its_parameter_order(tg):
    for pol in _policies(tg, True):
        ps = list(pol.parameters())
        nets = list(pol.actor.parameters()) + (list(pol.critic.parameters()) if pol.critic is not None else [])
        assert isinstance(pol.log_std, torch.nn.Parameter) and pol.log_std.dtype == torch.float32 and pol.log_std.shape == (2,)
        assert len(ps) == len(nets) + 1 and all(a is b for a, b in zip(ps, nets)) and ps[-1] is pol.log_std
        assert torch.allclose(pol.log_std.detach(), 0.5 * torch.log(torch.tensor([0.1, 0.4])))
        assert pol.metadata()["learn_std"] is True
        assert pol.metadata()["num_parameters"] == sum(p.numel() for p in nets) + 2


def test_cov_and_var_follow_log_std(tg):
    for pol in _policies(tg, True):
        with torch.no_grad():
            pol.log_std.copy_(torch.tensor([-0.3, 0.2]))
        want = torch.exp(2 * torch.tensor([-0.3, 0.2]))
        assert torch.allclose(pol.var, want) and torch.allclose(pol.cov, torch.diag(want))
        assert not pol.cov.requires_grad and pol.cov.device.type == "cpu"
        assert pol.metadata()["cov"] == pol.cov.tolist()
        ptr = pol.log_std.data_ptr()
        pol.cov = torch.diag(torch.tensor([0.25, 0.04]))                      # written in place
        assert pol.log_std.data_ptr() == ptr and torch.allclose(pol.log_std.detach(), torch.log(torch.tensor([0.5, 0.2])))
        with pytest.raises(ValueError):
            pol.cov = torch.tensor([[0.3, 0.1], [0.1, 0.2]])
        assert torch.allclose(pol.log_std.detach(), torch.log(torch.tensor([0.5, 0.2])))


def test_state_dict_round_trip_and_save_load(tg, tmp_path):
    for pol, fresh in zip(_policies(tg, True), _policies(tg, True)):
        with torch.no_grad():
            pol.log_std.copy_(torch.tensor([-0.7, 0.1]))
        sd = pol.state_dict()
        assert "log_std" in sd and torch.equal(sd["log_std"], pol.log_std.detach())
        if pol.critic is None:
            assert [k for k in sd if k != "log_std"] == list(pol.actor.state_dict())
        else:
            assert list(sd) == ["actor", "critic", "log_std"]
        fresh.load_state_dict(copy.deepcopy(sd))
        assert torch.equal(fresh.log_std.detach(), pol.log_std.detach())
        assert all(torch.equal(a, b) for a, b in zip(fresh.parameters(), pol.parameters()))
        pol.save(str(tmp_path))
        other = _policies(tg, True)[0 if pol.critic is None else 1]
        other.load(str(tmp_path))
        assert torch.equal(other.log_std.detach(), pol.log_std.detach())
        # a dict without the key keeps the current value
        nets_only = {k: v for k, v in sd.items() if k != "log_std"}
        other.load_state_dict(nets_only)
        assert torch.equal(other.log_std.detach(), pol.log_std.detach())


def test_log_std_into_a_fixed_policy_is_refused(tg):
    for learned, fixed in zip(_policies(tg, True), _policies(tg, False)):
        with pytest.raises(ValueError, match="log_std"):
            fixed.load_state_dict(learned.state_dict())


@pytest.mark.parametrize("name,cls,dims", [("cartpole_nn_grpo", "GaussianActor_NeuralNetwork", None),
                                           ("cartpole_nn_ppo", "GaussianActorCritic_NeuralNetwork", None),
                                           ("quadpole2d_nn_ppo", "GaussianActorCritic_NeuralNetwork", None)])
def test_published_checkpoints_load_and_leave_log_std_at_its_init(tg, name, cls, dims):
    sd = torch.load(os.path.join(PUBLISHED, name, "policy.pt"), weights_only=True, map_location="cpu")
    actor = sd["actor"] if "actor" in sd else sd
    ws = [v for k, v in actor.items() if k.endswith("weight")]
    S, A, hidden = ws[0].shape[1], ws[-1].shape[0], [w.shape[0] for w in ws[:-1]]
    pol = getattr(tg, cls)(S, A, hidden, cov=0.3, device="cpu", learn_std=True)
    init = pol.log_std.detach().clone()
    pol.load_state_dict(sd)
    assert torch.equal(pol.log_std.detach(), init)
    assert torch.equal(pol.actor.state_dict()["network.0.weight"], actor["network.0.weight"])


def test_fixed_policies_expose_exactly_todays_keys_and_metadata(tg):
    a, ac = _policies(tg, False)
    assert a.log_std is None and ac.log_std is None
    assert list(a.state_dict()) == list(a.actor.state_dict())
    assert list(ac.state_dict()) == ["actor", "critic"]
    for pol in (a, ac):
        assert sorted(pol.metadata()) == sorted(["input_dim", "output_dim", "hidden_dims", "activation", "cov", "num_parameters"])
        nets = list(pol.actor.parameters()) + (list(pol.critic.parameters()) if pol.critic is not None else [])
        assert all(x is y for x, y in zip(pol.parameters(), nets)) and len(list(pol.parameters())) == len(nets)


def _case(seed, n=257, A=3, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    mean = torch.randn(n, A, generator=g, dtype=dtype)
    log_std = torch.tensor([-0.9, -0.2, 0.3], dtype=dtype)[:A]
    act = mean + torch.exp(log_std) * torch.randn(n, A, generator=g, dtype=dtype)
    lp = Y.gaussian(mean, log_std).log_prob(act)
    old_lp = lp + 0.3 * torch.randn(n, generator=g, dtype=dtype)             # ratios on both sides of the clip range
    adv = torch.randn(n, generator=g, dtype=dtype)
    lp_ref = lp + 0.2 * torch.randn(n, generator=g, dtype=dtype)
    return mean, act, log_std, old_lp, adv, lp_ref


@pytest.mark.parametrize("terms", [dict(surr_coef=-1 / 257, kl_coef=0.5 / 257, entropy_coef=0.0),
                                   dict(surr_coef=-1 / 257, kl_coef=0.5 / 257, entropy_coef=0.01),
                                   dict(surr_coef=1 / 8),
                                   dict(surr_coef=1 / 8, ref_coef=0.04 / 8)])
def test_closed_form_gradient_equals_autograd_of_the_reference_loss(terms):
    """MultivariateNormal log-prob / entropy under fp64 autograd against the closed form, PPO's two KL-ish forms, the entropy
    bonus and GRPO's reference penalty included.  Both are fp64 sums of 257 terms of size <= ~1: 1e-12 is ~ 2^-40."""
    mean, act, log_std, old_lp, adv, lp_ref = _case(1)
    ls = log_std.clone().requires_grad_(True)
    kw = dict(epsilon=0.2, lp_ref=lp_ref if "ref_coef" in terms else None, **terms)
    Y.actor_loss(mean, act, ls, old_lp, adv, **kw).backward()
    want = Y.analytic_log_std_grad(mean, act, log_std, old_lp, adv, **kw)
    assert float((ls.grad - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
    if terms.get("entropy_coef"):
        base = Y.analytic_log_std_grad(mean, act, log_std, old_lp, adv, **{**kw, "entropy_coef": 0.0})
        assert torch.allclose(want - base, torch.full_like(want, -terms["entropy_coef"]), atol=1e-15)


def test_log_prob_and_entropy_autograd_equal_the_yardstick(tg):
    torch.manual_seed(0)
    for pol in _policies(tg, True):
        obs, act = torch.randn(33, 5), torch.randn(33, 2)
        lp, ent = pol.log_prob(obs, act)
        assert lp.shape == (33,) and ent.shape == (33,)
        w = torch.randn(33)
        ((lp * w).sum() + 0.7 * ent.mean()).backward()
        ls = pol.log_std.detach().double().requires_grad_(True)
        d = Y.gaussian(pol.actor(obs).detach().double(), ls)
        ((d.log_prob(act.double()) * w.double()).sum() + 0.7 * d.entropy().mean()).backward()
        assert torch.allclose(lp.detach().double(), d.log_prob(act.double()).detach(), atol=1e-5)
        assert abs(float(ent[0]) - float(d.entropy()[0])) < 1e-6
        assert torch.allclose(pol.log_std.grad.double(), ls.grad, rtol=1e-5, atol=1e-5)
        action, lp_s, _ = pol.forward(obs)
        assert action.shape == (33, 2) and lp_s.requires_grad


def test_new_symbols_are_declared_bound_and_exported(tg):
    N = tg._native
    names = ["tg_surrogate_loss_std", "tg_mlp_forward_chain_loss_std", "tg_mlp_f32_forward_backward_act_std",
             "tg_mlp_f32w_forward_backward_std", "tg_mlp_f32r_forward_backward_std", "tg_log_std_grad", "tg_log_std_grad_blocks"]
    header = open(os.path.join(HERE, "..", "include", "trajopt_grpo_hip.h")).read()
    lib = N.load()
    for n in names:
        assert n in N.SIGNATURES and f" {n}(" in header and hasattr(lib, n)
    assert "typedef struct tg_learned_std" in header
    assert lib.tg_abi_version() == 13 == N.ABI_VERSION
    assert lib.tg_log_std_grad_blocks() > 0
    import ctypes
    assert ctypes.sizeof(N.LearnedStd) == 16
