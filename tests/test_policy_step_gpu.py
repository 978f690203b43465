"""DeviceActor (tg_policy_step / tg_policy_values, csrc/policy_step.hip) against the float64 restatement in policy_step_ref.py.

Tolerance (the rule of test_learned_std_gpu.py, not tuned): per output, 4x the distance of torch's own float32 evaluation of the same
module and head on the same rows from the fp64 reference, floored at 4 x 2^-23 x max |reference|.  Added to it, where they apply:
  * 4u per Tanh activation (tanh is 1-Lipschitz), carried to the outputs through the inf-norms of the layers behind;
  * the kernel's eps is not torch's: it is held to philox_fp64's own bound (test_rng_fp64_gpu.eps_bound), so an action carries
    exp(ls) x that bound and a log-density |eps| x it (the squashed head 2 exp(ls) x it more: |d log(1 - tanh(u)^2 + 1e-6) / du| <= 2).
Every check prints its figures."""
import copy
import math

import numpy as np
import pytest
import torch

import policy_step_ref as R
from test_rng_fp64_gpu import U, eps_bound

pytestmark = pytest.mark.gpu

# (S, H, hidden layers, A, activation) of the actor; the critic has another depth and the other activation
NETS = [(5, 64, 2, 1, "Tanh"), (3, 64, 1, 1, "ReLU"), (10, 128, 3, 2, "Tanh"), (20, 256, 5, 4, "ReLU"), (20, 256, 2, 4, "Tanh")]
ROWS = [1, 64, 70, 130]


@pytest.fixture(scope="module")
def tg():
    import trajopt_grpo_amd as tg
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return tg


DEV = torch.device("cuda", 0)


def nets_for(S, H, nh, A, act, head="gaussian", scale=1.0):
    actor = R.make_net(S, H, nh, 2 * A if head == "squashed" else A, act, seed=11, scale=scale).to(DEV)
    critic = R.make_net(S, 128 if H == 64 else 64, nh % 3 + 1, 1, "ReLU" if act == "Tanh" else "Tanh", seed=12).to(DEV)
    return actor, critic


def tanh_term(net):
    """4u per Tanh activation, carried to the outputs: sum over the Tanh layers of 4u x the product of the later layers' inf-norms."""
    lin = [m for m in net if isinstance(m, torch.nn.Linear)]
    if not any(isinstance(m, torch.nn.Tanh) for m in net):
        return 0.0
    norms = [float(l.weight.detach().double().abs().sum(1).max()) for l in lin]
    return sum(4.0 * U * math.prod(norms[k:]) for k in range(1, len(lin)))


def bar(ref64, got32, extra=0.0):
    err32 = float(np.abs(np.asarray(got32, dtype=np.float64) - ref64).max())
    return 4.0 * max(err32, 2.0 ** -23 * float(np.abs(ref64).max())) + extra, err32


def torch32_head(out, e64, head, log_std, bounds):
    """The head in torch float32 on torch's own float32 outputs (the tools' lines), eps the fp64 one rounded to float32."""
    e = torch.tensor(e64, dtype=torch.float32, device=out.device)
    if head == "gaussian":
        mu, ls = out, log_std.detach().expand_as(out)
    else:
        mu, ls = out.split(out.shape[1] // 2, dim=-1)
        ls = ls.clamp(*bounds)
    u = mu + ls.exp() * e
    logp = (-0.5 * e.pow(2) - ls - R.HALF_LOG_2PI).sum(-1)
    if head == "gaussian":
        return u, logp, mu
    a = torch.tanh(u)
    return a, logp - torch.log(1.0 - a.pow(2) + 1e-6).sum(-1), torch.tanh(mu)


def check_call(tag, da, obs, calls, head, log_std=None, bounds=(-5.0, 2.0), deterministic=False):
    """One act() against the reference; -> the largest error / bar ratio."""
    action, logp, value = da.act(obs, deterministic=deterministic)
    x = obs.double().cpu().numpy()
    out64 = R.mlp(da.actor_net, x)
    e64, ur, ut, is_sin = R.eps(da.seed, da.env_offset, calls, da.A)
    eb = eps_bound(e64, ur, ut, is_sin)
    if deterministic:
        e64, eb = np.zeros_like(e64), np.zeros_like(eb)
    want = R.head(out64, e64, head, None if log_std is None else log_std.detach().double().cpu().numpy(), bounds)
    with torch.no_grad():
        a32, lp32, m32 = torch32_head(da.actor_net(obs), e64, head, log_std, bounds)
        v32 = da.critic_net(obs).squeeze(-1)
    sig = np.exp(np.clip(want["ls"], *bounds)) if head == "squashed" else np.exp(want["ls"])
    t_act, t_val = tanh_term(da.actor_net), tanh_term(da.critic_net)
    extra = {"mean": t_act, "action": t_act + sig * eb, "value": t_val,
             "logp": (np.abs(e64) * eb + (2.0 * sig * eb if head == "squashed" else 0.0)).sum(1)}
    worst = 0.0
    for name, got, ref64, got32 in (("mean", da.mean, want["mean"], m32), ("action", action, want["action"], a32),
                                    ("logp", logp, want["logp"], lp32), ("value", value, R.mlp(da.critic_net, x)[:, 0], v32)):
        b, err32 = bar(ref64, got32.double().cpu().numpy())
        err = np.abs(got.double().cpu().numpy() - ref64)
        ratio = float((err / (b + extra[name])).max())
        print(f"{tag} {name}: native err {err.max():.3e}  torch-fp32 err {err32:.3e}  bar {b:.3e} (+ {np.max(extra[name]):.3e})  ratio {ratio:.3f}")
        assert ratio <= 1.0, (tag, name, float(err.max()), b)
        worst = max(worst, ratio)
    if head == "gaussian" and not deterministic:   # eps itself: a = fl(mu + fl(sigma eps)), sigma = expf(ls) within 2u
        a, m = action.double().cpu().numpy(), da.mean.double().cpu().numpy()
        err = np.abs(a - m - sig * e64)
        assert (err <= sig * eb + 4.0 * U * (np.abs(sig * e64) + np.abs(a))).all(), (tag, "eps", float(err.max()))
    return worst


@pytest.mark.parametrize("S,H,nh,A,act", NETS)
def test_parity_with_fp64_over_row_counts_and_three_calls(tg, S, H, nh, A, act):
    actor, critic = nets_for(S, H, nh, A, act)
    log_std = torch.linspace(-0.7, 0.2, A, device=DEV)
    worst = 0.0
    for n in ROWS:
        da = tg.DeviceActor(actor, critic, num_envs=n, log_std=log_std, seed=0xA5A5 + n, env_offset=3, device=DEV)
        da._grid_limit = 2 if n == 130 else 0                     # 130 rows = 3 tiles on 2 workgroups: a second trip of the row loop
        for call in range(3):
            obs = torch.randn(n, S, device=DEV, generator=torch.Generator(DEV).manual_seed(100 * n + call))
            worst = max(worst, check_call(f"{(S, H, nh, A, act)} n={n} call={call}", da, obs, np.full(n, call), "gaussian", log_std))
        assert da.calls.tolist() == [3] * n
        x = torch.randn(n + 5, S, device=DEV, generator=torch.Generator(DEV).manual_seed(n))
        b, _ = bar(R.mlp(critic, x.double().cpu().numpy())[:, 0], critic(x).squeeze(-1).detach().double().cpu().numpy(), tanh_term(critic))
        assert float(np.abs(da.values(x).double().cpu().numpy() - R.mlp(critic, x.double().cpu().numpy())[:, 0]).max()) <= b
    print(f"{(S, H, nh, A, act)}: largest err / bar {worst:.3f}")


@pytest.mark.parametrize("S,H,nh,A,scale", [(5, 64, 2, 1, 40.0), (20, 256, 2, 4, 30.0)])
def test_squashed_head_with_clamped_log_std_and_saturated_actions(tg, S, H, nh, A, scale):
    actor, critic = nets_for(S, H, nh, A, "ReLU", head="squashed", scale=scale)
    n = 130
    da = tg.DeviceActor(actor, critic, num_envs=n, head="squashed", seed=77, device=DEV)
    obs = (3.0 * torch.randn(n, S, generator=torch.Generator().manual_seed(5))).to(DEV)
    out = R.mlp(actor, obs.double().cpu().numpy())
    want = R.head(out, R.eps(77, 0, np.zeros(n), A)[0], "squashed")
    assert (want["ls"] < -5).any() and (want["ls"] > 2).any() and (np.abs(want["u"]) > 4).any()       # the clamp and the 1e-6 term
    for call in range(2):
        check_call(f"squashed {(S, H, nh, A)} call={call}", da, obs, np.full(n, call), "squashed")


def test_deterministic_returns_the_mean_and_leaves_the_counters(tg):
    actor, critic = nets_for(10, 128, 3, 2, "Tanh")
    log_std = torch.tensor([-0.3, 0.1], device=DEV)
    obs = torch.randn(70, 10, device=DEV)
    da, twin = (tg.DeviceActor(actor, critic, num_envs=70, log_std=log_std, seed=9, device=DEV) for _ in range(2))
    check_call("deterministic", da, obs, np.zeros(70), "gaussian", log_std, deterministic=True)
    assert torch.equal(da.action, da.mean) and da.calls.tolist() == [0] * 70
    value = da.value.clone()
    got, want = [t.clone() for t in da.act(obs)], twin.act(obs)
    assert all(torch.equal(a, b) for a, b in zip(got, want)) and torch.equal(value, da.value) and da.calls.tolist() == [1] * 70


def test_fresh_weights_after_an_optimizer_step_and_a_data_copy(tg):
    actor, critic = nets_for(5, 64, 2, 1, "Tanh")
    log_std = torch.nn.Parameter(torch.full((1,), -0.5, device=DEV))
    params = list(actor.parameters()) + list(critic.parameters()) + [log_std]
    opt = torch.optim.Adam(params, lr=1e-2)
    obs = torch.randn(70, 5, device=DEV)
    da = tg.DeviceActor(actor, critic, num_envs=70, log_std=log_std, seed=4, device=DEV)
    da.act(obs)
    before = da.mean.clone()
    for update in ("adam", "copy"):
        if update == "adam":
            (actor(obs).pow(2).mean() + critic(obs).pow(2).mean() + log_std.sum()).backward()
            opt.step()
        else:
            with torch.no_grad():
                for p in params:
                    p.data.copy_(p.data * 1.25 + 0.01)
        fresh = tg.DeviceActor(copy.deepcopy(actor), copy.deepcopy(critic), num_envs=70, log_std=log_std.detach().clone(), seed=4, device=DEV)
        fresh.load_state_dict(da.state_dict())
        got, want = da.act(obs), fresh.act(obs)
        assert all(torch.equal(a, b) for a, b in zip(got, want)), update
        assert not torch.equal(da.mean, before), update
        before = da.mean.clone()


@pytest.mark.parametrize("update_between", [False, True])
def test_act_step_add_captured_once_equals_eager_steps_of_a_twin(tg, update_between):
    n, L = 70, 8
    actor, critic = nets_for(5, 64, 2, 1, "Tanh")
    log_std = torch.full((1,), -0.5, device=DEV)

    def build():
        venv = tg.DeviceVecEnv(tg.CartPole(max_steps=6), n, seed=3, device=DEV)
        st = tg.DeviceRolloutStorage.for_env(venv, L, seed=3)
        st.start(venv.reset(seed=3)[0])
        return venv, st, tg.DeviceActor.for_env(venv, actor, critic, log_std=log_std)

    def step(venv, st, da):
        act, logp, value = da.act(venv._obs)
        obs, rew, term, trunc, info = venv.step(act)
        st.add(act, logp, value, obs, rew, term, trunc, da.values(info["final_obs"]))

    def poke(k):
        with torch.no_grad():
            for p in list(actor.parameters()) + list(critic.parameters()):
                p.add_(0.01 * (k + 1))

    saved = [p.detach().clone() for p in list(actor.parameters()) + list(critic.parameters())]
    eager = build()
    for k in range(6):
        step(*eager)
        if update_between:
            poke(k)
    with torch.no_grad():
        for p, s in zip(list(actor.parameters()) + list(critic.parameters()), saved):
            p.copy_(s)
    graphed = build()
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        step(*graphed)                                            # (warm-up: the eager twin's first step)
    torch.cuda.current_stream(DEV).wait_stream(side)
    if update_between:
        poke(0)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step(*graphed)
    for k in range(1, 6):
        g.replay()
        if update_between:
            poke(k)
    torch.cuda.synchronize()
    for a, b in zip(eager, graphed):
        names = [k for k, v in vars(a).items() if isinstance(v, torch.Tensor)]
        assert names and all(torch.equal(getattr(a, k), getattr(b, k)) for k in names), [k for k in names if not torch.equal(getattr(a, k), getattr(b, k))]


def test_two_shards_equal_one_actor(tg):
    actor, critic = nets_for(20, 256, 2, 4, "Tanh")
    log_std = torch.linspace(-1, 0, 4, device=DEV)
    obs = torch.randn(130, 20, device=DEV)
    whole = tg.DeviceActor(actor, critic, num_envs=130, log_std=log_std, seed=21, device=DEV)
    parts = [tg.DeviceActor(actor, critic, num_envs=m, log_std=log_std, seed=21, env_offset=o, device=DEV) for o, m in ((0, 70), (70, 60))]
    for _ in range(2):
        want = whole.act(obs)
        got = [p.act(obs[o:o + p.num_envs].contiguous()) for p, o in zip(parts, (0, 70))]
        for k in range(3):
            assert torch.equal(torch.cat([g[k] for g in got]), want[k])
        assert torch.equal(torch.cat([p.mean for p in parts]), whole.mean)


@pytest.mark.parametrize("label,net,head,word", R.refused_nets() + [("float64", None, "gaussian", ""), ("obs", None, "gaussian", "")])
def test_refusals_raise_value_error_with_a_reason(tg, label, net, head, word):
    good = R.make_net(5, 64, 2, 1, "Tanh", 0).to(DEV)
    log_std = torch.zeros(5 if label == "O5" else 1, device=DEV)
    with pytest.raises(ValueError, match="DeviceActor: .{10,}"):
        if net is not None:
            tg.DeviceActor(net().to(DEV), num_envs=4, log_std=None if head == "squashed" else log_std, head=head, device=DEV)
        elif label == "float64":
            tg.DeviceActor(good.double(), num_envs=4, log_std=log_std, device=DEV).act(torch.zeros(4, 5, device=DEV))
        else:
            tg.DeviceActor(good, num_envs=4, log_std=log_std, device=DEV).act(torch.zeros(5, 5, device=DEV))
