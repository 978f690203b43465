"""DeviceActor.q_values / .sac_target (tg_policy_q_values / tg_policy_sac_target, csrc/policy_q.hip).

q_values is held to the float64 restatement (policy_step_ref.mlp on the rows [obs, act]) under test_policy_step_gpu.py's bar: 4x
torch's own float32 error against fp64, floored at 4 x 2^-23 x max |reference|, plus its tanh_term.  min(q1, q2) is the exact minimum
of the two returned vectors, so it lies within the larger of their two bars (min is 1-Lipschitz in the sup norm).  Everything about
sac_target is exact: its action and logp are act()'s of a twin, its q1 / q2 are q_values' on the action it returned, and y is the
float32 NumPy expression on what it returned."""
import numpy as np
import pytest
import torch

import policy_step_ref as R
from test_policy_step_gpu import DEV, bar, tanh_term

pytestmark = pytest.mark.gpu

# (S, A, H, actor hidden layers, critic hidden layers, activation): S % 4 != 0 and == 0, S + A = 32, a net without ring blocks beside
# nets with them, every width
CASES = [(3, 1, 64, 1, 2, "ReLU"), (10, 2, 128, 3, 1, "Tanh"), (20, 4, 256, 2, 2, "ReLU"), (28, 4, 64, 2, 2, "Tanh")]
ROWS = [1, 64, 70, 130]


@pytest.fixture(scope="module")
def tg():
    import trajopt_grpo_amd as tg
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return tg


def nets_for(S, A, H, nh_a, nh_q, act):
    return (R.make_net(S, H, nh_a, 2 * A, act, seed=21).to(DEV),
            tuple(R.make_net(S + A, H, nh_q, 1, act, seed=22 + k).to(DEV) for k in range(2)))


def rows_for(n, S, A, seed):
    g = torch.Generator(DEV).manual_seed(seed)
    return (torch.randn(n, S, device=DEV, generator=g), torch.tanh(torch.randn(n, A, device=DEV, generator=g)),
            torch.randn(n, device=DEV, generator=g), (torch.rand(n, device=DEV, generator=g) > 0.2).float() * 0.97)


def actor_with(tg, actor, q_nets, n, **kw):
    da = tg.DeviceActor(actor, q_nets=q_nets, num_envs=n, head="squashed", seed=0xBEEF + n, env_offset=5, device=DEV, **kw)
    da._grid_limit = 2 if n == 130 else 0                         # 130 rows = 3 tiles on 2 workgroups: a second trip of the row loop
    return da


def y_numpy(da, reward, discount, alpha):
    f = lambda t: t.detach().cpu().numpy().astype(np.float32)     # float32 arrays: NumPy rounds every operation
    return f(reward) + f(discount) * (np.minimum(f(da.q1), f(da.q2)) - np.float32(float(alpha)) * f(da.logp))


@pytest.mark.parametrize("S,A,H,nh_a,nh_q,act", CASES)
def test_q_values_against_fp64(tg, S, A, H, nh_a, nh_q, act):
    actor, qs = nets_for(S, A, H, nh_a, nh_q, act)
    for n in ROWS:
        obs, a, _, _ = rows_for(n, S, A, n)
        x = torch.cat([obs, a], 1)
        got = actor_with(tg, actor, qs, n).q_values(obs, a)
        bars = []
        for k, q in enumerate(qs):
            ref = R.mlp(q, x.double().cpu().numpy())[:, 0]
            b, err32 = bar(ref, q(x).squeeze(-1).detach().double().cpu().numpy(), tanh_term(q))
            err = float(np.abs(got[k].double().cpu().numpy() - ref).max())
            print(f"{(S, A, H, nh_q, act)} n={n} q{k + 1}: native err {err:.3e}  torch-fp32 err {err32:.3e}  bar {b:.3e}")
            assert err <= b
            bars.append((ref, b))
        assert torch.equal(got[2], torch.minimum(got[0], got[1]))
        assert float(np.abs(got[2].double().cpu().numpy() - np.minimum(bars[0][0], bars[1][0])).max()) <= max(bars[0][1], bars[1][1])
        one = actor_with(tg, actor, qs[0], n).q_values(obs, a)
        assert one[1] is None and one[2] is None and float(np.abs(one[0].double().cpu().numpy() - bars[0][0]).max()) <= bars[0][1]


@pytest.mark.parametrize("S,A,H,nh_a,nh_q,act", CASES)
def test_sac_target_is_act_then_q_values_then_the_float32_expression(tg, S, A, H, nh_a, nh_q, act):
    actor, qs = nets_for(S, A, H, nh_a, nh_q, act)
    alpha = torch.tensor(0.2, device=DEV)
    for n in ROWS:
        da, twin = actor_with(tg, actor, qs, n), actor_with(tg, actor, None, n)
        for call in range(3):
            obs, _, reward, discount = rows_for(n, S, A, 10 * n + call)
            alpha.fill_(0.2 + 0.3 * call)
            y = da.sac_target(obs, reward, discount, alpha)
            action, logp, _ = twin.act(obs)
            assert torch.equal(da.action, action) and torch.equal(da.logp, logp), (n, call)
            assert da.calls.tolist() == [call + 1] * n
            q1, q2, _ = da.q_values(obs, da.action)
            assert torch.equal(da.q1, q1) and torch.equal(da.q2, q2), (n, call)
            assert np.array_equal(y.cpu().numpy(), y_numpy(da, reward, discount, alpha)), (n, call)


def test_lerp_of_the_target_nets_and_a_new_alpha_are_followed_eagerly_and_on_replay(tg):
    S, A, H, nh_a, nh_q, act = CASES[0]
    n = 70
    actor, qs = nets_for(S, A, H, nh_a, nh_q, act)
    online = nets_for(S, A, H, nh_a, nh_q, act)[1]
    with torch.no_grad():
        for q in online:
            for p in q.parameters():
                p.mul_(1.5).add_(0.05)
    alpha = torch.tensor(0.2, device=DEV)
    obs, _, reward, discount = rows_for(n, S, A, 1)
    eager, graphed = actor_with(tg, actor, qs, n), actor_with(tg, actor, qs, n)

    def move(k):                                                  # a Polyak step of the targets and a new temperature, both in place
        with torch.no_grad():
            for q, src in zip(qs, online):
                for p, ps in zip(q.parameters(), src.parameters()):
                    p.lerp_(ps, 0.3)
            alpha.fill_(0.5 + k)

    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        graphed.sac_target(obs, reward, discount, alpha)          # (warm-up: the eager twin's first call)
    torch.cuda.current_stream(DEV).wait_stream(side)
    before = eager.sac_target(obs, reward, discount, alpha).clone()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        graphed.sac_target(obs, reward, discount, alpha)
    for k in range(3):
        move(k)
        y = eager.sac_target(obs, reward, discount, alpha)
        g.replay()
        torch.cuda.synchronize()
        assert not torch.equal(y, before)
        assert np.array_equal(y.cpu().numpy(), y_numpy(eager, reward, discount, alpha))
        q1, q2, _ = eager.q_values(obs, eager.action)             # (the moved nets: q_values reads them at this call)
        assert torch.equal(eager.q1, q1) and torch.equal(eager.q2, q2)
        for name in ("y", "action", "logp", "q1", "q2", "_calls"):
            assert torch.equal(getattr(graphed, name), getattr(eager, name)), (k, name)
        before = y.clone()


def test_wrong_rows_and_a_single_q_net_raise_value_error(tg):
    actor, qs = nets_for(*CASES[0])
    da = actor_with(tg, actor, qs[0], 4)
    z = torch.zeros(4, device=DEV)
    with pytest.raises(ValueError, match="pair of q_nets"):
        da.sac_target(torch.zeros(4, 3, device=DEV), z, z, 0.2)
    with pytest.raises(ValueError, match="act must be float32"):
        da.q_values(torch.zeros(4, 3, device=DEV), torch.zeros(4, 2, device=DEV))
