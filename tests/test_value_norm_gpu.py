"""Running value normalisation on the MI355X (policies: normalize_value=True; tg_scatter_rows_affine, tg_boot_values_affine,
tg_value_norm_merge; run with `-m gpu`):

  1. the two denormalising kernels against the torch expression `v * t1 + t0` (two kernels, two roundings), bit for bit;
  2. tg_value_norm_merge on given moments against tests/value_norm_fp64.py: count exact, mean / m2 / table bit for bit (both run the
     same f64 operations in the same order), NULL moments, and norm8's entries 2 and 3;
  3. the whole step, frozen: learn() of a frozen value-normalised policy equals a plain learner's learn() whose prologue the test
     patches (scatter + torch affine, tg_ppo_norm's entries 2 and 3 overwritten, the bootstrap product denormalised), bit for bit in
     every weight and loss -- per-layer, bf16-chain, fp32-chain and autograd learners, Monte Carlo and GAE, full batch and minibatch,
     bootstrap_truncated on and off;
  4. the whole step, unfrozen: after two learn() calls the statistics are the restatement's merge of the two batches' moments, which
     the test recomputes with K.ppo_returns on a grid it builds from the critic itself; norm8[0:2] of the second call show that V
     entered GAE denormalised; explained_variance and the other last_stats entries against their definitions;
  5. two ranks against one, and a checkpoint round trip that continues bit for bit."""
import math
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import value_norm_fp64 as Y
from value_norm_dist_worker import make_env

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
T0, G0, E0 = 32, 4, 40                      # n = 160: a tail for 64- and 256-wide launches alike
FACTORY = {"CartPole": (5, 1, (128, 128, 128), 0.5), "QuadPole2D": (10, 2, (128, 128, 128), 0.5)}
TABLE = (11.7, 53.9, 5000.0)                # frozen statistics (mean, var, count): sigma = 7.34..., no power of two in the table


@pytest.fixture(scope="module")
def tg():
    import trajopt_grpo_amd as tg
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return tg


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


# --------------------------------------------------------------------------------------------------------------------------------
# 1. the denormalising kernels
# --------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def table(dev):
    tab = torch.from_numpy(Y.table(5000.0, 97.3, 5000.0 * 1003.7, 1e-8)).to(dev)
    assert all(math.frexp(float(x))[0] != 0.5 for x in tab[:3])                         # no power of two
    return tab


@pytest.mark.parametrize("rows", [1, 63, 257, 1000])
def test_scatter_rows_affine_is_the_torch_expression_scattered(tg, dev, table, rows):
    K = tg.hip_ops
    g = torch.Generator(device="cpu").manual_seed(rows)
    cells = T0 * G0 * E0
    src = (torch.randn(rows, 8, generator=g) * 3.0).to(dev)                            # row stride 8: the padded critic output
    idx = torch.randperm(cells, generator=g)[:rows].to(dev)                              # permuted, not sorted
    want = torch.zeros(cells, device=dev)
    want[idx] = src[:, 0] * table[1] + table[0]
    got = torch.zeros(T0, G0 * E0, device=dev)
    K.scatter_rows(src, idx, got, table=table)
    plain = torch.zeros(T0, G0 * E0, device=dev)
    K.scatter_rows(src, idx, plain)
    torch.cuda.synchronize()
    assert torch.equal(bits(got.view(-1)), bits(want))
    untouched = torch.ones(cells, dtype=torch.bool, device=dev)
    untouched[idx] = False
    assert int(untouched.sum()) == cells - rows and not bool(got.view(-1)[untouched].any())     # padded grid entries stay 0
    assert torch.equal(plain.view(-1)[idx], src[:, 0]) and not bool(plain.view(-1)[untouched].any())
    assert torch.equal(bits(got.view(-1)), bits(torch.from_numpy(np.where(untouched.cpu().numpy(), np.float32(0),
                                                                           Y.denormalize(plain.view(-1).cpu().numpy(), table.cpu().numpy())))))


@pytest.mark.parametrize("n", [1, 63, 257, 1000])
def test_boot_values_affine_is_the_denormalised_product(tg, dev, table, n):
    K = tg.hip_ops
    g = torch.Generator(device="cpu").manual_seed(100 + n)
    out8 = (torch.randn(n, 8, generator=g) * 3.0).to(dev)
    v = out8[:, 0]                                                                       # stride 8
    timeout = (torch.rand(n, generator=g) < 0.5).to(torch.uint8)
    timeout[0] = 1
    if n > 1:
        timeout[1] = 0
        assert 0 < int(timeout.sum()) < n                                                # timeouts of both kinds
    timeout = timeout.to(dev)
    want = torch.mul(v * table[1] + table[0], timeout)
    got = K.boot_values_affine(v, timeout, table, out=torch.full((n,), float("nan"), device=dev))
    torch.cuda.synchronize()
    assert torch.equal(bits(got), bits(want))
    assert not bool(got[timeout == 0].any()) and bool((got[timeout == 1] != 0).all())
    ident = torch.tensor([0.0, 1.0, 1.0, 0.0], device=dev)
    assert torch.equal(K.boot_values_affine(v, timeout, ident), torch.mul(v, timeout))   # the identity table: today's product


# --------------------------------------------------------------------------------------------------------------------------------
# 2. the merge kernel
# --------------------------------------------------------------------------------------------------------------------------------
def _dev_stats(dev, count, mean, m2):
    return [torch.tensor([x], dtype=torch.float64, device=dev) for x in (count, mean, m2)]


def test_merge_kernel_runs_the_restatements_operations_bit_for_bit(tg, dev):
    """The kernel is compiled with contraction off and IEEE f64 divide / sqrt, the restatement rounds every NumPy float64 operation
    on its own: the same operations in the same order, so the bar is the bits, not the derived bound."""
    K = tg.hip_ops
    rng = np.random.default_rng(11)
    eps = 1e-8
    batches = [100.0 + 30.0 * rng.normal(size=n) for n in (4177, 160, 1, 20011)] + [np.full(7, 3.25), 1e-3 * rng.normal(size=50)]
    count, mean, m2 = 0.0, 0.0, 0.0
    stat = _dev_stats(dev, count, mean, m2)
    tab = torch.full((4,), float("nan"), device=dev)
    for i, r in enumerate(batches):
        mom = Y.moments(r)
        count, mean, m2 = Y.merge(count, mean, m2, mom)
        norm8 = torch.arange(8, dtype=torch.float32, device=dev) + 0.25
        K.value_norm_merge(torch.from_numpy(mom).to(dev), eps, *stat, tab, norm8 if i % 2 == 0 else None)
        torch.cuda.synchronize()
        want_tab = Y.table(count, mean, m2, eps)
        assert float(stat[0]) == count, i
        assert torch.equal(bits(stat[1]), bits(torch.tensor([mean], dtype=torch.float64))), (i, float(stat[1]), mean)
        assert torch.equal(bits(stat[2]), bits(torch.tensor([m2], dtype=torch.float64))), (i, float(stat[2]), m2)
        assert torch.equal(bits(tab), bits(torch.from_numpy(want_tab))), (i, tab.tolist(), want_tab.tolist())
        if i % 2 == 0:                                                                   # entries 2 and 3, the other six keep their bits
            want8 = torch.arange(8, dtype=torch.float32) + 0.25
            want8[2], want8[3] = float(want_tab[0]), float(want_tab[2])
            assert torch.equal(bits(norm8), bits(want8))
    assert count == float(sum(b.size for b in batches))
    # NULL moments (frozen, set, load_state) and an empty batch: the statistics' bits stand, the table is rewritten from them
    kept = [bits(t) for t in stat]
    for mom in (None, torch.tensor([0.0, 5.0, 25.0], dtype=torch.float64, device=dev)):
        tab.fill_(float("nan"))
        norm8 = torch.arange(8, dtype=torch.float32, device=dev) + 0.25
        K.value_norm_merge(mom, eps, *stat, tab, norm8)
        torch.cuda.synchronize()
        assert all(torch.equal(a, bits(t)) for a, t in zip(kept, stat))
        assert torch.equal(bits(tab), bits(torch.from_numpy(Y.table(count, mean, m2, eps))))
        assert norm8[2] == tab[0] and norm8[3] == tab[2] and norm8[[0, 1, 4, 5, 6, 7]].tolist() == [0.25, 1.25, 4.25, 5.25, 6.25, 7.25]
    # count == 0: the identity table, whatever mean and m2 hold
    stat = _dev_stats(dev, 0.0, 5.0, 2.0)
    K.value_norm_merge(None, eps, *stat, tab)
    torch.cuda.synchronize()
    assert tab.tolist() == [0.0, 1.0, 1.0, 0.0]
    # ValueNorm on the device: set() and the merge go through the same launch
    vn = tg.GaussianActorCritic_NeuralNetwork(5, 1, (64, 64), device=dev, normalize_value=True).value_norm
    ptr = vn.table.data_ptr()
    vn.set(*TABLE)
    torch.cuda.synchronize()
    assert vn.table.data_ptr() == ptr and np.array_equal(vn.table.cpu().numpy(), Y.table(TABLE[2], TABLE[0], TABLE[1] * TABLE[2], 1e-8))


# --------------------------------------------------------------------------------------------------------------------------------
# 3. the whole step, frozen
# --------------------------------------------------------------------------------------------------------------------------------
def _learner(tg, dev, name, kind, normalize_value, updates, monte_carlo, batch_size, boot, seed=5):
    """Policy, manager, sampled buffer and PPO from fixed seeds: two calls give bit-identical weights and trajectories."""
    S, A, hidden, cov = FACTORY[name]
    cdt = torch.bfloat16 if kind == "bf16" else None
    torch.manual_seed(seed)
    pol = tg.GaussianActorCritic_NeuralNetwork(S, A, hidden, cov=cov, device=dev, **({"normalize_value": True} if normalize_value else {}))
    mgr = tg.RolloutManager(lambda: make_env(tg, name, T0), pol, num_workers=G0,
                            num_episodes_per_worker=E0, seed=9, compute_dtype=cdt)
    buf = tg.Rollout_Buffer(mgr)
    buf.sample()
    algo = tg.PPO(epsilon=0.2, policy=pol, optimizer=torch.optim.Adam(pol.parameters(), lr=2e-4), ref_model=None,
                  updates_per_iter=updates, gamma=0.99, lam=0.95, batch_size=batch_size, monte_carlo=monte_carlo, seed=3,
                  autocast_dtype=cdt, fused_mlp=kind != "autograd", bootstrap_truncated=boot)
    if kind == "layer":                                       # the per-layer GEMM path at the factories' shape
        for net in (pol.actor, pol.critic):
            assert algo._mlp(net).disable_f32_chain()
    return pol, mgr, buf, algo


def _check_kind(algo, pol, kind):
    m_a, m_c = algo._mlp(pol.actor), algo._mlp(pol.critic)
    if kind == "autograd":
        assert m_a is None and m_c is None
    elif kind == "f32":
        assert m_a._f32 is not None and m_c._f32 is not None
    elif kind == "bf16":
        assert m_a._chain is not None and m_a._bchain is not None and m_c._bchain is not None
    else:
        assert m_a._f32 is None and m_a._chain is None and m_c._f32 is None and m_a.cd == torch.float32


FROZEN = [("f32", "CartPole", True, None, False), ("f32", "QuadPole2D", False, None, True), ("bf16", "QuadPole2D", True, None, True),
          ("bf16", "CartPole", False, None, False), ("layer", "CartPole", False, None, True), ("layer", "QuadPole2D", True, None, False),
          ("f32", "CartPole", False, 512, True), ("autograd", "CartPole", False, None, True)]


@pytest.mark.parametrize("kind,name,monte_carlo,batch_size,boot", FROZEN,
                         ids=[f"{k}-{n}-{'mc' if m else 'gae'}{'-mb' if b else ''}{'-boot' if t else ''}" for k, n, m, b, t in FROZEN])
def test_frozen_learn_equals_a_plain_learn_with_a_patched_prologue(tg, dev, monkeypatch, kind, name, monte_carlo, batch_size, boot):
    """Everything after the prologue is the plain learner's code: what the feature changes is three numbers' worth of prologue.  The
    plain learner's prologue is patched HERE, in torch: after hip_ops.scatter_rows the scattered entries become v * t1 + t0 (two
    torch kernels), tg_ppo_norm's entries 2 and 3 are overwritten with t0 and t2, and the bootstrap product is taken of the
    denormalised values.  Bit for bit in every actor and critic weight and in last_stats' losses."""
    K, A = tg.hip_ops, tg.algorithms
    pol_on, mgr_on, buf_on, algo_on = _learner(tg, dev, name, kind, True, 2, monte_carlo, batch_size, boot)
    vn = pol_on.value_norm
    vn.set(*TABLE)
    vn.freeze()
    tab = vn.table.clone()
    kept = [bits(t) for t in (vn.count, vn.mean, vn.m2, vn.table)]
    algo_on.learn(buf_on)
    torch.cuda.synchronize()
    _check_kind(algo_on, pol_on, kind)
    assert all(torch.equal(a, bits(t)) for a, t in zip(kept, (vn.count, vn.mean, vn.m2, vn.table)))      # frozen: not a bit moved
    # (built only now, as in test_obs_norm_gpu.py: a learner built before another learner's Adam step sees its raw-write count move)
    pol_off, mgr_off, buf_off, algo_off = _learner(tg, dev, name, kind, False, 2, monte_carlo, batch_size, boot)
    t_on, t_off = buf_on.device_traj, buf_off.device_traj
    for a, b in zip((t_on.obs, t_on.act, t_on.rew, t_on.mask, t_on.len), (t_off.obs, t_off.act, t_off.rew, t_off.mask, t_off.len)):
        assert torch.equal(a, b)
    assert int(t_on.len.min()) < T0 and int(t_on.mask.sum()) < T0 * t_on.n              # ragged masks
    calls = {"scatter": 0, "norm": 0, "mul": 0}
    scatter_rows, ppo_norm, mul = K.scatter_rows, K.ppo_norm, torch.mul

    def scatter_then_affine(src, idx, dst, table=None):
        assert table is None
        scatter_rows(src, idx, dst)
        flat = dst.view(-1)
        flat[idx] = flat[idx] * tab[1] + tab[0]
        calls["scatter"] += 1

    def norm_then_overwrite(moments, c1, kl, out=None):
        out = ppo_norm(moments, c1, kl, out=out)
        out[2], out[3] = tab[0], tab[2]
        calls["norm"] += 1
        return out

    def mul_denormalised(a, b, *, out=None):
        if torch.is_tensor(b) and b.dtype == torch.uint8 and out is not None:           # _bootstrap_values' product, nothing else
            calls["mul"] += 1
            a = a * tab[1] + tab[0]
        return mul(a, b, out=out)

    monkeypatch.setattr(K, "scatter_rows", scatter_then_affine)
    monkeypatch.setattr(K, "ppo_norm", norm_then_overwrite)
    monkeypatch.setattr(torch, "mul", mul_denormalised)
    try:
        algo_off.learn(buf_off)
        torch.cuda.synchronize()
    finally:
        monkeypatch.undo()
    assert calls == {"scatter": 1, "norm": 1, "mul": int(boot)}
    assert torch.equal(bits(algo_on.norm8), bits(algo_off.norm8)) and algo_on.norm8[2] == tab[0] and algo_on.norm8[3] == tab[2]
    if boot:
        b_on = algo_on._small_bufs["boot_value"]
        assert torch.equal(bits(b_on), bits(algo_off._small_bufs["boot_value"]))
        timeout = algo_on._small_bufs["boot_timeout"]
        assert 0 < int(timeout.sum()) < t_on.n and bool((b_on[timeout == 1] != 0).all())  # timeouts of both kinds
    for k, (p, q) in enumerate(zip(pol_on.parameters(), pol_off.parameters())):
        assert torch.equal(bits(p), bits(q)), k
    s_on, s_off = algo_on.last_stats, algo_off.last_stats
    for key in ("actor_loss", "critic_loss", "kl_div", "total_loss", "n_valid"):
        assert s_on[key] == s_off[key], key
    assert s_on["value_mean"] == TABLE[0] and s_on["value_count"] == TABLE[2] and "value_mean" not in s_off
    assert s_on["value_std"] == math.sqrt(TABLE[1] * TABLE[2] / TABLE[2] + 1e-8)
    # ... and the numbers are not the plain learner's own: an unpatched plain learn() ends elsewhere
    pol_raw, _, buf_raw, algo_raw = _learner(tg, dev, name, kind, False, 2, monte_carlo, batch_size, boot)
    algo_raw.learn(buf_raw)
    torch.cuda.synchronize()
    assert not all(torch.equal(p, q) for p, q in zip(pol_on.critic.parameters(), pol_raw.critic.parameters()))


# --------------------------------------------------------------------------------------------------------------------------------
# 4. the whole step, unfrozen
# --------------------------------------------------------------------------------------------------------------------------------
def _expected_moments(tg, algo, traj, table, boot_params=None):
    """The moments [2][3] learn() is about to form, recomputed outside it: the critic's no-grad pass on the valid rows (the learner's
    own path on freshly built weight layouts), denormalised with `table` in torch and scattered onto a zeroed [T][n] grid, then
    K.ppo_returns.  -> (moments, moments had the critic's RAW outputs been used)."""
    K = tg.hip_ops
    critic = algo.policy.critic
    m = algo._mlp(critic)
    m.refresh(force=True)
    idx = traj.mask.reshape(-1).nonzero().squeeze(1)
    X = traj.obs_rows().index_select(0, idx).float().contiguous()
    raw = m.forward(m.prepare_input(X), keep=False, padded=True)[:, 0].clone()
    out = []
    for v in (raw * table[1] + table[0], raw):
        grid = torch.zeros(traj.T * traj.n, device=raw.device)
        grid[idx] = v
        adv, ret = torch.empty_like(traj.rew), torch.empty_like(traj.rew)
        out.append(K.ppo_returns(traj.rew, grid.view(traj.T, traj.n), traj.mask, algo.gamma, algo.lam, algo.monte_carlo, adv, ret))
    torch.cuda.synchronize()
    return out


def test_two_unfrozen_learns_merge_the_two_batches_moments(tg, dev):
    """GAE at QuadPole2D 10-128x3 (the fp32 chain learner), one rank: the moments learn() merges are the bits the test computes from
    the same kernels on the same inputs, so the statistics after each call are the restatement's merge of them, bit for bit."""
    K = tg.hip_ops
    pol, mgr, buf, algo = _learner(tg, dev, "QuadPole2D", "f32", True, 2, False, None, False)
    vn = pol.value_norm
    count, mean, m2 = 0.0, 0.0, 0.0
    tab_ptr = vn.table.data_ptr()
    for call in range(2):
        if call:
            buf.sample()
        traj = buf.device_traj
        assert int(traj.len.min()) < T0 == int(traj.len.max())                           # ragged masks
        entry = vn.table.clone()                                                         # the identity on the first call
        assert (entry.tolist() == [0.0, 1.0, 1.0, 0.0]) == (call == 0)
        mom, mom_raw = _expected_moments(tg, algo, traj, entry)
        algo.learn(buf)
        torch.cuda.synchronize()
        count, mean, m2 = Y.merge(count, mean, m2, mom[1].cpu().numpy())
        want_tab = Y.table(count, mean, m2, vn.eps)
        assert float(vn.count) == count and vn.table.data_ptr() == tab_ptr
        assert float(vn.mean) == mean and float(vn.m2) == m2, (call, float(vn.mean), mean, float(vn.m2), m2)
        assert np.array_equal(vn.table.cpu().numpy(), want_tab)
        # the constants the loss heads read: the advantages' are tg_ppo_norm's of THESE moments (V entered GAE denormalised), the
        # critic's target is (R - mean) / sigma of the merged statistics
        want8 = K.ppo_norm(mom, algo.c1, algo.kl_coeff)
        raw8 = K.ppo_norm(mom_raw, algo.c1, algo.kl_coeff)
        torch.cuda.synchronize()
        assert torch.equal(bits(algo.norm8[[0, 1, 4, 5, 6, 7]]), bits(want8[[0, 1, 4, 5, 6, 7]]))
        assert float(algo.norm8[2]) == float(want_tab[0]) and float(algo.norm8[3]) == float(want_tab[2])
        if call:
            assert not torch.equal(want8[0:2], raw8[0:2])                                # (raw critic outputs would have shown here)
        else:
            assert torch.equal(bits(mom), bits(mom_raw))                                 # (the identity table: nothing to show yet)
        # last_stats against the definitions, on the same moments
        stats = algo.last_stats
        (na, a1, a2), (nr, r1, r2) = [[np.longdouble(x) for x in row] for row in mom.cpu().tolist()]
        ev = float(1 - ((a2 - a1 * a1 / na) / na) / ((r2 - r1 * r1 / nr) / nr))
        assert stats["explained_variance"] == pytest.approx(ev, rel=1e-9, abs=1e-9) and stats["explained_variance"] < 1.0
        assert stats["value_count"] == count and stats["value_mean"] == mean and stats["value_std"] == math.sqrt(m2 / count + vn.eps)
        assert stats["n_valid"] == float(mom[1, 0])
    assert count == float(vn.count) > float(mom[1, 0])                                   # two batches went in
    # frozen from here: a third learn() leaves every bit, and still trains the critic against the frozen table
    vn.freeze()
    kept = [bits(t) for t in (vn.count, vn.mean, vn.m2, vn.table)]
    buf.sample()
    algo.learn(buf)
    torch.cuda.synchronize()
    assert all(torch.equal(a, bits(t)) for a, t in zip(kept, (vn.count, vn.mean, vn.m2, vn.table)))
    assert float(algo.norm8[2]) == float(vn.table[0]) and float(algo.norm8[3]) == float(vn.table[2])
    # policy.value() hands out returns: the critic's output through the table
    x = traj.obs_rows()[:257].float()
    with torch.no_grad():
        assert torch.equal(pol.value(x), pol.critic(x).squeeze() * vn.table[1] + vn.table[0])


# --------------------------------------------------------------------------------------------------------------------------------
# 5. checkpoint, two ranks
# --------------------------------------------------------------------------------------------------------------------------------
def test_a_checkpoint_round_trip_on_the_device_continues_bit_for_bit(tg, dev, tmp_path):
    pol, mgr, buf, algo = _learner(tg, dev, "CartPole", "f32", True, 2, False, None, True)
    algo.learn(buf)
    torch.cuda.synchronize()
    pol.save(str(tmp_path))
    algo.save(str(tmp_path))
    S, A, hidden, cov = FACTORY["CartPole"]
    torch.manual_seed(77)                                                                # other initial weights: everything comes from the files
    pol2 = tg.GaussianActorCritic_NeuralNetwork(S, A, hidden, cov=cov, device=dev, normalize_value=True)
    algo2 = tg.PPO(epsilon=0.2, policy=pol2, optimizer=torch.optim.Adam(pol2.parameters(), lr=2e-4), ref_model=None, updates_per_iter=2,
                   gamma=0.99, lam=0.95, batch_size=None, monte_carlo=False, seed=3, bootstrap_truncated=True)
    pol2.load(str(tmp_path))
    algo2.load(str(tmp_path))
    algo2.sync_old_policy()
    vn, vn2 = pol.value_norm, pol2.value_norm
    assert float(vn2.count) == float(vn.count) > 0
    for a, b in ((vn.count, vn2.count), (vn.mean, vn2.mean), (vn.m2, vn2.m2), (vn.table, vn2.table)):
        assert torch.equal(bits(a), bits(b))
    plain = tg.GaussianActorCritic_NeuralNetwork(S, A, hidden, cov=cov, device=dev)
    with pytest.raises(ValueError, match="normalize_value=True"):
        plain.load(str(tmp_path))
    buf.sample()                                                                         # the next rollout, by the first policy
    algo.learn(buf)
    algo2.learn(buf)
    torch.cuda.synchronize()
    for k, (p, q) in enumerate(zip(pol.parameters(), pol2.parameters())):
        assert torch.equal(bits(p), bits(q)), k
    for a, b in ((vn.count, vn2.count), (vn.mean, vn2.mean), (vn.m2, vn2.m2), (vn.table, vn2.table)):
        assert torch.equal(bits(a), bits(b))
    s1, s2 = algo.last_stats, algo2.last_stats
    for key in ("actor_loss", "critic_loss", "total_loss", "value_mean", "value_std", "value_count", "explained_variance", "n_bootstrapped"):
        assert s1[key] == s2[key], key


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_ranks_reproduce_the_one_rank_statistics(tmp_path):
    """tests/value_norm_dist_worker.py as fresh child processes (the harness of test_distributed_gpu.py / test_bootstrap_gpu.py: gloo,
    both ranks on cuda:0, half the groups each).  Both ranks hold the same bits.  The ranks' returns, side by side, are the one-rank
    returns (asserted bit for bit in Monte Carlo mode, where no critic pass enters them; printed for GAE); the merged statistics of
    either world size lie within Y.merge_bounds -- the f64 reordering bound of the all-reduced sums S1, S2 carried through the merge
    -- of the exact statistics of its own returns, so the two world sizes differ by at most the sum of the two bounds (plus whatever
    the exact statistics themselves differ by: zero when the returns are the same bits); count exact; the table within 1 ulp of the
    table of its own statistics; norm8[2:4] the table's entries."""
    worker = os.path.join(HERE, "value_norm_dist_worker.py")
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
        for k in ("count", "mean", "m2", "table", "norm8"):
            assert torch.equal(bits(a[k]), bits(b[k])), (case, k)
        assert a["stats"] == b["stats"] and all(torch.equal(x, y) for x, y in zip(a["weights"], b["weights"]))
        assert torch.equal(torch.cat([a["mask"], b["mask"]], 1), rec["mask"]), case
        assert not bool(rec["mask"].all()) and bool(rec["mask"][-1].any())                  # ragged masks
        both = torch.cat([a["returns"], b["returns"]], 1)
        print(case, "the ranks' returns are the one-rank returns bit for bit:", bool(torch.equal(both, rec["returns"])))
        if case.endswith("_mc"):
            assert torch.equal(both, rec["returns"]), case
        exact, bound = {}, {}
        for w, x, grid in ((1, rec, rec["returns"]), (2, a, both)):
            r = grid[rec["mask"]].double().numpy()
            exact[w] = (c_ref, mean_ref, m2_ref) = Y.exact([r])
            bound[w] = (e_mean, e_m2) = Y.merge_bounds([r])
            count, mean, m2 = float(x["count"]), float(x["mean"]), float(x["m2"])
            print(case, "world", w, "err mean / bound", abs(mean - mean_ref) / e_mean, "err m2 / bound", abs(m2 - m2_ref) / e_m2)
            assert count == c_ref == x["stats"]["n_valid"] == x["stats"]["value_count"]
            assert abs(mean - mean_ref) <= e_mean + Y.U * abs(mean) and abs(m2 - m2_ref) <= e_m2 + Y.U * abs(m2), (case, w)
            want = Y.table(count, mean, m2, x["eps"])
            assert np.all(np.abs(x["table"].numpy().astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64))
            assert x["norm8"][2] == x["table"][0] and x["norm8"][3] == x["table"][2]
            assert x["stats"]["value_mean"] == mean and x["stats"]["value_std"] == math.sqrt(m2 / count + x["eps"])
        assert abs(float(a["mean"]) - float(rec["mean"])) <= bound[1][0] + bound[2][0] + abs(exact[1][1] - exact[2][1])
        assert abs(float(a["m2"]) - float(rec["m2"])) <= bound[1][1] + bound[2][1] + abs(exact[1][2] - exact[2][2])
        assert a["stats"]["explained_variance"] == pytest.approx(rec["stats"]["explained_variance"], rel=1e-9, abs=1e-12)
        for x, y in zip(a["weights"], rec["weights"]):
            assert float((x.double() - y.double()).norm()) <= 1e-6 * float(y.double().norm()), case
