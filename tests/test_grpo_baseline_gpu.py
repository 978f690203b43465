"""GRPO(baseline="step") on the GPU: tg_grpo_step_advantage against the NumPy restatement of its own order bit for bit and against
the order-free float64 version within its derived bounds (tests/grpo_baseline_fp64.py); learn() end to end against a default GRPO
fed the restatement's array, bit for bit, on every learner path; the default path untouched; two ranks; baseline_explained."""
import copy
import math
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import grpo_baseline_fp64 as F

HERE = os.path.dirname(os.path.abspath(__file__))
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tg():
    import trajopt_grpo_amd
    return trajopt_grpo_amd


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


# ------------------------------------------------------------------------------------------------------------------------------
# 1. the kernel
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", F.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_equals_the_restatement_bit_for_bit(tg, dev, shape):
    K = tg.hip_ops
    worst = 0.0
    for mk in F.MASKS:
        for vk in F.VALUES:
            R, mask, E = F.case(shape, mk, vk)
            Rd, md = torch.from_numpy(R).to(dev), torch.from_numpy(mask).to(dev)
            for scale in (True, False):
                tag = f"{shape} {mk} {vk} scale={scale}"
                A1, g1 = K.grpo_step_advantage(Rd, md, E, scale=scale)
                A2, g2 = K.grpo_step_advantage(Rd, md, E, scale=scale)
                A1, g1, A2, g2 = (x.cpu().numpy() for x in (A1, g1, A2, g2))
                assert np.array_equal(A1.view(np.uint32), A2.view(np.uint32)) and np.array_equal(g1.view(np.uint64), g2.view(np.uint64)), tag
                assert np.isfinite(A1).all() and np.isfinite(g1).all(), tag
                A, group, _ = F.kernel_order(R, mask, E, scale)
                bad = A1.view(np.uint32) != A.view(np.uint32)
                assert not bad.any(), f"{tag}: {int(bad.sum())} of {bad.size} advantages differ, first at {np.argwhere(bad)[0]}: " \
                                      f"{A1[bad][0]!r} vs {A[bad][0]!r}"
                assert np.array_equal(g1.view(np.uint64), group.view(np.uint64)), f"{tag}: {{Q, C, K}} {g1} vs {group}"
                worst = max(worst, F.check_against_order_free(tag, A1, g1, R, mask, E, scale))
                if vk in ("constant", "zeros") or E == 1:               # exactly +0 everywhere, never NaN / Inf
                    assert not A1.view(np.uint32).any() and not g1[:, 0].any(), tag
    print(f"{shape}: worst |kernel - fp64| / bound = {worst:.3f}")


def test_unaligned_views_take_the_scalar_loads(tg, dev):
    """E % 4 == 0 but the arrays start 4 B / 1 B past a 16-B boundary: the same bits as the aligned call."""
    K = tg.hip_ops
    R, mask, E = F.case((9, 2, 64), "holes", "offset")
    T, n = R.shape
    Rb, mb = torch.zeros(T * n + 1, device=dev), torch.zeros(T * n + 1, dtype=torch.uint8, device=dev)
    Rb[1:] = torch.from_numpy(R).to(dev).reshape(-1)
    mb[1:] = torch.from_numpy(mask).to(dev).reshape(-1)
    A, group, _ = F.kernel_order(R, mask, E, True)
    A1, g1 = K.grpo_step_advantage(Rb[1:].view(T, n), mb[1:].view(T, n), E, scale=True)
    assert np.array_equal(A1.cpu().numpy().view(np.uint32), A.view(np.uint32)) and np.array_equal(g1.cpu().numpy(), group)


# ------------------------------------------------------------------------------------------------------------------------------
# 2. learn() end to end
# ------------------------------------------------------------------------------------------------------------------------------
def _restated(algo, scale):
    """A default GRPO whose advantage source is the restatement's array (gathered as it is: no moments)."""
    def source(traj, rtg, moments):
        A, _, _ = F.kernel_order(rtg.cpu().numpy(), traj.mask.cpu().numpy(), traj.E, scale)
        return torch.from_numpy(A).to(rtg.device), None, 0
    algo._advantage_source = source
    return algo


def _native_path(algo, pol):
    m = algo._mlp(pol.actor)
    if m is None:
        return "autograd"
    if m._f32 is not None:
        return "f32_resident" if m._f32.res else ("f32_wide" if m._f32.wide else "f32_chain")
    if m._chain is not None and m._bchain is not None:
        return "bf16_chain"
    return "per_layer"


# name -> (env, T, S, A, hidden, restart, adv_scale, GRPO keywords, the path that must run)
LEARN_CASES = {
    "f32_chain": ("CartPole", 32, 5, 1, (64, 64), False, "std", {}, "f32_chain"),
    "f32_resident": ("CartPole", 32, 5, 1, (128, 128), False, "std", {}, "f32_resident"),
    "f32_resident_none": ("CartPole", 32, 5, 1, (128, 128), False, "none", {}, "f32_resident"),
    "bf16_chain": ("CartPole", 32, 5, 1, (128, 128, 128), False, "std", {"autocast_dtype": torch.bfloat16}, "bf16_chain"),
    "per_layer": ("CartPole", 32, 5, 1, (96, 96), False, "std", {}, "per_layer"),
    "autograd": ("CartPole", 32, 5, 1, (64, 64), False, "std", {"fused_mlp": False}, "autograd"),
    "three_chunks": ("CartPole", 32, 5, 1, (64, 64), False, "std", {"chunk_rows": "rows/3"}, "f32_chain"),
    "ref_model": ("CartPole", 32, 5, 1, (128, 128), False, "std", {"ref_model": True, "beta": 0.5}, "f32_resident"),
    "quadpole_restart": ("QuadPole", 16, 20, 4, (64, 64), True, "std", {}, "f32_chain"),
    # a swarm env (E counts env slots: 16 episodes x 2 agents), and the other learner options together
    "swarm_restart": ("QuadPoleSwarm", 16, 20, 4, (64, 64), True, "std", {}, "f32_chain"),
    "options": ("CartPole", 32, 5, 1, (64, 64), False, "std",
                {"policy_kw": {"learn_std": True, "normalize_obs": True}, "max_grad_norm": 0.5, "kl_stats": True}, "f32_chain"),
}


@pytest.mark.parametrize("name", sorted(LEARN_CASES))
def test_learn_equals_a_default_learner_fed_the_restatement(tg, dev, name):
    env_name, T, S, A, hidden, restart, adv_scale, kw, path = LEARN_CASES[name]
    kw = dict(kw)
    G, E = 8, 16
    torch.manual_seed(31)
    pols = [tg.GaussianActor_NeuralNetwork(S, A, hidden, cov=0.5, device=dev, **kw.pop("policy_kw", {}))]
    pols.append(copy.deepcopy(pols[0]))
    agents = 2 if env_name == "QuadPoleSwarm" else 1
    env_cls = (lambda max_steps: tg.QuadPoleSwarm(n_agents=2, max_steps=max_steps)) if agents > 1 else getattr(tg, env_name)
    cdt = {"compute_dtype": torch.bfloat16} if kw.get("autocast_dtype") is torch.bfloat16 else {}
    bufs = [tg.Rollout_Buffer(tg.RolloutManager(lambda: env_cls(max_steps=T), p, num_workers=G, num_episodes_per_worker=E, seed=5,
                                                restart=restart, **cdt)) for p in pols]
    for b in bufs:
        b.sample()
    t0, t1 = bufs[0].device_traj, bufs[1].device_traj
    assert torch.equal(t0.mask, t1.mask) and torch.equal(t0.rew, t1.rew) and (t0.T, t0.n, t0.E) == (T, G * E * agents, E * agents)
    rows = int(t0.mask.sum())
    if kw.get("chunk_rows") == "rows/3":
        kw["chunk_rows"] = -(-rows // 3)
        assert math.ceil(rows / kw["chunk_rows"]) == 3
    beta = kw.pop("beta", 0.0)
    algos = []
    for i, p in enumerate(pols):
        extra = dict(kw)
        if extra.pop("ref_model", False):
            torch.manual_seed(77)                                        # the same perturbed reference policy for both learners
            ref = copy.deepcopy(p)
            with torch.no_grad():
                for q in ref.actor.parameters():
                    q.add_(0.05 * torch.randn_like(q) * (q.abs().mean() + 1e-3))
            extra["ref_model"] = ref
        step = {"baseline": "step", "adv_scale": adv_scale} if i == 0 else {}
        algos.append(tg.GRPO(epsilon=0.2, beta=beta, gamma=0.9, policy=p, optimizer=torch.optim.Adam(p.parameters(), lr=3e-4),
                             updates_per_iter=2, **extra, **step))
    _restated(algos[1], adv_scale == "std")
    before = [q.detach().clone() for q in pols[0].parameters()]
    for it in range(2):
        if it:
            for b in bufs:
                b.sample()
            assert torch.equal(bufs[0].device_traj.mask, bufs[1].device_traj.mask) and torch.equal(bufs[0].device_traj.rew, bufs[1].device_traj.rew)
        stats = []
        for a, b in zip(algos, bufs):
            a.learn(b)
            stats.append(a.last_stats)
        assert _native_path(algos[0], pols[0]) == _native_path(algos[1], pols[1]) == path
        assert len(stats[0]["J"]) == 2 and stats[0]["J"] == stats[1]["J"], (name, it, stats[0]["J"], stats[1]["J"])
        assert all(math.isfinite(j) for j in stats[0]["J"])
        for (n_, x), y in zip(pols[0].actor.named_parameters(), pols[1].actor.parameters()):
            assert torch.equal(x, y), f"{name}: learn() {it}: {n_} differs from the learner fed the restatement"
        if getattr(pols[0], "log_std", None) is not None:
            assert torch.equal(pols[0].log_std, pols[1].log_std), f"{name}: learn() {it}: log_std"
        assert stats[0]["baseline"] == "step" and "baseline" not in stats[1]
        assert stats[0]["baseline_explained"] <= 1.0 + 1e-12
    assert any(not torch.equal(x, y) for x, y in zip(pols[0].parameters(), before)), "the updates moved nothing"


# ------------------------------------------------------------------------------------------------------------------------------
# 3. the default path
# ------------------------------------------------------------------------------------------------------------------------------
def test_default_path_never_reaches_the_new_entry_point(tg, dev, monkeypatch):
    calls = []
    plain = tg.hip_ops.grpo_step_advantage
    monkeypatch.setattr(tg.hip_ops, "grpo_step_advantage", lambda *a, **k: (calls.append(1), plain(*a, **k))[1])
    torch.manual_seed(9)
    pols = [tg.GaussianActor_NeuralNetwork(5, 1, (128, 128), cov=0.5, device=dev)]
    pols += [copy.deepcopy(pols[0]), copy.deepcopy(pols[0])]
    kws = [{}, {"baseline": "group"}, {"baseline": "step"}]
    counts = []
    for p, kw in zip(pols, kws):
        buf = tg.Rollout_Buffer(tg.RolloutManager(lambda: tg.CartPole(max_steps=32), p, num_workers=8, num_episodes_per_worker=16, seed=3))
        buf.sample()
        algo = tg.GRPO(epsilon=0.2, beta=0.0, gamma=0.9, policy=p, optimizer=torch.optim.Adam(p.parameters(), lr=3e-4), updates_per_iter=2, **kw)
        del calls[:]
        algo.learn(buf)
        st = algo.last_stats
        counts.append(len(calls))
        assert ("baseline" in st) == (kw.get("baseline") == "step")
    assert counts == [0, 0, 1]
    for x, y, z in zip(*(p.parameters() for p in pols)):
        assert torch.equal(x, y)
    assert any(not torch.equal(x, z) for x, z in zip(pols[0].parameters(), pols[2].parameters())), "the step baseline changed nothing"


# ------------------------------------------------------------------------------------------------------------------------------
# 4. two ranks
# ------------------------------------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_ranks_equal_one_rank(tmp_path):
    """tests/grpo_baseline_dist_worker.py as fresh child processes (the harness of test_distributed_gpu.py: gloo, both ranks on cuda:0,
    half the groups each).  Groups are whole on a rank: each shard's advantages are the one-rank run's columns bit for bit; the
    post-update weights agree to that harness's 1e-6 (relative L2) of an fp32 GRPO learner; both ranks report the same statistics."""
    worker = os.path.join(HERE, "grpo_baseline_dist_worker.py")
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
        n = rec["adv"].shape[1]
        assert a["adv"].shape[1] == b["adv"].shape[1] == n // 2 and (n // 2) % rec["E"] == 0
        for r, shard in enumerate((a, b)):
            cols = slice(r * n // 2, (r + 1) * n // 2)
            assert torch.equal(shard["mask"], rec["mask"][:, cols]), f"{case}: rank {r}'s trajectory shard"
            assert torch.equal(shard["adv"].view(torch.int32), rec["adv"][:, cols].contiguous().view(torch.int32)), f"{case}: rank {r}'s advantages"
        assert rec["mask"].any() and rec["adv"].abs().max() > 0
        assert all(torch.equal(x, y) for x, y in zip(a["weights"], b["weights"])) and a["J"] == b["J"]
        assert a["baseline"] == rec["baseline"] == "step" and a["baseline_explained"] == b["baseline_explained"]
        assert abs(a["baseline_explained"] - rec["baseline_explained"]) <= 1e-9
        for x, y in zip(a["weights"], rec["weights"]):
            assert float((x.double() - y.double()).norm()) <= 1e-6 * float(y.double().norm()), case
        print(case, "J", rec["J"], a["J"], "baseline_explained", rec["baseline_explained"])


# ------------------------------------------------------------------------------------------------------------------------------
# 5. baseline_explained
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["per_episode", "per_step"])
def test_baseline_explained_is_0_for_per_episode_returns_and_1_for_per_step_returns(tg, dev, kind):
    """gamma = 0 makes the return-to-go the reward itself; every (t, e) valid.  Returns that do not depend on t: the step means are
    the group mean, nothing is explained -- 0 up to the rounding of b to float32 (relative 2 u |mean| / std per residual, < 1e-5 at
    |mean| / std <= 10).  Returns that depend on t alone: every residual is exactly +0, Q = 0, explained = 1 exactly."""
    torch.manual_seed(13)
    G, E, T = 4, 16, 12
    pol = tg.GaussianActor_NeuralNetwork(5, 1, (64, 64), cov=0.5, device=dev)
    buf = tg.Rollout_Buffer(tg.RolloutManager(lambda: tg.CartPole(max_steps=T), pol, num_workers=G, num_episodes_per_worker=E, seed=2))
    buf.sample()
    traj = buf.device_traj
    gen = torch.Generator().manual_seed(4)
    traj.mask.fill_(1)                                                   # a hand-built trajectory: the mask itself is counted
    traj.host_valid_rows = None
    traj.obs.copy_(torch.randn(traj.obs.shape, generator=gen).to(traj.obs))
    traj.act.copy_(torch.randn(traj.act.shape, generator=gen).to(traj.act))
    if kind == "per_episode":
        rew = torch.randn(1, G * E, generator=gen).expand(T, G * E)
    else:
        rew = torch.randn(T, 1, generator=gen).expand(T, G * E)
    traj.rew.copy_(rew.to(traj.rew))
    algo = tg.GRPO(epsilon=0.2, beta=0.0, gamma=0.0, policy=pol, optimizer=torch.optim.Adam(pol.parameters(), lr=3e-4), updates_per_iter=1,
                   baseline="step")
    algo.learn(buf)
    got = algo.last_stats["baseline_explained"]
    print(kind, got)
    if kind == "per_episode":
        assert abs(got) < 1e-5
    else:
        assert got == 1.0
