"""PopArt on the MI355X (policies: normalize_value=True, popart=True; tg_value_norm_merge_popart; run with `-m gpu`):

  1. the kernel against tests/popart_fp64.py: the head bit for bit, the statistics / table / norm8 bit for bit what tg_value_norm_merge
     writes on the same inputs -- at hidden 8 (248 idle threads), 32, 256 (exactly one trip), 264 (a second, ragged trip) and 2048;
  2. the device's own rescaled heads preserve the denormalised outputs of 64 hidden rows within the restatement's bound;
  3. learn() against a twin: a plain normalize_value learner whose _merge the test wraps (the original call, then the head rewritten
     on the host from the restatement through torch, so that the version keys move) -- bit for bit in every weight, statistic and
     last_stats entry after three learn() calls, on every critic path.  A derived layout left stale shows here;
  4. frozen statistics: the bits of a plain normalize_value learner; popart=False never reaches the new wrapper;
  5. two ranks on one device hold identical heads and statistics; popart_scale against the one-rank run;
  6. a checkpoint loads into a PopArt policy and into a plain normalize_value policy with the same values."""
import functools
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import popart_fp64 as P
import value_norm_fp64 as Y
from value_norm_dist_worker import make_env

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
T0, G0, E0 = 32, 4, 40                      # n = 160, as tests/test_value_norm_gpu.py
EPS = 1e-8
HIDDEN = [8, 32, 256, 264, 2048]
PAD = 64                                    # sentinel floats behind the head's weights: nothing may be stored there
# statistics cases: (rescales?, eps).  History: 5000 returns of mean 100, sigma 30 (see _case)
CASES = {"empty": (False, EPS), "doubles": (True, EPS), "halves": (True, EPS), "none": (False, EPS), "n0": (False, EPS),
         "identical": (True, EPS), "eps0_flat": (False, 0.0)}


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


def _dev_stats(dev, stats):
    return [torch.tensor([x], dtype=torch.float64, device=dev) for x in stats]


# --------------------------------------------------------------------------------------------------------------------------------
# 1 / 2. the kernel
# --------------------------------------------------------------------------------------------------------------------------------
def _case(name):
    """(statistics before, moments of the batch or None, eps)."""
    rng = np.random.default_rng(sorted(CASES).index(name))
    hist = 100.0 + 30.0 * rng.normal(size=5000)
    before = Y.merge(0.0, 0.0, 0.0, Y.moments(hist))
    eps = CASES[name][1]
    if name == "empty":
        return (0.0, 0.0, 0.0), Y.moments(hist), eps
    if name == "doubles":
        return before, Y.moments(180.0 + 56.0 * rng.normal(size=20000)), eps
    if name == "halves":
        return before, Y.moments(60.0 + 13.0 * rng.normal(size=200000)), eps
    if name == "none":
        return before, None, eps
    if name == "n0":
        return before, np.array([0.0, 5.0, 25.0]), eps
    if name == "identical":
        return before, Y.moments(hist), eps                      # the same mean and variance again: r rounds near 1
    flat = Y.merge(0.0, 0.0, 0.0, Y.moments(np.full(7, 3.25)))   # eps = 0, a history without variance: sigma_a = 0
    assert flat[2] == 0.0
    return flat, Y.moments(np.array([1.0, 2.0, 4.0])), eps


@functools.lru_cache(maxsize=None)
def _run(hidden, name):
    """One launch of each entry point on the case's inputs -> everything both wrote, on the host (computed once, shared by 1 and 2)."""
    import trajopt_grpo_amd as tg
    K = tg.hip_ops
    dev = torch.device("cuda", 0)
    before, mom, eps = _case(name)
    rng = np.random.default_rng(1000 + hidden)
    w = (rng.normal(size=hidden) / np.sqrt(hidden)).astype(np.float32)
    b = np.array([0.3], dtype=np.float32)
    with_norm8 = (hidden + sorted(CASES).index(name)) % 2 == 0
    mom_d = None if mom is None else torch.from_numpy(np.asarray(mom, dtype=np.float64)).to(dev)
    out = {}
    for which in ("plain", "popart"):
        stat = _dev_stats(dev, before)
        tab = torch.full((4,), float("nan"), device=dev)
        norm8 = (torch.arange(8, dtype=torch.float32, device=dev) + 0.25) if with_norm8 else None
        if which == "plain":
            K.value_norm_merge(mom_d, eps, *stat, tab, norm8)
        else:
            big = torch.full((hidden + PAD,), -7.5, device=dev)
            big[:hidden] = torch.from_numpy(w).to(dev)
            bias = torch.from_numpy(np.array([b[0], -7.5], dtype=np.float32)).to(dev)
            K.value_norm_merge_popart(mom_d, eps, *stat, tab, norm8, big[:hidden].view(1, hidden), bias[:1])
            torch.cuda.synchronize()
            out["w"], out["b"] = big[:hidden].cpu().numpy().copy(), bias[:1].cpu().numpy().copy()
            out["guard"] = torch.cat([big[hidden:], bias[1:]]).cpu()
        torch.cuda.synchronize()
        out[which] = {"stat": [t.cpu().clone() for t in stat], "table": tab.cpu().clone(), "norm8": None if norm8 is None else norm8.cpu().clone()}
    out.update(w0=w, b0=b, before=before, mom=mom, eps=eps, with_norm8=with_norm8)
    return out


@pytest.mark.parametrize("hidden", HIDDEN)
def test_the_kernel_is_the_restatement_and_its_merge_is_the_plain_merge(tg, hidden):
    seen8 = set()
    for name, (moves, _) in CASES.items():
        r = _run(hidden, name)
        plain, pop = r["plain"], r["popart"]
        for a, b in zip(plain["stat"], pop["stat"]):
            assert torch.equal(bits(a), bits(b)), name
        assert torch.equal(bits(plain["table"]), bits(pop["table"])), name
        seen8.add(r["with_norm8"])
        if r["with_norm8"]:
            assert torch.equal(bits(plain["norm8"]), bits(pop["norm8"])), name
            assert pop["norm8"][2] == pop["table"][0] and pop["norm8"][3] == pop["table"][2]
        (after, table, w1, b1) = P.merge_and_rescale(*r["before"], r["mom"], r["eps"], r["w0"], r["b0"])
        assert tuple(float(t) for t in pop["stat"]) == after, name
        assert np.array_equal(pop["table"].numpy().view(np.int32), table.view(np.int32)), name
        assert P.rescaled(r["before"], after, r["eps"]) == moves, name
        assert np.array_equal(r["w"].view(np.int32), w1.view(np.int32)), name
        assert np.array_equal(r["b"].view(np.int32), b1.view(np.int32)), name
        if moves:
            if name != "identical":
                assert not np.array_equal(r["b"], r["b0"]) and not np.any(r["w"] == r["w0"]), name
            else:                                                 # r within a few ulp of 1: the weights move by an ulp at the most
                sa, sn = float(P.sigma(r["before"], r["eps"])), float(P.sigma(after, r["eps"]))
                assert abs(sa / sn - 1.0) < 1e-12 and np.all(np.abs(r["w"] - r["w0"]) <= np.spacing(np.abs(r["w0"])))
        else:
            assert np.array_equal(r["w"].view(np.int32), r["w0"].view(np.int32)), name
            assert np.array_equal(r["b"].view(np.int32), r["b0"].view(np.int32)), name
        assert bool((r["guard"] == -7.5).all()), name            # nothing stored behind the head
    assert seen8 == {True, False}                                 # norm8 given and not given


@pytest.mark.parametrize("hidden", HIDDEN)
def test_the_device_heads_preserve_the_denormalised_outputs(tg, hidden):
    rng = np.random.default_rng(2000 + hidden)
    h = np.maximum(rng.normal(size=(64, hidden)), 0.0).astype(np.float32)
    for name, (moves, _) in CASES.items():
        if not moves:
            continue
        r = _run(hidden, name)
        before, after, eps = r["before"], tuple(float(t) for t in r["popart"]["stat"]), r["eps"]
        y, y1 = P.predict(r["w0"], r["b0"], before, eps, h), P.predict(r["w"], r["b"], after, eps, h)
        bound = P.preservation_bound(r["w"], r["b"], r["b0"], before, after, eps, h)
        err = np.abs(y1 - y).astype(np.float64)
        print(name, hidden, "max |y' - y| / bound", float((err / bound).max()))
        assert np.all(err <= bound), name
        if name != "identical":                                   # ... which the un-rescaled head misses by far
            miss = np.abs(P.predict(r["w0"], r["b0"], after, eps, h) - y).astype(np.float64)
            assert np.all(miss >= 100.0 * bound), name


# --------------------------------------------------------------------------------------------------------------------------------
# 3. learn() against a twin
# --------------------------------------------------------------------------------------------------------------------------------
# kind -> (env, obs, act, hidden, activation, compute dtype)
PATHS = {"layer": ("CartPole", 5, 1, (32, 32), "ReLU", None), "bf16": ("QuadPole", 20, 4, (128, 128, 128), "ReLU", torch.bfloat16),
         "res": ("CartPole", 5, 1, (128, 128), "ReLU", None), "chain": ("CartPole", 5, 1, (64, 64, 64), "ReLU", None),
         "wide": ("CartPole", 5, 1, (256, 256), "ReLU", None), "autograd": ("CartPole", 5, 1, (32, 32), "Tanh", None)}


def _env(tg, name):
    return tg.QuadPole(max_steps=T0) if name == "QuadPole" else make_env(tg, name, T0)


def _learner(tg, dev, kind, popart, monte_carlo=True, batch_size=None, boot=False, normalize_value=True):
    """Policy, manager, buffer and PPO from fixed seeds: two calls give bit-identical weights and trajectories."""
    name, S, A, hidden, act, cdt = PATHS[kind]
    torch.manual_seed(5)
    kw = {"normalize_value": True} if normalize_value else {}
    if popart:
        kw["popart"] = True
    pol = tg.GaussianActorCritic_NeuralNetwork(S, A, hidden, activation=act, cov=0.5, device=dev, **kw)
    mgr = tg.RolloutManager(lambda: _env(tg, name), pol, num_workers=G0, num_episodes_per_worker=E0, seed=9, compute_dtype=cdt)
    buf = tg.Rollout_Buffer(mgr)
    algo = tg.PPO(epsilon=0.2, policy=pol, optimizer=torch.optim.Adam(pol.parameters(), lr=2e-4), ref_model=None, updates_per_iter=2,
                  gamma=0.99, lam=0.95, batch_size=batch_size, monte_carlo=monte_carlo, seed=3, autocast_dtype=cdt, bootstrap_truncated=boot)
    return pol, mgr, buf, algo


def _check_path(algo, pol, kind):
    m = algo._mlp(pol.critic)
    if kind == "autograd":
        assert m is None
    elif kind == "layer":
        assert m is not None and m._f32 is None and m._chain is None and m.cd == torch.float32
    elif kind == "bf16":
        assert m._chain is not None and m._bchain is not None
    else:
        assert type(m._f32).__name__ == {"res": "F32ResStream", "chain": "F32ChainStream", "wide": "F32WideStream"}[kind]


def _stats_of(vn):
    return float(vn.count), float(vn.mean), float(vn.m2)


def _wrap_twin(algo, pol, log):
    """The twin's _merge: the original call, then the head rewritten on the host from the restatement -- through torch, so the version
    keys move and the learner's own key-driven refresh rebuilds what was derived from it."""
    vn, head = pol.value_norm, pol.critic.network[-1]
    orig = vn._merge

    def merge(moments=None, norm8=None, head_arg=None):
        assert head_arg is None
        before = _stats_of(vn)
        orig(moments, norm8)
        after = _stats_of(vn)
        if P.rescaled(before, after, vn.eps):
            w1, b1 = P.rescale(head.weight.detach().cpu().numpy(), head.bias.detach().cpu().numpy(), before, after, vn.eps)
            with torch.no_grad():
                head.weight.copy_(torch.from_numpy(w1).to(head.weight.device))
                head.bias.copy_(torch.from_numpy(b1).to(head.bias.device))
                head.weight.add_(0.0)                             # (an in-place torch op: the version keys move)
            algo._refresh(pol.critic)
            log.append((float(P.sigma(before, vn.eps)) / float(P.sigma(after, vn.eps)), before[1] - after[1]))
        else:
            log.append((1.0, 0.0))
    vn._merge = merge


TWINS = [("layer", True, None, False), ("bf16", True, None, False), ("res", True, None, False), ("chain", True, None, False),
         ("wide", True, None, False), ("autograd", True, None, False), ("chain", True, 512, False), ("res", False, None, True)]


@pytest.mark.parametrize("kind,monte_carlo,batch_size,boot", TWINS,
                         ids=[f"{k}{'' if m else '-gae'}{'-mb' if b else ''}{'-boot' if t else ''}" for k, m, b, t in TWINS])
def test_learn_equals_a_twin_whose_head_is_rewritten_on_the_host(tg, dev, kind, monte_carlo, batch_size, boot):
    runs = {}
    log = []
    for which in ("popart", "twin"):                              # (the twin is built after the first has taken its Adam steps)
        pol, mgr, buf, algo = _learner(tg, dev, kind, which == "popart", monte_carlo, batch_size, boot)
        if which == "twin":
            _wrap_twin(algo, pol, log)
        heads, stats = [], []
        for call in range(3):
            buf.sample()
            algo.learn(buf)
            torch.cuda.synchronize()
            stats.append(algo.last_stats)
            heads.append(pol.critic.network[-1].weight.detach().clone())
        _check_path(algo, pol, kind)
        runs[which] = (pol, stats, buf.device_traj.obs.clone())
    (pol_p, stats_p, obs_p), (pol_t, stats_t, obs_t) = runs["popart"], runs["twin"]
    assert torch.equal(obs_p, obs_t)                               # the third rollout: the actors stayed the same bits too
    for k, (p, q) in enumerate(zip(pol_p.parameters(), pol_t.parameters())):
        assert torch.equal(bits(p), bits(q)), k
    vp, vt = pol_p.value_norm, pol_t.value_norm
    for a, b in ((vp.count, vt.count), (vp.mean, vt.mean), (vp.m2, vt.m2), (vp.table, vt.table)):
        assert torch.equal(bits(a), bits(b))
    assert len(log) == 3 and log[0] == (1.0, 0.0) and all(s != 1.0 and d != 0.0 for s, d in log[1:])    # the first only fills
    for call, (sp, st) in enumerate(zip(stats_p, stats_t)):
        assert set(sp) == set(st) | {"popart_scale", "popart_shift"}
        for key in st:
            assert sp[key] == st[key] or (sp[key] != sp[key] and st[key] != st[key]), (call, key)
        assert (sp["popart_scale"], sp["popart_shift"]) == log[call], call


# --------------------------------------------------------------------------------------------------------------------------------
# 4. frozen statistics, and the flag off
# --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["chain", "bf16"])
def test_frozen_statistics_give_the_bits_of_a_plain_learner(tg, dev, kind):
    out = []
    for popart in (True, False):
        pol, mgr, buf, algo = _learner(tg, dev, kind, popart)
        pol.value_norm.set(11.7, 53.9, 5000.0)
        pol.value_norm.freeze()
        head = [p.detach().clone() for p in pol.critic.network[-1].parameters()]
        kept = [bits(t) for t in (pol.value_norm.count, pol.value_norm.mean, pol.value_norm.m2, pol.value_norm.table)]
        for _ in range(2):
            buf.sample()
            algo.learn(buf)
        torch.cuda.synchronize()
        assert all(torch.equal(a, bits(t)) for a, t in zip(kept, (pol.value_norm.count, pol.value_norm.mean, pol.value_norm.m2,
                                                                  pol.value_norm.table)))
        assert not torch.equal(head[0], pol.critic.network[-1].weight)                   # (trained, not rescaled)
        out.append((pol, algo.last_stats))
    (pol_p, s_p), (pol_o, s_o) = out
    for k, (p, q) in enumerate(zip(pol_p.parameters(), pol_o.parameters())):
        assert torch.equal(bits(p), bits(q)), k
    assert s_p["popart_scale"] == 1.0 and s_p["popart_shift"] == 0.0 and "popart_scale" not in s_o
    for key in s_o:
        assert s_p[key] == s_o[key] or (s_p[key] != s_p[key] and s_o[key] != s_o[key]), key


def test_without_the_flag_the_new_wrapper_is_never_called(tg, dev, monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("value_norm_merge_popart was called by a policy without popart=True")
    monkeypatch.setattr(tg.hip_ops, "value_norm_merge_popart", refuse)
    for normalize_value in (True, False):
        pol, mgr, buf, algo = _learner(tg, dev, "chain", False, normalize_value=normalize_value)
        for _ in range(2):
            buf.sample()
            algo.learn(buf)
        torch.cuda.synchronize()
        assert "popart_scale" not in algo.last_stats
    # ... and with it the learner does reach it
    pol, mgr, buf, algo = _learner(tg, dev, "chain", True)
    buf.sample()
    with pytest.raises(AssertionError, match="without popart=True"):
        algo.learn(buf)


# --------------------------------------------------------------------------------------------------------------------------------
# 5. two ranks, 6. checkpoints
# --------------------------------------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _scale_and_tolerance(batches, eps):
    """(sigma_a / sigma_n of the EXACT statistics of batches[:1] and batches[:2], a bound on what statistics merged within
    Y.merge_bounds can make of it).  sigma^2 = m2 / count + eps: an error e of m2 moves sigma by e / (2 count sigma) to first order,
    plus three roundings (divide, add, sqrt) of relative size u each at the most; the quotient adds one more; the relative errors of
    numerator and denominator add.  Second-order terms: the factor 1 + 2^-20."""
    sig, rel = [], []
    for k in (1, 2):
        count, _, m2 = Y.exact(batches[:k])
        _, e_m2 = Y.merge_bounds(batches[:k])
        s2 = m2 / count + eps
        sig.append(np.sqrt(s2))
        rel.append(e_m2 / count / (2.0 * s2) + 3.0 * Y.U)
    scale = sig[0] / sig[1]
    return scale, scale * (rel[0] + rel[1] + Y.U) * (1.0 + 2.0 ** -20)


def test_two_ranks_hold_identical_heads_and_statistics(tmp_path):
    worker = os.path.join(HERE, "popart_dist_worker.py")
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
    a, b = [torch.load(f, weights_only=False) for f in outs[2]]
    for k in ("count", "mean", "m2", "table", "head_w", "head_b"):
        assert torch.equal(bits(a[k]), bits(b[k])), k
    assert all(torch.equal(x, y) for x, y in zip(a["weights"], b["weights"]))
    assert [l["stats"] for l in a["learns"]] == [l["stats"] for l in b["learns"]]
    exact, tol = {}, {}
    for w, recs in ((1, [one]), (2, [a, b])):
        batches = []
        for call in range(2):
            grid = torch.cat([r["learns"][call]["returns"] for r in recs], 1)
            mask = torch.cat([r["learns"][call]["mask"] for r in recs], 1)
            assert not bool(mask.all())                            # ragged masks
            batches.append(grid[mask].double().numpy())
        exact[w], tol[w] = _scale_and_tolerance(batches, one["eps"])
        first, second = recs[0]["learns"][0]["stats"], recs[0]["learns"][1]["stats"]
        assert first["popart_scale"] == 1.0 and first["popart_shift"] == 0.0            # empty statistics: nothing to preserve
        assert second["value_count"] == float(batches[0].size + batches[1].size)
        print("world", w, "popart_scale", second["popart_scale"], "exact", exact[w], "tolerance", tol[w])
        assert second["popart_scale"] != 1.0 and abs(second["popart_scale"] - exact[w]) <= tol[w], w
    s1, s2 = one["learns"][1]["stats"]["popart_scale"], a["learns"][1]["stats"]["popart_scale"]
    assert abs(s1 - s2) <= tol[1] + tol[2] + abs(exact[1] - exact[2])


def test_a_checkpoint_loads_into_a_popart_and_into_a_plain_policy(tg, dev, tmp_path):
    pol, mgr, buf, algo = _learner(tg, dev, "chain", True)
    for _ in range(2):
        buf.sample()
        algo.learn(buf)
    torch.cuda.synchronize()
    assert algo.last_stats["popart_scale"] != 1.0
    pol.save(str(tmp_path))
    name, S, A, hidden, act, _ = PATHS["chain"]
    x = buf.device_traj.obs_rows()[:64].float()
    with torch.no_grad():
        want = pol.value(x)
    assert float(want.abs().max()) > 0
    for kw in ({"popart": True}, {}):
        torch.manual_seed(77)                                      # other initial weights: everything comes from the file
        other = tg.GaussianActorCritic_NeuralNetwork(S, A, hidden, activation=act, cov=0.5, device=dev, normalize_value=True, **kw)
        other.load(str(tmp_path))
        with torch.no_grad():
            got = other.value(x)
        assert torch.equal(bits(got), bits(want)), kw
        for k, (p, q) in enumerate(zip(pol.parameters(), other.parameters())):
            assert torch.equal(bits(p), bits(q)), (kw, k)
