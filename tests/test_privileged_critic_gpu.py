"""The privileged critic on the MI355X (policies: privileged_critic={name: (lo, hi)}; tg_privileged_rows; run with `-m gpu`):

  1. the kernel against tests/privileged_fp64.py bit for bit (NaN-filled destination, unsorted indices, unequal pads, both dtypes, the
     index-free form, a hi == lo column), and every refusal without a launch;
  2. locality in situ: overwriting env j's column of engine.env_params between sample() and learn() moves the V grid in column j only;
  3. the whole step: two learn() calls against the same two calls with the one row-building method patched to assemble the rows in
     torch from the restatement -- every weight and every last_stats entry bit for bit, on the per-layer, bf16-chain, fp32-chain and
     autograd learners;
  4. forward equivalence: zero weights on the privileged columns give the plain policy's V grid and norm8 bit for bit;
  5. the learners' critic gradients at the first-layer widths the feature brings (7, 17, 29) against fp64, at test_gpu_parity.py's bars;
  6. two ranks against one; 7. a checkpoint round trip that continues bit for bit; 8. the learner's refusals.

T = 32, n = 160 throughout.  QuadPole2D has six randomisable parameters, so its critic reads 10 + 6 = 16 columns and the fp32 learners
pad actor and critic alike (16); the unequal fp32 pads (24 and 32) are covered in situ by QuadPole with seven parameters."""
import copy
import ctypes as C
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import privileged_fp64 as Y
from privileged_dist_worker import RANGES, make_env

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
T0, G0, E0 = 32, 4, 40                      # n = 160: a tail for 64- and 256-wide launches alike
N0 = G0 * E0
FACTORY = {"CartPole": (5, 1, (128, 128, 128), 0.5), "QuadPole2D": (10, 2, (128, 128, 128), 0.5), "QuadPole": (20, 4, (128, 128, 128), 0.3)}


@pytest.fixture(scope="module")
def tg():
    import trajopt_grpo_amd as tg
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return tg


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def bits(t):
    return t.detach().cpu().contiguous().view({torch.float32: torch.int32, torch.float64: torch.int64, torch.bfloat16: torch.int16}[t.dtype])


def _np_bits(t):
    """The bit patterns of a device tensor as unsigned NumPy integers (uint32 for f32, uint16 for bf16)."""
    b = bits(t).numpy()
    return b.view(np.uint16 if t.dtype == torch.bfloat16 else np.uint32)


# --------------------------------------------------------------------------------------------------------------------------------
# 1. the kernel
# --------------------------------------------------------------------------------------------------------------------------------
SHAPES = [(3, 1, 8, 8, False, -1), (10, 6, 16, 16, False, -1), (10, 7, 16, 24, False, -1), (5, 4, 32, 32, False, 31),
          (20, 9, 32, 32, True, 31), (20, 12, 32, 32, True, -1)]


def _spec_and_table(tg, P, n, seed, flat_column=None):
    """A spec of P columns over shuffled p[] slots, nominal values and ranges free of powers of two, and a table nominal * U(lo, hi) in
    the listed slots (anything in the others).  flat_column: that column's range is hi == lo."""
    rng = np.random.default_rng(seed)
    index = rng.permutation(12)[:P]
    nominal = rng.uniform(0.3, 9.7, size=P) * rng.choice([-1.0, 1.0], size=P, p=[0.2, 0.8])
    lo = rng.uniform(0.45, 0.95, size=P)
    hi = lo + rng.uniform(0.15, 1.3, size=P)
    if flat_column is not None:
        hi[flat_column] = lo[flat_column]
    ranges = {f"p{k}": (float(lo[k]), float(hi[k])) for k in range(P)}
    center, scale = Y.center_scale(ranges)
    ptab = rng.normal(size=(12, n)) * 3.0
    ptab[index] = nominal[:, None] * (lo[:, None] + (hi - lo)[:, None] * rng.uniform(size=(P, n)))
    spec = tg._native.PrivilegedSpec()
    spec.count = P
    for k in range(P):
        spec.index[k], spec.nominal[k], spec.center[k], spec.scale[k] = int(index[k]), float(nominal[k]), center[k], scale[k]
    return spec, ptab, (index, nominal, center, scale)


@pytest.mark.parametrize("rows", [1, 63, 257, 1000])
@pytest.mark.parametrize("S,P,src_pad,dst_pad,bf16,ones_col", SHAPES, ids=[f"S{s}P{p}-{a}to{b}-{'bf16' if h else 'f32'}" for s, p, a, b, h, _ in SHAPES])
def test_rows_kernel_is_the_restatement_bit_for_bit(tg, dev, rows, S, P, src_pad, dst_pad, bf16, ones_col):
    K = tg.hip_ops
    dt = torch.bfloat16 if bf16 else torch.float32
    g = torch.Generator(device="cpu").manual_seed(1000 * rows + 10 * S + P)
    spec, ptab, (index, nominal, center, scale) = _spec_and_table(tg, P, N0, seed=rows + S)
    src = (torch.randn(rows, src_pad, generator=g) * 3.0).to(dt).to(dev)                 # every source column carries bits, padding too
    idx = torch.randperm(T0 * N0, generator=g)[:rows]                                    # an unsorted draw from the 5,120 cells
    table = torch.from_numpy(ptab).to(dev)
    out = torch.full((rows + 3, dst_pad), float("nan"), dtype=dt, device=dev)            # (three rows beyond: not to be written)
    got = K.privileged_rows(src, S, idx.to(dev), N0, table, spec, out, ones_col)
    torch.cuda.synchronize()
    want = Y.rows(_np_bits(src), S, idx.numpy(), N0, ptab, index, nominal, center, scale, dst_pad, bf16, ones_col)
    assert got.shape == (rows, dst_pad) and np.array_equal(_np_bits(got), want)
    assert bool(torch.isnan(out[rows:].float()).all()) and not bool(torch.isnan(got.float()).any())
    x = got[:, S:S + P].float().cpu().numpy()
    assert np.all(np.abs(x) <= 1.0) and np.any(x != 0)                                    # the drawn range lies on [-1, 1]


@pytest.mark.parametrize("S,P,src_pad,dst_pad,bf16,ones_col", [SHAPES[2], SHAPES[4]], ids=["f32", "bf16"])
def test_rows_kernel_without_an_index_and_with_a_flat_range(tg, dev, S, P, src_pad, dst_pad, bf16, ones_col):
    """d_idx == NULL: row r is env r (the bootstrap rows, rows = n).  A hi == lo column: scale 0, the column is all zeros."""
    K = tg.hip_ops
    dt = torch.bfloat16 if bf16 else torch.float32
    flat = P // 2
    spec, ptab, (index, nominal, center, scale) = _spec_and_table(tg, P, N0, seed=77 + S, flat_column=flat)
    assert scale[flat] == 0.0
    g = torch.Generator(device="cpu").manual_seed(5 + S)
    src = (torch.randn(N0, src_pad, generator=g) * 3.0).to(dt).to(dev)
    table = torch.from_numpy(ptab).to(dev)
    got = K.privileged_rows(src, S, None, N0, table, spec, torch.full((N0, dst_pad), float("nan"), dtype=dt, device=dev), ones_col)
    torch.cuda.synchronize()
    want = Y.rows(_np_bits(src), S, None, N0, ptab, index, nominal, center, scale, dst_pad, bf16, ones_col)
    assert np.array_equal(_np_bits(got), want)
    assert not bool(got[:, S + flat].float().any()) and bool(got[:, S + (flat + 1) % P].float().any())
    # the same rows through an explicit index: t * n + e for any t
    idx = (torch.arange(N0) + N0 * torch.randint(0, T0, (N0,), generator=g)).to(dev)
    again = K.privileged_rows(src, S, idx, N0, table, spec, torch.full((N0, dst_pad), float("nan"), dtype=dt, device=dev), ones_col)
    torch.cuda.synchronize()
    assert torch.equal(bits(again), bits(got))


def test_every_refusal_returns_its_status_without_a_launch(tg, dev):
    N = tg._native
    lib = N.load()
    spec, ptab, _ = _spec_and_table(tg, 2, N0, seed=3)
    src = torch.randn(16, 8, device=dev)
    dst = torch.full((16, 8), float("nan"), device=dev)
    idx = torch.arange(16, device=dev)
    table = torch.from_numpy(ptab).to(dev)
    ok = dict(src=src.data_ptr(), src_pad=8, S=5, idx=idx.data_ptr(), rows=16, n=N0, ptab=table.data_ptr(), spec=spec, dst=dst.data_ptr(),
              dst_pad=8, bf16=0, ones=-1)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.tg_privileged_rows(a["src"], a["src_pad"], a["S"], a["idx"], a["rows"], a["n"], a["ptab"],
                                      None if a["spec"] is None else C.byref(a["spec"]), a["dst"], a["dst_pad"], a["bf16"], a["ones"],
                                      N.stream_ptr(dev))

    def changed(**kw):
        s = N.PrivilegedSpec.from_buffer_copy(spec)
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(s, k)[v[0]] = v[1]
            else:
                setattr(s, k, v)
        return s

    i0 = int(spec.index[0])
    refused = [dict(src=None), dict(ptab=None), dict(spec=None), dict(dst=None), dict(spec=changed(count=0)), dict(spec=changed(count=13)),
               dict(spec=changed(index=(1, 12))), dict(spec=changed(index=(0, -1))), dict(spec=changed(index=(1, i0))),
               dict(S=0), dict(S=9), dict(S=7), dict(ones=0), dict(ones=6), dict(ones=8), dict(src_pad=6), dict(dst_pad=12, bf16=1),
               dict(src_pad=12, bf16=1), dict(dst_pad=68), dict(src_pad=68), dict(spec=changed(nominal=(0, 0.0))),
               dict(spec=changed(nominal=(1, float("inf")))), dict(spec=changed(nominal=(1, float("nan")))),
               dict(spec=changed(center=(0, float("nan")))), dict(spec=changed(scale=(1, float("inf")))), dict(n=0), dict(n=-4),
               dict(idx=None, rows=N0 + 1)]
    for kw in refused:
        assert call(**kw) == N.TG_ERR_ARG and b"tg_privileged_rows" in lib.tg_last_error(), kw
    assert call(rows=0) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(dst).all())                                                   # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool(torch.isnan(dst).any()) and torch.equal(dst[:, :5], src[:, :5])


# --------------------------------------------------------------------------------------------------------------------------------
# the learners
# --------------------------------------------------------------------------------------------------------------------------------
def _learner(tg, dev, name, kind, updates, monte_carlo=True, batch_size=None, boot=False, seed=5, privileged=True, extras=False,
             randomize=True):
    """Policy, manager, sampled buffer and PPO from fixed seeds: two calls give bit-identical weights and trajectories."""
    S, A, hidden, cov = FACTORY[name]
    cdt = torch.bfloat16 if kind == "bf16" else None
    ranges = RANGES[name]
    torch.manual_seed(seed)
    kw = dict(privileged_critic=ranges) if privileged else {}
    if extras:
        kw.update(normalize_obs=True, normalize_value=True, learn_std=True)
    pol = tg.GaussianActorCritic_NeuralNetwork(S, A, hidden, cov=cov, device=dev, **kw)
    mgr = tg.RolloutManager(lambda: make_env(tg, name, T0).randomize(ranges if randomize else None, seed=21), pol, num_workers=G0,
                            num_episodes_per_worker=E0, seed=9, compute_dtype=cdt)
    buf = tg.Rollout_Buffer(mgr)
    buf.sample()
    algo = tg.PPO(epsilon=0.2, policy=pol, optimizer=torch.optim.Adam(pol.parameters(), lr=2e-4), ref_model=None,
                  updates_per_iter=updates, gamma=0.99, lam=0.95, batch_size=batch_size, monte_carlo=monte_carlo, seed=3,
                  autocast_dtype=cdt, fused_mlp=kind != "autograd", bootstrap_truncated=boot, **({"max_grad_norm": 0.7} if extras else {}))
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
    return m_a, m_c


def _torch_rows(calls):
    """PPO._privileged_rows restated: the destination rows assembled on the host by tests/privileged_fp64.py and copied over."""
    def build(self, priv, src, S, idx, n, out, ones_col):
        spec, table = priv
        P, rows, bf16 = spec.count, src.shape[0], src.dtype == torch.bfloat16
        want = Y.rows(_np_bits(src), S, None if idx is None else idx.cpu().numpy(), n, table.cpu().numpy(), list(spec.index)[:P],
                      list(spec.nominal)[:P], list(spec.center)[:P], list(spec.scale)[:P], out.shape[1], bf16, ones_col)
        host = torch.from_numpy(want.view(np.int16 if bf16 else np.int32)).view(src.dtype)
        out[:rows].copy_(host.to(out.device))
        calls.append((rows, src.shape[1], out.shape[1], idx is None, ones_col))
        return out[:rows]
    return build


# kind, env, monte_carlo, batch_size, bootstrap_truncated, normalize_obs + normalize_value + learn_std (+ max_grad_norm)
WHOLE = [("f32", "CartPole", True, None, False, False), ("f32", "QuadPole2D", False, None, True, False), ("f32", "QuadPole", False, None, True, False),
         ("bf16", "QuadPole2D", True, None, True, False), ("bf16", "CartPole", False, None, False, True), ("layer", "CartPole", False, None, True, False),
         ("layer", "QuadPole2D", True, None, False, False), ("f32", "CartPole", False, 512, True, False), ("f32", "QuadPole2D", True, None, True, True),
         ("autograd", "CartPole", False, None, True, False), ("autograd", "QuadPole2D", True, 512, False, False)]


@pytest.mark.parametrize("kind,name,monte_carlo,batch_size,boot,extras", WHOLE,
                         ids=[f"{k}-{n}-{'mc' if m else 'gae'}{'-mb' if b else ''}{'-boot' if t else ''}{'-all' if x else ''}" for k, n, m, b, t, x in WHOLE])
def test_two_learns_equal_two_learns_on_torch_assembled_rows(tg, dev, monkeypatch, kind, name, monte_carlo, batch_size, boot, extras):
    """Everything but the critic's rows is the same code on both sides; the rows of the second side are assembled in torch from the
    restatement.  Bit for bit in every weight and every last_stats entry after two learn() calls (a second rollout in between)."""
    A = tg.algorithms

    def two_learns(patched):
        pol, mgr, buf, algo = _learner(tg, dev, name, kind, 2, monte_carlo, batch_size, boot, extras=extras)
        calls = []
        if patched:
            monkeypatch.setattr(A.PPO, "_privileged_rows", _torch_rows(calls))
        try:
            algo.learn(buf)
            first = dict(algo.last_stats)
            buf.sample()
            algo.learn(buf)
            torch.cuda.synchronize()
        finally:
            monkeypatch.undo()
        return pol, mgr, buf, algo, calls, first

    pol, mgr, buf, algo, _, first = two_learns(False)
    m_a, m_c = _check_kind(algo, pol, kind)
    S, P = FACTORY[name][0], len(RANGES[name])
    assert pol.critic.network[0].in_features == S + P and pol.actor.network[0].in_features == S
    if m_a is not None:                                                                   # each net keeps its own learner and pad
        want_pads = {"f32": ((S + 7) // 8 * 8, (S + P + 7) // 8 * 8), "bf16": (32, 32), "layer": (32, 32)}[kind]
        assert (m_a.in_pad, m_c.in_pad) == want_pads and (name != "QuadPole" or want_pads == (24, 32))
    traj = buf.device_traj
    assert int(traj.len.min()) < T0 and int(traj.mask.sum()) < T0 * traj.n               # ragged masks
    eng = mgr.engine
    assert eng.env_params is not None and tuple(eng.env_params.shape) == (12, N0)
    pol2, mgr2, buf2, algo2, calls, first2 = two_learns(True)
    assert torch.equal(eng.env_params, mgr2.engine.env_params) and torch.equal(traj.obs, buf2.device_traj.obs)
    assert len(calls) == 2 * (1 + int(boot)) and {c[3] for c in calls} == ({False, True} if boot else {False})
    for k, (p, q) in enumerate(zip(pol.parameters(), pol2.parameters())):
        assert torch.equal(bits(p), bits(q)), k
    assert torch.equal(bits(algo.norm8), bits(algo2.norm8))
    for s1, s2 in ((first, first2), (algo.last_stats, algo2.last_stats)):
        assert set(s1) == set(s2) and {"actor_loss", "critic_loss", "total_loss", "n_valid"} <= set(s1)
        for key in s1:
            assert s1[key] == s2[key] or (s1[key] != s1[key] and s2[key] != s2[key]), key
    if extras:
        assert {"grad_norm", "obs_count", "value_mean", "explained_variance", "log_std"} <= set(algo.last_stats)
    if boot:
        assert "n_bootstrapped" in algo.last_stats


@pytest.mark.parametrize("kind", ["f32", "bf16", "autograd"])
def test_overwriting_one_envs_parameters_moves_only_its_column_of_the_value_grid(tg, dev, kind):
    pol, mgr, buf, algo = _learner(tg, dev, "QuadPole2D", kind, 0, monte_carlo=False)     # (no update: the weights stand)
    eng, traj = mgr.engine, buf.device_traj

    def v_grid():
        algo.learn(buf)
        torch.cuda.synchronize()
        return algo._ws._buf["V"][:T0 * N0].view(T0, N0).clone()

    v0 = v_grid()
    assert torch.equal(bits(v0), bits(v_grid()))                                          # the same buffer twice: the same grid
    mask = traj.mask.bool()
    assert bool((v0[mask] != 0).all()) and not bool(v0[~mask].any())
    j = int(traj.len.argmax())                                                            # an env with a long episode
    kept = eng.env_params.clone()
    for name, (lo, hi) in RANGES["QuadPole2D"].items():                                   # env j becomes the vehicle at the top of every range
        i = eng.env.RANDOMIZABLE[name]
        eng.env_params[i, j] = float(eng.params.p[i]) * hi
    assert not torch.equal(eng.env_params[:, j], kept[:, j])
    v1 = v_grid()
    others = torch.ones(N0, dtype=torch.bool, device=dev)
    others[j] = False
    assert torch.equal(bits(v1[:, others]), bits(v0[:, others]))                          # every other entry keeps its bits
    changed = v1[:, j] != v0[:, j]
    assert bool(changed[mask[:, j]].all()) and not bool(changed[~mask[:, j]].any())


@pytest.mark.parametrize("kind", ["f32", "bf16", "layer"])
def test_zero_weights_on_the_privileged_columns_give_the_plain_critic(tg, dev, kind):
    """CartPole, P = 2: both nets pad alike on every learner.  The privileged critic's first layer is the plain critic's with two
    zero columns behind it: the V grid and norm8 of a learn() are the plain policy's bit for bit."""
    plain, _, buf_p, algo_p = _learner(tg, dev, "CartPole", kind, 0, monte_carlo=False, privileged=False)
    pol, _, buf, algo = _learner(tg, dev, "CartPole", kind, 0, monte_carlo=False)     # (the same seed: the same actor, the same rollout)
    S = 5
    with torch.no_grad():
        for p, q in zip(pol.actor.parameters(), plain.actor.parameters()):
            p.copy_(q)
        for (n_, p), q in zip(pol.critic.named_parameters(), plain.critic.parameters()):
            if n_ == "network.0.weight":
                p.zero_()
                p[:, :S].copy_(q)
            else:
                p.copy_(q)
    algo.sync_old_policy()
    assert torch.equal(buf.device_traj.obs, buf_p.device_traj.obs) and torch.equal(buf.device_traj.act, buf_p.device_traj.act)
    grids = []
    for a, b in ((algo_p, buf_p), (algo, buf)):
        a.learn(b)
        torch.cuda.synchronize()
        grids.append((a._ws._buf["V"][:T0 * N0].clone(), a.norm8.clone()))
    m_a, m_c = algo._mlp(pol.actor), algo._mlp(pol.critic)
    assert m_a is None or m_a.in_pad == m_c.in_pad
    assert bool(grids[0][0].any()) and torch.equal(bits(grids[0][0]), bits(grids[1][0])) and torch.equal(bits(grids[0][1]), bits(grids[1][1]))


def test_a_checkpoint_round_trip_continues_bit_for_bit(tg, dev, tmp_path):
    pol, mgr, buf, algo = _learner(tg, dev, "CartPole", "f32", 2, monte_carlo=False, boot=True)
    algo.learn(buf)
    torch.cuda.synchronize()
    pol.save(str(tmp_path))
    algo.save(str(tmp_path))
    S, A, hidden, cov = FACTORY["CartPole"]
    torch.manual_seed(77)                                                                 # other initial weights: everything comes from the files
    pol2 = tg.GaussianActorCritic_NeuralNetwork(S, A, hidden, cov=cov, device=dev, privileged_critic=RANGES["CartPole"])
    algo2 = tg.PPO(epsilon=0.2, policy=pol2, optimizer=torch.optim.Adam(pol2.parameters(), lr=2e-4), ref_model=None, updates_per_iter=2,
                   gamma=0.99, lam=0.95, batch_size=None, monte_carlo=False, seed=3, bootstrap_truncated=True)
    pol2.load(str(tmp_path))
    algo2.load(str(tmp_path))
    algo2.sync_old_policy()
    plain = tg.GaussianActorCritic_NeuralNetwork(S, A, hidden, cov=cov, device=dev)
    with pytest.raises(ValueError, match="privileged_critic"):
        plain.load(str(tmp_path))
    buf.sample()                                                                          # the next rollout, by the first policy
    algo.learn(buf)
    algo2.learn(buf)
    torch.cuda.synchronize()
    for k, (p, q) in enumerate(zip(pol.parameters(), pol2.parameters())):
        assert torch.equal(bits(p), bits(q)), k
    s1, s2 = algo.last_stats, algo2.last_stats
    for key in ("actor_loss", "critic_loss", "total_loss", "kl_div", "n_valid", "n_bootstrapped"):
        assert s1[key] == s2[key], key


def test_the_learner_refuses_an_env_that_does_not_draw_what_the_critic_reads(tg, dev):
    # randomisation off
    pol, mgr, buf, algo = _learner(tg, dev, "CartPole", "f32", 1, randomize=False)
    before = [p.detach().clone() for p in pol.parameters()]
    with pytest.raises(ValueError, match="privileged_critic.*randomisation None"):
        algo.learn(buf)
    # other names, other ranges: both sides are named
    for other in ({"length": (0.6, 1.7), "masspole": (0.75, 1.3)}, {"length": (0.6, 1.7), "masscart": (0.75, 1.25)}, {"length": (0.6, 1.7)}):
        mgr.engine.env.randomize(other, seed=21)
        buf.sample()
        with pytest.raises(ValueError, match="privileged_critic.*masscart.*randomisation.*length"):
            algo.learn(buf)
    # a hand-built buffer: no engine to read the table from
    class Bare:
        device_traj = buf.device_traj
    with pytest.raises(ValueError, match="privileged_critic.*no rollout engine"):
        algo.learn(Bare())
    torch.cuda.synchronize()
    assert all(torch.equal(p, q) for p, q in zip(pol.parameters(), before))              # refused before any update
    # the right mapping in another order is the same mapping
    mgr.engine.env.randomize(dict(reversed(list(RANGES["CartPole"].items()))), seed=21)
    buf.sample()
    algo.learn(buf)
    torch.cuda.synchronize()
    assert not all(torch.equal(p, q) for p, q in zip(pol.parameters(), before))


def test_a_plain_learn_never_enters_the_privileged_path(tg, dev, monkeypatch):
    K, A = tg.hip_ops, tg.algorithms

    def boom(*a, **k):
        raise AssertionError("the privileged path was entered by a plain policy")

    pol, mgr, buf, algo = _learner(tg, dev, "CartPole", "f32", 1, monte_carlo=False, boot=True, privileged=False)
    for obj, attr in ((K, "privileged_rows"), (A, "privileged_spec"), (K.N, "PrivilegedSpec"), (A.PPO, "_critic_rows"), (A.PPO, "_privileged_rows")):
        monkeypatch.setattr(obj, attr, boom)
    lib = K.N.load()
    monkeypatch.setattr(lib, "tg_privileged_rows", boom)
    algo.learn(buf)
    torch.cuda.synchronize()
    assert "xin_c" not in algo._ws._buf and not any(k.startswith("boot_xin_c") or k.startswith("boot_priv") for k in algo._small_bufs)
    assert np.isfinite(algo.last_stats["total_loss"]).all()


# --------------------------------------------------------------------------------------------------------------------------------
# 5. the existing learner kernels at the critic's new first-layer widths
# --------------------------------------------------------------------------------------------------------------------------------
WIDTHS = [(5, 2), (10, 7), (20, 9)]                                                      # in_dim 7, 17, 29


def _critic_problem(tg, dev, S, P, rows, hidden):
    """A critic of S + P inputs, its torch-assembled rows (observations, then the restatement's features of a drawn table), returns."""
    torch.manual_seed(100 * S + P)
    net = tg.NeuralNetwork(S + P, 1, hidden, "ReLU").to(dev)
    spec, ptab, (index, nominal, center, scale) = _spec_and_table(tg, P, N0, seed=S)
    g = torch.Generator(device="cpu").manual_seed(S + P)
    env = torch.randint(0, N0, (rows,), generator=g).numpy()
    x = Y.features_of_table(ptab, env, index, nominal, center, scale)
    X = torch.cat([torch.randn(rows, S, generator=g), torch.from_numpy(x)], dim=1).to(dev)
    ret = torch.randn(rows, generator=g).to(dev)
    return net, X, ret


@pytest.mark.parametrize("S,P", WIDTHS)
def test_f32_chain_critic_gradients_at_the_new_widths_match_fp64(tg, dev, S, P):
    """test_gpu_parity.py::test_f32_chain_update_matches_fp64_autograd's comparison of the value head (kind 1), unchanged: fp64 with
    the KERNEL's ReLU masks (checked against the fp64 pre-activations: at most 1e-4 of them differ, each within rounding of zero),
    loss sums to 2e-6, every parameter gradient to 2e-5 x max(1, sqrt(rows / 1000)) of its scale."""
    from trajopt_grpo_amd import mlp as M
    rows, hidden = 4000, (128, 128, 128)
    net, X, ret = _critic_problem(tg, dev, S, P, rows, hidden)
    norm, cc = [0.1, 1.3, -0.2, 0.7], 0.5 / rows
    m = M.GemmMLP(net, torch.float32)
    assert m._f32 is not None and m.in_dim == S + P and m.in_pad == (S + P + 7) // 8 * 8
    m.f32_store_all = True
    for p in net.parameters():
        p.grad = torch.zeros_like(p)
    s = m.forward_loss(m.prepare_input(X), 1, ret=ret, norm=norm[2:4], critic_coef=cc).clone()
    acts = [t.clone() for t in m._acts[1:]]
    m.backward_fused()
    torch.cuda.synchronize()
    got = [p.grad.clone() for p in net.parameters()]
    lin = [mod for mod in copy.deepcopy(net).double().network if isinstance(mod, torch.nn.Linear)]
    W, B = [l.weight.detach() for l in lin], [l.bias.detach() for l in lin]
    masks = [(a > 0) for a in acts]
    hs, h = [], X.double()
    for l in range(len(hidden)):
        z = h @ W[l].t() + B[l]
        flips = (z > 0) != masks[l]
        assert float(flips.float().mean()) <= 1e-4 and (not bool(flips.any()) or float(z[flips].abs().max()) <= 1e-5 * (1.0 + float(z.abs().max()))), l
        h = z * masks[l]
        hs.append(h)
    out = (h @ W[-1].t() + B[-1]).requires_grad_()
    d = out[:, 0] - (ret.double() - norm[2]) * norm[3]
    (cc * (d * d).sum()).backward()
    gout = out.grad
    assert abs(float(s[1]) - float((d * d).sum().detach())) <= 2e-6 * (abs(float((d * d).sum().detach())) + 1.0) and float(s[3]) == rows
    nh = len(hidden)
    ref_w, ref_b = [None] * (nh + 1), [None] * (nh + 1)
    ref_w[nh], ref_b[nh] = gout.t() @ hs[-1], gout.sum(0)
    dh = gout @ W[nh]
    for l in range(nh - 1, -1, -1):
        dz = dh * masks[l]
        ref_w[l], ref_b[l] = dz.t() @ (hs[l - 1] if l > 0 else X.double()), dz.sum(0)
        dh = dz @ W[l]
    ref = [t for pair in zip(ref_w, ref_b) for t in pair]
    for i, (gg, r) in enumerate(zip(got, ref)):
        scale = float(r.abs().max()) + 1e-12
        err = float((gg.double() - r).abs().max())
        print(f"f32 chain, in_dim {S + P}, parameter {i}: err / scale {err / scale:.3e}")
        assert err <= (2e-5 * max(1.0, (rows / 1000) ** 0.5)) * scale, (i, err / scale)
    assert bool(got[0][:, S:].any())                                                      # the privileged columns have gradients


@pytest.mark.parametrize("cd", [torch.float32, torch.bfloat16], ids=["layer", "bf16"])
@pytest.mark.parametrize("S,P", WIDTHS)
def test_per_layer_and_bf16_critic_gradients_at_the_new_widths(tg, dev, S, P, cd):
    """test_gpu_parity.py::test_gemm_mlp_matches_autograd's comparison with its bars, the truth taken in fp64: fp32 per-layer path --
    relative L2 5e-6 on the head, 3e-3 below it; bf16 chain kernels -- no further from the truth than torch's own autocast pipeline
    (x 1.3 + 2e-3)."""
    from trajopt_grpo_amd import mlp as M
    rows, hidden = 3 * 8192 + 777, (128, 128, 128)
    net, X, ret = _critic_problem(tg, dev, S, P, rows, hidden)
    m = M.GemmMLP(net, cd)
    if cd == torch.float32:
        assert m.disable_f32_chain() and m._f32 is None
    else:
        assert m._chain is not None and m._bchain is not None
    assert m.in_pad == 32 and m.in_dim == S + P
    g = torch.randn(rows, 1, device=dev)
    for p in net.parameters():
        p.grad = torch.zeros_like(p)
    out = m.forward(m.prepare_input(X), keep=True)
    m.backward(g)
    torch.cuda.synchronize()
    got = [p.grad.clone() for p in net.parameters()]
    net64 = copy.deepcopy(net).double()
    for p in net64.parameters():
        p.grad = None
    ref = net64(X.double())
    ref.backward(g.double())
    truth = [p.grad.clone() for p in net64.parameters()]
    bf = cd == torch.bfloat16
    assert float((out.double() - ref.detach()).abs().max()) <= (2e-2 if bf else 2e-6) * float(ref.abs().max())
    names = [n for n, _ in net.named_parameters()]
    if bf:
        for p in net.parameters():
            p.grad = None
        with torch.autocast("cuda", dtype=torch.bfloat16):
            ac = net(X)
        ac.float().backward(g)
        for n, a, t, p in zip(names, got, truth, net.parameters()):
            err, err_ac = float((a.double() - t).norm() / t.norm()), float((p.grad.double() - t).norm() / t.norm())
            print(f"bf16 chain, in_dim {S + P}, {n}: err {err:.3e}, autocast {err_ac:.3e}")
            assert err <= 1.3 * err_ac + 2e-3, (n, err, err_ac)
    else:
        for n, a, t in zip(names, got, truth):
            rel = float((a.double() - t).norm() / t.norm())
            print(f"per-layer fp32, in_dim {S + P}, {n}: rel {rel:.3e}")
            assert rel <= (5e-6 if n.startswith(f"network.{2 * len(hidden)}.") else 3e-3), (n, rel)


# --------------------------------------------------------------------------------------------------------------------------------
# 6. two ranks
# --------------------------------------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_ranks_reproduce_the_one_rank_learn(tmp_path):
    """tests/privileged_dist_worker.py as fresh child processes (the harness of test_value_norm_gpu.py: gloo, both ranks on cuda:0,
    half the groups each).  The table and the row indices are rank-local: the ranks' tables side by side are the one-rank table, their
    critic rows are the one-rank rows of their envs, both ranks end with the same bits, and the weights lie within 1e-6 (relative
    L2, test_value_norm_gpu.py's bar) of the one-rank weights."""
    worker = os.path.join(HERE, "privileged_dist_worker.py")
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
        assert a["stats"] == b["stats"] and all(torch.equal(x, y) for x, y in zip(a["weights"], b["weights"])), case
        assert torch.equal(torch.cat([a["env_params"], b["env_params"]], 1), rec["env_params"]), case
        assert torch.equal(torch.cat([a["mask"], b["mask"]], 1), rec["mask"]) and not bool(rec["mask"].all()), case
        # the privileged columns of every valid cell, on the [T][n] grid: each rank read its own envs' parameters
        both = torch.cat([a["features"], b["features"]], 1)
        assert torch.equal(both.view(torch.int32), rec["features"].view(torch.int32)) and bool(rec["features"].any()), case
        assert a["stats"]["n_valid"] == rec["stats"]["n_valid"]
        for x, y in zip(a["weights"], rec["weights"]):
            assert float((x.double() - y.double()).norm()) <= 1e-6 * float(y.double().norm()), case
