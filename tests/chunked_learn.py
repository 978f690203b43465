"""Helpers of tests/test_chunked_learn_cpu.py and tests/test_chunked_learn_gpu.py: learn() walked in several chunks (`chunk_rows`)
against the one-chunk learn() of the same learner.

Every arm is a deep copy of one policy behind a plain torch.optim.Adam(lr=0.0): the optimizer keeps its fused step (and the rider
of the one-chunk fp32 GRPO update) while the weights never move, so every update of a learn() sees the same weights, the gradients
left in .grad are those of a first update, and two arms differ in fp32 summation order only -- no Adam step turns noise into +-lr.

The comparison of two arms' gradients lives in gradients_agree() / grad_bar(): per tensor, max |a - b| <= 2e-5 (max |a| + 1e-9)
max(1, sqrt(rows / 1000)) -- the bar of tests/test_gpu_parity.py wherever two runs differ in fp32 summation order only (e.g.
test_backward_chain_forms_the_first_layer_gradient)."""
import contextlib
import copy
import math

import numpy as np
import torch

ARMS = (None, "N", "N+1", "N-1", 257, 96)               # chunk_rows of the arms; the strings are resolved against the buffer's row count
STATS_RTOL, STATS_ATOL = 1e-5, 1e-7                     # test_f32_learn_is_independent_of_the_chunk_size's bound on the loss statistics
# the loss-head entry points of the learner families (and their _ref / _std / _act forms)
FAMILY_BASES = {"bf16": "tg_mlp_forward_chain_loss", "f32w": "tg_mlp_f32w_forward_backward", "f32r": "tg_mlp_f32r_forward_backward",
                "f32": "tg_mlp_f32_forward_backward", "layer": "tg_surrogate_loss", "torch": "tg_surrogate_loss"}
HAND_WRITTEN = ("bf16", "f32w", "f32r", "f32")          # a row's result does not depend on its chunk-mates
ROW_ARGS = ("act", "logp_old", "adv", "ret", "logp_old_out", "logp_ref", "std_out")      # forward_loss()'s per-row arguments


# ---------------------------------------------------------------------------------------------------------------------------------
# the comparison
# ---------------------------------------------------------------------------------------------------------------------------------
def grad_bar(ref: torch.Tensor, rows: int) -> float:
    return 2e-5 * (float(ref.detach().abs().max()) + 1e-9) * max(1.0, math.sqrt(rows / 1000.0))


def grad_distances(ref: dict, got: dict, rows: int, yardstick: dict = None):
    """[(name, max |ref - got|, bar)] of two {name: gradient} dictionaries with the same keys.  yardstick ({name: distance}): the bar
    is 4 x that distance, floored at grad_bar() (the learners on library GEMMs, whose summation order is not ours to derive)."""
    assert list(ref) == list(got), (list(ref), list(got))
    out = []
    for name, a in ref.items():
        b = got[name]
        assert a.shape == b.shape, name
        bar = grad_bar(a, rows)
        if yardstick is not None:
            bar = max(bar, 4.0 * yardstick[name])
        d = float((a.detach().double() - b.detach().double()).abs().max())
        out.append((name, d if math.isfinite(d) else float("inf"), bar))
    return out


def gradients_agree(ref: dict, got: dict, rows: int, yardstick: dict = None) -> bool:
    return all(d <= bar for _, d, bar in grad_distances(ref, got, rows, yardstick))


def worst(dists):
    """The (name, distance, bar) with the largest distance / bar."""
    return max(dists, key=lambda t: t[1] / t[2])


def stats_distance(ref: dict, got: dict):
    """max over the entries of two last_stats of |a - b| / (STATS_ATOL + STATS_RTOL |a|): <= 1 is np.testing.assert_allclose's verdict
    at the bound.  Both must hold the same keys, list lengths and finite numbers."""
    assert sorted(ref) == sorted(got), (sorted(ref), sorted(got))
    worst_ratio, worst_key = 0.0, None
    for k in ref:
        a, b = np.asarray(ref[k], dtype=np.float64), np.asarray(got[k], dtype=np.float64)
        assert a.shape == b.shape and np.isfinite(a).all() and np.isfinite(b).all(), (k, ref[k], got[k])
        if a.size == 0:
            continue
        r = float((np.abs(a - b) / (STATS_ATOL + STATS_RTOL * np.abs(a))).max())
        if r > worst_ratio:
            worst_ratio, worst_key = r, k
    return worst_ratio, worst_key


def chunk_bounds(rows: int, chunk: int):
    return [(lo, min(lo + chunk, rows)) for lo in range(0, rows, chunk)]


def resolve_arm(arm, rows: int):
    return {None: None, "N": rows, "N+1": rows + 1, "N-1": rows - 1}.get(arm, arm)


# ---------------------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------------------
BF16 = torch.bfloat16
# name -> (learner, env, S, A, hidden, activation, compute dtype, G, E, T, family)
CASES = {
    "ppo_bf16_256x5": ("PPO", "QuadPole", 20, 4, (256,) * 5, "ReLU", BF16, 3, 11, 32, "bf16"),
    "grpo_bf16_128x3": ("GRPO", "CartPole", 5, 1, (128,) * 3, "ReLU", BF16, 4, 16, 32, "bf16"),
    "ppo_f32_wide_256x2": ("PPO", "QuadPole", 20, 4, (256, 256), "ReLU", None, 3, 11, 32, "f32w"),
    "grpo_f32_resident_128x2": ("GRPO", "CartPole", 5, 1, (128, 128), "ReLU", None, 4, 16, 32, "f32r"),
    "grpo_f32_chain_64x1": ("GRPO", "CartPole", 5, 1, (64,), "ReLU", None, 4, 16, 32, "f32"),
    "grpo_f32_chain_128x4": ("GRPO", "CartPole", 5, 1, (128,) * 4, "ReLU", None, 4, 16, 32, "f32"),
    "grpo_f32_chain_tanh_128x3": ("GRPO", "CartPole", 5, 1, (128,) * 3, "Tanh", None, 4, 16, 32, "f32"),
    "ppo_per_layer_40x2": ("PPO", "CartPole", 5, 1, (40, 40), "ReLU", None, 4, 16, 32, "layer"),
    "ppo_autograd_sigmoid_32x2": ("PPO", "CartPole", 5, 1, (32, 32), "Sigmoid", None, 4, 16, 32, "torch"),
}
# (case, feature): the plain cases, then every optional feature on one bf16 and one fp32 case (the privileged critic: the bf16 PPO case)
RUNS = [(c, None) for c in CASES] + [
    ("grpo_bf16_128x3", "ref"), ("grpo_f32_chain_128x4", "ref"),
    ("ppo_bf16_256x5", "learn_std"), ("ppo_f32_wide_256x2", "learn_std"),
    ("grpo_bf16_128x3", "clip"), ("ppo_f32_wide_256x2", "clip"),
    ("ppo_bf16_256x5", "privileged"),
    ("ppo_bf16_256x5", "minibatch"), ("ppo_f32_wide_256x2", "minibatch"),
    ("grpo_bf16_128x3", "stale_old"), ("grpo_f32_chain_128x4", "stale_old"),
]
MINIBATCH = 512
# QuadPole.randomize's mapping of the privileged critic (an order that is not the parameter table's; no power of two among the ends)
PRIVILEGED = {"tether_length": (0.6, 1.9), "mass": (0.7, 1.4), "Izz": (0.8, 1.25), "load_mass": (0.6, 1.5), "Ixx": (0.8, 1.3),
              "gravity": (0.95, 1.05), "Iyy": (0.85, 1.2)}

_SETUPS = {}


def setup(tg, dev, case, feature=None, small=False):
    """(policy, buffer, valid rows, reference policy or None) of one case, rolled out once per module: every arm deep-copies the policy.
    small: a second, smaller rollout of the same policy (fewer episodes, a shorter horizon)."""
    learn_std, privileged = feature == "learn_std", feature == "privileged"
    key = (case, learn_std, privileged)
    learner, env_name, S, A, hidden, act, cdt, G, E, T, _ = CASES[case]
    if key not in _SETUPS:
        torch.manual_seed(7)
        cls = tg.GaussianActorCritic_NeuralNetwork if learner == "PPO" else tg.GaussianActor_NeuralNetwork
        kw = {"learn_std": True} if learn_std else {}
        if privileged:
            kw["privileged_critic"] = PRIVILEGED
        pol = cls(S, A, hidden, activation=act, cov=[0.5, 0.3, 0.4, 0.6][:A], device=dev, **kw)
        if learner == "PPO":
            # d loss / d (the critic's output bias) = 2 c1 mean(V - normalised return): the batch-normalised returns sum to zero and a
            # fresh critic predicts ~0, so that one scalar would be what is left of N terms of size 1e-3 cancelling to 2e-3 of their sum
            # of magnitudes -- a relative bar on it measures the cancellation, not the learner (measured on ppo_bf16_256x5: |g| 2.2e-3,
            # chunks of 96 away by 1.5e-7 = one rounding of the 0.5-sized partial sums, bar 4.4e-8).  A critic that predicts 0.25 on
            # average gives the scalar a scale of its own; every other tensor is as it was
            with torch.no_grad():
                pol.critic.network[-1].bias.fill_(0.25)
        torch.manual_seed(23)
        ref = tg.GaussianActor_NeuralNetwork(S, A, hidden, activation=act, cov=0.45, device=dev)
        with torch.no_grad():                                       # close to the policy: D stays small
            for p, q in zip(ref.actor.parameters(), pol.actor.parameters()):
                p.copy_(q + 0.01 * torch.randn_like(q))
        _SETUPS[key] = {"pol": pol, "ref": ref}
    s = _SETUPS[key]
    which = "small" if small else "buf"
    if which not in s:
        env_cls = getattr(tg, env_name)
        e, t, seed = (max(E // 3, 2), T // 2, 29) if small else (E, T, 19)

        def make_env():
            env = env_cls(max_steps=t)
            return env.randomize(PRIVILEGED, seed=21) if privileged else env
        mgr = tg.RolloutManager(make_env, s["pol"], num_workers=G, num_episodes_per_worker=e, seed=seed,
                                **({"compute_dtype": cdt} if cdt is not None else {}))
        buf = tg.Rollout_Buffer(mgr)
        buf.sample()
        s[which] = (buf, int(buf.group_masks.sum()))                # the mask's own count, on the host
    buf, rows = s[which]
    return s["pol"], buf, rows, s["ref"]


def named_grads(pol):
    out = {}
    for net in ("actor", "critic"):
        if getattr(pol, net, None) is not None:
            for k, p in getattr(pol, net).named_parameters():
                out[f"{net}.{k}"] = p.grad.detach().clone()
    if getattr(pol, "log_std", None) is not None:
        out["log_std"] = pol.log_std.grad.detach().clone()
    return out


@contextlib.contextmanager
def counted_entries(tg):
    """{entry point: calls} of every loss-head entry point, counted by wrapping the loaded library's attributes for the duration."""
    lib, calls, saved = tg._native.load(), {}, {}
    bases = tuple(set(FAMILY_BASES.values()))

    def wrap(name, fn):
        def counted(*args):
            calls[name] = calls.get(name, 0) + 1
            return fn(*args)
        return counted
    for name in tg._native.SIGNATURES:
        if name.startswith(bases):
            saved[name] = getattr(lib, name)
            setattr(lib, name, wrap(name, saved[name]))
    try:
        yield calls
    finally:
        for name, fn in saved.items():
            setattr(lib, name, fn)


@contextlib.contextmanager
def captured_loss_sums(tg):
    """The f64 loss-sum table learn() hands to its "loss_stats" all-reduce (GRPO [updates][4], PPO [steps][actor | critic][4])."""
    D, seen = tg.distributed, []
    plain = D.allreduce_sum_

    def spy(t, group=None, tag="other"):
        if tag == "loss_stats":
            seen.append(t)
        return plain(t, group, tag)
    D.allreduce_sum_ = spy
    try:
        yield seen
    finally:
        D.allreduce_sum_ = plain


def shorten_last_chunk(m, n_chunks):
    """The control arm: forward_loss() of GemmMLP `m` takes the last of every `n_chunks` calls with every row slice one row short
    (an ordinary launch on rows - 1)."""
    plain, calls = m.forward_loss, [0]

    def forward_loss(xp, kind, **kw):
        k = calls[0]
        calls[0] += 1
        if k % n_chunks == n_chunks - 1:
            assert xp.shape[0] >= 2
            xp = xp[:-1]
            kw = {key: (v[:-1] if key in ROW_ARGS and v is not None else v) for key, v in kw.items()}
        return plain(xp, kind, **kw)
    m.forward_loss = forward_loss


def build(tg, pol, case, feature, chunk, updates, ref=None, perm=None):
    """The learner of one arm on `pol` (a deep copy of the case's policy): plain Adam at lr = 0."""
    learner, _, S, A, hidden, act, cdt, *_ = CASES[case]
    opt = torch.optim.Adam(pol.parameters(), lr=0.0)
    kw = dict(policy=pol, optimizer=opt, updates_per_iter=updates, gamma=0.99, chunk_rows=chunk, autocast_dtype=cdt)
    if feature == "clip":
        kw["max_grad_norm"] = 0.5
    if learner == "PPO":
        algo = tg.PPO(epsilon=0.2, ref_model=None, batch_size=MINIBATCH if feature == "minibatch" else None,
                      entropy=0.05 if feature == "learn_std" else 0.01, **kw)
        if feature == "minibatch":
            algo.permutation_fn = lambda rows, device: perm.to(device)
    else:
        algo = tg.GRPO(epsilon=0.2, beta=0.04 if feature == "ref" else 0.0, ref_model=ref if feature == "ref" else None, **kw)
        if feature == "stale_old":                                  # an old policy that is not the policy: ratios != 1, the no-grad old pass
            gen = torch.Generator().manual_seed(31)
            with torch.no_grad():
                for p in algo.old_policy.actor.parameters():
                    p.add_((0.01 * torch.randn(p.shape, generator=gen)).to(p.device))
    return algo


def run_arm(tg, dev, case, feature, chunk, updates=3, control=False, history=False):
    """One learn() of one arm from the case's state -> a record of everything the tests compare.  chunk: chunk_rows (None: one chunk).
    control: the last chunk of every update one row short.  history: the learner first runs learn() on the case's smaller buffer."""
    base, buf, rows, ref = setup(tg, dev, case, feature)
    learner, _, S, A, hidden, act, cdt, G, E, T, family = CASES[case]
    pol = copy.deepcopy(base)
    perm = torch.randperm(rows, generator=torch.Generator().manual_seed(rows)) if feature == "minibatch" else None
    algo = build(tg, pol, case, feature, chunk, updates, ref=ref, perm=perm)
    nets = [pol.actor] + ([pol.critic] if learner == "PPO" else [])
    if history:
        _, small, small_rows, _ = setup(tg, dev, case, feature, small=True)
        assert 0 < small_rows < rows
        algo.learn(small)
        _ = algo.last_stats
    rode, logps, step_grads = [], [], []
    if feature == "minibatch":                                      # every optimizer step's gradients, not only the last (short) minibatch's
        plain_step = algo._optimizer_step

        def spy_step(*a, **k):
            step_grads.append(named_grads(pol))
            return plain_step(*a, **k)
        algo._optimizer_step = spy_step
    if learner == "GRPO":
        plain_rider = algo._adam_rider

        def spy_rider(*a, **k):
            r = plain_rider(*a, **k)
            rode.append(r is not None)
            return r
        algo._adam_rider = spy_rider
    plain_logp = algo._logp_nograd

    def spy_logp(*a, **k):
        out = plain_logp(*a, **k)
        logps.append(out)
        return out
    algo._logp_nograd = spy_logp
    n_chunks = len(chunk_bounds(rows, chunk or rows))
    if control:
        assert n_chunks >= 2 and feature is None
        for net in nets:
            shorten_last_chunk(algo._mlp(net), n_chunks)
    with counted_entries(tg) as calls, captured_loss_sums(tg) as sums:
        algo.learn(buf)
        torch.cuda.synchronize()
    stats = dict(algo.last_stats)
    traj = buf.device_traj
    ws = algo._ws._buf
    rec = {"rows": rows, "chunk": chunk, "n_chunks": n_chunks, "stats": stats, "grads": named_grads(pol), "calls": dict(calls),
           "rode": rode, "step_grads": step_grads, "sums": sums[0].detach().clone(), "logps": [t.detach().clone() for t in logps],
           "weights_kept": all(torch.equal(p, q) for p, q in zip(pol.parameters(), base.parameters())),
           "mlps": [algo._mlp(net) for net in nets], "per_row": {}}
    assert len(sums) == 1
    per_row = rec["per_row"]
    for name, n in (("old_logp", rows), ("ref_logp", rows), ("V", traj.T * traj.n), ("row0", rows), ("row1", rows)):
        if name in ws:
            per_row[name] = ws[name][:n].detach().clone()
    if learner == "PPO":
        per_row["norm8"] = algo.norm8.detach().clone()
    return rec


def expected_calls(case, feature, rows, chunk, updates=3):
    """Loss-head launches of one learn(): per optimizer step and net, one per chunk (the per-layer and autograd learners: one
    tg_surrogate_loss for both nets)."""
    learner, family = CASES[case][0], CASES[case][-1]
    nets = 2 if (learner == "PPO" and family in HAND_WRITTEN) else 1
    steps = [hi - lo for lo, hi in chunk_bounds(rows, MINIBATCH)] if feature == "minibatch" else [rows]
    return updates * nets * sum(len(chunk_bounds(r, chunk or r)) for r in steps)


def check_family(rec, case, feature, updates=3):
    """The kernel family the case names really ran: the GemmMLPs' own marks and the calls of the family's entry points."""
    learner, _, S, A, hidden, act, cdt, G, E, T, family = CASES[case]
    base = FAMILY_BASES[family]
    mine = {k: v for k, v in rec["calls"].items() if k.startswith(base)}
    assert mine and mine == rec["calls"], (case, feature, rec["calls"])
    assert sum(mine.values()) == expected_calls(case, feature, rec["rows"], rec["chunk"], updates), (case, feature, rec["chunk"], mine)
    for m in rec["mlps"]:
        if family == "bf16":
            assert m.cd == BF16 and m._chain is not None and m._bchain is not None and m._dw_ws is not None
        elif family in ("f32", "f32w", "f32r"):
            assert m._f32 is not None and m._f32.machine == family and m._f32.wide == (family == "f32w") and m._f32.res == (family == "f32r")
            assert m._dw_ws is not None
        elif family == "layer":
            assert m is not None and m._f32 is None and m._chain is None and m.cd == torch.float32
        else:
            assert m is None
    if act == "Tanh":
        assert set(mine) == {base + "_act"}, mine
    want = {"ref": "_ref", "learn_std": "_std"}.get(feature)
    if want is not None:
        assert any(k.endswith(want) for k in mine), mine
    # one-chunk fp32 GRPO takes the Adam rider (the optimizer owns exactly the net, no clipping) from its second update on -- the first
    # step of a fresh learner is the plain launch that gathers the derived layouts the rider then keeps current; several chunks never do
    if learner == "GRPO":
        assert len(rec["rode"]) == updates * rec["n_chunks"]
        if family in ("f32", "f32r") and feature in (None, "ref", "stale_old") and rec["n_chunks"] == 1:
            assert rec["rode"] == [False] + [True] * (updates - 1), (case, rec["chunk"], rec["rode"])
        else:
            assert not any(rec["rode"]), (case, rec["chunk"], rec["rode"])


# ---------------------------------------------------------------------------------------------------------------------------------
# the measured yardstick of the learners on library GEMMs: torch float32 autograd over all rows against the sum over the chunks
# ---------------------------------------------------------------------------------------------------------------------------------
def torch_chunk_yardstick(base, buf, rec, chunk):
    """{name: max |all rows - sum over chunks|} of plain torch float32 autograd of PPO's loss on the arm's own rows, weights, gathered
    advantages / returns and device constants (norm8): once over all valid rows, once accumulated chunk by chunk into .grad."""
    pol = copy.deepcopy(base)
    traj = buf.device_traj
    idx = traj.mask.reshape(-1).nonzero().squeeze(1)
    X = traj.obs_rows().index_select(0, idx).float().contiguous()
    act = traj.act_rows().index_select(0, idx).contiguous()
    adv, ret, n8 = rec["per_row"]["row0"], rec["per_row"]["row1"], rec["per_row"]["norm8"]
    var = torch.as_tensor(pol.var, dtype=torch.float32).to(X.device).reshape(-1)
    A = act.shape[1]

    def logp(x, a):
        mean = pol.actor(x)
        return -0.5 * ((a - mean) ** 2 / var).sum(1) - 0.5 * A * math.log(2 * math.pi) - 0.5 * torch.log(var).sum()
    with torch.no_grad():
        lpo = logp(X, act)

    def loss(lo, hi):
        lp = logp(X[lo:hi], act[lo:hi])
        rho = torch.exp(lp - lpo[lo:hi])
        a = (adv[lo:hi] - n8[0]) * n8[1]
        surr = torch.minimum(rho * a, rho.clamp(0.8, 1.2) * a)
        kl = torch.exp(lpo[lo:hi]) * (lpo[lo:hi] - lp)
        d = pol.critic(X[lo:hi]).reshape(-1) - (ret[lo:hi] - n8[2]) * n8[3]
        return n8[4] * surr.sum() + n8[5] * (d * d).sum() + n8[6] * kl.sum()
    params = [p for net in (pol.actor, pol.critic) for p in net.parameters()]
    out = []
    for bounds in ([(0, X.shape[0])], chunk_bounds(X.shape[0], chunk)):
        for p in params:
            p.grad = None
        for lo, hi in bounds:
            loss(lo, hi).backward()
        out.append({f"{net}.{k}": p.grad.detach().clone() for net in ("actor", "critic") for k, p in getattr(pol, net).named_parameters()})
    return {k: float((out[0][k].double() - out[1][k].double()).abs().max()) for k in out[0]}
