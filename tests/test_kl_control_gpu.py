"""kl_stats / desired_kl on the GPU: tg_lr_adapt bit for bit against its NumPy restatement, tg_policy_shift against float64 on exact
(dyadic) and on general inputs with the bounds of tests/kl_control_fp64.py, the learners (per-layer, bf16 chain, fp32 chain, autograd
Tanh) with the measurement on against the same learners without it, and two ranks against one.  Every case runs once."""
import copy
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import kl_control_fp64 as F

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def tg():
    import trajopt_grpo_amd as tg
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return tg


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


# ------------------------------------------------------------------------------------------------------------------------------
# 1. tg_lr_adapt: bit for bit
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(F.LR_CASES))
def test_lr_adapt_is_the_restated_rule_bit_for_bit(tg, dev, name):
    sums, desired_kl, factor, lr_min, lr_max, lr = F.LR_CASES[name]
    out = torch.full((4,), -7.0, dtype=torch.float64, device=dev)
    tg.hip_ops.lr_adapt(torch.tensor(sums, dtype=torch.float64, device=dev), desired_kl, factor, lr_min, lr_max, lr, out)
    got, want = out.cpu().numpy(), F.lr_rule(sums, desired_kl, factor, lr_min, lr_max, lr)
    print(name, got, want)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan) and np.array_equal(F.bits(got)[~nan], F.bits(want)[~nan]), (name, got, want)


# ------------------------------------------------------------------------------------------------------------------------------
# 2. tg_policy_shift
# ------------------------------------------------------------------------------------------------------------------------------
def _shift(tg, dev, mean_buf, A, act, old, epsilon, var=None, log_std=None, act_t=False, chunks=None):
    """-> (sums float64 [4], partials float64 [n][4]) of tg_policy_shift over `chunks` ((lo, hi) pairs, default one chunk) + finish.
    The partials buffer has two guard rows behind the last slot (NaN before and after)."""
    K = tg.hip_ops
    rows = mean_buf.shape[0]
    chunks = [(0, rows)] if chunks is None else chunks
    mean = torch.from_numpy(mean_buf).to(dev)[:, :A]
    a = torch.from_numpy(np.ascontiguousarray(act.T)).to(dev).t() if act_t else torch.from_numpy(act).to(dev)
    o = torch.from_numpy(old).to(dev)
    ls = None if log_std is None else torch.from_numpy(log_std).to(dev)
    n_part = sum(F.blocks(hi - lo) for lo, hi in chunks)
    partials = torch.full((n_part + 2, 4), float("nan"), dtype=torch.float64, device=dev)
    lo_, hi_ = F.log_bounds(epsilon)
    slot = 0
    for lo, hi in chunks:
        wrote = K.policy_shift(mean[lo:hi], a[lo:hi], o[lo:hi], var, lo_, hi_, partials, slot, log_std=ls)
        assert wrote == F.blocks(hi - lo) == K.policy_shift_blocks(hi - lo)
        slot += wrote
    sums = torch.full((4,), float("nan"), dtype=torch.float64, device=dev)
    K.policy_shift_finish(partials, slot, sums)
    p = partials.cpu().numpy()
    assert np.isnan(p[n_part:]).all() and not np.isnan(p[:n_part]).any(), "a partial outside the chunk's slots was written / one inside was not"
    return sums.cpu().numpy(), p[:n_part]


def _block_rows(rows):
    """Rows that workgroup b of a launch over `rows` rows adds: its 4096-row pieces, grid-stride."""
    nb = F.blocks(rows)
    out = np.zeros(nb)
    for piece in range(-(-rows // F.ROWS_PER_BLOCK)):
        out[piece % nb] += min(F.ROWS_PER_BLOCK, rows - piece * F.ROWS_PER_BLOCK)
    return out


@pytest.mark.parametrize("rows", F.EXACT_ROWS)
@pytest.mark.parametrize("A", [1, 4])
def test_policy_shift_on_exact_inputs(tg, dev, A, rows):
    mean, act, old, var = F.dyadic_inputs(A, rows)
    ref = F.dyadic_reference(mean, act, old, 0.2)
    assert ref["n_edge"] == 0
    sums, partials = _shift(tg, dev, mean, A, act, old, 0.2, var=var)
    assert partials.shape[0] == F.blocks(rows) and np.array_equal(partials[:, 0], _block_rows(rows))
    F.check_sums(sums, ref, f"A={A} rows={rows}")
    assert sums[2] == ref["sums"][2]                                         # (no edge rows: the clipped count is exact)
    again, partials2 = _shift(tg, dev, mean, A, act, old, 0.2, var=var)
    assert np.array_equal(F.bits(sums), F.bits(again)) and np.array_equal(F.bits(partials), F.bits(partials2))


@pytest.mark.parametrize("A", [1, 4])
def test_policy_shift_two_chunks_into_slots_0_and_1(tg, dev, A):
    rows = 4096 + 65
    mean, act, old, var = F.dyadic_inputs(A, rows, seed=5)
    ref = F.dyadic_reference(mean, act, old, 0.2)
    sums, partials = _shift(tg, dev, mean, A, act, old, 0.2, var=var, chunks=[(0, 4096), (4096, rows)])
    assert np.array_equal(partials[:, 0], [4096.0, 65.0])
    F.check_sums(sums, ref, f"A={A} two chunks")
    assert sums[2] == ref["sums"][2]
    for j in range(4):                                                      # finish: the partials in index order
        assert sums[j] == partials[0, j] + partials[1, j]
    # each chunk alone is the one-chunk launch on its rows, bit for bit
    for (lo, hi), p in zip([(0, 4096), (4096, rows)], partials):
        _, alone = _shift(tg, dev, mean[lo:hi], A, act[lo:hi], old[lo:hi], 0.2, var=var)
        assert np.array_equal(F.bits(alone[0]), F.bits(p))


@pytest.mark.parametrize("name", sorted(F.GENERAL_CASES))
def test_policy_shift_on_general_inputs(tg, dev, name):
    inp = F.general_inputs(name)
    A = inp["A"]
    ref = F.general_reference(inp["mean_buf"][:, :A], inp["act"], inp["logp_old"], F.GENERAL_EPSILON, inp.get("var"), inp.get("log_std"))
    sums, _ = _shift(tg, dev, inp["mean_buf"], A, inp["act"], inp["logp_old"], F.GENERAL_EPSILON, var=inp.get("var"),
                     log_std=inp.get("log_std"), act_t=inp["act_t"])
    F.check_sums(sums, ref, name)


def test_a_learned_std_is_not_read_on_the_host(tg, dev, monkeypatch):
    """With log_std on the device the call never forms a host variance array, and `var` is not looked at."""
    inp = F.general_inputs("a4_log_std_stride8")
    monkeypatch.setattr(tg.hip_ops, "_var_array", lambda var: pytest.fail("a host variance array was formed"))
    ref = F.general_reference(inp["mean_buf"][:, :4], inp["act"], inp["logp_old"], F.GENERAL_EPSILON, log_std=inp["log_std"])
    sums, _ = _shift(tg, dev, inp["mean_buf"], 4, inp["act"], inp["logp_old"], F.GENERAL_EPSILON, var=object(), log_std=inp["log_std"])
    F.check_sums(sums, ref, "log_std on the device")


# ------------------------------------------------------------------------------------------------------------------------------
# 3. the learners
# ------------------------------------------------------------------------------------------------------------------------------
# name -> (learner, env, S, A, hidden, activation, compute dtype, G, E, T, chunk_rows, desired_kl, learn_std)
# desired_kl = 10: every measured kl lies far below desired_kl / 2 (the rate grows by lr_factor per learn()); 1e-12: far above
# 2 desired_kl (it shrinks) -- either way each kl is more than 1 % away from both thresholds, which the test asserts.
# f32_chain_h64_band: a desired_kl of the size of the measured kl, so that the rate stays on some learn() calls and moves on others
# (BAND_BRANCHES: what the four calls do); the margins to the thresholds are asserted on the measured kl like everywhere else
BAND_KL, BAND_BRANCHES = 2e-4, ["stay", "up", "stay", "stay"]             # (measured kl: 1.09e-4, 0.98e-4, 1.75e-4, 1.07e-4 against 1e-4 / 4e-4)
LEARNERS = {
    "per_layer": ("PPO", "CartPole", 5, 1, (40, 40), "ReLU", None, 4, 16, 32, 257, 10.0, False),
    "bf16_chain_h128": ("GRPO", "CartPole", 5, 1, (128,) * 3, "ReLU", BF16, 4, 16, 32, None, 1e-12, False),
    "f32_chain_h64": ("GRPO", "CartPole", 5, 1, (64,), "ReLU", None, 4, 8, 16, None, 10.0, False),
    "autograd_tanh": ("PPO", "CartPole", 5, 1, (32, 32), "Tanh", None, 4, 8, 16, None, 1e-12, False),
    "f32_chain_learned_std": ("PPO", "QuadPole", 20, 4, (64, 64), "ReLU", None, 4, 8, 8, None, 10.0, True),
    "f32_chain_h64_band": ("GRPO", "CartPole", 5, 1, (64,), "ReLU", None, 4, 8, 16, None, BAND_KL, False),
}
N_LEARNS = {"f32_chain_h64_band": 4}                                         # (default 3)
LR0, EPS = 3e-4, 0.2
_RUNS = {}


def _make_algo(tg, case, pol, **kw):
    learner, _, _, _, _, _, cdt, _, _, _, chunk_rows, _, _ = LEARNERS[case]
    opt = torch.optim.Adam(pol.parameters(), lr=LR0)
    if learner == "PPO":
        return tg.PPO(epsilon=EPS, policy=pol, optimizer=opt, ref_model=None, updates_per_iter=2, gamma=0.99, batch_size=None,
                      autocast_dtype=cdt, chunk_rows=chunk_rows, **kw)
    return tg.GRPO(epsilon=EPS, beta=0.0, gamma=0.9, policy=pol, optimizer=opt, updates_per_iter=2, autocast_dtype=cdt,
                   chunk_rows=chunk_rows, **kw)


def _weights(pol):
    return [p.detach().clone() for p in pol.parameters()]


class _Spy:
    """Records what the measurement hands to hip_ops.policy_shift / policy_shift_finish / lr_adapt (copies, taken in stream order)."""
    def __init__(self, tg):
        self.K, self.saved, self.chunks, self.sums, self.rows, self.calls = tg.hip_ops, {}, [], [], [], 0

    def __enter__(self):
        K = self.K
        for name in ("policy_shift", "policy_shift_finish", "lr_adapt"):
            self.saved[name] = getattr(K, name)

        def policy_shift(mean, act, logp_old, var, log_lo, log_hi, partials, slot=0, log_std=None):
            self.chunks.append({"mean": mean.detach().cpu().numpy().copy(), "act": act.detach().cpu().numpy().copy(),
                                "old": logp_old.detach().cpu().numpy().copy(), "log_lo": log_lo, "log_hi": log_hi, "slot": slot,
                                "var": None if log_std is not None else np.asarray([float(v) for v in var], dtype=np.float32),
                                "log_std": None if log_std is None else log_std.detach().cpu().numpy().copy(), "learn": len(self.sums)})
            return self.saved["policy_shift"](mean, act, logp_old, var, log_lo, log_hi, partials, slot, log_std=log_std)

        def policy_shift_finish(partials, n_partials, sums):
            out = self.saved["policy_shift_finish"](partials, n_partials, sums)
            self.sums.append(sums.detach().cpu().numpy().copy())
            return out

        def lr_adapt(sums, desired_kl, factor, lr_min, lr_max, lr, out):
            res = self.saved["lr_adapt"](sums, desired_kl, factor, lr_min, lr_max, lr, out)
            self.rows.append({"sums": sums.detach().cpu().numpy().copy(), "args": (desired_kl, factor, lr_min, lr_max, lr),
                              "out": out.detach().cpu().numpy().copy()})
            return res
        K.policy_shift, K.policy_shift_finish, K.lr_adapt = policy_shift, policy_shift_finish, lr_adapt
        return self

    def __exit__(self, *exc):
        for name, fn in self.saved.items():
            setattr(self.K, name, fn)


def _counted(tg, name):
    """[calls] of one native entry point, counted on the loaded library's attribute; undo with the returned function."""
    lib, calls = tg._native.load(), [0]
    plain = getattr(lib, name)

    def counted(*args):
        calls[0] += 1
        return plain(*args)
    setattr(lib, name, counted)
    return calls, lambda: setattr(lib, name, plain)


def _run(tg, dev, case):
    """Once per case: one policy, one buffer; the arm with desired_kl takes three learn() calls on it under the spy; the plain arm (a
    deep copy, no keyword) takes the same three with its optimizer's lr set by hand to the restated sequence."""
    if case in _RUNS:
        return _RUNS[case]
    learner, env_name, S, A, hidden, act, cdt, G, E, T, _, desired_kl, learn_std = LEARNERS[case]
    torch.manual_seed(11)
    cls = tg.GaussianActorCritic_NeuralNetwork if learner == "PPO" else tg.GaussianActor_NeuralNetwork
    kw = {"learn_std": True} if learn_std else {}
    pol = cls(S, A, hidden, activation=act, cov=[0.5, 0.3, 0.4, 0.6][:A], device=dev, **kw)
    env_cls = getattr(tg, env_name)
    mkw = {"compute_dtype": cdt} if cdt is not None else {}
    mgr = tg.RolloutManager(lambda: env_cls(max_steps=T), pol, num_workers=G, num_episodes_per_worker=E, seed=13, **mkw)
    buf = tg.Rollout_Buffer(mgr)
    buf.sample()
    pol_kl, pol_plain = copy.deepcopy(pol), copy.deepcopy(pol)
    algo_kl, algo_plain = _make_algo(tg, case, pol_kl, desired_kl=desired_kl), _make_algo(tg, case, pol_plain)
    n = N_LEARNS.get(case, 3)
    rec = {"weights_kl": [], "weights_plain": [], "stats": [], "lr_seq": [LR0], "desired_kl": desired_kl, "n": n, "pol": pol, "buf": buf}
    calls, undo = _counted(tg, "tg_policy_shift")
    try:
        with _Spy(tg) as spy:
            for i in range(n):
                algo_kl.learn(buf)
                rec["weights_kl"].append(_weights(pol_kl))
                rec["stats"].append(dict(algo_kl.last_stats))
        rec["calls_kl"] = calls[0]
        calls[0] = 0
        for i in range(n):
            row = F.lr_rule(spy.rows[i]["sums"], desired_kl, 1.5, 1e-5, 1e-2, rec["lr_seq"][i])
            rec["lr_seq"].append(float(row[3]))
            for g in algo_plain.optimizer.param_groups:
                g["lr"] = rec["lr_seq"][i]
            algo_plain.learn(buf)
            rec["weights_plain"].append(_weights(pol_plain))
        rec["stats_plain"] = dict(algo_plain.last_stats)
        rec["calls_plain"] = calls[0]
    finally:
        undo()
    rec["spy"], rec["algo_kl"], rec["A"] = spy, algo_kl, A
    _RUNS[case] = rec
    return rec


@pytest.mark.parametrize("case", sorted(LEARNERS))
def test_the_measurement_leaves_the_update_untouched(tg, dev, case):
    """(a) After one learn() from the same weights with the same lr, every weight is bit-identical with and without desired_kl; the
    plain learner never calls tg_policy_shift and reports none of the new statistics."""
    rec = _run(tg, dev, case)
    for a, b in zip(rec["weights_kl"][0], rec["weights_plain"][0]):
        assert torch.equal(a, b)
    assert rec["calls_plain"] == 0 and rec["calls_kl"] >= 3
    assert not {"approx_kl", "clip_fraction", "log_ratio_mean", "lr"} & set(rec["stats_plain"])
    assert {"approx_kl", "clip_fraction", "log_ratio_mean", "lr"} <= set(rec["stats"][0])


@pytest.mark.parametrize("case", sorted(LEARNERS))
def test_the_sums_against_float64_on_the_captured_inputs(tg, dev, case):
    """(b) What learn() handed to K.policy_shift, restated in float64, against the sums it got back."""
    rec = _run(tg, dev, case)
    spy, A = rec["spy"], rec["A"]
    lo, hi = F.log_bounds(EPS)
    for i in range(rec["n"]):
        ch = [c for c in spy.chunks if c["learn"] == i]
        assert ch and all(c["log_lo"] == lo and c["log_hi"] == hi for c in ch)
        if case == "per_layer":
            assert len(ch) > 1 and [c["slot"] for c in ch] == list(range(len(ch)))         # chunks of 257 rows: one partial each
        if case == "f32_chain_learned_std":
            assert all(c["log_std"] is not None for c in ch)
        mean, act, old = (np.concatenate([c[k] for c in ch]) for k in ("mean", "act", "old"))
        ref = F.general_reference(mean[:, :A], act, old, EPS, ch[0]["var"], ch[0]["log_std"])
        F.check_sums(spy.sums[i], ref, f"{case} learn {i}")
        assert np.array_equal(F.bits(spy.sums[i]), F.bits(spy.rows[i]["sums"]))               # one rank: the all-reduce changes nothing
        row = F.lr_rule(spy.rows[i]["sums"], *spy.rows[i]["args"])
        assert np.array_equal(F.bits(row), F.bits(spy.rows[i]["out"]))
        st = rec["stats"][i]
        assert st["approx_kl"] == row[0] and st["clip_fraction"] == row[1] and st["lr"] == row[3]
        assert st["log_ratio_mean"] == spy.sums[i][3] / spy.sums[i][0]
        assert st["approx_kl"] > 0.0 and 0.0 <= st["clip_fraction"] <= 1.0


@pytest.mark.parametrize("case", sorted(LEARNERS))
def test_three_learns_equal_a_plain_learner_with_the_restated_lr_sequence(tg, dev, case):
    """(c) Bit-identical weights after each of three learn() calls; every kl at least 1 % away from both thresholds; the rate moved."""
    rec = _run(tg, dev, case)
    d = rec["desired_kl"]
    for i in range(rec["n"]):
        kl = rec["stats"][i]["approx_kl"]
        print(case, "learn", i, "kl", kl, "clip_fraction", rec["stats"][i]["clip_fraction"], "lr", rec["lr_seq"][i], "->", rec["lr_seq"][i + 1])
        assert abs(kl - 2.0 * d) >= 0.01 * 2.0 * d and abs(kl - 0.5 * d) >= 0.01 * 0.5 * d
        assert rec["spy"].rows[i]["args"][4] == rec["lr_seq"][i]                              # the lr each measurement was given, by value
        for a, b in zip(rec["weights_kl"][i], rec["weights_plain"][i]):
            assert torch.equal(a, b), (case, i)
    branches = []
    for i, (a, b) in enumerate(zip(rec["lr_seq"], rec["lr_seq"][1:])):     # the branch the measured kl selects, and the rate it gives
        kl = rec["stats"][i]["approx_kl"]
        branches.append("down" if kl > 2.0 * d else "up" if kl < 0.5 * d else "stay")
        assert b == {"down": max(a / 1.5, 1e-5), "up": min(a * 1.5, 1e-2), "stay": a}[branches[-1]]
    print(case, branches)
    if case == "f32_chain_h64_band":
        assert branches == BAND_BRANCHES and "stay" in branches and len(set(branches)) > 1
    else:                                                                   # (kl << desired_kl / 2: up; kl >> 2 desired_kl: down)
        assert branches == ["up" if d > 1 else "down"] * rec["n"]
    assert rec["algo_kl"].optimizer.param_groups[0]["lr"] == rec["lr_seq"][rec["n"]]


def test_back_to_back_learns_pick_the_adapted_lr_up_themselves(tg, dev):
    """The path of a training loop that never reads last_stats: three learn() calls with nothing in between.  Each call applies the
    previous call's result itself (after its prologue), so every measurement is given the restated lr by value and the final weights
    are those of the plain learner stepped through the same sequence."""
    case = "f32_chain_h64"
    rec = _run(tg, dev, case)
    pol = copy.deepcopy(rec["pol"])
    algo = _make_algo(tg, case, pol, desired_kl=rec["desired_kl"])
    with _Spy(tg) as spy:
        for _ in range(3):
            algo.learn(rec["buf"])
    assert [r["args"][4] for r in spy.rows] == rec["lr_seq"][:3]
    assert algo.optimizer.param_groups[0]["lr"] == rec["lr_seq"][2]         # (the third result is still pending)
    for a, b in zip(_weights(pol), rec["weights_plain"][2]):
        assert torch.equal(a, b)
    assert algo.last_stats["lr"] == rec["lr_seq"][3] == algo.optimizer.param_groups[0]["lr"]


def test_exact_zero_when_nothing_moves(tg, dev):
    """(d) kl_stats alone, an optimizer lr of 0.0, two updates in PPO's minibatch mode (the old log-probabilities come from the same
    no-grad pass over the same weights): every statistic is exactly zero."""
    torch.manual_seed(3)
    pol = tg.GaussianActorCritic_NeuralNetwork(5, 1, (64, 64), cov=0.5, device=dev)
    mgr = tg.RolloutManager(lambda: tg.CartPole(max_steps=16), pol, num_workers=4, num_episodes_per_worker=8, seed=5)
    buf = tg.Rollout_Buffer(mgr)
    buf.sample()
    algo = tg.PPO(epsilon=EPS, policy=pol, optimizer=torch.optim.Adam(pol.parameters(), lr=0.0), ref_model=None, updates_per_iter=2,
                  gamma=0.99, batch_size=64, kl_stats=True)
    algo.learn(buf)
    st = algo.last_stats
    print({k: st[k] for k in ("approx_kl", "clip_fraction", "log_ratio_mean", "lr", "n_valid")})
    assert st["approx_kl"] == 0.0 and st["clip_fraction"] == 0.0 and st["log_ratio_mean"] == 0.0 and st["lr"] == 0.0
    assert st["n_valid"] > 64


def test_checkpoint_holds_the_adapted_lr_and_the_user_wins(tg, dev, tmp_path):
    """(e) save() right after learn() (nobody has read last_stats) writes the adapted lr; an lr the user sets after learn() stays."""
    torch.manual_seed(4)
    pol = tg.GaussianActor_NeuralNetwork(5, 1, (64,), cov=0.5, device=dev)
    mgr = tg.RolloutManager(lambda: tg.CartPole(max_steps=16), pol, num_workers=4, num_episodes_per_worker=8, seed=6)
    buf = tg.Rollout_Buffer(mgr)
    buf.sample()
    algo = tg.GRPO(epsilon=EPS, beta=0.0, gamma=0.9, policy=pol, optimizer=torch.optim.Adam(pol.parameters(), lr=LR0), updates_per_iter=2,
                   desired_kl=10.0, lr_factor=2.0, lr_bounds=(1e-5, 5e-4))
    algo.learn(buf)
    assert algo.optimizer.param_groups[0]["lr"] == LR0                      # (not applied yet: the host has not asked)
    algo.save(str(tmp_path))
    sd = torch.load(os.path.join(str(tmp_path), "optimizer.pth"), weights_only=True)
    assert sd["param_groups"][0]["lr"] == 5e-4 == algo.optimizer.param_groups[0]["lr"]       # LR0 * 2 clamped at lr_max
    algo.learn(buf)
    algo.optimizer.param_groups[0]["lr"] = 7e-5                             # the user's own value, set before the result is applied
    st = algo.last_stats
    assert st["lr"] == 7e-5 == algo.optimizer.param_groups[0]["lr"]
    assert algo.metadata()["desired_kl"] == 10.0 and algo.metadata()["lr_bounds"] == [1e-5, 5e-4]


# ------------------------------------------------------------------------------------------------------------------------------
# 4. ranks
# ------------------------------------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_ranks_agree_with_each_other_and_with_one_rank(tmp_path):
    """tests/kl_control_dist_worker.py as fresh child processes, each under its own `timeout` (gloo, both ranks on cuda:0, half the
    groups each).  Both ranks hold the same lr and statistics bits; the lr decisions are the one-rank run's; where the measured rows
    are the same bits at every world size (the stale-old-policy case: no update runs), approx_kl differs from the one-rank run's by
    at most the float64 reordering of its n terms, 2 (n - 1) 2^-53 sum |k3| / n."""
    worker = os.path.join(HERE, "kl_control_dist_worker.py")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="2")
    procs, outs = [], {}
    for world in (1, 2):
        port = _free_port()
        outs[world] = [str(tmp_path / f"w{world}_r{r}.pt") for r in range(world)]
        for r in range(world):
            procs.append(subprocess.Popen(["timeout", "-k", "10", "240", sys.executable, worker, str(r), str(world), str(port), outs[world][r]],
                                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env))
    for p in procs:
        log, _ = p.communicate()
        assert p.returncode == 0, log.decode("utf-8", "replace")[-3000:]
    one = torch.load(outs[1][0], weights_only=False)
    two = [torch.load(f, weights_only=False) for f in outs[2]]
    for case, rec in one.items():
        a, b = two[0][case], two[1][case]
        print(case, "one rank", rec["stats"], "two ranks", a["stats"])
        assert a["bits"] == b["bits"] and len(a["bits"]) == len(rec["bits"]) > 0
        assert [s["lr"] for s in a["stats"]] == [s["lr"] for s in rec["stats"]]
        assert all(s["lr"] != rec["lr0"] for s in rec["stats"])
        assert a["n_valid"] == rec["n_valid"]
        if rec["same_rows"]:
            n = rec["n_valid"]
            for s2, s1 in zip(a["stats"], rec["stats"]):
                bound = 2.0 * (n - 1) * F.U53 * s1["approx_kl"] * F.SLACK
                assert s1["approx_kl"] > 0.0 and abs(s2["approx_kl"] - s1["approx_kl"]) <= bound, (s2["approx_kl"], s1["approx_kl"], bound)
                assert s2["clip_fraction"] == s1["clip_fraction"]
