"""target_kl / kl_every on the GPU: tg_kl_control bit for bit against its NumPy restatement (tests/kl_stop_fp64.py), the `_ctl` Adam
launches against the plain ones byte for byte (open gate) and against nothing at all (latched gate), a stop against the learner
that was given fewer updates, per-update adaptation against a learner whose lr is set by hand, the combinations, two ranks, and
the launches of a learner without the keywords.  Every learner case runs at 64 envs."""
import copy
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import kl_stop_fp64 as S

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
BF16 = torch.bfloat16
CTL_ADAM = ["tg_adam_step_ctl", "tg_adam_step_push_ctl", "tg_adam_step_ctl_clip", "tg_adam_step_push_ctl_clip"]
NEW = ["tg_kl_control"] + CTL_ADAM


@pytest.fixture(scope="module")
def tg():
    import trajopt_grpo_amd as tg
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return tg


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


class _Counted:
    """Calls of native entry points, counted on the loaded library's attributes."""
    def __init__(self, tg, names):
        self.lib, self.names, self.calls, self.plain = tg._native.load(), names, {n: 0 for n in names}, {}

    def __enter__(self):
        for name in self.names:
            self.plain[name] = plain = getattr(self.lib, name)

            def counted(*args, _name=name, _plain=plain):
                self.calls[_name] += 1
                return _plain(*args)
            setattr(self.lib, name, counted)
        return self

    def __exit__(self, *exc):
        for name, fn in self.plain.items():
            setattr(self.lib, name, fn)

    def total(self, names=None):
        return sum(self.calls[n] for n in (names or self.names))


# ------------------------------------------------------------------------------------------------------------------------------
# 1. tg_kl_control: bit for bit
# ------------------------------------------------------------------------------------------------------------------------------
def _control(tg, dev, ctl, sums, *args):
    block = torch.tensor(np.asarray(ctl, dtype=np.float64), device=dev)
    tg.hip_ops.kl_control(torch.tensor(sums, dtype=torch.float64, device=dev), *args, block)
    return block.cpu().numpy()


@pytest.mark.parametrize("name", sorted(S.CASES))
def test_kl_control_is_the_restated_rule_bit_for_bit(tg, dev, name):
    ctl, sums, *args = S.CASES[name]
    got, want = _control(tg, dev, ctl, sums, *args), S.kl_control(ctl, sums, *args)
    print(name, got, want)
    assert S.same_bits(got, want), (name, got, want)
    if name == "latched_stays":
        assert np.array_equal(S.bits(got), S.bits(ctl))


def test_five_checks_through_one_block(tg, dev):
    """adapt, adapt, latch, two no-ops: the device block after each check is the restated one."""
    block = torch.tensor(S.init_block(1e-3), device=dev)
    for j, (sums, want) in enumerate(zip(S.SEQUENCE_SUMS, S.run_sequence(1e-3))):
        tg.hip_ops.kl_control(torch.tensor(sums, dtype=torch.float64, device=dev), *S.SEQUENCE_ARGS, j + 1, block)
        got = block.cpu().numpy()
        print(j, got)
        assert S.same_bits(got, want), (j, got, want)
    assert got[S.STOPPED] == 1.0 and got[S.STOP_UPDATE] == 3.0 and got[S.CHECKS] == 3.0


# ------------------------------------------------------------------------------------------------------------------------------
# 2. the `_ctl` Adam launches
# ------------------------------------------------------------------------------------------------------------------------------
SIZES = [1, 255, 771]                   # 1027 elements: four full workgroups of 256 and three threads of a fifth; none a multiple of 4
ADAM = (1e-3, 0.9, 0.999, 1e-8)
STEP = 3


class _Table:
    """Parameters, gradients and moments of SIZES, the device tensor table, and two derived layouts with their push tables: an f32
    layout (every element once, padding between the tensors) and a bf16 layout (every second element)."""
    def __init__(self, dev, seed=0):
        g = torch.Generator(device="cpu").manual_seed(seed)
        mk = lambda n, scale: (torch.randn(n, generator=g) * scale).to(dev)
        self.p = [mk(n, 1.0) for n in SIZES]
        self.g = [mk(n, 0.1) for n in SIZES]
        self.m = [mk(n, 0.05) for n in SIZES]
        self.v = [mk(n, 0.01).abs() for n in SIZES]
        firsts = np.concatenate([[0], np.cumsum(SIZES)[:-1]])
        self.total = int(sum(SIZES))
        self.table = torch.tensor([[p.data_ptr(), g_.data_ptr(), m.data_ptr(), v.data_ptr(), int(f)]
                                   for p, g_, m, v, f in zip(self.p, self.g, self.m, self.v, firsts)], dtype=torch.int64).to(dev)
        codes_a, codes_b = [], []
        for t, n in enumerate(SIZES):
            codes_a += [(t << 24) | i for i in range(n)] + [-1, -1, -1]
            codes_b += [(t << 24) | i for i in range(0, n, 2)]
        self.codes = [torch.tensor(c, dtype=torch.int32, device=dev) for c in (codes_a, codes_b)]
        self.dst = [torch.full((len(codes_a),), -5.0, dtype=torch.float32, device=dev),
                    torch.full((len(codes_b),), -5.0, dtype=torch.bfloat16, device=dev)]
        seg_first = [0, len(codes_a)]
        self.seg = torch.tensor([[d.data_ptr(), c.data_ptr(), f, b] for d, c, f, b in zip(self.dst, self.codes, seg_first, (0, 1))],
                                dtype=torch.int64).to(dev)
        elem, dst = [], []
        for si, code in enumerate((codes_a, codes_b)):
            for j, c in enumerate(code):
                if c >= 0:
                    elem.append(int(firsts[c >> 24]) + (c & 0xFFFFFF))
                    dst.append((si << 26) | j)
        order = np.argsort(np.asarray(elem), kind="stable")
        counts = np.bincount(np.asarray(elem), minlength=self.total)
        inv_start = np.concatenate([[0], np.cumsum(counts)])
        self.inv_start = torch.tensor(inv_start, dtype=torch.int32, device=dev)
        self.inv_dst = torch.tensor(np.asarray(dst)[order], dtype=torch.int32, device=dev)
        self.coef = torch.tensor([0.625], dtype=torch.float32, device=dev)

    def gather(self, tg):
        """The layouts as tg_gather_streams builds them from the current parameters (padding included)."""
        N = tg._native
        N.check(N.load().tg_gather_streams(self.seg.data_ptr(), 2, sum(d.numel() for d in self.dst), self.table.data_ptr(), N.stream_ptr()))

    def state(self):
        torch.cuda.synchronize()
        return [t.clone() for t in self.p + self.g + self.m + self.v + self.dst]

    def launch(self, tg, push, clip, zero_grads, ctl=None, lr_from_ctl=0, lr=ADAM[0]):
        N = tg._native
        name = "tg_adam_step" + ("_push" if push else "") + ("" if ctl is None else "_ctl") + ("_clip" if clip else "")
        args = [self.table.data_ptr(), len(SIZES), self.total, lr, *ADAM[1:], STEP, 1 if zero_grads else 0]
        if push:
            args += [self.seg.data_ptr(), 2, self.inv_start.data_ptr(), self.inv_dst.data_ptr()]
        if clip:
            args += [self.coef.data_ptr()]
        if ctl is not None:
            args += [ctl.data_ptr(), lr_from_ctl, 1.0 - ADAM[1] ** STEP]
        N.check(getattr(N.load(), name)(*args, N.stream_ptr()), name)


def _equal_bytes(a, b):
    return all(x.dtype == y.dtype and torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(a, b))


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("push", [False, True])
def test_ctl_adam_open_gate_is_the_plain_launch_byte_for_byte(tg, dev, push, clip):
    for zero_grads in (False, True):
        ref = _Table(dev)
        ref.gather(tg)
        ref.launch(tg, push, clip, zero_grads)
        want = ref.state()
        for lr_from_ctl in (0, 1):
            t = _Table(dev)
            t.gather(tg)
            before = t.state()
            # lr_from_ctl = 1: the rate is the block's and the by-value lr is not read; 0: the other way round
            block = torch.tensor(S.init_block(ADAM[0] if lr_from_ctl else 7.0), device=dev)
            t.launch(tg, push, clip, zero_grads, ctl=block, lr_from_ctl=lr_from_ctl, lr=7.0 if lr_from_ctl else ADAM[0])
            got = t.state()
            assert _equal_bytes(got, want), (push, clip, zero_grads, lr_from_ctl)
            assert not _equal_bytes(got[:len(SIZES)], before[:len(SIZES)])          # (the parameters did move)
            assert np.array_equal(S.bits(block.cpu().numpy())[:4], S.bits(S.init_block(ADAM[0] if lr_from_ctl else 7.0))[:4])


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("push", [False, True])
def test_ctl_adam_latched_gate_changes_nothing_but_the_gradients_it_is_asked_to_zero(tg, dev, push, clip):
    n = len(SIZES)
    for zero_grads in (False, True):
        for lr_from_ctl in (0, 1):
            t = _Table(dev)
            t.gather(tg)
            before = t.state()
            block = torch.tensor([1.0, ADAM[0], 2.0, 0.5, 0.5, 0.1, 2.0, 0.0], dtype=torch.float64, device=dev)
            t.launch(tg, push, clip, zero_grads, ctl=block, lr_from_ctl=lr_from_ctl)
            got = t.state()
            assert _equal_bytes(got[:n], before[:n]) and _equal_bytes(got[2 * n:], before[2 * n:]), (push, clip, zero_grads, lr_from_ctl)
            if zero_grads:
                assert all(bool((g == 0).all()) and not bool(torch.signbit(g).any()) for g in got[n:2 * n])
            else:                                                           # (the clip product is not written back)
                assert _equal_bytes(got[n:2 * n], before[n:2 * n])


# ------------------------------------------------------------------------------------------------------------------------------
# 3. the learners
# ------------------------------------------------------------------------------------------------------------------------------
# name -> (env, S, A, hidden, compute dtype, G, E, T): 64 envs each
SHAPES = {
    "per_layer": ("CartPole", 5, 1, (24, 24), None, 4, 16, 32),
    "bf16_chain_h128": ("CartPole", 5, 1, (128,) * 3, BF16, 4, 16, 32),
    "f32_chain_h64": ("CartPole", 5, 1, (64,), None, 4, 16, 16),
    "f32_chain_quadpole": ("QuadPole", 20, 4, (64, 64), None, 4, 16, 8),
}
LR, EPS, UPDATES = 1e-3, 0.2, 6
_BASE = {}


def _base(tg, dev, algo_name, shape, **pol_kw):
    """(policy, buffer) of a case, made once: every learner of the case starts from a deep copy of the policy on the same buffer."""
    key = (algo_name, shape, tuple(sorted(pol_kw.items())))
    if key not in _BASE:
        env_name, S_, A, hidden, cdt, G, E, T = SHAPES[shape]
        torch.manual_seed(21)
        cls = tg.GaussianActorCritic_NeuralNetwork if algo_name == "PPO" else tg.GaussianActor_NeuralNetwork
        pol = cls(S_, A, hidden, cov=[0.5, 0.3, 0.4, 0.6][:A], device=dev, **pol_kw)
        env_cls = getattr(tg, env_name)
        mgr = tg.RolloutManager(lambda: env_cls(max_steps=T), pol, num_workers=G, num_episodes_per_worker=E, seed=17,
                                **({"compute_dtype": cdt} if cdt is not None else {}))
        buf = tg.Rollout_Buffer(mgr)
        buf.sample()
        _BASE[key] = (pol, buf)
    return _BASE[key]


def _make(tg, algo_name, shape, pol0, updates, opt=None, lr=LR, **kw):
    pol = copy.deepcopy(pol0)
    cdt = SHAPES[shape][4]
    optimizer = opt(pol.parameters()) if opt is not None else torch.optim.Adam(pol.parameters(), lr=lr)
    if algo_name == "PPO":
        kw.setdefault("batch_size", None)
        return tg.PPO(epsilon=EPS, policy=pol, optimizer=optimizer, ref_model=None, updates_per_iter=updates, gamma=0.99, autocast_dtype=cdt, **kw)
    return tg.GRPO(epsilon=EPS, beta=0.0, gamma=0.9, policy=pol, optimizer=optimizer, updates_per_iter=updates, autocast_dtype=cdt, **kw)


def _snapshot(algo):
    """Everything a stop must leave as the shorter learn() leaves it, read after the reconciliation (last_stats): the weights, Adam's
    moments and step counters, old_policy, and every derived layout of the policy's and the old policy's nets."""
    stats = dict(algo.last_stats)
    torch.cuda.synchronize()
    out = {"w": [p.detach().clone() for p in algo.policy.parameters()], "old": [p.detach().clone() for p in algo.old_policy.parameters()],
           "m": [], "v": [], "step": [], "layouts": [], "stats": stats}
    for g in algo.optimizer.param_groups:
        for p in g["params"]:
            st = algo.optimizer.state[p]
            out["m"].append(st["exp_avg"].clone())
            out["v"].append(st["exp_avg_sq"].clone())
            out["step"].append(float(st["step"]))
    for pol in (algo.policy, algo.old_policy):
        for name in ("actor", "critic"):
            net = getattr(pol, name, None)
            m = algo._mlps.get(id(net)) if net is not None else None
            if m is not None:
                # (a layout that is marked stale -- torch's own optimizer step leaves them to the next reader -- is rebuilt as that
                # reader would; one that is marked fresh is taken as it stands, so a launch that marked what it did not write shows)
                m.refresh()
                for what, stream in m.streams():
                    m._fresh(what)
                    out["layouts"] +=[(pol is algo.policy, name, what, dst.clone()) for dst, _ in stream.outputs]
    return out


def _assert_same(a, b, tag):
    for key in ("w", "old", "m", "v"):
        assert len(a[key]) == len(b[key]) > 0
        for i, (x, y) in enumerate(zip(a[key], b[key])):
            assert torch.equal(x, y), (tag, key, i, float((x - y).abs().max()))
    assert a["step"] == b["step"], (tag, a["step"], b["step"])
    assert [l[:3] for l in a["layouts"]] == [l[:3] for l in b["layouts"]], tag
    for (_, name, what, x), (_, _, _, y) in zip(a["layouts"], b["layouts"]):
        assert x.dtype == y.dtype and torch.equal(x.view(torch.uint8), y.view(torch.uint8)), (tag, name, what)


def _learn_counted(tg, algo, buf, lag="default"):
    if lag != "default":
        algo._KL_BREAK_LAG = lag
    with _Counted(tg, NEW) as c:
        algo.learn(buf)
    return c


def _pick(kls, first=2):
    """From the kl after every step: the first step j >= first whose kl exceeds every earlier one by more than 1 %, and the target_kl
    that puts the stop threshold 1.5 target_kl halfway between them."""
    for j in range(first, len(kls) + 1):
        before = max(kls[:j - 1])
        if kls[j - 1] > 1.01 * before:
            return j, (before + kls[j - 1]) / 2.0 / 1.5
    raise AssertionError(f"no step of {kls} exceeds the ones before it")


@pytest.mark.parametrize("shape", ["per_layer", "bf16_chain_h128", "f32_chain_h64"])
@pytest.mark.parametrize("algo_name", ["PPO", "GRPO"])
def test_a_stop_is_a_truncation(tg, dev, algo_name, shape):
    """kl_j from plain learners with updates_per_iter = j; target_kl between max(kl_1, kl_2) and kl_3: the learner stops after three
    of its six updates and is, bit for bit, the plain learner that was given three -- with the host never breaking (the device gate
    alone) and with the host following one check behind (fewer updates enqueued)."""
    pol0, buf = _base(tg, dev, algo_name, shape)
    kls, plain3 = [], None
    for j in range(1, 6):
        a = _make(tg, algo_name, shape, pol0, j, kl_stats=True)
        a.learn(buf)
        kls.append(a.last_stats["approx_kl"])
        if j == 3:
            plain3 = _snapshot(a)
    print(algo_name, shape, "kl_j", kls)
    assert max(kls[0], kls[1]) < kls[2], kls
    target = (max(kls[0], kls[1]) + kls[2]) / 2.0 / 1.5
    per_step = "J" if algo_name == "GRPO" else "actor_loss"
    assert len(plain3["stats"][per_step]) == 3
    for lag in (None, 1):
        a = _make(tg, algo_name, shape, pol0, UPDATES, target_kl=target)
        calls = _learn_counted(tg, a, buf, lag)
        snap = _snapshot(a)
        st = snap["stats"]
        print(algo_name, shape, "lag", lag, {k: st[k] for k in ("n_updates", "kl_stopped", "kl_checks", "approx_kl")}, calls.calls)
        assert st["n_updates"] == 3 and st["kl_stopped"] is True
        assert st["kl_checks"] == kls[:3] and st["approx_kl"] == kls[2]     # a check is the end-of-learn() measurement's own sequence
        assert st[per_step] == plain3["stats"][per_step]                    # (cut to the updates applied)
        _assert_same(snap, plain3, (algo_name, shape, lag))
        enqueued = calls.total(CTL_ADAM)
        if lag is None:
            assert enqueued == UPDATES and calls.calls["tg_kl_control"] == UPDATES - 1
        else:
            assert 3 <= enqueued < UPDATES
    huge = _make(tg, algo_name, shape, pol0, UPDATES, target_kl=1e30)
    plain = _make(tg, algo_name, shape, pol0, UPDATES)
    huge.learn(buf)
    plain.learn(buf)
    s_huge, s_plain = _snapshot(huge), _snapshot(plain)
    assert s_huge["stats"]["n_updates"] == UPDATES and s_huge["stats"]["kl_stopped"] is False and len(s_huge["stats"]["kl_checks"]) == UPDATES - 1
    assert "n_updates" not in s_plain["stats"]
    _assert_same(s_huge, s_plain, (algo_name, shape, "huge"))


# ------------------------------------------------------------------------------------------------------------------------------
# 4. per-update adaptation
# ------------------------------------------------------------------------------------------------------------------------------
def _hand_set_lr(algo, seq):
    """The plain learner's param-group lr before every optimizer step <- seq[steps taken so far] (its step may ride on the backward
    pass's last launch: the rate is set where either form reads it)."""
    def set_lr():
        st = algo.optimizer.state
        p0 = algo.optimizer.param_groups[0]["params"][0]
        k = int(st[p0]["step"]) if p0 in st and "step" in st[p0] else 0
        for g in algo.optimizer.param_groups:
            g["lr"] = seq[k]
    rider, step = algo._adam_rider, algo._optimizer_step

    def adam_rider(*a, **kw):
        set_lr()
        return rider(*a, **kw)

    def optimizer_step(*a, **kw):
        set_lr()
        return step(*a, **kw)
    algo._adam_rider, algo._optimizer_step = adam_rider, optimizer_step


@pytest.mark.parametrize("algo_name,shape", [("GRPO", "f32_chain_h64"), ("PPO", "bf16_chain_h128"), ("PPO", "per_layer")])
def test_per_update_adaptation_equals_a_hand_set_lr_sequence(tg, dev, algo_name, shape):
    """desired_kl far below every measured kl with kl_every = 1: the rate is divided by 1.5 behind every update until lr_min holds
    it (1e-3 -> 6.67e-4 -> 4.44e-4 -> 4e-4 -> 4e-4 ...), on the device; a plain learner stepped through the recorded sequence is
    bit-identical."""
    pol0, buf = _base(tg, dev, algo_name, shape)
    a = _make(tg, algo_name, shape, pol0, UPDATES, desired_kl=1e-12, kl_every=1, lr_bounds=(4e-4, 1e-2))
    calls = _learn_counted(tg, a, buf)
    snap = _snapshot(a)
    st = snap["stats"]
    print(algo_name, shape, st["lr_checks"], st["kl_checks"], st["lr"], calls.calls)
    assert st["n_updates"] == UPDATES and st["kl_stopped"] is False and len(st["lr_checks"]) == UPDATES - 1
    assert st["lr_checks"] == [LR / 1.5, LR / 1.5 / 1.5, 4e-4, 4e-4, 4e-4] and len(set(st["lr_checks"])) >= 3
    assert all(k > 2e-12 for k in st["kl_checks"])
    assert st["lr"] == 4e-4 == a.optimizer.param_groups[0]["lr"]             # (the end-of-learn() measurement holds the bound too)
    assert calls.total(CTL_ADAM) == UPDATES and calls.calls["tg_kl_control"] == UPDATES         # five checks + the end of learn()
    plain = _make(tg, algo_name, shape, pol0, UPDATES)
    _hand_set_lr(plain, [LR] + st["lr_checks"])
    plain.learn(buf)
    _assert_same(snap, _snapshot(plain), (algo_name, shape))


# ------------------------------------------------------------------------------------------------------------------------------
# 5. combinations
# ------------------------------------------------------------------------------------------------------------------------------
def _stop_against_truncation(tg, dev, algo_name, shape, pol_kw=None, expect=None, **kw):
    """The learner with a target_kl that never fires gives the kl behind every step; a target_kl between two of them stops the same
    learner there, and it equals the learner that was given that many updates."""
    pol0, buf = _base(tg, dev, algo_name, shape, **(pol_kw or {}))
    probe = _make(tg, algo_name, shape, pol0, UPDATES, target_kl=1e30, **kw)
    probe.learn(buf)
    kls = probe.last_stats["kl_checks"]
    j, target = _pick(kls)
    print(algo_name, shape, kw.keys(), "kl", kls, "stop at", j, "target_kl", target)
    assert 2 <= j < UPDATES
    a = _make(tg, algo_name, shape, pol0, UPDATES, target_kl=target, **kw)
    calls = _learn_counted(tg, a, buf)
    snap = _snapshot(a)
    assert snap["stats"]["n_updates"] == j and snap["stats"]["kl_stopped"] is True and snap["stats"]["kl_checks"] == kls[:j]
    short = _make(tg, algo_name, shape, pol0, j, **kw)
    short.learn(buf)
    _assert_same(snap, _snapshot(short), (algo_name, shape, tuple(kw)))
    if expect is not None:
        expect(calls, snap, j)
    return snap, j


def test_stop_with_max_grad_norm(tg, dev):
    def expect(calls, snap, j):
        assert calls.total(["tg_adam_step_ctl_clip", "tg_adam_step_push_ctl_clip"]) == calls.total(CTL_ADAM) > j
        assert len(snap["stats"]["grad_norm"]) == j
    _stop_against_truncation(tg, dev, "GRPO", "f32_chain_h64", max_grad_norm=0.05, expect=expect)


def test_stop_with_a_learned_std(tg, dev):
    def expect(calls, snap, j):
        assert calls.total(CTL_ADAM) > j and len(snap["stats"]["entropy"]) == j and len(snap["stats"]["log_std"]) == 4
    _stop_against_truncation(tg, dev, "PPO", "f32_chain_quadpole", pol_kw={"learn_std": True}, expect=expect)


def test_stop_with_adamw_waits_for_every_check(tg, dev):
    """An optimizer the fused step does not take: the host reads each check before the next step and does not take a step behind a
    latch -- no `_ctl` launch at all, and nothing to reconcile."""
    def expect(calls, snap, j):
        assert calls.total(CTL_ADAM) == 0 and calls.calls["tg_kl_control"] == j
    opt = lambda params: torch.optim.AdamW(params, lr=LR, weight_decay=0.01)
    _stop_against_truncation(tg, dev, "PPO", "f32_chain_h64", opt=opt, expect=expect)


def test_per_update_adaptation_with_adamw_writes_the_lr_at_every_check(tg, dev):
    pol0, buf = _base(tg, dev, "GRPO", "f32_chain_h64")
    opt = lambda params: torch.optim.AdamW(params, lr=LR, weight_decay=0.01)
    a = _make(tg, "GRPO", "f32_chain_h64", pol0, UPDATES, opt=opt, desired_kl=1e-12, kl_every=1, lr_bounds=(4e-4, 1e-2))
    a.learn(buf)
    snap = _snapshot(a)
    assert snap["stats"]["lr_checks"] == [LR / 1.5, LR / 1.5 / 1.5, 4e-4, 4e-4, 4e-4] and snap["stats"]["lr"] == 4e-4
    plain = _make(tg, "GRPO", "f32_chain_h64", pol0, UPDATES, opt=opt)
    _hand_set_lr(plain, [LR] + snap["stats"]["lr_checks"])
    plain.learn(buf)
    _assert_same(snap, _snapshot(plain), "adamw adapt")


def test_minibatch_stop_with_and_without_the_host_break(tg, dev):
    """PPO's minibatch mode: a check behind every minibatch step; the stop falls inside an update, and the learner that never breaks
    on the host (every later launch gated on the device) equals the one that follows one check behind."""
    pol0, buf = _base(tg, dev, "PPO", "f32_chain_h64")
    probe = _make(tg, "PPO", "f32_chain_h64", pol0, 2, target_kl=1e30, batch_size=128, seed=5)
    probe.learn(buf)
    kls = probe.last_stats["kl_checks"]
    j, target = _pick(kls, first=3)
    n_steps = probe.last_stats["n_updates"]
    print("minibatch kl", kls, "stop at", j, "of", n_steps)
    assert 3 <= j < n_steps - 1
    snaps = {}
    for lag in (None, 1):
        a = _make(tg, "PPO", "f32_chain_h64", pol0, 2, target_kl=target, batch_size=128, seed=5)
        calls = _learn_counted(tg, a, buf, lag)
        snaps[lag] = _snapshot(a)
        st = snaps[lag]["stats"]
        assert st["n_updates"] == j and st["kl_stopped"] is True and st["kl_checks"] == kls[:j] and len(st["actor_loss"]) == j
        assert calls.total(CTL_ADAM) == (n_steps if lag is None else j + 1)
    _assert_same(snaps[None], snaps[1], "minibatch")


# ------------------------------------------------------------------------------------------------------------------------------
# 6. two ranks
# ------------------------------------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_ranks_stop_at_the_same_update(tmp_path):
    """tests/kl_stop_dist_worker.py as fresh child processes, each under its own `timeout` (gloo, both ranks on cuda:0, half the groups
    each): both ranks report the same n_updates and hold the same bits; the stop falls where the one-rank run's does, and the weights
    equal the one-rank run's to the 1e-6 (relative L2) that tests/test_grad_clip_gpu.py holds the same comparison to."""
    worker = os.path.join(HERE, "kl_stop_dist_worker.py")
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
        print(case, "one rank", rec["n_updates"], rec["kl_checks"], "two ranks", a["n_updates"], a["kl_checks"])
        assert a["n_updates"] == b["n_updates"] == rec["n_updates"] and a["kl_stopped"] and b["kl_stopped"] and rec["kl_stopped"]
        assert 2 <= rec["n_updates"] < rec["updates"]
        assert a["kl_bits"] == b["kl_bits"] and a["steps"] == b["steps"] == rec["steps"]
        assert all(torch.equal(x, y) for x, y in zip(a["weights"], b["weights"]))
        for x, y in zip(a["weights"], rec["weights"]):
            assert float((x.double() - y.double()).norm()) <= 1e-6 * float(y.double().norm()), case


# ------------------------------------------------------------------------------------------------------------------------------
# 7. flag off
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo_name", ["PPO", "GRPO"])
def test_without_the_keywords_no_new_entry_point_is_called(tg, dev, algo_name):
    pol0, buf = _base(tg, dev, algo_name, "f32_chain_h64")
    for kw in ({}, {"kl_stats": True}, {"desired_kl": 0.01}, {"max_grad_norm": 0.5}):
        a = _make(tg, algo_name, "f32_chain_h64", pol0, 3, **kw)
        calls = _learn_counted(tg, a, buf)
        _ = a.last_stats
        assert calls.total() == 0 and a._kl_run is None and not a._kl_rows, (kw, calls.calls)
        assert not {"n_updates", "kl_stopped", "kl_checks", "lr_checks"} & set(a.last_stats)
    on = _make(tg, algo_name, "f32_chain_h64", pol0, 3, target_kl=1e30)
    calls = _learn_counted(tg, on, buf)
    assert calls.total(CTL_ADAM) == 3 and calls.calls["tg_kl_control"] == 2
