"""The learned per-dimension log-std on the GPU: one PPO / GRPO learn() per head family against the fp64 yardstick
(tests/learned_std_fp64.py) run on the same trajectory and pre-update weights.

Tolerance (set by the issue, not tuned): the distance of torch's own float32 autograd of the same step (bf16 nets: under bf16
autocast) from the fp64 yardstick, times 4 -- floored at 4 x 2^-23 x |reference| (learned_std_fp64.bar), an addition of this module:
torch's own error can be one rounding or exactly zero, and that floor is what decides every post-step log_std check.  Every
test prints the measured error of the native path, of torch's float32 run, and the resulting bar.

Measured on an MI355X (max |error| of log_std's gradient against fp64: native / torch float32 / bar):
  PPO   f32 chain ReLU 3.2e-9 / 4.9e-8 / 2.0e-7    Tanh 1.2e-9 / 1.2e-9 / 5.0e-8     wide 3.0e-9 / 1.8e-7 / 7.3e-7
        resident 2.3e-9 / 5.2e-9 / 5.1e-8          bf16 chain 3.6e-5 / 3.5e-5 / 1.4e-4   per-layer 1.6e-9 / 1.7e-8 / 6.6e-8
  GRPO  resident 7.3e-7 / 1.3e-5 / 5.2e-5 (ref: 1.4e-7 / 7.3e-6 / 2.9e-5)   f32 chain 2.9e-7 / 1.5e-5 / 5.9e-5 (ref: 4.5e-7 / 1.4e-5 / 5.7e-5)
        bf16 chain 9.2e-3 / 7.4e-3 / 3.0e-2 (ref: 9.0e-3 / 7.8e-3 / 3.1e-2; |g| ~ 26)   per-layer 5.2e-7 / 3.1e-6 / 1.2e-5
  post-step log_std: 9.8e-9 native and torch alike (the float32 rounding of the value), bar 1.7e-7 .. 2.9e-7 (the floor);
  entropy on - off: -0.01 to within 2.1e-9 on every head."""
import copy
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import learned_std_fp64 as Y
import philox_fp64 as P
from test_rng_fp64_gpu import U, eps_bound

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
LR = 3e-4

# name -> (env, S, A, hidden, activation, compute dtype, G, E, T, the `_std` entry point the actor's update must take)
CASES = {
    "f32_chain_relu": ("CartPole", 5, 1, (128,) * 3, "ReLU", None, 4, 16, 32, "tg_mlp_f32_forward_backward_act_std"),
    "f32_chain_tanh": ("CartPole", 5, 1, (128,) * 3, "Tanh", None, 4, 16, 32, "tg_mlp_f32_forward_backward_act_std"),
    "f32_wide": ("QuadPole", 20, 4, (256, 256), "ReLU", None, 3, 11, 24, "tg_mlp_f32w_forward_backward_std"),
    "f32_resident": ("CartPole", 5, 1, (128, 128), "ReLU", None, 4, 16, 32, "tg_mlp_f32r_forward_backward_std"),
    "bf16_chain": ("QuadPole", 20, 4, (256,) * 3, "ReLU", torch.bfloat16, 3, 11, 24, "tg_mlp_forward_chain_loss_std"),
    "per_layer": ("CartPole", 5, 1, (32, 32), "Sigmoid", None, 4, 16, 32, "tg_surrogate_loss_std"),
}


@pytest.fixture(scope="module")
def tg():
    import trajopt_grpo_amd as tg
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return tg


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


STD_ENTRIES = ["tg_surrogate_loss_std", "tg_mlp_forward_chain_loss_std", "tg_mlp_f32_forward_backward_act_std",
               "tg_mlp_f32w_forward_backward_std", "tg_mlp_f32r_forward_backward_std", "tg_log_std_grad"]


@pytest.fixture
def std_calls(tg, monkeypatch):
    """{entry point: calls} of the `_std` entries and tg_log_std_grad, counted by wrapping the loaded library's attributes for the
    duration of one test (the binding itself keeps no log)."""
    lib, calls = tg._native.load(), {}

    def wrap(name, fn):
        def counted(*args):
            calls[name] = calls.get(name, 0) + 1
            return fn(*args)
        return counted
    for name in STD_ENTRIES:
        monkeypatch.setattr(lib, name, wrap(name, getattr(lib, name)))
    return calls


_SETUPS = {}


def _setup(tg, dev, case, critic, learn_std=True):
    """(policy, buffer) of one case, rolled out once per module: every test deep-copies the policy."""
    key = (case, critic, learn_std)
    if key not in _SETUPS:
        env_name, S, A, hidden, act, cdt, G, E, T, _ = CASES[case]
        torch.manual_seed(7)
        cls = tg.GaussianActorCritic_NeuralNetwork if critic else tg.GaussianActor_NeuralNetwork
        pol = cls(S, A, hidden, activation=act, cov=[0.5, 0.3, 0.4, 0.6][:A], device=dev, **({"learn_std": True} if learn_std else {}))
        env_cls = getattr(tg, env_name)
        mgr = tg.RolloutManager(lambda: env_cls(max_steps=T), pol, num_workers=G, num_episodes_per_worker=E, seed=19,
                                **({"compute_dtype": cdt} if cdt is not None else {}))
        buf = tg.Rollout_Buffer(mgr)
        buf.sample()
        _SETUPS[key] = (pol, buf)
    return _SETUPS[key]


def _traj(buf):
    return tuple(t.detach().cpu() for t in (buf.group_observations, buf.group_actions, buf.group_rewards, buf.group_masks))


def _sd(net):
    return {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}


def _ppo(tg, pol, case, **kw):
    cdt = CASES[case][5]
    args = dict(epsilon=0.2, policy=pol, optimizer=torch.optim.Adam(pol.parameters(), lr=LR), ref_model=None, updates_per_iter=1,
                gamma=0.99, batch_size=None, autocast_dtype=cdt)
    args.update(kw)
    return tg.PPO(**args)


def _check(what, got, ref64, ref32):
    bar, err32 = Y.bar(ref64, ref32)
    err = float((got.detach().double().cpu() - ref64).abs().max())
    print(f"{what}: native err {err:.3e}  torch-fp32 err {err32:.3e}  bar {bar:.3e}  ref {ref64.tolist()}")
    assert err <= bar, (what, err, bar)


def _yardsticks(fn, *args, case, **kw):
    act, cdt = CASES[case][4], CASES[case][5]
    r64 = fn(*args, activation=act, dtype=torch.float64, **kw)
    r32 = fn(*args, activation=act, dtype=torch.float32, autocast=cdt is not None, **kw)
    return r64, r32


@pytest.mark.parametrize("case", list(CASES))
def test_ppo_one_update_matches_the_yardstick_and_the_entropy_bonus_is_real(tg, dev, case, std_calls):
    base, buf = _setup(tg, dev, case, critic=True)
    traj = _traj(buf)
    grads = {}
    for ent in (0.0, 0.01):
        pol = copy.deepcopy(base)
        ls0 = pol.log_std.detach().clone()
        sd_a, sd_c = _sd(pol.actor), _sd(pol.critic)
        std_calls.clear()
        algo = _ppo(tg, pol, case, entropy=ent)
        algo.learn(buf)
        torch.cuda.synchronize()
        assert std_calls == {CASES[case][9]: 1, "tg_log_std_grad": 1}, std_calls
        r64, r32 = _yardsticks(Y.ppo_steps, sd_a, sd_c, ls0, *traj, case=case, entropy=ent, lr=LR)
        _check(f"{case} entropy={ent} grad", pol.log_std.grad, r64["grad"][0], r32["grad"][0])
        _check(f"{case} entropy={ent} log_std", pol.log_std, r64["log_std"][0], r32["log_std"][0])
        grads[ent] = pol.log_std.grad.detach().double().cpu()
        st = algo.last_stats
        assert isinstance(st["entropy"], list) and len(st["entropy"]) == 1 and abs(st["entropy"][0] - r64["entropy"][0]) < 1e-5
        assert torch.allclose(torch.tensor(st["log_std"]), pol.log_std.detach().cpu())
    # -entropy * mean(H) adds exactly -entropy to every component: two float32 roundings of a gradient of size |g|
    diff = grads[0.01] - grads[0.0]
    tol = 2.0 ** -22 * max(1.0, float(grads[0.0].abs().max()))
    print(case, "entropy difference", diff.tolist(), "tol", tol)
    assert float((diff + 0.01).abs().max()) <= tol


@pytest.mark.parametrize("with_ref", [False, True])
@pytest.mark.parametrize("case", ["f32_resident", "f32_chain_relu", "bf16_chain", "per_layer"])
def test_grpo_one_update_matches_the_yardstick(tg, dev, case, with_ref, std_calls):
    env_name, S, A, hidden, act, cdt, G, E, T, entry = CASES[case]
    base, buf = _setup(tg, dev, case, critic=False)
    traj = _traj(buf)
    pol = copy.deepcopy(base)
    ls0, sd_a = pol.log_std.detach().clone(), _sd(pol.actor)
    ref = None
    if with_ref:
        torch.manual_seed(23)
        ref = tg.GaussianActor_NeuralNetwork(S, A, hidden, activation=act, cov=0.45, device=dev)
        with torch.no_grad():                                   # close to the policy: D stays small
            for p, q in zip(ref.actor.parameters(), pol.actor.parameters()):
                p.copy_(q + 0.01 * torch.randn_like(q))
    beta = 0.04 if with_ref else 0.0
    std_calls.clear()
    algo = tg.GRPO(epsilon=0.2, beta=beta, gamma=0.99, policy=pol, optimizer=torch.optim.Adam(pol.parameters(), lr=LR), ref_model=ref,
                   updates_per_iter=1, autocast_dtype=cdt)
    algo.learn(buf)
    torch.cuda.synchronize()
    assert std_calls == {entry: 1, "tg_log_std_grad": 1}, std_calls
    kw = dict(beta=beta, ref_sd=_sd(ref.actor), ref_var=ref.var, ref_activation=act) if with_ref else {}
    r64, r32 = _yardsticks(Y.grpo_steps, sd_a, ls0, *traj, case=case, lr=LR, **kw)
    _check(f"grpo {case} ref={with_ref} grad", pol.log_std.grad, r64["grad"][0], r32["grad"][0])
    _check(f"grpo {case} ref={with_ref} log_std", pol.log_std, r64["log_std"][0], r32["log_std"][0])
    assert torch.equal(algo.old_policy.log_std.detach(), pol.log_std.detach())
    assert "log_std" in algo.last_stats


def test_ppo_minibatch_mode_matches_the_yardstick(tg, dev):
    case = "f32_chain_relu"
    base, buf = _setup(tg, dev, case, critic=True)
    pol = copy.deepcopy(base)
    ls0, sd_a, sd_c = pol.log_std.detach().clone(), _sd(pol.actor), _sd(pol.critic)
    n = int(buf.group_masks.sum())
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(n))
    algo = _ppo(tg, pol, case, batch_size=700, entropy=0.01)
    algo.permutation_fn = lambda rows, device: perm.to(device)
    algo.learn(buf)
    torch.cuda.synchronize()
    batches = [perm[lo:lo + 700] for lo in range(0, n, 700)]
    r64, r32 = _yardsticks(Y.ppo_steps, sd_a, sd_c, ls0, *_traj(buf), case=case, entropy=0.01, lr=LR, batches=batches)
    _check("minibatch last grad", pol.log_std.grad, r64["grad"][-1], r32["grad"][-1])
    _check("minibatch log_std", pol.log_std, r64["log_std"][-1], r32["log_std"][-1])
    assert len(algo.last_stats["entropy"]) == len(batches)


def test_max_grad_norm_includes_the_log_std_gradient(tg, dev):
    case = "f32_chain_relu"
    base, buf = _setup(tg, dev, case, critic=True)
    pol = copy.deepcopy(base)
    ls0, sd_a, sd_c = pol.log_std.detach().clone(), _sd(pol.actor), _sd(pol.critic)
    probe = Y.ppo_steps(sd_a, sd_c, ls0, *_traj(buf), entropy=0.01, lr=LR)
    max_norm = probe["norm"][0] / 4.0
    algo = _ppo(tg, pol, case, entropy=0.01, max_grad_norm=max_norm)
    algo.learn(buf)
    torch.cuda.synchronize()
    r64, r32 = _yardsticks(Y.ppo_steps, sd_a, sd_c, ls0, *_traj(buf), case=case, entropy=0.01, lr=LR, max_grad_norm=max_norm)
    norm = algo.last_stats["grad_norm"][0]
    bar, err32 = Y.bar(torch.tensor([r64["norm"][0]]), torch.tensor([r32["norm"][0]]))
    print("norm", norm, r64["norm"][0], "bar", bar)
    assert abs(norm - r64["norm"][0]) <= bar
    # the norm WITHOUT log_std's component is measurably smaller: the component is in
    without = (r64["norm"][0] ** 2 - float((r64["grad"][0] ** 2).sum())) ** 0.5
    assert abs(norm - without) > 10 * bar, "the test's shape must make log_std's share of the norm visible"
    _check("clipped log_std", pol.log_std, r64["log_std"][0], r32["log_std"][0])


def test_three_updates_move_log_std_at_every_step_without_a_host_read(tg, dev, monkeypatch):
    """Two proxies for "no update reads log_std on the host".  (a) Every host view of it goes through policy.cov; learn() may read it at
    its entry (once per policy object it scores with), never once per update.  (b) torch's sync debug mode ("warn") reports every
    synchronizing torch call (.item(), .tolist(), a blocking copy to the host ...): learn() has a few at its entry (the row count, the
    covariance) and the fused optimizer step builds its tables with blocking uploads during its first two steps; the learned std may
    add none per update: (a) is the same with three updates as with one, and (b) is the same with five updates as with three (past
    the optimizer's set-up: 15 and 15 when this was written, 7 with one update) -- no update synchronizes with the host at all.
    The per-step entropies recorded on the device differ from step to step: log_std moved at every step."""
    import warnings
    case = "f32_chain_relu"
    base, buf = _setup(tg, dev, case, critic=True)
    P = tg.policies._GaussianBase
    reads = [0]
    orig = P.cov.fget
    monkeypatch.setattr(P, "cov", property(lambda self: (reads.__setitem__(0, reads[0] + 1), orig(self))[1], P.cov.fset))
    counts = {}
    for updates in (1, 5, 3):
        pol = copy.deepcopy(base)
        ls0, sd_a, sd_c = pol.log_std.detach().clone(), _sd(pol.actor), _sd(pol.critic)
        algo = _ppo(tg, pol, case, entropy=0.01, updates_per_iter=updates)
        reads[0] = 0
        torch.cuda.synchronize()
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            torch.cuda.set_sync_debug_mode("warn")
            try:
                algo.learn(buf)
            finally:
                torch.cuda.set_sync_debug_mode("default")
        sync = [w for w in seen if "synchroniz" in str(w.message).lower()]
        counts[updates] = (reads[0], len(sync))
        if updates == 3:
            print("synchronizing calls at", sorted({f"{os.path.basename(w.filename)}:{w.lineno}" for w in sync}))
        torch.cuda.synchronize()
    print("host reads of cov / synchronizing torch calls per learn():", counts)
    assert counts[3][0] == counts[1][0], counts
    assert counts[5][1] == counts[3][1], counts
    ent = algo.last_stats["entropy"]
    assert len(ent) == 3 and ent[0] != ent[1] != ent[2]
    r64, r32 = _yardsticks(Y.ppo_steps, sd_a, sd_c, ls0, *_traj(buf), case=case, entropy=0.01, lr=LR, updates=3)
    for i in range(3):
        assert abs(ent[i] - r64["entropy"][i]) < 1e-5
    _check("three updates log_std", pol.log_std, r64["log_std"][-1], r32["log_std"][-1])
    _check("three updates last grad", pol.log_std.grad, r64["grad"][-1], r32["grad"][-1])


@pytest.mark.parametrize("case", ["f32_chain_relu", "bf16_chain"])
def test_a_fixed_covariance_learner_touches_no_new_entry_point(tg, dev, case, std_calls):
    """learn_std=False: the launches of the parent commit -- none of the `_std` entries, no tg_log_std_grad -- and two runs from the
    same weights give the same bits."""
    base, buf = _setup(tg, dev, case, critic=True, learn_std=False)
    out = []
    for _ in range(2):
        pol = copy.deepcopy(base)
        algo = _ppo(tg, pol, case, updates_per_iter=2)
        algo.learn(buf)
        torch.cuda.synchronize()
        out.append([p.detach().clone() for p in pol.parameters()])
        assert isinstance(algo.last_stats["entropy"], float) and "log_std" not in algo.last_stats
    assert std_calls == {}, std_calls
    assert all(torch.equal(a, b) for a, b in zip(*out))
    assert not any(torch.equal(a, b) for a, b in zip(out[0], base.parameters()))


@pytest.mark.parametrize("rows", [1, 255, 2049, (1 << 20) + 3])
def test_log_std_grad_reduction_against_float64(tg, dev, rows):
    """tg_log_std_grad: fp64 column sums, added into the window with `add`, twice the same bits.  |error| <= one float32 rounding of
    the result plus the float64 accumulation error (rows 2^-53 of the sum of magnitudes)."""
    from trajopt_grpo_amd import hip_ops as K
    g = torch.Generator(device=dev).manual_seed(rows)
    x = torch.randn(rows, 4, device=dev, generator=g)
    for A in (1, 3, 4):
        start = torch.tensor([0.5, -1.0, 2.0, 0.25], device=dev)[:A].contiguous()
        a, b = start.clone(), start.clone()
        K.log_std_grad(x, A, a, add=-0.01)
        K.log_std_grad(x, A, b, add=-0.01)
        want = start.double().cpu() + x[:, :A].double().sum(0).cpu() + float(torch.tensor(-0.01, dtype=torch.float32))
        assert torch.equal(a, b)
        tol = 2.0 ** -24 * want.abs() + rows * 2.0 ** -53 * x[:, :A].double().abs().sum(0).cpu()
        assert bool(((a.double().cpu() - want).abs() <= tol).all()), (rows, A, a.tolist(), want.tolist())


# --------------------------------------------------------------------------------------------------------------------------------
# the next rollout samples with the moved log_std
# --------------------------------------------------------------------------------------------------------------------------------
ROLLOUT_PATHS = {"fused_bf16": dict(hidden=(128, 128), kw=dict(compute_dtype=torch.bfloat16, fused=True), cdt=torch.bfloat16),
                 "fused_f32": dict(hidden=(64, 64), kw=dict(fused=True), cdt=None),
                 "per_step": dict(hidden=(64, 64), kw=dict(fused=False), cdt=None)}


@pytest.mark.parametrize("path", list(ROLLOUT_PATHS))
def test_the_next_rollout_samples_with_the_moved_log_std(tg, dev, path):
    """learn() (eight updates at a large learning rate) moves every log_std component by more than 0.01 (1 % of sigma: 1e4 times
    the bound below); the actor's weights are then
    zeroed in place (mean exactly 0 on every path), so the actions of the NEXT rollout are exp(log_std) * eps: eps from the fp64
    Philox / Box-Muller replay of stream 1 (tests/philox_fp64.py) within test_rng_fp64_gpu's bound times sigma, plus 8 float32
    roundings of the product (exp and sqrt of the host's sigma, the cast, the multiply).  A sigma left at its value before the
    learn() is off by > 1 % of |eps| and fails.  per_step: the engine would replay a hipGraph for a fixed covariance
    (use_graph on by default there); with a learned std it must not capture one."""
    c = ROLLOUT_PATHS[path]
    S, A, G, E, T, seed = 20, 4, 3, 37, 12, 91
    torch.manual_seed(5)
    pol = tg.GaussianActor_NeuralNetwork(S, A, c["hidden"], cov=[0.5, 0.3, 0.4, 0.6], device=dev, learn_std=True)
    mgr = tg.RolloutManager(lambda: tg.QuadPole(max_steps=T), pol, num_workers=G, num_episodes_per_worker=E, seed=seed, **c["kw"])
    buf = tg.Rollout_Buffer(mgr)
    buf.sample()
    eng = mgr.engine
    assert eng.fused == (path != "per_step") and (path != "per_step" or eng.use_graph)
    ls0 = pol.log_std.detach().clone()
    algo = tg.GRPO(epsilon=0.2, beta=0.0, gamma=0.99, policy=pol, optimizer=torch.optim.Adam(pol.parameters(), lr=0.05),
                   updates_per_iter=8, autocast_dtype=c["cdt"])
    algo.learn(buf)
    with torch.no_grad():
        for p in pol.actor.parameters():
            p.zero_()
    moved = (pol.log_std.detach() - ls0).abs().cpu()
    print(path, "log_std", ls0.tolist(), "->", pol.log_std.tolist())
    assert bool((moved > 0.01).all()), moved
    buf.sample()                                                          # rollout 1 of this engine: stream 1
    torch.cuda.synchronize()
    assert eng._graph is None, "a learned-std policy must take the plain per-step launches, not a captured graph"
    tr = eng.traj
    got = tr.act.double().cpu().numpy()
    mask = tr.mask.bool().cpu().numpy()
    eps, ur, ut, is_sin = P.sample_eps(seed, 1, np.arange(eng.n), T, A)
    sigma = np.exp(pol.log_std.detach().double().cpu().numpy())[:, None, None]
    want = sigma * eps
    m = np.broadcast_to(mask, got.shape)
    assert bool(mask[0].all()) and not got[~m].any()
    err = np.abs(got - want)[m]
    bound = (sigma * eps_bound(eps, ur, ut, is_sin) + 8 * U * np.abs(want))[m]
    stale = np.abs(np.exp(ls0.double().cpu().numpy())[:, None, None] * eps - want)[m]
    print(path, "max |act - exp(log_std) eps|", err.max(), "max err / bound", (err / bound).max(), "a stale sigma would be off by up to", stale.max())
    assert (err <= bound).all(), (path, float(err.max()), float((err / bound).max()))
    assert float(np.median(stale / bound)) > 100, "the check must be able to tell the old sigma from the new one"


# --------------------------------------------------------------------------------------------------------------------------------
# two ranks
# --------------------------------------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_ranks_reproduce_the_one_rank_run(tmp_path):
    """tests/learned_std_dist_worker.py as fresh child processes (the harness of test_distributed_gpu.py / test_bootstrap_gpu.py: gloo,
    both ranks on cuda:0, half the groups each).  The ranks' trajectories are the one-rank run's, bit for bit; weights and log_std
    after one learn() reproduce the one-rank run at that harness's bar (1e-6 in relative L2); both ranks end with the same bits;
    the entropy bonus entered once, not once per rank: log_std's all-reduced gradient agrees with the one-rank gradient to 1e-6 max(1, |g|)
    (each rank's float64 sum is rounded to float32 once, 6e-8 of its size, before the all-reduce) -- one more -entropy (0.01) would
    be 1e4 times that."""
    worker = os.path.join(HERE, "learned_std_dist_worker.py")
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
        assert torch.equal(torch.cat([a["actions"], b["actions"]], 0), rec["actions"]), case
        assert all(torch.equal(x, y) for x, y in zip(a["weights"], b["weights"])) and torch.equal(a["log_std"], b["log_std"])
        assert torch.equal(a["grad"], b["grad"])
        for x, y in zip(a["weights"], rec["weights"]):
            assert float((x.double() - y.double()).norm()) <= 1e-6 * float(y.double().norm()), case
        g1, g2 = rec["grad"].double(), a["grad"].double()
        print(case, "log_std", rec["log_std0"].tolist(), "->", rec["log_std"].tolist(), "two ranks", a["log_std"].tolist(),
              "grad", g1.tolist(), g2.tolist())
        assert not torch.equal(rec["log_std"], rec["log_std0"])
        assert float((a["log_std"].double() - rec["log_std"].double()).norm()) <= 1e-6 * float(rec["log_std"].double().norm()), case
        assert float((g2 - g1).norm()) <= 1e-6 * max(1.0, float(g1.norm())), case
        assert a["stats_log_std"] == a["log_std"].tolist()
