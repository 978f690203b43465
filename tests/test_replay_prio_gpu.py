"""DeviceReplayBuffer(prioritized=True) on the MI355X (run with `-m gpu`): the sum tree of csrc/replay_prio.hip against
tests/replay_prio_ref.py.  After every add() and update_priorities() every level read back from the device equals the restatement's
sums of the device's own leaves bit for bit (and tg_replay_prio_rebuild's); the sampled indices equal the restatement's descent on the
read-back tree exactly; every sampled row is the storage row its index names; the normalised weights are raw / raw.max() bit for bit.

Only the two pow() results are held by a bound: new leaves and raw weights against float64, bar = 4 x the largest relative error of
torch's own float32 torch.pow on the same device inputs, floored at 4 x 2^-24 (the convention of tests/test_learned_std_gpu.py); both
figures are printed.  Measured on an MI355X (profiles/r22_replay_prio_probe.md): leaves native 4.9e-8 .. 5.7e-8, torch 8.4e-8 .. 1.2e-7,
bar 3.3e-7 .. 4.8e-7; weights native <= 4.6e-8, torch <= 4.6e-8, bar 2.4e-7 (the floor)."""
import numpy as np
import pytest
import torch

import replay_prio_ref as PR
import replay_ref as RR
from test_replay_gpu import assert_same, bits, check_batch, dev, fill, push_random, random_inputs, tg, to_dev  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu
ENTRIES = ("tg_replay_start", "tg_replay_push", "tg_replay_sample", "tg_replay_prio_push", "tg_replay_prio_update",
           "tg_replay_prio_sample", "tg_replay_prio_rebuild")
# (n, K, n_step, S, A): K n = 1, 64, 70 (slots straddle a node), 4096 (one full level), 130 x 33, 262,145 (four levels above the leaves)
SIZES = [(1, 1, 1, 5, 1), (16, 4, 2, 5, 1), (10, 7, 3, 10, 2), (64, 64, 3, 20, 4), (130, 33, 2, 5, 1), (4033, 65, 2, 3, 1)]


@pytest.fixture
def calls(tg, monkeypatch):
    """{entry point: calls}, counted by wrapping the loaded library's attributes for one test."""
    lib, seen = tg._native.load(), {}
    for name in ENTRIES:
        monkeypatch.setattr(lib, name, (lambda name, fn: lambda *a: (seen.__setitem__(name, seen.get(name, 0) + 1), fn(*a))[1])(name, getattr(lib, name)))
    return seen


def check_tree(buf, where, rebuild=False):
    """-> the device's levels, equal to the restatement's sums of the device's own leaves (and to a rebuild of them)."""
    def read():
        flat = buf._tree.cpu().numpy()
        return [flat[off:off + -(-size // 64) * 64] for off, size in buf.tree_levels]
    tree = read()
    assert buf.tree_levels == PR.levels(buf.capacity)[0]
    for l, (got, want) in enumerate(zip(tree, PR.build(tree[0][:buf.capacity]))):
        assert np.array_equal(bits(got), bits(want)), f"level {l} differs {where}"
    if rebuild:
        buf._tree[buf.capacity:].zero_()                                    # every level above the leaves forgotten
        buf.rebuild_tree()
        assert all(np.array_equal(bits(got), bits(want)) for got, want in zip(read(), tree)), f"the rebuild differs {where}"
    return tree


def within_pow_bar(got, base64, exponent, what):
    """got (device float32) against base64 ** exponent: at most 4 x torch's own float32 error on the same inputs, floored at 4 x 2^-24."""
    want = base64 ** exponent
    own = float(((torch.pow(base64.float(), float(exponent)).double() - want).abs() / want).max())
    err = float(((got.double() - want).abs() / want).max())
    print(f"{what}: native max rel err {err:.3e}, torch float32 pow {own:.3e}, bar {4 * max(own, 2.0 ** -24):.3e}")
    assert err <= 4 * max(own, 2.0 ** -24), (what, err, own)


def update_and_check(buf, rng, dev, where):
    """One update_priorities() with duplicates, indices outside the stored rows and non-finite errors."""
    R, cap, B = len(buf), buf.capacity, 97
    before, top = buf.priorities.cpu().numpy().copy(), bits(buf._max_priority)[0]
    idx = rng.integers(0, R, B)
    idx[:8] = idx[8:16]                                                     # duplicates
    idx[20:26] = [-1, R, cap, 2 ** 40, -2 ** 40, cap + 63]
    td = (rng.standard_normal(B) * 10.0 ** rng.uniform(-3, 2, B)).astype(np.float32)
    td[30:34] = [np.nan, np.inf, -np.inf, 0.0]
    idx_d, td_d = to_dev(dev, idx.astype(np.int64), td)
    buf.update_priorities(idx_d, td_d)
    used = (idx >= 0) & (idx < R) & np.isfinite(td)
    after = buf.priorities.cpu().numpy()
    # every named leaf holds one of its candidates to the bar, and none of its candidates is larger: the largest won
    u_idx, u_td = idx_d[torch.from_numpy(used).to(dev)], td_d[torch.from_numpy(used).to(dev)]
    cand = (u_td.double().abs() + buf.priority_eps) ** buf.alpha
    best = torch.zeros(cap, dtype=torch.float64, device=dev).scatter_reduce_(0, u_idx, cand, "amax")
    won = cand == best[u_idx]
    within_pow_bar(buf.priorities[u_idx[won]], u_td[won].double().abs() + buf.priority_eps, buf.alpha, f"leaves {where}")
    untouched = np.ones(cap, bool)
    untouched[idx[used]] = False
    assert np.array_equal(bits(after[untouched]), bits(before[untouched])), "an unnamed leaf changed"
    assert bits(buf._max_priority)[0] == max(top, bits(after[idx[used]]).max()), "the running maximum is not the largest priority so far"
    check_tree(buf, where + " after update", rebuild=True)


def sample_and_check(buf, where):
    tree = check_tree(buf, where)
    R, root = len(buf), np.float64(tree[-1][0])
    for B in (1, 64, 257):
        ordinal = buf._ordinal
        out = buf.sample(B)
        assert len(out) == 7 and out[6].shape == (B,) and out[6].dtype == torch.float32
        idx = out[5].cpu().numpy()
        assert np.array_equal(idx, PR.descend(tree, buf.seed, ordinal, B)), f"B={B}: not the restatement's descent {where}"
        assert idx.min() >= 0 and idx.max() < R and (tree[0][idx] > 0).all(), "an unfilled or zero-priority row was drawn"
        for got, store in zip(out[:5], (buf.obs, buf.act, buf.rew, buf.next_obs, buf.disc)):
            assert np.array_equal(bits(got), bits(store[out[5]])), "a sampled row is not the storage row its index names"
        base = torch.from_numpy(R * tree[0][idx].astype(np.float64) / root).to(buf.device)
        within_pow_bar(buf.raw_weight, base, -buf.beta, f"weights B={B} {where}")
        raw = buf.raw_weight.cpu().numpy()
        assert np.array_equal(bits(out[6]), bits(raw / raw.max())), "weight is not raw / raw.max()"
    given = [0, R - 1, -1, R, 0]                                            # given rows: their weights; NaN outside the stored rows
    out = buf.sample(indices=torch.tensor(given, dtype=torch.int64, device=buf.device), beta=1.0)
    for k, row in enumerate(given):
        if 0 <= row < R and tree[0][row] > 0:
            assert abs(float(buf.raw_weight[k]) * R * np.float64(tree[0][row]) / root - 1) <= 4 * 2.0 ** -24
            assert bits(out[2])[k] == bits(buf.rew)[row]
        else:
            assert np.isnan(float(buf.raw_weight[k])) and np.isnan(float(out[6][k])) and bool(torch.isnan(out[0][k]).all())


@pytest.mark.parametrize("n, K, n_step, S, A", SIZES)
def test_tree_draws_and_weights_follow_the_restatement(tg, dev, calls, n, K, n_step, S, A):
    rng = np.random.default_rng(n + K)
    buf = tg.DeviceReplayBuffer(S, A, n, K, n_step=n_step, seed=0xBEEF0000 + n, device=dev, prioritized=True, alpha=0.6, beta=0.4)
    buf.start(*to_dev(dev, rng.standard_normal((n, S)).astype(np.float32)))
    pushes = 2 * K + 1 if K < 10 else K + 2                                  # the ring wraps
    stops = {0 if K < 10 else 1, K - 1, pushes - 1}                          # partly filled, full, wrapped
    for t in range(pushes):
        before = buf.priorities.cpu().numpy().copy()
        act, obs, rew, fin = random_inputs(rng, n, S, A)
        done = rng.random(n) < 0.25
        a, o, r, f, te, tr = to_dev(dev, act, obs, rew, fin, done & (rng.random(n) < 0.5), np.zeros(n, bool))
        buf.add(a, o, r, te, tr, {"final_obs": f})
        leaves = check_tree(buf, f"after push {t}")[0][:buf.capacity]
        slot = np.arange(buf.capacity) // n == t % K
        assert (bits(leaves[slot]) == bits(buf._max_priority)[0]).all(), "a new row did not enter with the running maximum"
        assert np.array_equal(bits(leaves[~slot]), bits(before[~slot])), "another slot's priorities changed"
        if t in stops:
            sample_and_check(buf, f"after push {t}")
            update_and_check(buf, rng, dev, f"after push {t}")
            sample_and_check(buf, f"after push {t} and an update")
    assert calls["tg_replay_prio_push"] == calls["tg_replay_push"] == pushes and "tg_replay_sample" not in calls
    buf.priorities.zero_()                                                  # an empty tree: nothing can be drawn
    buf.rebuild_tree()
    out = buf.sample(5)
    assert (out[5] == -1).all() and all(torch.isnan(t).all() for t in out[:5] + out[6:])
    buf.clear()
    assert float(buf._tree.abs().sum()) == 0 and float(buf._max_priority) == 1.0


def test_step_add_sample_update_replay_from_a_captured_graph(tg, dev):
    n, K, replays = 70, 4, 6
    made = []
    for _ in range(2):
        venv = tg.DeviceVecEnv(tg.CartPole(max_steps=8), n, seed=3, device=dev)
        buf = tg.DeviceReplayBuffer.for_env(venv, K, n_step=3, gamma=0.9, seed=5, prioritized=True)
        buf.start(venv.reset()[0])
        made.append((venv, buf))
    (venv_g, buf_g), (venv_e, buf_e) = made
    feed = (torch.rand(replays + 1, n, venv_g.A, generator=torch.Generator().manual_seed(9)) * 2 - 1).to(dev)
    actions = feed[0].clone()

    def one(venv, buf, act):
        buf.add(act, *venv.step(act))
        out = buf.sample(33)
        buf.update_priorities(out[5], out[2] * out[6] + out[0][:, 0])        # any elementwise function of the batch, on the device
        buf._ordinal = 0                                                     # the ordinal is by value: a graph repeats its stream
    for venv, buf in made:                                                   # one eager round each: nothing is first-called under capture
        one(venv, buf, actions)
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):                             # one stream, a linear chain
        one(venv_g, buf_g, actions)
    for k in range(replays):                                                 # several replays against the eager twin
        actions.copy_(feed[k + 1])
        graph.replay()
        one(venv_e, buf_e, feed[k + 1])
    torch.cuda.synchronize()
    assert_same(buf_g, buf_e, "graph against eager")
    for got, want in ((buf_g._tree, buf_e._tree), (buf_g._max_priority, buf_e._max_priority), (buf_g._out[7], buf_e._out[7]),
                      (buf_g._out[5], buf_e._out[5])):
        assert np.array_equal(bits(got), bits(want))
    assert len(np.unique(bits(buf_g.priorities))) > 2
    check_tree(buf_g, "after the replays")


def test_checkpoint_round_trip_carries_the_priorities(tg, dev):
    S, A, n, K = 10, 2, 70, 4
    buf = tg.DeviceReplayBuffer(S, A, n, K, n_step=3, seed=77, device=dev, prioritized=True)
    fill(buf, RR.ReplayRef(S, A, n, K, n_step=3, seed=77), dev, 6)
    update_and_check(buf, np.random.default_rng(3), dev, "before saving")
    sd = buf.state_dict()
    assert sd["priorities"].data_ptr() != buf.priorities.data_ptr() and "tree" not in sd
    twin = tg.DeviceReplayBuffer(S, A, n, K, n_step=3, seed=1, device=dev, prioritized=True)
    twin.load_state_dict(sd)
    assert np.array_equal(bits(twin._tree), bits(buf._tree)) and np.array_equal(bits(twin._max_priority), bits(buf._max_priority))
    for b in (buf, twin):
        push_random(b, RR.ReplayRef(S, A, n, K, n_step=3), dev, 2, np.random.default_rng(4))
    first, second = [t.clone() for t in buf.sample(64)], twin.sample(64)
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(first, second))
    with pytest.raises(ValueError, match="priorities"):
        twin.load_state_dict(tg.DeviceReplayBuffer(S, A, n, K, n_step=3, device=dev).state_dict())


def test_prioritized_false_is_the_uniform_path(tg, dev, calls):
    S, A, n, K = 5, 1, 70, 4
    buf = tg.DeviceReplayBuffer(S, A, n, K, n_step=3, seed=11, device=dev, prioritized=False)
    ref = RR.ReplayRef(S, A, n, K, n_step=3, seed=11)
    fill(buf, ref, dev, 6)
    assert_same(buf, ref, "after six pushes")
    out = buf.sample(63)
    assert len(out) == 6
    check_batch(out, ref.sample(63), buf)
    assert calls == {"tg_replay_start": 1, "tg_replay_push": 6, "tg_replay_sample": 1}
    assert set(buf.state_dict()) == set(tg.DeviceReplayBuffer(S, A, n, K, n_step=3, device=dev).state_dict()) and not hasattr(buf, "_tree")
    assert "priorities" not in buf.state_dict()
    with pytest.raises(RuntimeError, match="prioritized=True"):
        buf.update_priorities(out[5], out[2])
    with pytest.raises(ValueError, match="prioritized=True"):
        buf.sample(4, beta=0.5)
