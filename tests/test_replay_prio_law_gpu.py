"""DeviceReplayBuffer(prioritized=True).sample() on the MI355X (run with `-m gpu`) against the definition of proportional sampling
(tests/replay_prio_law.py: a float64 cumulative sum of the leaves read back, no tree, none of the kernel's steps).

Integer leaves (0 .. 31, total < 2^24: every float32 sum is exact): the drawn rows equal searchsorted's for every element.  Real
leaves: every target lies within the derived `tol` of its drawn row's interval; the worst ratio and tol / median leaf are printed.
tol is sharper than a leaf up to 4096 leaves and looser than one at 262,145 (tests/test_replay_prio_law_cpu.py says where); the
integer cases are exact at every size.  The fallback child ("the last positive one") is reached by a drawn target only by chance,
about 64 L 2^-24 of all draws: the CPU file drives the restatement through it with targets given by hand, and
tests/test_replay_prio_gpu.py holds the device to the restatement bit for bit.

Measured on an MI355X (profiles/r23_replay_prio_law.md): every integer case exact; worst violation / tol 0.047 (4096 leaves, uniform),
at most 0.014 at the other sizes, 0 up to 70 leaves; tol / median leaf 7e-7 .. 1.5e-2 up to 4290 uniform leaves, 1.31 at 262,145."""
import numpy as np
import pytest
import torch

import replay_prio_law as LAW
import test_replay_prio_gpu as PG
from test_replay_gpu import bits, dev, fill, tg, to_dev  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu
BATCHES, ORDINALS = (1, 64, 257), (0, 1, 2 ** 32 + 5)                       # the last ordinal reaches the draw's `sub` word
CASES = [(size, stage) for size in PG.SIZES for stage in ("partly filled", "full") if size[1] > 1 or stage == "full"]


class Widths:
    """What fill() / push_random() ask of their second argument, without the restatement's storage: these tests read the device's."""
    def __init__(self, n, S, A):
        self.n, self.S, self.A = n, S, A

    def start(self, obs):
        pass

    def push(self, *step):
        pass


def filled_buffer(tg, dev, size, stage, **kw):
    n, K, n_step, S, A = size
    buf = tg.DeviceReplayBuffer(S, A, n, K, n_step=n_step, seed=0xBEEF0000 + n, device=dev, prioritized=True, **kw)
    rng = fill(buf, Widths(n, S, A), dev, K // 2 if stage == "partly filled" else K + 1, seed=n + K)
    assert len(buf) == (K // 2 if stage == "partly filled" else K) * n and (len(buf) < buf.capacity) == (stage == "partly filled")
    assert LAW.levels_above(buf.capacity) == len(buf.tree_levels) - 1
    return buf, rng


def set_leaves(buf, leaves):
    """priorities[:R] by hand (the rows beyond stay 0), the levels above rebuilt -> (the leaves as read back, the float32 root)."""
    buf.priorities.zero_()
    buf.priorities[:len(leaves)] = torch.from_numpy(leaves).to(buf.device)
    buf.rebuild_tree()
    return read_back(buf)


def read_back(buf):
    return buf.priorities.cpu().numpy(), buf._tree[buf.tree_levels[-1][0]].cpu().numpy()


def draw(buf, B, ordinal):
    """One sample(B) at `ordinal` -> the drawn rows; every sampled row is the storage row its index names."""
    buf._ordinal = ordinal
    out = buf.sample(B)
    assert buf._ordinal == ordinal + 1 and out[5].shape == (B,)
    for got, store in zip(out[:5], (buf.obs, buf.act, buf.rew, buf.next_obs, buf.disc)):
        assert np.array_equal(bits(got), bits(store[out[5]])), "a sampled row is not the storage row its index names"
    return out[5].cpu().numpy()


def batches(R, name):
    return BATCHES + ((1000,) if name == "total 3" else ()) + ((4 * R,) if R <= 4290 and name.startswith(("random", "uniform")) else ())


@pytest.mark.parametrize("size, stage", CASES)
def test_integer_leaves_draw_exactly_the_rows_of_the_definition(tg, dev, size, stage):
    buf, _ = filled_buffer(tg, dev, size, stage)
    R = len(buf)
    for name, leaves in LAW.integer_leaf_sets(R, np.random.default_rng(R)).items():
        back, root = set_leaves(buf, leaves)
        assert np.array_equal(back[:R], leaves) and not back[R:].any() and float(root) == leaves.astype(np.float64).sum() < 2 ** 24
        for B in batches(R, name):
            for ordinal in ORDINALS:
                idx = draw(buf, B, ordinal)
                want = LAW.exact_rows(back, root, buf.seed, ordinal, B)
                assert np.array_equal(idx, want), (f"{name}, B={B}, ordinal={ordinal}: {int((idx != want).sum())} of {B} rows differ, first at "
                                                   f"b={int(np.argmax(idx != want))}: drew {idx[np.argmax(idx != want)]}, the law {want[np.argmax(idx != want)]}")
                assert idx.max() < R and (back[idx] > 0).all()


@pytest.mark.parametrize("size, stage", CASES)
def test_real_leaves_draw_within_the_derived_tolerance(tg, dev, size, stage):
    buf, rng = filled_buffer(tg, dev, size, stage)
    R, worst = len(buf), {}

    def check(name, back, root):
        tol = LAW.tolerance(buf.capacity, root)
        for B in batches(R, name):
            for ordinal in ORDINALS:
                ratio = LAW.check_draws(draw(buf, B, ordinal), back, root, buf.seed, ordinal, B, R)
                worst[name] = max(worst.get(name, 0.0), ratio)
                assert ratio <= 1.0, f"{name}, B={B}, ordinal={ordinal}: a target lies {ratio} tol outside its drawn row's interval"
        print(f"{buf.capacity:7d} leaves, {R:7d} stored, {name}: worst violation / tol = {worst[name]:.4f}, "
              f"tol / median positive leaf = {tol / np.median(back[back > 0]):.3e}")

    for name, leaves in LAW.real_leaf_sets(R, np.random.default_rng(R)).items():
        check(name, *set_leaves(buf, leaves))
    buf.priorities[:R] = 1.0                                                # as add() left them, then three real updates
    buf.rebuild_tree()
    for k in range(3):
        PG.update_and_check(buf, rng, dev, f"update {k}")
    check("after three update_priorities", *read_back(buf))


def test_extreme_errors_and_exponents(tg, dev):
    """update_priorities caps a new priority at 2^96, so no sum of fewer than 2^31 leaves that push and update wrote leaves float32:
    two errors of 3e38 at alpha = 1 give two leaves of 2^96, a finite root, drawn rows with mass and finite weights."""
    size, cap = (10, 7, 3, 10, 2), np.float32(2.0 ** 96)
    buf, _ = filled_buffer(tg, dev, size, "full", alpha=1.0)
    R = len(buf)
    assert R == 70
    rows = torch.tensor([3, 69], dtype=torch.int64, device=dev)
    buf.update_priorities(rows, torch.full((2,), 3e38, dtype=torch.float32, device=dev))
    back, root = read_back(buf)
    assert (back[[3, 69]] == cap).all() and (np.delete(back, [3, 69]) == 1.0).all() and float(buf._max_priority) == cap
    assert np.isfinite(root) and root == np.float32(2.0 ** 97)
    PG.check_tree(buf, "after two capped leaves", rebuild=True)
    for B in (1, 64, 257):
        idx = draw(buf, B, 0)
        assert LAW.check_draws(idx, back, root, buf.seed, 0, B, R) <= 1.0 and set(idx) <= {3, 69}
        assert bool(torch.isfinite(buf.raw_weight).all()) and bool((buf.sample(B)[6] == 1.0).all())
    out = buf.sample(indices=torch.tensor([3, 0], dtype=torch.int64, device=dev), beta=1.0)   # a row of priority 1 beside 2^96
    assert bool(torch.isfinite(buf.raw_weight).all()) and float(out[6][1]) == 1.0 and 0 < float(out[6][0]) < 2.0 ** -90
    # alpha = 0: every updated leaf is exactly 1; beta = 0: every weight is exactly 1
    buf, rng = filled_buffer(tg, dev, size, "full", alpha=0.0, beta=0.0)
    buf.priorities[:R] = torch.from_numpy(rng.uniform(0.5, 2.0, R).astype(np.float32)).to(dev)
    buf.rebuild_tree()
    idx = torch.arange(0, R, 2, dtype=torch.int64, device=dev)
    td = to_dev(dev, (rng.standard_normal(len(idx)) * 10.0 ** rng.uniform(-30, 30, len(idx))).astype(np.float32))[0]
    td[:2] = torch.tensor([0.0, 3e38])
    buf.update_priorities(idx, td)
    back, root = read_back(buf)
    assert (back[0:R:2] == 1.0).all() and (back[1:R:2] != 1.0).all()
    out = buf.sample(257)
    assert bool((buf.raw_weight == 1.0).all()) and bool((out[6] == 1.0).all())
    assert LAW.check_draws(out[5].cpu().numpy(), back, root, buf.seed, buf._ordinal - 1, 257, R) <= 1.0
    # eps = 0 and td = 0: the leaf is 0, never drawn, and has no weight when named
    buf, rng = filled_buffer(tg, dev, size, "full", priority_eps=0.0)
    gone = torch.tensor([0, 5, 64, 69], dtype=torch.int64, device=dev)
    buf.update_priorities(gone, torch.zeros(4, dtype=torch.float32, device=dev))
    back, root = read_back(buf)
    assert (back[[0, 5, 64, 69]] == 0).all() and root == 66.0
    for ordinal in ORDINALS:
        idx = draw(buf, 280, ordinal)
        assert np.array_equal(idx, LAW.exact_rows(back, root, buf.seed, ordinal, 280)) and not np.isin(idx, [0, 5, 64, 69]).any()
    out = buf.sample(indices=torch.tensor([0, 1, 69], dtype=torch.int64, device=dev))
    assert np.isnan(out[6].cpu().numpy()).tolist() == [True, False, True] and np.isnan(buf.raw_weight.cpu().numpy()).tolist() == [True, False, True]
    assert bool(torch.isnan(out[0][0]).all()) and not bool(torch.isnan(out[0][1]).any())
