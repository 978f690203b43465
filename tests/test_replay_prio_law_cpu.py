"""CPU: the definition of proportional sampling (tests/replay_prio_law.py: a float64 cumulative sum, no tree) against the restatement of
the kernel's descent (tests/replay_prio_ref.py), on the leaf sets tests/test_replay_prio_law_gpu.py puts on the device.

The restatement passes: on integer leaves its rows ARE searchsorted's, on real leaves every target lies within `tol` of its drawn row's
interval.  That is what makes the derived `tol` legitimate for the device, whose tree and descent equal the restatement's bit for bit
(tests/test_replay_prio_gpu.py).  Worst check_draws ratio of the restatement over every case below (printed by the test): 0.0436, at
4096 uniform leaves; 0.0279 over the targets placed by hand at the interval ends, which take the fallback child 271 times.  The bound is
a worst case over every rounding, the errors met are a twentieth of it; it is left as derived.

The checks have teeth: an exclusive prefix and a dropped `t -= before` fail both of them.  The third slip, `>=` for `>` against t, differs
from the law only where a target equals a prefix exactly; a 53-bit target times a float32 root does that with probability < 2^-29 per
draw, so on drawn targets the mutant draws the restatement's rows (asserted: if that ever fails, the seeds found such a draw and the
first assertion names it).  It is caught where the targets are given on the boundaries: the exact check fails there.  The interval
check cannot fail for it, by construction: at t = C[i] both row i and row i + 1 satisfy the closed interval, and they should, since
the two differ by an event of measure zero -- `>=` is not a departure from p_i / sum p that any tolerance-based check may call one."""
import numpy as np
import pytest

import replay_prio_law as LAW
import replay_prio_ref as PR

CAPACITIES = (1, 64, 70, 4096, 4290, 262145)                                # K n of the device test's SIZES
BATCHES, ORDINALS, SEED = (1, 64, 257), (0, 1, 2 ** 32 + 5), 0xBEEF0000


def stored_rows(cap):
    """Partly filled (none for one row), and full."""
    return ([cap // 2] if cap > 1 else []) + [cap]


def tree_of(leaves, cap):
    return PR.build(np.concatenate([leaves, np.zeros(cap - len(leaves), np.float32)]))


def descend_variant(tree, t, exclusive=False, subtract=True, ge=False):
    """The descent with its three slips switchable -> (rows, steps that fell back to the last positive child).  All off: PR.descend."""
    t = np.array(t, dtype=np.float64)
    node, fell, lanes = np.zeros(len(t), np.int64), 0, np.arange(len(t))
    for level in tree[-2::-1]:
        child = level.reshape(-1, 64)[node]
        prefix, pos = PR.scan(child).astype(np.float64), child > 0
        against = np.concatenate([np.zeros((len(t), 1)), prefix[:, :-1]], axis=1) if exclusive else prefix
        over = pos & ((against >= t[:, None]) if ge else (against > t[:, None]))
        last = np.where(pos.any(1), 63 - np.argmax(pos[:, ::-1], axis=1), 0)
        chosen = np.where(over.any(1), np.argmax(over, axis=1), last)
        fell += int((~over.any(1) & pos.any(1)).sum())
        if subtract:
            t = t - np.where(chosen > 0, prefix[lanes, np.maximum(chosen - 1, 0)], 0.0)
        node = node * 64 + chosen
    return node, fell


MUTANTS = {"exclusive prefix": dict(exclusive=True), "no t -= before": dict(subtract=False), ">= against t": dict(ge=True)}


def cases(kind):
    """(capacity, R, name, leaves [R], tree) of every leaf set."""
    for cap in CAPACITIES:
        for R in stored_rows(cap):
            rng = np.random.default_rng(1000 * cap + R)
            sets = LAW.integer_leaf_sets(R, rng) if kind == "integer" else LAW.real_leaf_sets(R, rng)
            if kind == "real":                                              # and leaves like update_priorities leaves them
                td = rng.standard_normal(R) * 10.0 ** rng.uniform(-3, 2, R)
                sets["(|td| + 1e-6) ** 0.6 on a third of ones"] = np.where(rng.random(R) < 1 / 3, (np.abs(td) + 1e-6) ** 0.6, 1.0).astype(np.float32)
            for name, leaves in sets.items():
                yield cap, R, name, leaves, tree_of(leaves, cap)


def batches(R, name):
    return BATCHES + ((1000,) if name == "total 3" else ()) + ((4 * R,) if R <= 4290 and name.startswith(("random", "uniform")) else ())


def test_levels_and_tolerance_are_the_documented_ones():
    for cap in CAPACITIES + (65, 4097, 2 ** 31 - 1):
        assert LAW.levels_above(cap) == len(PR.levels(cap)[0]) - 1
    assert [LAW.levels_above(c) for c in CAPACITIES] == [1, 1, 2, 2, 3, 4]
    for cap, root in ((70, 100.0), (262145, 3e5)):
        L = LAW.levels_above(cap)
        first_order = 3 * L * (L + 3) * 2.0 ** -24 * root
        assert first_order < LAW.tolerance(cap, root) < first_order * (1 + 1e-4)


def test_the_restatement_draws_the_laws_rows_on_integer_leaves():
    fell = 0
    for cap, R, name, leaves, tree in cases("integer"):
        full = tree[0][:cap]
        for B in batches(R, name):
            for ordinal in ORDINALS:
                got = PR.descend(tree, SEED, ordinal, B)
                want = LAW.exact_rows(full, tree[-1][0], SEED, ordinal, B)
                assert np.array_equal(got, want), f"{cap} leaves, {R} stored, {name}, B={B}, ordinal={ordinal}"
                assert LAW.check_draws(got, full, tree[-1][0], SEED, ordinal, B, R) == 0.0      # exact sums: no slack is used at all
                mine, f = descend_variant(tree, LAW.targets(tree[-1][0], SEED, ordinal, B))
                assert np.array_equal(mine, got), "descend_variant with nothing switched is not the restatement"
                fell += f
    assert fell == 0, "exact sums never need the fallback child"


def test_the_restatement_stays_within_the_derived_tolerance_on_real_leaves():
    worst, fell = {}, {}
    for cap, R, name, leaves, tree in cases("real"):
        full = tree[0][:cap]
        for B in batches(R, name):
            for ordinal in ORDINALS:
                got = PR.descend(tree, SEED, ordinal, B)
                ratio = LAW.check_draws(got, full, tree[-1][0], SEED, ordinal, B, R)
                assert ratio <= 1.0, f"{cap} leaves, {R} stored, {name}, B={B}, ordinal={ordinal}: {ratio}"
                worst[cap, name] = max(worst.get((cap, name), 0.0), ratio)
                fell[name] = fell.get(name, 0) + descend_variant(tree, LAW.targets(tree[-1][0], SEED, ordinal, B))[1]
    for (cap, name), ratio in worst.items():
        print(f"{cap:7d} leaves, {name}: worst violation / tol = {ratio:.4f}")
    print(f"worst of all drawn targets: {max(worst.values()):.4f}; fallback steps among them: {fell}")
    # The fallback child is taken only where a target falls into the rounding gap between a parent's prefix and its child's own sum:
    # about 64 L u of all draws, so a drawn batch reaches it by chance only.  Targets placed a few float32 ulps either side of every
    # interval's end reach it at will, and the bound has to hold there too.
    for cap in (70, 4290, 262145):
        leaves = LAW.real_leaf_sets(cap, np.random.default_rng(cap))["log-uniform 2^-40 .. 2^20"]
        tree = tree_of(leaves, cap)
        C, root = np.cumsum(leaves.astype(np.float64)), np.float64(tree[-1][0])
        ends = C[:-1][:: max(1, cap // 20000)] * (root / C[-1])
        t = np.concatenate([ends * (1 + s * 2.0 ** -k) for s in (-1, 1) for k in (22, 24, 26)])
        t = t[t < root]
        rows, f = descend_variant(tree, t)
        ratio = LAW.check_draws(rows, leaves, root, 0, 0, len(t), cap, t=t)
        print(f"{cap:7d} leaves, log-uniform, {len(t)} targets at the interval ends: {f} fallback steps, worst violation / tol = {ratio:.4f}")
        assert ratio <= 1.0, (cap, f, ratio)
        worst[cap, "ends"], fell["ends"] = ratio, fell.get("ends", 0) + f
    assert fell["ends"] > 0, "no target reached the fallback child"
    print(f"worst of all: {max(worst.values()):.4f}")


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_the_checks_catch_a_mutated_descent(mutant):
    failed_exact = failed_interval = differs = 0
    for kind in ("integer", "real"):
        for cap, R, name, leaves, tree in cases(kind):
            if cap > 4290:
                continue
            full, root = tree[0][:cap], tree[-1][0]
            for ordinal in ORDINALS:
                got = descend_variant(tree, LAW.targets(root, SEED, ordinal, 257), **MUTANTS[mutant])[0]
                differs += not np.array_equal(got, PR.descend(tree, SEED, ordinal, 257))
                if kind == "integer":
                    failed_exact += not np.array_equal(got, LAW.exact_rows(full, root, SEED, ordinal, 257))
                failed_interval += not LAW.check_draws(got, full, root, SEED, ordinal, 257, R) <= 1.0
    if mutant != ">= against t":
        assert failed_exact > 0 and failed_interval > 0, (failed_exact, failed_interval)
        print(f"{mutant}: failed the exact check in {failed_exact} cases, the interval check in {failed_interval}")
        return
    # `>=`: the same rows on every drawn target (see the module docstring); on the boundaries themselves the exact check tells them apart
    assert differs == 0 and failed_exact == 0 and failed_interval == 0, "a drawn target equals a float32 prefix exactly"
    for cap in (70, 4290):
        leaves = LAW.integer_leaf_sets(cap, np.random.default_rng(cap))["random, 30 % zeros"]
        tree, C = tree_of(leaves, cap), np.cumsum(leaves.astype(np.float64))
        t = np.unique(C[C > 0])[:-1]                                        # every boundary between two positive rows
        sound, slipped = descend_variant(tree, t)[0], descend_variant(tree, t, ge=True)[0]
        assert np.array_equal(sound, LAW.rows_at(C, t)) and not np.array_equal(slipped, LAW.rows_at(C, t))
        assert (leaves[slipped] > 0).all() and (C[slipped] == t).all(), "the slip draws the row that ends at t, not the one that starts there"
        assert LAW.check_draws(slipped, leaves, tree[-1][0], 0, 0, len(t), cap, t=t) == 0.0


def test_the_tolerance_is_sharper_than_a_leaf_on_trees_of_two_levels():
    """Leaves in [0.5, 2): a draw displaced by one leaf misses its interval by at least 0.5.  Up to 4096 leaves tol is below 1/8 of the
    smallest leaf, so no displaced draw hides in it.  tol grows with the root, i.e. with n: at 262,145 leaves it exceeds a leaf and the
    interval check there only bounds the displacement (the integer cases, which are exact at every size, carry that size)."""
    for cap in CAPACITIES:
        leaves = LAW.real_leaf_sets(cap, np.random.default_rng(cap))["uniform [0.5, 2)"]
        tol = LAW.tolerance(cap, PR.build(leaves)[-1][0])
        loose = tol >= leaves.min() / 8
        print(f"{cap:7d} leaves: tol / median leaf = {tol / np.median(leaves):.3e}" + (" -- LOOSE: a neighbouring leaf can pass" if loose else ""))
        assert not loose or cap > 4096, (cap, tol, leaves.min())
    assert loose, "262,145 leaves were expected to be the loose size; say so above if this changed"
