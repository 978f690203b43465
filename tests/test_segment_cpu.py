"""CPU: the NumPy restatement of the rollout storage's GAE (tests/segment_ref.py) against the fp64 per-row definition within the bound
derived from the float32 operations on a row's chain; the restated permutation is a bijection; the ABI (four entry points, still 13)."""
import os
import re

import numpy as np
import pytest

import trajopt_grpo_amd as tg
import segment_ref as SR

HEADER = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "trajopt_grpo_hip.h")).read()
ROWS = [1, 2, 3, 64, 65, 1190, 4097]
KINDS = {(True, False), (False, True), (True, True)}                        # (terminated, truncated) of an ending


def segment_case(L, n, seed):
    """Inputs of one segment, [L][n].  Every column but those with i % 7 == 3 (no ending at all) ends at t = 0, L // 2 and L - 1 and,
    with p = 0.3, elsewhere; the kind of a column's j-th ending cycles through KINDS, so from L = 3 on every such column has all
    three.  final_value is NaN wherever the slot did not end."""
    rng = np.random.default_rng(seed)
    reward, val, fv = (rng.standard_normal((L, n)).astype(np.float32) for _ in range(3))
    term, trunc = np.zeros((L, n), bool), np.zeros((L, n), bool)
    for i in range(n):
        if i % 7 != 3:
            for j, t in enumerate(sorted({0, L // 2, L - 1} | set(np.flatnonzero(rng.random(L) < 0.3).tolist()))):
                term[t, i], trunc[t, i] = (i + j) % 3 != 1, (i + j) % 3 != 0
    fv[~(term | trunc)] = np.nan
    return reward, term, trunc, fv, val, rng.standard_normal(n).astype(np.float32)


def restated(reward, term, trunc, fv, val, last, gamma, lam):
    rew, flags = np.empty_like(reward), np.empty(reward.shape, np.uint8)
    for t in range(reward.shape[0]):
        SR.push(rew[t], flags[t], reward[t], term[t], trunc[t], fv[t], gamma)
    return rew, flags, SR.gae(rew, val, flags, last, gamma, lam)


@pytest.mark.parametrize("L", [1, 2, 3, 8, 9, 17, 64])
@pytest.mark.parametrize("gamma, lam", [(0.99, 0.95), (1.0, 1.0), (0.9, 0.5)])
def test_restated_gae_is_the_fp64_definition_within_the_operation_count_bound(L, gamma, lam):
    case = segment_case(L, 23, seed=L)
    reward, term, trunc, fv, val, last = case
    for i in range(23 if L >= 3 else 0):                                     # the flags are what the docstring above promises
        kinds = {(bool(a), bool(b)) for a, b in zip(term[:, i], trunc[:, i]) if a or b}
        assert kinds == (set() if i % 7 == 3 else KINDS) and (i % 7 == 3 or (term | trunc)[[0, L - 1], i].all()), i
    rew, flags, (adv, ret) = restated(*case, gamma, lam)
    assert not np.isnan(rew).any(), "final_value was read where the slot did not end with a truncation alone"
    want_adv, want_ret, mag, ops = SR.gae_fp64(*case, gamma, lam)
    bound_adv, bound_ret = SR.gae_bound(mag, ops, val)
    print(f"L={L}: max err / bound: adv {np.max(np.abs(adv - want_adv) / bound_adv):.3f} ret {np.max(np.abs(ret - want_ret) / bound_ret):.3f}")
    assert (np.abs(adv - want_adv) <= bound_adv).all() and (np.abs(ret - want_ret) <= bound_ret).all() and ops.max() <= 6 + 3 * L


@pytest.mark.parametrize("rows", ROWS)
def test_restated_permutation_is_a_bijection(rows):
    perms = [SR.permutation(rows, seed=0xC0FFEE, ordinal=o) for o in (0, 1, 2 ** 32 + 5)]
    assert all(idx.dtype == np.int64 and np.array_equal(np.sort(idx), np.arange(rows)) for idx, _ in perms)
    bits = SR.permute_bits(rows)
    assert bits % 2 == 0 and bits >= 2 and 2 ** bits >= rows and (bits == 2 or 2 ** (bits - 2) < rows)
    print(f"rows={rows}: {bits} bits, longest cycle walk {max(walks for _, walks in perms)}")
    assert rows <= 3 or not np.array_equal(perms[0][0], perms[1][0])


def test_symbols_are_declared_bound_and_exported_and_the_abi_is_still_13():
    N, lib = tg._native, tg._native.load()
    for name in ("tg_segment_push", "tg_segment_gae", "tg_segment_permute", "tg_segment_gather"):
        declared = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\);", HEADER).group(1).split(",")
        assert len(declared) == len(N.SIGNATURES[name][1]) and declared[0].strip() == "const tg_segment* s" and hasattr(lib, name), name
    body = re.search(r"typedef struct tg_segment \{(.*?)\} tg_segment;", HEADER, re.S).group(1)
    assert re.findall(r"\s([a-z_]+);", body) == [name for name, _ in N.Segment._fields_]
    assert lib.tg_abi_version() == N.ABI_VERSION == int(re.search(r"#define\s+TG_ABI_VERSION\s+(\d+)", HEADER).group(1)) == 13
    assert tg.DeviceRolloutStorage is tg.storage.DeviceRolloutStorage and "DeviceRolloutStorage" in tg.__all__
