"""tests/row_kernels_ref.py held to account without a GPU: (a) its restatements against torch's own operations -- `mask.nonzero()`,
`obs_rows[idx]` with GemmMLP.prepare_input's padding, `.to(torch.bfloat16)`, `v * sigma + mean`, the clamp expression of the
observation normalisation, the fp64 group normalisation of returns_loss_fp64 -- on every shape, mask pattern and row format the
GPU module runs; (b) sixteen WRONG kernels, each of which the checker the GPU module uses must reject on that module's own inputs;
(c) the properties the shape table and the mask patterns exist for.  The shapes are explained in row_kernels_ref's docstring."""
import math

import numpy as np
import pytest
import torch

import returns_loss_fp64 as F
import row_kernels_ref as R

CASES = R.compact_cases()
ON_CASES = R.on_cases()
SMALL = [c for c in CASES if (c.T, c.n) != R.BIG]
GUARD = 5


def _ids(cases):
    return [c.id for c in cases]


# ------------------------------------------------------------------------------------------------------------------------------
# (c) the tables
# ------------------------------------------------------------------------------------------------------------------------------
def test_the_shape_table_reaches_what_it_is_for():
    R.check_shape_table()
    assert {(c.T, c.n) for c in CASES} == set(R.SHAPES)
    for fmt in R.SWEEP_FORMATS:                                    # every shape and pattern on the two sweep formats (BIG: S = 5 only)
        for T, n in R.SHAPES:
            if (T, n) == R.BIG and fmt[0] != 5:
                continue
            got = {c.pattern for c in CASES if (c.T, c.n, c.S, c.in_pad, c.bf16, c.ones_col) == (T, n) + fmt}
            assert got >= set(R.patterns_for(T, n)), (T, n, fmt)
    for fmt in R.FORMATS:                                          # every row format on both format shapes, f32 and f64 observations
        for T, n in R.FORMAT_SHAPES:
            sel = [c for c in CASES if (c.T, c.n, c.S, c.in_pad, c.bf16, c.ones_col) == (T, n) + fmt]
            assert sel, (fmt, T, n)
        assert {c.obs_f64 for c in CASES if (c.S, c.in_pad, c.bf16, c.ones_col) == fmt} == {False, True}, fmt
    assert all(c.S == 5 and c.A == 1 for c in CASES if (c.T, c.n) == R.BIG)
    assert {c.A for c in CASES} == set(R.ACTION_DIMS) and {c.srcs for c in CASES} == {"both", "src0", "none"}
    assert {c.norm_mode for c in CASES if c.srcs != "none"} == {None, 0, 1}
    assert any(c.group_size == c.n for c in CASES if c.norm_mode is not None)
    assert any(c.group_size != c.n and c.group_size % 4 for c in CASES if c.norm_mode is not None)
    assert {c.on for c in ON_CASES} == {5.0, math.inf} and {c.obs_f64 for c in ON_CASES} == {False, True}
    assert {c.bf16 for c in ON_CASES} == {False, True}


@pytest.mark.parametrize("T,n", R.SHAPES)
def test_every_mask_pattern_has_its_property(T, n):
    assert [p for p in R.PATTERNS if p not in R.patterns_for(T, n)] == ([] if T * n > R.CHUNK else list(R.MULTI_CHUNK))
    for pattern in R.patterns_for(T, n):
        R.check_pattern(R.make_mask(T, n, pattern), pattern)
    if (T, n) == R.BIG:
        for pattern in ("empty_chunk", "full_chunk"):              # both sides of the scan's trip boundary, and valid rows past it
            cnt = R.chunk_counts(R.make_mask(T, n, pattern))
            want = 0 if pattern == "empty_chunk" else R.CHUNK
            assert cnt[1023] == cnt[1024] == want and cnt[:1023].any() and cnt[1025:].any()


# ------------------------------------------------------------------------------------------------------------------------------
# (a) the restatements against torch
# ------------------------------------------------------------------------------------------------------------------------------
def _torch_rows(c, x, idx, tab=None, clip=None):
    """obs_rows().index_select(0, idx), then GemmMLP.prepare_input's padding; -> the bit patterns."""
    obs = torch.from_numpy(np.array(x.obs))
    X = obs[:, :c.T, :].permute(1, 2, 0).reshape(c.T * c.n, c.S).index_select(0, idx).float()
    if tab is not None:
        t = torch.from_numpy(tab)
        X = (X - t[0]) * t[1]
        X = X if math.isinf(clip) else torch.clamp(X, -clip, clip)
    xp = torch.zeros(X.shape[0], c.in_pad, dtype=torch.bfloat16 if c.bf16 else torch.float32)
    xp[:, :c.S].copy_(X)
    if c.ones_col >= 0:
        xp[:, c.ones_col] = 1.0
    return xp.view(torch.int16 if c.bf16 else torch.int32).numpy().view(np.uint16 if c.bf16 else np.uint32)


@pytest.mark.parametrize("c", CASES + ON_CASES, ids=_ids(CASES + ON_CASES))
def test_compact_ref_is_torchs_own_prologue(c):
    x = R.case_inputs(c)
    ref = R.case_ref(c, x)
    M = c.T * c.n
    idx0 = np.flatnonzero(x.mask)
    assert np.array_equal(ref.idx, idx0) and ref.idx.dtype == np.int64 and ref.total == ref.written == idx0.size
    assert np.array_equal(idx0, torch.from_numpy(x.mask.copy()).reshape(-1).nonzero().squeeze(1).numpy())
    cnt = R.chunk_counts(x.mask)
    assert np.array_equal(ref.offsets.astype(np.int64), np.cumsum(cnt) - cnt) and ref.offsets.size == R.chunks(M)
    idx = torch.from_numpy(idx0)
    want = _torch_rows(c, x, idx, x.obs_tab, c.on)
    assert ref.xin.shape == want.shape and R._same_bits(ref.xin, want)
    if c.on is not None and x.nan_at is not None:                  # the NaN observation of a valid row stays a NaN, whatever the clip
        r = int(np.searchsorted(idx0, x.nan_at))
        col = ref.xin[r, c.S - 1]
        assert (col & 0x7F80) == 0x7F80 and (col & 0x7F) if c.bf16 else np.isnan(col.view(np.float32))
        if not math.isinf(c.on):                                   # ... and some value of the case lies beyond the clip
            raw = R.case_ref(c, x, mutant="no_clamp")
            assert not np.array_equal(raw.xin, ref.xin)
    if c.A is None:
        assert ref.act_rows is None
    else:
        a = torch.from_numpy(np.array(x.act)).permute(1, 2, 0).reshape(M, c.A).index_select(0, idx)
        assert np.array_equal(ref.act_rows, a.contiguous().view(torch.int32).numpy().view(np.uint32))
    assert (ref.dst0 is None) == (c.srcs == "none") and (ref.dst1 is None) == (c.srcs != "both")
    if ref.dst1 is not None:
        assert np.array_equal(ref.dst1, R.f32_bits(x.src1.reshape(-1)[idx0]))
    if ref.dst0 is not None and c.norm_mode is None:
        assert np.array_equal(ref.dst0, R.f32_bits(x.src0.reshape(-1)[idx0]))
    # rows the capacity cuts off are not written
    if ref.total >= 2:
        short = R.case_ref(c, x, rows_cap=ref.total - 1)
        assert short.total == ref.total and short.written == ref.total - 1 and np.array_equal(short.idx, ref.idx[:-1])
        assert np.array_equal(short.xin, ref.xin[:-1])


def _group_counts(c):
    return (R.make_mask(c.T, c.n, c.pattern) != 0).reshape(c.T, c.n // c.group_size, c.group_size).sum((0, 2))


# the fp64 yardstick's own scope: every group holds enough valid entries for its one-pass variance term to stay below 2^-24
NORM_CASES = [c for c in SMALL if c.norm_mode is not None and _group_counts(c).min() >= 16]


@pytest.mark.parametrize("c", NORM_CASES, ids=_ids(NORM_CASES))
def test_the_row_normalisation_is_the_fp64_group_normalisation(c):
    """compact_ref's dst0, scattered back onto the [T][n] grid, inside returns_loss_fp64's bound of the fp64 group normalisation."""
    x = R.case_inputs(c)
    ref = R.case_ref(c, x)
    grid = np.zeros(c.T * c.n, dtype=np.float32)
    grid[ref.idx] = ref.dst0.view(np.float32)
    F.check_normalize(grid.reshape(c.T, c.n), x.src0, x.mask, c.group_size, c.norm_mode, tag=c.id)


def test_the_fp64_check_covers_both_modes_and_group_sizes():
    assert {c.norm_mode for c in NORM_CASES} == {0, 1} and {c.group_size == c.n for c in NORM_CASES} == {False, True}
    assert len(NORM_CASES) >= 12
    for c in SMALL:                                                # every normalised row of every case is a finite number
        if c.norm_mode is not None:
            assert np.isfinite(R.case_ref(c, R.case_inputs(c)).dst0.view(np.float32)).all(), c.id


@pytest.mark.parametrize("rows", [r for r in R.ROW_COUNTS if r])
def test_affine_ref_is_torchs_two_operations(rows):
    src, idx, cells = R.row_inputs(rows, 4)
    tab = torch.from_numpy(R.AFFINE_TABLE)
    want = torch.from_numpy(src[:, 0].copy()) * tab[1] + tab[0]
    got = R.affine_ref(src[:, 0], R.AFFINE_TABLE)
    assert got.dtype == np.float32 and np.array_equal(R.f32_bits(got), R.f32_bits(want.numpy()))
    timeout = (np.arange(rows) % 3 != 0).astype(np.uint8)
    boot = torch.mul(want, torch.from_numpy(timeout))
    assert np.array_equal(R.f32_bits(R.boot_affine_ref(src[:, 0], timeout, R.AFFINE_TABLE)), R.f32_bits(boot.numpy()))
    dst = R.sentinel(np.float32, (cells,))
    out = R.scatter_ref(src, idx, dst)
    keep = np.ones(cells, dtype=bool)
    keep[idx] = False
    assert np.array_equal(out[idx], src[:, 0]) and np.array_equal(R.f32_bits(out[keep]), R.sentinel(np.uint32, (int(keep.sum()),)))
    g0, g1 = R.gather2_ref(idx, out, R.sentinel(np.float32, (rows + 3,)), dst, R.sentinel(np.float32, (rows + 3,)))
    assert np.array_equal(g0[:rows], src[:, 0]) and np.array_equal(R.f32_bits(g0[rows:]), R.sentinel(np.uint32, (3,)))
    assert np.array_equal(R.f32_bits(g1), R.sentinel(np.uint32, (rows + 3,)))


def test_bf16_bits_is_torchs_conversion():
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.standard_normal(100000).astype(np.float32) * 3.0,
                        np.array([0.0, -0.0, 1.0, np.inf, -np.inf, 1.00390625, 1.01171875, 3.3895314e38], dtype=np.float32)])   # ties, overflow
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(R.bf16_bits(x), want)
    assert np.mean(R.bf16_bits(x) != R.bf16_bits(x, truncate=True)) >= 0.25


def test_region_sizes_and_arena_layout():
    assert R.region_bytes(5, 3, 5, 1, False) == [360, 60, 60, 15, 12, 32] and R.region_bytes(5, 3, 5, 1, True) == [720, 60, 120, 15, 12, 32]
    assert sorted({b % 16 for b in R.region_bytes(5, 3, 5, 1, False) if b % 16}) == [8, 12, 15]
    for T, n, S, A in R.BEGIN_SHAPES:
        for f64 in (False, True):
            sizes = R.region_bytes(T, n, S, A, f64)
            offs, total = R.arena_layout(sizes)
            ends = [o + b for o, b in zip(offs, sizes)]
            assert all(o % 16 == 0 for o in offs) and offs[0] >= 32 and total - ends[-1] >= 32
            assert all(offs[k + 1] - ends[k] >= 32 for k in range(5))
            img = R.zero_regions_ref(total, offs, sizes)
            assert int((img == 0).sum()) == sum(sizes) and int((img == R.SENTINEL_BYTE).sum()) == total - sum(sizes)
            R.check_arena(img, offs, sizes)


@pytest.mark.parametrize("T,n", R.FINISH_SHAPES)
def test_finish_ref_counts_only_ended_slots(T, n):
    ln, rew = R.finish_inputs(T, n, False)
    ref = R.finish_ref(ln, rew, (13, 2 ** 64 - 1))
    assert ref.counters == (int(ln[ln > 0].sum()), int((ln > 0).sum())) and ref.stats1 == n and ref.stats2 == ref.counters[0]
    assert ref.rng == (13, 0) and R.finish_ref(ln, rew, None).rng is None
    assert (ln < 0).any() and (n < 3 or ((ln == 0).any() and (ln > 0).any()))
    assert abs(float(np.sum(rew.astype(np.float64))) - ref.reward_sum) <= ref.reward_bound


# ------------------------------------------------------------------------------------------------------------------------------
# (b) the mutants
# ------------------------------------------------------------------------------------------------------------------------------
def _rejected(c, x, mutant):
    ref = R.case_ref(c, x)
    alloc = ref.written + GUARD
    try:
        R.check_compact(R.compact_image(R.case_ref(c, x, mutant=mutant), alloc), ref, alloc, tag=c.id)
    except AssertionError:
        return True
    return False


def _tail_valid(c):
    M = c.T * c.n
    return M % 4 != 0 and bool(R.make_mask(c.T, c.n, c.pattern).reshape(-1)[M - M % 4:].any())


# mutant -> (the cases it must be rejected on, the least number of them)
COMPACT_MUTANTS = {
    "env_major": (lambda c: c.T > 1 and c.n > 1 and c.pattern in ("prefix", "holes", "ones"), 20),                      # 1
    "drop_tail": (_tail_valid, 8),                                                                                        # 2
    "inclusive_offsets": (lambda c: c.pattern in ("prefix", "holes", "ones") and c.T * c.n > 8, 20),                                      # 3
    "carry_lost": (lambda c: (c.T, c.n) == R.BIG and c.pattern not in ("zeros", "last_entry", "last_chunk"), 5),        # 4
    "bf16_truncate": (lambda c: c.bf16 and c.pattern in ("prefix", "holes", "ones") and c.T * c.n > 8, 10),            # 5
    "ones_anyway": (lambda c: c.ones_col < 0 and c.S < c.in_pad and c.pattern in ("prefix", "holes") and c.T * c.n > 8, 4),               # 6
    "ones_shifted": (lambda c: c.ones_col > c.S and c.pattern in ("prefix", "holes") and c.T * c.n > 8, 6),            # 6
    "pad_unwritten": (lambda c: c.S < c.in_pad and c.pattern in ("prefix", "holes") and c.T * c.n > 8, 10),            # 7
    "act_transposed": (lambda c: (c.A or 0) > 1 and c.pattern in ("prefix", "holes", "ones") and c.T * c.n > 8, 10),   # 8
    "no_eps": (lambda c: c.norm_mode == 1 and c.pattern in ("prefix", "holes", "ones") and c.T * c.n > 1000, 4),       # 9
    "fused_normalise": (lambda c: c.norm_mode is not None and c.pattern in ("prefix", "holes", "ones") and c.T * c.n > 1000, 8),   # 10
}


@pytest.mark.parametrize("mutant", list(COMPACT_MUTANTS))
def test_the_checker_rejects_a_wrong_compaction(mutant):
    applies, least = COMPACT_MUTANTS[mutant]
    pool = CASES if mutant == "carry_lost" else SMALL
    hit = [c for c in pool if applies(c)]
    assert len(hit) >= least, (mutant, len(hit))
    for c in hit:
        assert _rejected(c, R.case_inputs(c), mutant), (mutant, c.id)
    for c in SMALL[:3] + SMALL[-3:]:                               # ... and accepts the restatement itself
        assert not _rejected(c, R.case_inputs(c), None)


def test_truncation_changes_a_quarter_of_the_bf16_elements():
    """Mutant 5's input condition: on the observation columns of every bf16 case with rows, truncation changes >= 25 % of the
    elements (a random mantissa: 50 %)."""
    seen = 0
    for c in SMALL:
        if not c.bf16 or c.T * c.n < 1000 or c.pattern not in ("prefix", "holes", "ones"):
            continue
        x = R.case_inputs(c)
        a, b = R.case_ref(c, x).xin[:, :c.S], R.case_ref(c, x, mutant="bf16_truncate").xin[:, :c.S]
        assert np.mean(a != b) >= 0.25, c.id
        seen += 1
    assert seen >= 10


def test_the_checker_rejects_an_unclamped_normalised_observation():                                                       # 11
    hit = [c for c in ON_CASES if not math.isinf(c.on)]
    assert len(hit) >= 4
    for c in hit:
        assert _rejected(c, R.case_inputs(c), "no_clamp"), c.id
    for c in ON_CASES:                                             # mean 0, rstd 1, no clamp: the plain entry's rows
        x = R.case_inputs(c)
        if math.isinf(c.on):
            plain = R.case_ref(c, x, obs_tab=None)
            assert R._same_bits(R.case_ref(c, x, obs_tab=R.identity_table(c.S)).xin, plain.xin)
            assert not R._same_bits(R.case_ref(c, x).xin, plain.xin)


@pytest.mark.parametrize("rows", [r for r in R.ROW_COUNTS if r >= 255])
def test_the_scatter_inputs_tell_a_fused_multiply_add(rows):                                                              # 12
    src, idx, cells = R.row_inputs(rows, 4)
    assert R.fused_share(src[:, 0], R.AFFINE_TABLE) >= 0.05
    dst = R.sentinel(np.float32, (cells,))
    good, bad = R.scatter_ref(src, idx, dst, R.AFFINE_TABLE), R.scatter_ref(src, idx, dst, R.AFFINE_TABLE, mutant="fused")
    assert not np.array_equal(R.f32_bits(good), R.f32_bits(bad))
    x = np.random.default_rng(1).standard_normal(100000).astype(np.float32)
    assert 0.15 <= R.fused_share(x, R.AFFINE_TABLE) <= 0.35        # (about 23 % on plain normals)


@pytest.mark.parametrize("mutant", ["no_tail", "round_up"])                                                             # 13, 14
def test_the_arena_check_rejects_wrong_region_ends(mutant):
    for T, n, S, A in R.BEGIN_SHAPES:
        for f64 in (False, True):
            sizes = R.region_bytes(T, n, S, A, f64)
            offs, total = R.arena_layout(sizes)
            assert any(b % 16 for b in sizes)
            with pytest.raises(AssertionError):
                R.check_arena(R.zero_regions_ref(total, offs, sizes, mutant=mutant), offs, sizes)


@pytest.mark.parametrize("T,n", R.FINISH_SHAPES)
def test_the_finish_check_rejects_summed_negative_lengths(T, n):                                                          # 15
    ln, rew = R.finish_inputs(T, n, False)
    ref, bad = R.finish_ref(ln, rew, None), R.finish_ref(ln, rew, None, mutant="negative_lengths")
    R.check_finish(ref.counters, ref)
    with pytest.raises(AssertionError):
        R.check_finish(bad.counters, ref)


@pytest.mark.parametrize("n_tensors", list(R.DIFFER_TABLES))
def test_differ_ref_compares_bits_not_values(n_tensors):                                                                  # 16
    cases = R.differ_cases(n_tensors)
    assert set(cases) == {"equal", "last_of_last", "first_of_middle", "signed_zero"}
    assert R.differ_ref(cases["equal"][0], mutant="values") == 1 != cases["equal"][1]              # NaN != NaN
    sizes = R.DIFFER_TABLES[n_tensors]
    zero = [(np.zeros(s, np.float32), np.zeros(s, np.float32)) for s in sizes]
    zero[0][1][0] = -0.0
    assert R.differ_ref(zero) == 1 and R.differ_ref(zero, mutant="values") == 0                    # +0 == -0
    if n_tensors > 1:
        assert any(b % 256 for b in np.cumsum(sizes)[:-1])         # a tensor boundary inside a 256-thread block
