"""NumPy restatements, inputs and checkers for the kernels between a rollout and the learner's first forward pass: tg_learn_count /
tg_learn_compact[_on] (which rows, in which order, with what padding), tg_scatter_rows[_affine], tg_gather_rows2,
tg_boot_values_affine, tg_rollout_begin (zero_regions_kernel), tg_rollout_finish[_stats] and tg_params_differ -- the yardstick of
test_row_kernels_cpu.py (restatements against torch, mutants against the checkers) and test_row_kernels_gpu.py (the kernels).

Every one of these kernels is exact: integer work, copies, or a handful of separately rounded IEEE operations.  So the restatements
return BIT PATTERNS (uint16 for bf16, uint32 for f32) and the checkers compare bits; the only tolerance in this file is the reward
sum's, |sum - fsum| <= (M - 1) 2^-53 sum |r| (a double sum of M terms in any order; an f32 reward is exact in f64).  A NaN compares
as "is a NaN" (the contract is that it stays one, not which payload it carries).

Shapes (T, n) of the flat time-major mask, M = T n, 1,024 entries per chunk (a workgroup: 256 threads x 4 entries):
    (1, 1)        fewer than 4 entries: load_mask4's byte path from the first thread on
    (3, 7)        M % 4 == 1
    (1, 1023)     M % 4 == 3, one chunk
    (1, 1024)     exactly one chunk
    (1, 1025)     one chunk plus a 1-entry chunk
    (5, 205)      the same M with n > 1: a thread's 4 entries wrap from one time step into the next
    (33, 1000)    33 chunks
    (257, 4099)   M % 4 == 3; 1,029 chunks > 1,024: the second trip of chunk_scan_kernel's loop; M > 256 x 2,048: the reward
                  partials' 256-block cap; tg_rollout_begin's 16-byte units exceed its grid of 16 workgroups per CU x 256 threads
check_shape_table() asserts these properties, so that an edit of the table cannot weaken them silently.

Mask patterns: episode prefixes, prefixes with holes, all zero, all one, only the last flat entry, entries in the last chunk only, a
wholly empty chunk between non-empty ones (two chunks: the empty one first), a wholly full chunk; in the largest shape the empty /
full chunks include 1,023 and 1,024, the two sides of the scan's trip boundary.  Non-zero bytes are 1, 2, 128 or 255: the kernels
test for != 0.  Row formats (S, in_pad, bf16, ones_col): FORMATS below -- in_pad 8 / 24 / 32 / 40 / 64, S == in_pad (no padding),
a ones column in the first and in a second 8-column group, none on bf16 rows.

Values are normals with full mantissas (bf16 and f32 rounding both visible); ~0.5 % of the observations are 50 times larger, beyond
the +-5 clip of the `_on` table.  src0 is 0.02 + 0.05 N(0, 1): its group std is below 0.125, where 1e-8f is more than half an ulp, so
that norm_mode 1 differs from norm_mode 0, and its mean is small against its spread, so that v - mean is inexact in f32 (the
difference of two floats of like magnitude is exact, and a fused subtract-divide would then give the same bits).  Group moments are inputs of the kernel: moments_of() sums them in f64; a group with
fewer than 2 valid entries (out of scope, as in returns_loss_fp64) gets a stand-in triple so that nothing divides by zero."""
import functools
import math
from types import SimpleNamespace

import numpy as np

import obs_norm_fp64 as ON

CHUNK = 1024
SHAPES = [(1, 1), (3, 7), (1, 1023), (1, 1024), (1, 1025), (5, 205), (33, 1000), (257, 4099)]
BIG = (257, 4099)
FORMAT_SHAPES = [(5, 205), (33, 1000)]
PATTERNS = ["prefix", "holes", "zeros", "ones", "last_entry", "last_chunk", "empty_chunk", "full_chunk"]
MULTI_CHUNK = ("last_chunk", "empty_chunk", "full_chunk")
MASK_BYTES = np.array([1, 1, 1, 2, 128, 255], dtype=np.uint8)
# (S, in_pad, bf16, ones_col)
FORMATS = [(5, 32, True, 31), (20, 32, True, 31), (32, 32, True, -1), (5, 8, False, -1), (20, 24, False, -1), (10, 32, False, -1),
           (64, 64, True, -1), (64, 64, False, -1), (33, 40, True, 39)]
SWEEP_FORMATS = [(20, 32, True, 31), (5, 8, False, -1)]       # every shape and pattern runs on these two (BIG: the second only)
ACTION_DIMS = [1, 4, 16, None]
SENTINEL_BYTE = 0xA5
GRID_CAP_ROWS = 4096 * 256                                    # scatter / gather: rows past this take the grid-stride loop
ROW_COUNTS = [0, 1, 255, 256, 257, GRID_CAP_ROWS + 3]
FINISH_SHAPES = [(1, 1), (23, 89), (2, 1024), (3, 683), BIG]  # M = 1, 2,047, 2,048, 2,049, 1,053,443
BEGIN_SHAPES = [(5, 3, 5, 1), (257, 4099, 5, 1)]              # (T, n, S, A)
DIFFER_TABLES = {1: [1000], 3: [255, 257, 1000], 64: [(1, 255, 257, 1000, 3, 64)[k % 6] for k in range(64)]}
AFFINE_TABLE = np.array([-0.4173, 1.7331, 1.0 / 1.7331, 0.0], dtype=np.float32)      # {mean, sigma, 1 / sigma, 0}


def chunks(M):
    return -(-M // CHUNK)


def sentinel(dtype, shape=()):
    """An array whose every byte is SENTINEL_BYTE."""
    dt = np.dtype(dtype)
    return np.full(int(np.prod(shape, dtype=np.int64)) * dt.itemsize, SENTINEL_BYTE, dtype=np.uint8).view(dt).reshape(shape)


def check_shape_table(cus=256):
    """What the shapes are for, asserted.  cus: the device's compute units (tg_rollout_begin launches at most 16 workgroups each)."""
    Ms = [T * n for T, n in SHAPES]
    assert Ms[:7] == [1, 21, 1023, 1024, 1025, 1025, 33000] and Ms[7] == 1053443
    assert Ms[0] < 4 and Ms[1] % 4 == 1 and Ms[2] % 4 == 3 and chunks(Ms[2]) == 1 and chunks(Ms[3]) == 1 and Ms[3] % CHUNK == 0
    assert chunks(Ms[4]) == 2 and Ms[4] % CHUNK == 1 and SHAPES[5][1] > 1 and SHAPES[5][1] % 4 != 0 and chunks(Ms[6]) == 33
    T, n = BIG
    assert SHAPES[-1] == BIG and Ms[7] % 4 == 3 and chunks(Ms[7]) == 1029 > 1024 and Ms[7] > 256 * 2048
    units = sum(-(-b // 16) for b in region_bytes(T, n, 5, 1, False))
    assert units > cus * 16 * 256, "tg_rollout_begin's grid cap is not reached"
    assert all(s in SHAPES for s in FORMAT_SHAPES) and all(f in FORMATS for f in SWEEP_FORMATS)
    assert ROW_COUNTS[-1] > GRID_CAP_ROWS and {255, 256, 257} <= set(ROW_COUNTS)
    assert [t * m for t, m in FINISH_SHAPES] == [1, 2047, 2048, 2049, 1053443]
    pads = {(p, b) for _, p, b, _ in FORMATS}
    assert (64, True) in pads and (64, False) in pads and any(S == 33 and o >= 32 for S, _, _, o in FORMATS)
    assert any(b and o == -1 for _, _, b, o in FORMATS)


def patterns_for(T, n):
    return [p for p in PATTERNS if p not in MULTI_CHUNK or T * n > CHUNK]


def chunk_counts(mask):
    flat = (np.asarray(mask).reshape(-1) != 0)
    pad = np.zeros(chunks(flat.size) * CHUNK, dtype=np.int64)
    pad[:flat.size] = flat
    return pad.reshape(-1, CHUNK).sum(1)


def chunk_sizes(M):
    return np.minimum(CHUNK, M - CHUNK * np.arange(chunks(M)))


def special_chunks(M):
    """Chunks that `empty_chunk` empties and `full_chunk` fills."""
    nc = chunks(M)
    if nc == 2:
        return [0]
    return [1] + ([1023, 1024] if nc > 1025 else [])


@functools.lru_cache(maxsize=None)
def make_mask(T, n, pattern, seed=0):
    rng = np.random.default_rng([seed, T, n, PATTERNS.index(pattern)])
    M, nc = T * n, chunks(T * n)
    if pattern in ("prefix", "holes"):
        lens = rng.integers(1, T + 1, size=n)
        m = np.arange(T)[:, None] < lens[None, :]
        if pattern == "holes":
            m &= rng.random((T, n)) > 0.15
            m[T // 3, ::5] = False
        flat = m.reshape(-1)
    elif pattern == "zeros":
        flat = np.zeros(M, dtype=bool)
    elif pattern == "ones":
        flat = np.ones(M, dtype=bool)
    elif pattern == "last_entry":
        flat = np.zeros(M, dtype=bool)
        flat[-1] = True
    elif pattern == "last_chunk":
        flat = np.zeros(M, dtype=bool)
        flat[(nc - 1) * CHUNK:] = rng.random(M - (nc - 1) * CHUNK) < 0.5
        flat[-1] = True
    else:
        assert pattern in ("empty_chunk", "full_chunk") and nc >= 2
        flat = rng.random(M) < 0.5
        flat[-1] = pattern == "empty_chunk"                        # (the last chunk: not empty there, not full here)
        for c in special_chunks(M):
            flat[c * CHUNK:(c + 1) * CHUNK] = pattern == "full_chunk"
    out = np.where(flat, rng.choice(MASK_BYTES, size=M), 0).astype(np.uint8).reshape(T, n)
    out.setflags(write=False)
    return out


def check_pattern(mask, pattern):
    """The host-side properties of the generated patterns."""
    T, n = mask.shape
    M, cnt = T * n, chunk_counts(mask)
    if pattern == "zeros":
        assert not mask.any()
    elif pattern == "ones":
        assert mask.all()
    elif pattern == "last_entry":
        assert np.flatnonzero(mask).tolist() == [M - 1]
    elif pattern == "last_chunk":
        assert not cnt[:-1].any() and cnt[-1] >= 1
    elif pattern == "empty_chunk":
        empty = np.flatnonzero(cnt == 0)
        assert empty.size >= 1 and cnt[empty[0] + 1:].any() and (chunks(M) == 2 or cnt[:empty[0]].any())
        assert all(cnt[c] == 0 for c in special_chunks(M))
    elif pattern == "full_chunk":
        assert all(cnt[c] == CHUNK for c in special_chunks(M)) and (cnt < chunk_sizes(M)).any()       # (full ones and others)
    else:
        c = int(cnt.sum())
        assert (0 < c == M or 0 < c < M) if pattern == "prefix" else (c < M and (c > 0 or M < 8))
    if int(cnt.sum()) >= 16:
        assert len(set(np.unique(mask).tolist()) - {0, 1}) >= 1, "non-zero mask bytes other than 1"


@functools.lru_cache(maxsize=8)
def make_inputs(T, n, S, A, obs_f64, seed=0):
    """obs [S][T + 1][n] f32 / f64, act [A][T][n] f32 (A None: none), src0 / src1 [T][n] f32."""
    rng = np.random.default_rng([seed, T, n, S, A or 0, int(obs_f64)])
    obs = rng.standard_normal((S, T + 1, n))
    obs *= np.where(rng.random(obs.shape) < 0.005, 50.0, 1.0)
    obs = obs if obs_f64 else obs.astype(np.float32)
    act = None if A is None else rng.standard_normal((A, T, n)).astype(np.float32)
    src0 = (0.02 + 0.05 * rng.standard_normal((T, n))).astype(np.float32)
    src1 = rng.standard_normal((T, n)).astype(np.float32)
    for a in (obs, act, src0, src1):
        if a is not None:
            a.setflags(write=False)
    return SimpleNamespace(obs=obs, act=act, src0=src0, src1=src1)


def with_nan(obs, mask):
    """A copy of obs with a NaN in the last feature of the middle valid entry (none valid: obs itself); -> (obs, flat entry or None)."""
    idx = np.flatnonzero(mask)
    if idx.size == 0:
        return obs, None
    f = int(idx[idx.size // 2])
    T, n = mask.shape
    out = obs.copy()
    out[-1, f // n, f % n] = np.nan
    return out, f


def obs_table(S, seed=0):
    """f32 [2][S] = {mean, rstd} of an ObsNorm, nothing a power of two."""
    rng = np.random.default_rng([seed, S, 77])
    return np.stack([0.3 * rng.standard_normal(S), 1.0 / (0.5 + np.abs(rng.standard_normal(S)))]).astype(np.float32)


def identity_table(S):
    return np.stack([np.zeros(S, np.float32), np.ones(S, np.float32)])


def group_sizes(n):
    """n itself and, where n has one, its largest proper divisor > 1 that is no multiple of 4."""
    ds = [d for d in range(n - 1, 1, -1) if n % d == 0 and d % 4 != 0]
    return [n] + ds[:1]


STAND_IN = (7.0, 0.2, 0.03)                        # {count, sum, sum of squares} of a group with < 2 valid entries: mean 0.029, std 0.064


def moments_of(x, mask, group_size):
    """f64 [n / group_size][3] = {count, sum, sum of squares} over the valid entries of each group of envs."""
    T, n = x.shape
    G = n // group_size
    w = (mask != 0).reshape(T, G, group_size)
    xg = np.where(w, x.astype(np.float64).reshape(T, G, group_size), 0.0)
    out = np.stack([w.sum((0, 2)).astype(np.float64), xg.sum((0, 2)), (xg * xg).sum((0, 2))], axis=1)
    bad = out[:, 0] < 2
    out[bad] = STAND_IN
    var = (out[:, 2] - out[:, 1] * (out[:, 1] / out[:, 0])) / (out[:, 0] - 1.0)
    out[~bad & ~(var > 1e-6)] = STAND_IN           # (constant values: out of scope)
    return out


def group_normalize_rows(v, env, moments, mode, group_size, mutant=None):
    """compact_rows_body's normalisation of src0 values v f32 [R] of envs env [R]: mean = s1 / cnt, var = (s2 - s1 mean) / (cnt - 1)
    in f64, then (float) mean, (float) sqrt(var), den = std (mode 0) or std + 1e-8f (mode 1), (v - mean) / den -- every f32
    operation rounded on its own (group_normalize_kernel's arithmetic, returns_loss_fp64's "Group normalisation")."""
    mo = moments[np.asarray(env) // group_size]
    cnt, s1, s2 = mo[:, 0], mo[:, 1], mo[:, 2]
    mean = s1 / cnt
    var = (s2 - s1 * mean) / (cnt - 1.0)
    meanf = mean.astype(np.float32)
    stdf = np.sqrt(np.where(var > 0.0, var, np.where(np.isnan(var), var, 0.0))).astype(np.float32)
    den = stdf if mode == 0 or mutant == "no_eps" else (stdf + np.float32(1e-8)).astype(np.float32)
    v = np.asarray(v, dtype=np.float32)
    if mutant == "fused_normalise":
        return ((v.astype(np.float64) - meanf.astype(np.float64)) / den.astype(np.float64)).astype(np.float32)
    return ((v - meanf).astype(np.float32) / den).astype(np.float32)


def bf16_bits(x32, truncate=False):
    """f32 -> the bf16 bit pattern (uint16), round to nearest even (truncate: the WRONG conversion of the mutation tests)."""
    u = np.ascontiguousarray(x32, dtype=np.float32).view(np.uint32)
    if truncate:
        return (u >> 16).astype(np.uint16)
    r = ((u + (np.uint32(0x7FFF) + ((u >> 16) & np.uint32(1)))) >> 16).astype(np.uint16)
    return np.where(np.isnan(x32), np.uint16(0x7FC0) | (u >> 16).astype(np.uint16), r).astype(np.uint16)


def f32_bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def compact_ref(mask, obs, act, src0, src1, moments, norm_mode, group_size, in_pad, bf16, ones_col, obs_tab, clip, rows_cap, mutant=None):
    """tg_learn_count + tg_learn_compact[_on], restated.  -> namespace: offsets uint32 [chunks] (exclusive), total, written =
    min(total, rows_cap), idx int64 [written] (ascending flat indices of the non-zero mask bytes), xin uint16 / uint32 [written]
    [in_pad] (bit patterns), act_rows uint32 [written][A] or None, dst0 / dst1 uint32 [written] or None.  Rows >= written are "not
    written".  mutant: one of the WRONG kernels of test_row_kernels_cpu.py."""
    T, n = mask.shape
    M, S = T * n, obs.shape[0]
    flat = np.asarray(mask).reshape(-1) != 0
    if mutant == "drop_tail" and M % 4:
        flat = flat.copy()
        flat[M - M % 4:] = False
    counts = chunk_counts(flat)
    inclusive = np.cumsum(counts)
    offsets = inclusive - counts
    total = int(inclusive[-1])
    if mutant == "inclusive_offsets":
        offsets = inclusive
    if mutant == "carry_lost" and counts.size > 1024:
        offsets = offsets.copy()
        offsets[1024:] -= offsets[1024]
        total = int(counts[1024:].sum())
    idx = np.flatnonzero(flat).astype(np.int64)
    if mutant == "env_major":
        idx = (lambda e, t: t * n + e)(*np.nonzero(flat.reshape(T, n).T)).astype(np.int64)
    written = min(total, int(rows_cap))
    idx = idx[:written]
    x32 = np.asarray(obs)[:, :T, :].reshape(S, M)[:, idx].T.astype(np.float32)           # an f64 observation: rounded to f32 first
    if obs_tab is not None:
        x32 = ON.normalize(x32, obs_tab, None if (mutant == "no_clamp" or math.isinf(clip)) else clip)
    rows = np.zeros((written, in_pad), dtype=np.float32)
    rows[:, :S] = x32
    one = ones_col
    if mutant == "ones_anyway" and ones_col < 0 and S < in_pad:
        one = in_pad - 1
    if mutant == "ones_shifted" and ones_col > S:
        one = ones_col - 1
    if one >= 0:
        rows[:, one] = 1.0
    xin = bf16_bits(rows, truncate=mutant == "bf16_truncate") if bf16 else f32_bits(rows)
    if mutant == "pad_unwritten":
        xin = xin.copy()
        xin[:, S:] = sentinel(xin.dtype)
    out = SimpleNamespace(offsets=offsets.astype(np.uint32), total=total, written=written, idx=idx, xin=xin, act_rows=None, dst0=None, dst1=None,
                          in_pad=in_pad, bf16=bf16)
    if act is not None:
        A = act.shape[0]
        a = act.reshape(A, M)
        out.act_rows = f32_bits(a.reshape(-1)[idx[:, None] * A + np.arange(A)] if mutant == "act_transposed" else a[:, idx].T)
    if src0 is not None:
        v = src0.reshape(-1)[idx]
        if moments is not None:
            v = group_normalize_rows(v, idx % n, moments, norm_mode, group_size, mutant)
        out.dst0 = f32_bits(v)
    if src1 is not None:
        out.dst1 = f32_bits(src1.reshape(-1)[idx])
    return out


COMPACT_BUFFERS = ("idx", "xin", "act_rows", "dst0", "dst1")


def capped(ref, rows_cap):
    """The same compaction under another row capacity: rows >= min(total, rows_cap) are not written."""
    out = SimpleNamespace(**vars(ref))
    out.written = min(ref.total, int(rows_cap))
    assert out.written <= ref.written
    return out


def compact_image(ref, rows_alloc):
    """What a kernel that computed `ref` leaves in sentinel-filled buffers of rows_alloc rows (and the count workspace, whose 4
    spare words it never touches): name -> array."""
    img = {"offsets": np.concatenate([ref.offsets, sentinel(np.uint32, (4,))]), "total": ref.total}
    for name in COMPACT_BUFFERS:
        a = getattr(ref, name)
        if a is None:
            continue
        buf = sentinel(a.dtype, (rows_alloc,) + a.shape[1:])
        buf[:ref.written] = a[:ref.written]
        img[name] = buf
    return img


def _same_bits(got, want):
    """Bit-equal, or NaN where NaN is expected (uint16: bf16 patterns, uint32: f32 patterns; int64: plain equality)."""
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if np.array_equal(got, want):
        return True
    if want.dtype == np.uint16:
        nan = lambda a: ((a & 0x7F80) == 0x7F80) & ((a & 0x007F) != 0)
    elif want.dtype == np.uint32:
        nan = lambda a: ((a & 0x7F800000) == 0x7F800000) & ((a & 0x007FFFFF) != 0)
    else:
        return False
    return bool(np.all((got == want) | (nan(got) & nan(want))))


def check_compact(got, ref, rows_alloc, tag="compact"):
    """got: name -> array as compact_image() lays them out (what came back from the device, guard rows included)."""
    want = compact_image(ref, rows_alloc)
    assert set(got) == set(want), (tag, sorted(got), sorted(want))
    assert int(got["total"]) == want["total"], f"{tag}: total {int(got['total'])}, want {want['total']}"
    for name, w in want.items():
        if name == "total":
            continue
        g = np.asarray(got[name])
        if not _same_bits(g, w):
            bad = np.flatnonzero((g != w).reshape(g.shape[0], -1).any(1)) if g.shape == w.shape else []
            where = f"first at row {int(bad[0])} of {g.shape[0]} ({ref.written} written)" if len(bad) else f"shape {g.shape} / {w.shape}"
            raise AssertionError(f"{tag}: {name} differs, {where}")


# ------------------------------------------------------------------------------------------------------------------------------
# the cases both test modules run
# ------------------------------------------------------------------------------------------------------------------------------
def _case(i, T, n, pattern, fmt, big=False, on=None):
    """Case number i: the action width, the observation dtype, the per-row scalars, the normalisation mode and the group size cycle
    with i, so that the sweep meets every value of each without running their product.  on: None or the `_on` clip."""
    S, in_pad, bf16, ones_col = fmt
    srcs = ("both", "src0", "none")[i % 3]
    gs = group_sizes(n)
    c = SimpleNamespace(T=T, n=n, pattern=pattern, S=S, in_pad=in_pad, bf16=bf16, ones_col=ones_col, A=1 if big else ACTION_DIMS[i % 4],
                        obs_f64=False if big else bool(i % 2), srcs=srcs, norm_mode=None if srcs == "none" else (0, 1, None)[(i // 3) % 3],
                        group_size=gs[(i // 2) % len(gs)], on=on)
    c.id = (f"{T}x{n}-{pattern}-S{S}p{in_pad}{'bf16' if bf16 else 'f32'}o{ones_col}-A{c.A}-{'f64' if c.obs_f64 else 'f32'}-{srcs}"
            f"-m{c.norm_mode}g{c.group_size}" + ("" if on is None else f"-on{on}"))
    return c


def compact_cases():
    """Every shape and mask pattern on the two SWEEP_FORMATS (BIG: S = 5, A = 1 only), then every row format on FORMAT_SHAPES."""
    out = []
    for T, n in SHAPES:
        for fmt in SWEEP_FORMATS:
            if (T, n) == BIG and fmt[0] != 5:
                continue
            for pattern in patterns_for(T, n):
                out.append(_case(len(out), T, n, pattern, fmt, big=(T, n) == BIG))
    for fmt in FORMATS:
        for T, n in FORMAT_SHAPES:
            for pattern in ("holes", "prefix"):
                out.append(_case(len(out), T, n, pattern, fmt))
    return out


def on_cases():
    """tg_learn_compact_on: a finite clip and +inf, f32 and f64 observations, bf16 and f32 rows."""
    out = []
    for fmt in ((20, 32, True, 31), (5, 8, False, -1), (33, 40, True, 39), (64, 64, False, -1)):
        for T, n in FORMAT_SHAPES:
            for clip in (5.0, math.inf):
                out.append(_case(len(out), T, n, "holes", fmt, on=clip))
    return out


def case_inputs(c):
    """-> namespace: mask, obs, act, src0, src1, moments (None where the case has none), obs_tab, nan_at (flat entry or None)."""
    mask = make_mask(c.T, c.n, c.pattern)
    x = make_inputs(c.T, c.n, c.S, c.A, c.obs_f64)
    src0 = x.src0 if c.srcs in ("both", "src0") else None
    src1 = x.src1 if c.srcs == "both" else None
    moments = moments_of(src0, mask, c.group_size) if src0 is not None and c.norm_mode is not None else None
    obs, nan_at, tab = x.obs, None, None
    if c.on is not None:
        obs, nan_at = with_nan(obs, mask)
        tab = obs_table(c.S)
    return SimpleNamespace(mask=mask, obs=obs, act=x.act, src0=src0, src1=src1, moments=moments, obs_tab=tab, nan_at=nan_at)


def case_ref(c, x, rows_cap=None, mutant=None, obs_tab="case"):
    return compact_ref(x.mask, x.obs, x.act, x.src0, x.src1, x.moments, c.norm_mode or 0, c.group_size, c.in_pad, c.bf16, c.ones_col,
                       x.obs_tab if isinstance(obs_tab, str) else obs_tab, c.on if c.on is not None else math.inf,
                       c.T * c.n if rows_cap is None else rows_cap, mutant)


# ------------------------------------------------------------------------------------------------------------------------------
# scatter, gather, bootstrap values
# ------------------------------------------------------------------------------------------------------------------------------
def affine_ref(v, table, mutant=None):
    """v * table[1] + table[0] in f32, the multiply and the add each rounded on its own (fused: the WRONG single rounding)."""
    v = np.asarray(v, dtype=np.float32)
    if mutant == "fused":
        return (v.astype(np.float64) * np.float64(table[1]) + np.float64(table[0])).astype(np.float32)
    return ((v * np.float32(table[1])).astype(np.float32) + np.float32(table[0])).astype(np.float32)


def scatter_ref(src, idx, dst, table=None, mutant=None):
    """dst.flat[idx[r]] = src[r][0] (table: affine_ref of it); -> a copy of dst, entries outside idx untouched."""
    out = np.array(dst, copy=True).reshape(-1)
    v = np.asarray(src)[:len(idx), 0]
    out[idx] = v if table is None else affine_ref(v, table, mutant)
    return out.reshape(np.shape(dst))


def gather2_ref(idx, src0, dst0, src1=None, dst1=None):
    """dst0[r] = src0.flat[idx[r]] (and dst1 / src1) for r < len(idx); -> copies, rows past len(idx) untouched."""
    outs = []
    for s, d in ((src0, dst0), (src1, dst1)):
        if s is None:
            outs.append(None)
            continue
        o = np.array(d, copy=True)
        o[:len(idx)] = np.asarray(s).reshape(-1)[idx]
        outs.append(o)
    return outs


def boot_affine_ref(v, timeout, table):
    """(v * table[1] + table[0]) * (float) timeout: three separately rounded f32 operations."""
    return (affine_ref(v, table) * np.asarray(timeout).astype(np.float32)).astype(np.float32)


@functools.lru_cache(maxsize=4)
def row_inputs(rows, stride, seed=0):
    """src f32 [rows][stride] (column 0 is read), idx: a random strictly increasing subset of [0, cells), cells."""
    rng = np.random.default_rng([seed, rows, stride])
    cells = rows + rows // 3 + 17
    keep = np.zeros(cells, dtype=bool)
    keep[rng.permutation(cells)[:rows]] = True
    idx = np.flatnonzero(keep).astype(np.int64)
    assert idx.size == rows and (rows < 2 or bool((idx[1:] > idx[:-1]).all()))
    src = (3.0 * rng.standard_normal((rows, stride))).astype(np.float32)
    return src, idx, cells


def fused_share(v, table):
    """The share of values whose fused multiply-add differs from the two separately rounded operations."""
    return float(np.mean(f32_bits(affine_ref(v, table)) != f32_bits(affine_ref(v, table, "fused")))) if len(v) else 0.0


# ------------------------------------------------------------------------------------------------------------------------------
# tg_rollout_begin
# ------------------------------------------------------------------------------------------------------------------------------
def region_bytes(T, n, S, A, f64):
    """Bytes of obs [S][T + 1][n], act f32 [A][T][n], rew [T][n], mask u8 [T][n], len i32 [n], counters u64 [4]."""
    rs = 8 if f64 else 4
    return [S * (T + 1) * n * rs, A * T * n * 4, T * n * rs, T * n, n * 4, 32]


def arena_layout(sizes, guard=32):
    """16-byte-aligned offsets of the regions inside one arena with at least `guard` bytes between them; -> (offsets, arena bytes)."""
    offs, at = [], -(-guard // 16) * 16
    for b in sizes:
        offs.append(at)
        at = -(-(at + b + guard) // 16) * 16
    return offs, at + guard


def zero_regions_ref(arena_bytes, offsets, sizes, mutant=None):
    """The arena after tg_rollout_begin: SENTINEL_BYTE everywhere but 0 in [offset, offset + size) of every region."""
    out = np.full(arena_bytes, SENTINEL_BYTE, dtype=np.uint8)
    for o, b in zip(offsets, sizes):
        if mutant == "no_tail":
            b = b // 16 * 16
        elif mutant == "round_up":
            b = -(-b // 16) * 16
        out[o:o + b] = 0
    return out


def check_arena(got, offsets, sizes, tag="rollout_begin"):
    want = zero_regions_ref(got.size, offsets, sizes)
    bad = np.flatnonzero(np.asarray(got) != want)
    if bad.size:
        b = int(bad[0])
        k = max([i for i, o in enumerate(offsets) if o <= b], default=-1)
        raise AssertionError(f"{tag}: byte {b} is {int(got[b]):#x}, want {int(want[b]):#x} (region {k}: offset {offsets[k]}, {sizes[k]} bytes)")


# ------------------------------------------------------------------------------------------------------------------------------
# tg_rollout_finish[_stats]
# ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def finish_inputs(T, n, f64, seed=0):
    """len i32 [n]: values in [1, T], zeros and negatives (a running Pendulum slot holds minus its balanced steps); rew [T][n]."""
    rng = np.random.default_rng([seed, T, n, int(f64)])
    ln = rng.integers(1, T + 1, size=n).astype(np.int32)
    kind = rng.random(n)
    ln[kind < 0.2] = 0
    ln[kind > 0.8] = -rng.integers(1, T + 1, size=int((kind > 0.8).sum())).astype(np.int32)
    if n >= 3:
        ln[:3] = (-max(T // 2, 1), 0, T)
    else:
        ln[0] = -1
    rew = rng.standard_normal((T, n))
    return ln, (rew if f64 else rew.astype(np.float32))


def finish_ref(ln, rew, rng, mutant=None):
    """-> namespace: counters (steps, ended) as Python ints mod 2^64, stats[1:3], the RNG pair afterwards (rng None: None), the
    reward sum by math.fsum and the bound of a double sum of its M terms in any order."""
    ln = np.asarray(ln).astype(np.int64)
    steps = int(ln.sum()) % 2 ** 64 if mutant == "negative_lengths" else int(np.maximum(ln, 0).sum())
    r = np.asarray(rew, dtype=np.float64).reshape(-1)
    return SimpleNamespace(counters=(steps, int((ln > 0).sum())), stats1=float(ln.size), stats2=float(steps),
                           rng=None if rng is None else (int(rng[0]), (int(rng[1]) + 1) % 2 ** 64),
                           reward_sum=math.fsum(r.tolist()), reward_bound=(r.size - 1) * 2.0 ** -53 * math.fsum(np.abs(r).tolist()))


def check_finish(counters, ref, tag="finish"):
    assert (int(counters[0]), int(counters[1])) == ref.counters, f"{tag}: counters {int(counters[0])}, {int(counters[1])}, want {ref.counters}"


# ------------------------------------------------------------------------------------------------------------------------------
# tg_params_differ
# ------------------------------------------------------------------------------------------------------------------------------
def differ_ref(pairs, mutant=None):
    """1 when any element of any pair differs in its BITS (values: the WRONG comparison -- NaN != NaN, +0 == -0)."""
    if mutant == "values":
        return int(any(bool(np.any(a != b)) for a, b in pairs))
    return int(any(bool(np.any(f32_bits(a) != f32_bits(b))) for a, b in pairs))


def differ_cases(n_tensors, seed=0):
    """name -> (pairs, expected flag): tensors of DIFFER_TABLES[n_tensors] elements each, boundaries inside 256-thread blocks."""
    sizes = DIFFER_TABLES[n_tensors]
    assert len(sizes) == n_tensors and any(s % 256 for s in np.cumsum(sizes)[:-1]) or n_tensors == 1
    rng = np.random.default_rng([seed, n_tensors])
    base = [rng.standard_normal(s).astype(np.float32) for s in sizes]
    base[-1][0] = np.nan                                           # equal bits on both sides: no difference
    base[0][-1] = np.float32(-0.0)
    same = lambda: [(a.copy(), a.copy()) for a in base]
    mid = n_tensors // 2
    cases = {"equal": same(), "last_of_last": same(), "first_of_middle": same(), "signed_zero": same()}
    a, b = cases["last_of_last"][-1]
    b[-1] = np.nextafter(a[-1] if np.isfinite(a[-1]) else np.float32(1.0), np.float32(9.0))
    a, b = cases["first_of_middle"][mid]
    b[0] = np.float32(1.0) if np.isnan(a[0]) else np.nextafter(a[0], np.float32(9.0))
    a, b = cases["signed_zero"][0]
    a[a.size // 2], b[a.size // 2] = np.float32(0.0), np.float32(-0.0)
    want = {"equal": 0, "last_of_last": 1, "first_of_middle": 1, "signed_zero": 1}
    for name, pairs in cases.items():
        diff = sum(int(np.sum(f32_bits(x) != f32_bits(y))) for x, y in pairs)
        assert diff == want[name], (name, diff)                    # exactly one element differs, or none
        assert differ_ref(pairs) == want[name]
    return {name: (pairs, want[name]) for name, pairs in cases.items()}
