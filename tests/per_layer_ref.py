"""NumPy restatements, inputs, case tables and checkers for the five kernels of csrc/mlp_kernels.hip that GemmMLP._backward_relu (the
per-layer learner: every ReLU net outside the tuned chain shapes) runs beside library GEMMs: tg_relu_bwd_bias, tg_head_bwd_relu_bias,
tg_dw_finish, tg_colsum_finish, tg_head_prep -- the yardstick of test_per_layer_cpu.py (restatements against torch, planted wrong
kernels against the checkers) and test_per_layer_gpu.py (the kernels).

Two input families.

INTEGER inputs: every operand is a small integer (dA, dout, W_head, partials, tail operands, bucket contents in {-3 .. 3}; an
activation is one of a few positive values or +0 / -0 / -1).  Every product is then exact, every bf16 rounding is exact (|v| <= 72
< 256), and an fp32 sum is exact in any order as long as sum |terms| < 2^24 per output -- assert_exact() checks that from the
reference's own absolute sums on every case.  The checker is check_image(): BITWISE equality of every buffer the kernel may write,
guard words included.  Rows carry a nonzero passed AND a nonzero masked entry in every thread's column group (make_acts / make_dA), and
partials and tail operands have no zero at all, so that a dropped, doubled or misplaced row or batch changes the result.

REAL inputs, for the rounding itself.  The fp64 reference is formed from the kernel's own inputs:
  * tg_relu_bwd_bias copies or zeroes: dZ is held bit for bit to where(a > 0, dA, +0) in both families.
  * tg_head_bwd_relu_bias forms s = sum_{k<A} d_k w_k in fp32, A multiplications and A additions (the first onto 0, exact), or A
    fused multiply-adds: at most 2 A - 1 roundings of partial results, each bounded by 2^-24 sum_k |d_k w_k| (1 + O(2^-23)), so
    |s - ref| <= A 2^-23 sum_k |d_k| |w_k| covers either contraction.  In bf16 the stored value is one round-to-nearest-even of s and
    rounding is monotone: stored in [RNE(ref - b), RNE(ref + b)] (head_interval(): the fp64 ends are first moved OUTWARD to fp32).
  * a partial row is an fp32 sum of the n values a block wrote, in some order (one chain per thread, then the threads in order):
    |partial - sum| <= (n - 1) 2^-24 sum |v| (1 + 2^-14) -- the factor covers the second-order terms for n <= 2^9 per chain.
  * tg_head_prep rounds once: its bf16 dZ is the RNE of dout bit for bit, its fp32 dZ is dout.
  * the rounding-mode probe (rne_probe()): A = 1, dout = 1, weights that are the exact fp32 midpoints between bf16 neighbours (even and
    odd lower neighbour, both signs) and the fp32 values just below and above them: s = w exactly, the stored bf16 must be RNE(w).

Mask bits: cols bits per row as tg_mlp_forward_chain writes them, [lane half h][cols / 64 words]; feature 32 mt + 16 h + r is bit
(mt & 1) 8 + (r >> 1) + 16 (r & 1) of word h (cols / 64) + (mt >> 1) (pack_mask_bits / unpack_mask_bits; the layout test_gpu_parity's
_pack_mask_bits documents).

Launch shapes restated: a workgroup of 256 threads, `per` columns per thread (8, or 4 in tg_relu_bwd_bias's fp32 form), tpr = cols /
per threads per row, rpp = 256 / tpr rows per pass (threads >= tpr rpp idle), 2,048 workgroups, block (r / rpp) % 2048 owns row r;
tg_head_prep: 1,024 workgroups of 256 rows.  Every block writes its partial row, also one that owns no rows (zeros)."""
import functools
from types import SimpleNamespace

import numpy as np

import row_kernels_ref as RK

THREADS, BLOCKS, PREP_BLOCKS = 256, 2048, 1024
G = 64                                                            # guard words on either side of every buffer (16-byte multiples)
NAN32, NAN16 = np.uint32(0x7FC00000), np.uint16(0x7FC0)
TWO24 = float(2 ** 24)
NONZERO = np.array([-3, -2, -1, 1, 2, 3], dtype=np.float64)

# activation bit patterns: passed (> 0) -- 1.0, 2.5, the smallest positive subnormal, the smallest positive normal; masked -- +0, -0, -1.0
POS_BITS = {True: np.array([0x3F80, 0x4020, 0x0001, 0x0080], dtype=np.uint16),
            False: np.array([0x3F800000, 0x40200000, 0x00000001, 0x00800000], dtype=np.uint32)}
NEG_BITS = {True: np.array([0x0000, 0x8000, 0xBF80], dtype=np.uint16), False: np.array([0x00000000, 0x80000000, 0xBF800000], dtype=np.uint32)}


def per_of(bf16, head=False):
    return 8 if (bf16 or head) else 4


def rpp_of(cols, per):
    return THREADS // (cols // per)


def row_counts(cols, per):
    r = rpp_of(cols, per)
    return sorted({0, 1, r - 1, r, r + 1, BLOCKS * r - 1, BLOCKS * r + 1})


def from_bits(bits):
    """uint16 (bf16) / uint32 (f32) patterns -> float32 values."""
    bits = np.asarray(bits)
    return (bits.astype(np.uint32) << 16).view(np.float32) if bits.dtype == np.uint16 else bits.view(np.float32)


def to_bits(x, bf16, truncate=False):
    x32 = np.ascontiguousarray(x, dtype=np.float32)
    return RK.bf16_bits(x32, truncate=truncate) if bf16 else RK.f32_bits(x32)


def nan_bits(n, bf16):
    return np.full(int(n), NAN16 if bf16 else NAN32, dtype=np.uint16 if bf16 else np.uint32)


def guarded(bits):
    """[G NaN words | bits | G NaN words], flat: what a kernel leaves in a buffer allocated between guards."""
    bits = np.asarray(bits).reshape(-1)
    g = nan_bits(G, bits.dtype == np.uint16)
    return np.concatenate([g, bits, g])


def block_sums(v, rows_per_block, n_blocks):
    """f64 [n_blocks][cols]: block (r / rows_per_block) % n_blocks sums row r of v [rows][cols]."""
    v = np.asarray(v, dtype=np.float64)
    rows, cols = v.shape
    groups = -(-rows // rows_per_block) if rows else 0
    trips = max(-(-groups // n_blocks), 1)
    pad = np.zeros((trips * n_blocks * rows_per_block, cols))
    pad[:rows] = v
    return pad.reshape(trips, n_blocks, rows_per_block, cols).sum((0, 2))


def block_counts(rows, rows_per_block, n_blocks):
    return block_sums(np.ones((rows, 1)), rows_per_block, n_blocks)[:, 0]


def assert_exact(*abs_sums):
    """The exactness condition of the integer family: sum |terms| < 2^24 on every output."""
    for s in abs_sums:
        s = np.asarray(s)
        assert s.size == 0 or float(s.max()) < TWO24, float(s.max())


def check_image(got, want, tag=""):
    """Bitwise equality of every buffer (name -> flat unsigned array, guards included)."""
    assert set(got) == set(want), (tag, sorted(got), sorted(want))
    for name, w in want.items():
        g = np.asarray(got[name]).reshape(-1)
        w = np.asarray(w).reshape(-1)
        assert g.dtype == w.dtype and g.shape == w.shape, (tag, name, g.dtype, w.dtype, g.shape, w.shape)
        bad = np.flatnonzero(g != w)
        if bad.size:
            b = int(bad[0])
            where = "guard before" if b < G else ("guard after" if b >= g.size - G else f"element {b - G} of {g.size - 2 * G}")
            raise AssertionError(f"{tag}: {name} differs at {bad.size} words, first at {where}: {int(g[b]):#x}, want {int(w[b]):#x}")


# ------------------------------------------------------------------------------------------------------------------------------
# masks
# ------------------------------------------------------------------------------------------------------------------------------
def mask_of(a_bits, mutant=None):
    """a > 0 as IEEE compares it (+0, -0 and negatives masked; subnormals passed)."""
    a = from_bits(a_bits)
    if mutant == "neg_zero_positive":
        return (np.asarray(a_bits) != 0) & ~(a < 0)               # the WRONG test "any bit set and not below zero": -0 passes
    m = a > 0
    if mutant == "mask_shift":
        m = np.roll(m, 1, axis=1)
    return m


def _bit_places(cols, swapped=False):
    f = np.arange(cols)
    mt, h, r = f >> 5, (f >> 4) & 1, f & 15
    if swapped:
        h = 1 - h
    return h * (cols // 64) + (mt >> 1), (mt & 1) * 8 + (r >> 1) + 16 * (r & 1)


def pack_mask_bits(mask):
    """bool [rows][cols] -> uint32 [rows][cols / 32] in tg_mlp_forward_chain's layout (cols a multiple of 64)."""
    rows, cols = mask.shape
    word, bit = _bit_places(cols)
    out = np.zeros((rows, cols // 32), dtype=np.uint32)
    for w in range(cols // 32):
        sel = word == w
        out[:, w] = (mask[:, sel].astype(np.uint32) << bit[sel].astype(np.uint32)[None, :]).sum(1, dtype=np.uint32)
    return out


def unpack_mask_bits(words, cols, mutant=None):
    word, bit = _bit_places(cols, swapped=mutant == "halves_swapped")
    return ((np.asarray(words)[:, word] >> bit.astype(np.uint32)[None, :]) & 1).astype(bool)


def _forced(rows, cols, per):
    """Per row and column group: the column that is passed with a nonzero value (j0) and the one that is masked with one (j1)."""
    c = np.arange(cols)
    j0 = (np.arange(rows)[:, None] + (c // per)[None, :]) % per
    j = (c % per)[None, :]
    return j == j0, j == (j0 + 1) % per


def make_acts(rng, rows, cols, per, bf16):
    """-> (activation bit patterns [rows][cols], the mask a > 0)."""
    on, off = _forced(rows, cols, per)
    mask = np.where(on, True, np.where(off, False, rng.random((rows, cols)) < 0.5))
    pos, neg = POS_BITS[bf16], NEG_BITS[bf16]
    bits = np.where(mask, pos[rng.integers(0, pos.size, size=(rows, cols))], neg[rng.integers(0, neg.size, size=(rows, cols))])
    # the forced entries cycle through the special values: -0 / +0 masked, every passed pattern in turn (a one-row case has a -0 too)
    cyc = np.arange(rows)[:, None] + (np.arange(cols) // per)[None, :]
    bits = np.where(off, neg[(cyc + 1) % 2], np.where(on, pos[cyc % pos.size], bits))
    return bits.astype(pos.dtype), mask


def make_dA(rng, rows, cols, per, real):
    """f32 [rows][cols]: integers in {-3 .. 3}, nonzero where _forced() says so -- or N(0, 1) values (real)."""
    if real:
        return rng.standard_normal((rows, cols)).astype(np.float32)
    on, off = _forced(rows, cols, per)
    return np.where(on | off, rng.choice(NONZERO, size=(rows, cols)), rng.integers(-3, 4, size=(rows, cols))).astype(np.float32)


def _processed(rows, rpp, mutant):
    """Which rows a (wrong) kernel handles."""
    keep = np.ones(rows, dtype=bool)
    if mutant == "drop_last_row" and rows:
        keep[-1] = False
    if mutant == "drop_wrap_row" and rows > BLOCKS * rpp:
        keep[BLOCKS * rpp] = False
    return keep


def _partials(dz_bits, keep, rows_per_block, n_blocks, mutant):
    """-> (f32 bit patterns [n_blocks][cols] of the block sums, f64 sums, f64 sums of magnitudes, rows per block)."""
    v = np.where(keep[:, None], from_bits(dz_bits).astype(np.float64), 0.0)
    p64, abs64 = block_sums(v, rows_per_block, n_blocks), block_sums(np.abs(v), rows_per_block, n_blocks)
    n = block_counts(v.shape[0], rows_per_block, n_blocks)
    bits = RK.f32_bits(p64.astype(np.float32)).copy()
    if mutant == "partial_unwritten":
        bits[n == 0] = NAN32                                       # a block that owns no rows returns early: the prefill stays
    return bits, p64, abs64, n


# ------------------------------------------------------------------------------------------------------------------------------
# tg_relu_bwd_bias
# ------------------------------------------------------------------------------------------------------------------------------
RELU_COLS = {True: [8, 24, 96, 136, 2048], False: [4, 12, 96, 1000, 1024]}


def relu_cases():
    return [SimpleNamespace(bf16=bf, cols=c, rows=r, id=f"{'bf16' if bf else 'f32'}-c{c}-r{r}")
            for bf in (True, False) for c in RELU_COLS[bf] for r in row_counts(c, per_of(bf))]


@functools.lru_cache(maxsize=2)
def relu_inputs(bf16, cols, rows, real=False):
    rng = np.random.default_rng([11, int(bf16), cols, rows, int(real)])
    per = per_of(bf16)
    a_bits, mask = make_acts(rng, rows, cols, per, bf16)
    dA_bits = to_bits(make_dA(rng, rows, cols, per, real), bf16)
    return SimpleNamespace(bf16=bf16, cols=cols, rows=rows, a_bits=a_bits, dA_bits=dA_bits, mask=mask, rpp=rpp_of(cols, per))


def relu_ref(x, mutant=None):
    """dZ = where(a > 0, dA, +0) in place, partial[b] = the column sums of block b's rows."""
    keep = _processed(x.rows, x.rpp, mutant)
    mask = mask_of(x.a_bits, mutant)
    dz = np.where(keep[:, None], np.where(mask, x.dA_bits, 0), x.dA_bits).astype(x.dA_bits.dtype)
    pbits, p64, abs64, n = _partials(dz, keep, x.rpp, BLOCKS, mutant)
    return SimpleNamespace(dz_bits=dz, partial_bits=pbits, p64=p64, abs64=abs64, n=n)


def relu_image(ref, mutant=None):
    img = {"dz": guarded(ref.dz_bits), "partial": guarded(ref.partial_bits)}
    if mutant == "guard_overwrite":
        img["dz"][G + ref.dz_bits.size] = 0
    return img


def partial_bound(abs64, n):
    return np.maximum(n - 1, 0)[:, None] * 2.0 ** -24 * abs64 * (1 + 2.0 ** -14)


def check_partial_real(got_partial_bits, got_dz_bits, rows_per_block, n_blocks, tag=""):
    """The partial rows against the fp64 block sums of what the kernel itself wrote; -> worst error / bound."""
    v = from_bits(got_dz_bits).astype(np.float64)
    p64, abs64 = block_sums(v, rows_per_block, n_blocks), block_sums(np.abs(v), rows_per_block, n_blocks)
    bound = partial_bound(abs64, block_counts(v.shape[0], rows_per_block, n_blocks))
    err = np.abs(from_bits(got_partial_bits).astype(np.float64).reshape(p64.shape) - p64)
    assert not np.isnan(err).any() and bool((err <= bound).all()), (tag, float(err.max()), float(bound.max()))
    return float((err / np.maximum(bound, 1e-300)).max())


# ------------------------------------------------------------------------------------------------------------------------------
# tg_head_bwd_relu_bias
# ------------------------------------------------------------------------------------------------------------------------------
HEAD_COLS = {"f32": [8, 40, 96, 128, 256, 2048], "bf16": [8, 40, 96, 128, 256, 2048], "bits": [128, 256]}
HEAD_SWEEP = {"f32": (40, 128), "bf16": (40, 2048), "bits": (128, 256)}       # the full row sweep; {1, rpp + 1} on the other widths


def ka_of(a_dim):
    return 1 if a_dim <= 1 else 2 if a_dim <= 2 else 4 if a_dim <= 4 else 8


def head_cases():
    """Every form meets every act_dim 1..8 (it cycles with the case number), every width, and the row sweep on two widths."""
    out = []
    for form in ("f32", "bf16", "bits"):
        k = 0
        for cols in HEAD_COLS[form]:
            rp = rpp_of(cols, 8)
            for rows in (row_counts(cols, 8) if cols in HEAD_SWEEP[form] else [1, rp + 1]):
                a_dim = 1 + k % 8
                k += 1
                out.append(SimpleNamespace(form=form, bf16=form != "f32", cols=cols, rows=rows, a_dim=a_dim, id=f"{form}-c{cols}-r{rows}-A{a_dim}"))
        assert {c.a_dim for c in out if c.form == form} == set(range(1, 9))
    # the act_dims whose guards `k < a_dim` matter (3 of KA = 4; 5, 6, 7 of KA = 8) past the second grid-stride trip, on every form
    for form, cols in (("f32", 96), ("bf16", 96), ("bits", 128)):
        for a_dim in (3, 5, 6, 7):
            rows = BLOCKS * rpp_of(cols, 8) + 1
            out.append(SimpleNamespace(form=form, bf16=form != "f32", cols=cols, rows=rows, a_dim=a_dim, id=f"{form}-c{cols}-r{rows}-A{a_dim}"))
    return out


@functools.lru_cache(maxsize=2)
def head_inputs(form, cols, rows, a_dim, real=False):
    """dout f32 [rows][a_dim] and W f32 [a_dim][cols], each EXACTLY that long (the device copies are followed by NaN guards), the
    activations of the form's dtype and their mask."""
    bf16 = form != "f32"
    rng = np.random.default_rng([12, ("f32", "bf16", "bits").index(form), cols, rows, a_dim, int(real)])
    a_bits, mask = make_acts(rng, rows, cols, 8, bf16)
    if real:
        dout, W = rng.standard_normal((rows, a_dim)).astype(np.float32), (rng.standard_normal((a_dim, cols)) / 3).astype(np.float32)
    else:
        dout, W = rng.choice(NONZERO, size=(rows, a_dim)).astype(np.float32), rng.choice(NONZERO, size=(a_dim, cols)).astype(np.float32)
    return SimpleNamespace(form=form, bf16=bf16, cols=cols, rows=rows, a_dim=a_dim, dout=dout, W=W, a_bits=a_bits, mask=mask, rpp=rpp_of(cols, 8))


def head_ref(x, mutant=None, mask=None):
    """dZ = (dout . W) * mask in the form's dtype, NaN (the prefill) where a wrong kernel writes nothing; partials as relu_ref."""
    A, KA = x.a_dim, ka_of(x.a_dim)
    d64 = x.dout.astype(np.float64)
    if mutant == "dout_stride_ka":                                # the WRONG row stride: reads run into the next rows and the guard
        flat = np.concatenate([d64.reshape(-1), np.full(x.rows * (KA - A) + KA, np.nan)])
        d64 = flat[np.arange(x.rows)[:, None] * KA + np.arange(A)[None, :]]
    W64 = x.W.astype(np.float64)
    with np.errstate(invalid="ignore"):
        v64 = d64 @ W64 + 0.0
        if mutant == "w_leak" and KA > A:                         # weight rows A .. KA-1 read (the NaN guard) and multiplied by 0
            v64 = v64 + 0.0 * np.nan
    absv = np.abs(x.dout.astype(np.float64)) @ np.abs(W64)
    if mask is None:
        mask = mask_of(x.a_bits, mutant) if x.form != "bits" else unpack_mask_bits(pack_mask_bits(x.mask), x.cols, mutant)
    keep = _processed(x.rows, x.rpp, mutant)
    with np.errstate(invalid="ignore"):
        vbits = to_bits(v64.astype(np.float32), x.bf16, truncate=mutant == "bf16_truncate")
    dz = np.where(keep[:, None], np.where(mask, vbits, 0), NAN16 if x.bf16 else NAN32).astype(vbits.dtype)
    pbits, p64, abs64, n = _partials(np.where(keep[:, None], dz, 0).astype(dz.dtype), keep, x.rpp, BLOCKS, mutant)
    return SimpleNamespace(dz_bits=dz, partial_bits=pbits, v64=v64, absv=absv, mask=mask, p64=p64, abs64=abs64, n=n)


def head_image(ref, mutant=None):
    img = {"dz": guarded(ref.dz_bits), "partial": guarded(ref.partial_bits)}
    if mutant == "guard_overwrite":
        img["partial"][G - 1] = 0
    return img


def head_interval(v64, absv, a_dim, bf16):
    """The closed interval (as values of the storage dtype, f64) the stored product may lie in."""
    b = a_dim * 2.0 ** -23 * absv
    lo, hi = v64 - b, v64 + b
    lo32, hi32 = lo.astype(np.float32), hi.astype(np.float32)
    lo32 = np.where(lo32.astype(np.float64) > lo, np.nextafter(lo32, np.float32(-np.inf)), lo32).astype(np.float32)
    hi32 = np.where(hi32.astype(np.float64) < hi, np.nextafter(hi32, np.float32(np.inf)), hi32).astype(np.float32)
    if not bf16:
        return lo, hi
    return from_bits(RK.bf16_bits(lo32)).astype(np.float64), from_bits(RK.bf16_bits(hi32)).astype(np.float64)


def check_head_real(got_dz_bits, x, ref, tag=""):
    """Masked entries are +0 exactly, the others lie in head_interval(); -> worst |error| / (b + one storage rounding)."""
    got_bits = np.asarray(got_dz_bits).reshape(x.rows, x.cols)
    got = from_bits(got_bits).astype(np.float64)
    assert not bool(got_bits[~ref.mask].any()), f"{tag}: a masked entry is not +0"
    lo, hi = head_interval(ref.v64, ref.absv, x.a_dim, x.bf16)
    ok = (got >= lo) & (got <= hi)
    assert bool(ok[ref.mask].all()), (tag, int((~ok & ref.mask).sum()), float(np.abs(got - ref.v64)[ref.mask].max()))
    # (the figure that is printed: the error over b + the storage rounding; the assertion is the interval above)
    scale = x.a_dim * 2.0 ** -23 * ref.absv + (2.0 ** -8 if x.bf16 else 0.0) * np.abs(ref.v64) + 1e-300
    return float((np.abs(got - ref.v64) / scale)[ref.mask].max()) if ref.mask.any() else 0.0


def rne_probe(seed=0):
    """-> (W f32 [1][96], the bf16 patterns RNE must store): 32 bf16 values b (both signs, both parities of the last bit); for each the
    fp32 midpoint between b and the next bf16 away from zero, and the fp32 values just below and above that midpoint."""
    rng = np.random.default_rng([13, seed])
    b = (rng.integers(0x3000, 0x4800, size=32).astype(np.uint32) & 0x7FFF)
    b[:16] &= 0xFFFE                                               # even lower neighbour: the tie rounds DOWN (towards b)
    b[16:] |= 1                                                    # odd: the tie rounds UP
    b[::2] |= 0x8000
    mid = (b << 16) | np.uint32(0x8000)
    w_bits = np.stack([mid - 1, mid, mid + 1], axis=1).reshape(-1).astype(np.uint32)
    want = np.stack([b, b + (b & 1), b + 1], axis=1).reshape(-1).astype(np.uint16)
    assert np.array_equal(RK.bf16_bits(w_bits.view(np.float32)), want)
    assert not np.array_equal(RK.bf16_bits(w_bits.view(np.float32), truncate=True), want)
    return w_bits.view(np.float32).reshape(1, 96).copy(), want


# ------------------------------------------------------------------------------------------------------------------------------
# tg_dw_finish
# ------------------------------------------------------------------------------------------------------------------------------
DW_WINDOWS = [(8, 32, 8, 32, 32), (8, 64, 4, 64, 64), (64, 32, 64, 20, 20), (24, 40, 24, 40, 47), (1, 1, 1, 1, 1)]   # (M, K, m_out, k_out, grad_ld)
DW_BATCHES = [0, 1, 7, 8, 9, 15, 16, 17]
DW_TAILS = [0, 1, 7, 8, 9, 127, 4096]
DW_OFFSET = 5                                                     # the window starts 5 floats into the bucket (after the guard)


def dw_pairs(window):
    """(n_batches, tail): the full product on the first window; on the others every value of each axis once, and (0, 0)."""
    if window == DW_WINDOWS[0]:
        return [(nb, t) for nb in DW_BATCHES for t in DW_TAILS]
    k = DW_WINDOWS.index(window)
    return [(DW_BATCHES[i], DW_TAILS[(i + k) % len(DW_TAILS)]) for i in range(len(DW_BATCHES))] + [(0, 0)]


@functools.lru_cache(maxsize=4)
def dw_inputs(window, n_batches, tail, seed=0):
    M, K, m_out, k_out, ld = window
    rng = np.random.default_rng([14, M, K, m_out, k_out, ld, n_batches, tail, seed])
    size = DW_OFFSET + (m_out - 1) * ld + k_out + 3 if m_out else DW_OFFSET + 3
    return SimpleNamespace(window=window, n_batches=n_batches, tail=tail,
                           partial=rng.choice(NONZERO, size=(n_batches, M, K)).astype(np.float32),
                           dz_tail=rng.choice(NONZERO, size=(tail, M)).astype(np.float32), a_tail=rng.choice(NONZERO, size=(tail, K)).astype(np.float32),
                           bucket=rng.choice(NONZERO, size=size).astype(np.float32))


def dw_ref(x, mutant=None):
    """grad[m][k] += sum_b partial[b][m][k] + sum_r dz_tail[r][m] a_tail[r][k] on the window; -> (guarded bucket image, sum |terms|)."""
    M, K, m_out, k_out, ld = x.window
    nb, t = x.n_batches, x.tail
    if mutant == "drop_remainder":
        nb -= nb % 8
    if mutant == "drop_tail_last":
        t = max(t - 1, 0)
    p, dz, a = x.partial.astype(np.float64), x.dz_tail.astype(np.float64), x.a_tail.astype(np.float64)
    s = (p[:nb].sum(0) + dz[:t].T @ a[:t])[:m_out, :k_out]
    out = x.bucket.astype(np.float64)
    idx = (DW_OFFSET + np.arange(m_out)[:, None] * ld + np.arange(k_out)[None, :]).reshape(-1)
    terms = np.abs(out[idx]) + (np.abs(p).sum(0) + np.abs(dz).T @ np.abs(a))[:m_out, :k_out].reshape(-1)
    out[idx] = s.reshape(-1) + (0.0 if mutant == "overwrite" else out[idx])
    if mutant == "guard_overwrite":
        out[DW_OFFSET - 1] = 0.0
    return {"bucket": guarded(RK.f32_bits(out.astype(np.float32)))}, terms


# ------------------------------------------------------------------------------------------------------------------------------
# tg_colsum_finish
# ------------------------------------------------------------------------------------------------------------------------------
CS_BLOCKS = [0, 1, 15, 16, 17, 1024, 2049]
CS_WIDTHS = [1, 3, 63, 64, 65, 96, 2048]
CS_GAP = 3                                                        # bucket words between two gradient vectors
MAX_ELEMS = 2 ** 23 + 2 ** 16


def colsum_cases():
    """(n_blocks, n_vec, width): every (n_blocks, width) pair with n_vec cycling through 1..8, lowered until the partials fit."""
    out = []
    for i, nb in enumerate(CS_BLOCKS):
        for j, w in enumerate(CS_WIDTHS):
            nv = 1 + (i * 3 + j) % 8
            while nv > 1 and nb * nv * w > MAX_ELEMS:
                nv -= 1
            out.append((nb, nv, w))
    assert {nv for _, nv, _ in out} == set(range(1, 9)) and any((nv * w) % 64 for _, nv, w in out)
    return out


@functools.lru_cache(maxsize=2)
def colsum_inputs(n_blocks, n_vec, width):
    rng = np.random.default_rng([15, n_blocks, n_vec, width])
    offs = [CS_GAP + v * (width + CS_GAP) for v in range(n_vec)]
    return SimpleNamespace(n_blocks=n_blocks, n_vec=n_vec, width=width, offs=offs,
                           partial=rng.choice(NONZERO, size=(n_blocks, n_vec, width)).astype(np.float32),
                           bucket=rng.choice(NONZERO, size=offs[-1] + width + CS_GAP).astype(np.float32))


def colsum_ref(x, mutant=None):
    """out[v][c] += sum_b partial[b][v][c]; -> (guarded bucket image, sum |terms|)."""
    out = x.bucket.astype(np.float64)
    s, sa = x.partial.astype(np.float64).sum(0), np.abs(x.partial).astype(np.float64).sum(0)
    terms = []
    for v, o in enumerate(x.offs):
        terms.append(np.abs(out[o:o + x.width]) + sa[v])
        out[o:o + x.width] = s[v] + (0.0 if mutant == "overwrite" else out[o:o + x.width])
    if mutant == "guard_overwrite":
        out[x.offs[-1] + x.width] = 0.0
    return {"bucket": guarded(RK.f32_bits(out.astype(np.float32)))}, np.concatenate(terms)


# ------------------------------------------------------------------------------------------------------------------------------
# tg_head_prep
# ------------------------------------------------------------------------------------------------------------------------------
PREP_ROWS = [0, 1, 255, 256, 257, 262144, 262145, 524291]


def prep_cases():
    """(bf16, rows, a_dim, out_pad): both dtypes x every row count x every act_dim; both paddings up to 257 rows, alternating above."""
    out = []
    for bf in (True, False):
        for rows in PREP_ROWS:
            for a_dim in range(1, 9):
                for pad in ((8, 16) if rows <= 257 else ((8, 16)[(a_dim + PREP_ROWS.index(rows)) % 2],)):
                    out.append((bf, rows, a_dim, pad))
    return out


@functools.lru_cache(maxsize=2)
def prep_inputs(rows, a_dim, real=False):
    rng = np.random.default_rng([16, rows, a_dim, int(real)])
    return (rng.standard_normal((rows, a_dim)) if real else rng.choice(NONZERO, size=(rows, a_dim))).astype(np.float32)


def prep_ref(dout, out_pad, bf16, mutant=None):
    """dz [rows][out_pad] = dout in the compute dtype, zero padded; partial [1024][a_dim] = block sums of dout (256 rows per block)."""
    rows, A = dout.shape
    keep = _processed(rows, THREADS, mutant)
    dz = np.zeros((rows, out_pad), dtype=np.uint16 if bf16 else np.uint32)
    dz[:, :A] = to_bits(dout, bf16, truncate=mutant == "bf16_truncate")
    if mutant == "pad_unwritten":
        dz[:, A:] = NAN16 if bf16 else NAN32
    dz[~keep] = NAN16 if bf16 else NAN32
    pbits, p64, abs64, n = _partials(RK.f32_bits(dout), keep, THREADS, PREP_BLOCKS, mutant)
    return SimpleNamespace(dz_bits=dz, partial_bits=pbits, p64=p64, abs64=abs64, n=n)


def prep_image(ref):
    return {"dz": guarded(ref.dz_bits), "partial": guarded(ref.partial_bits)}


# ------------------------------------------------------------------------------------------------------------------------------
# GemmMLP._dw / _dw_into and the end-to-end nets
# ------------------------------------------------------------------------------------------------------------------------------
DW_GEMM_ROWS = [1, 8191, 8192, 8193, 16385, 3 * 8192 + 777]
DW_GEMM_SHAPES = [(96, 96), (64, 32), (8, 96)]
DW_SPLIT_ROWS = [524288, 524288 + 127, 524288 + 128]              # the fixed-batch-count split: 128 batches and a tail of 0, 127, 0 rows


@functools.lru_cache(maxsize=2)
def dw_gemm_inputs(rows, M, K):
    """dz [rows][M], a [rows][K], grad0 [M][K]: nonzero integers; -> (dz, a, grad0, the exact fp64 product + grad0, sum |terms|)."""
    rng = np.random.default_rng([17, rows, M, K])
    dz, a = rng.choice(NONZERO, size=(rows, M)).astype(np.float32), rng.choice(NONZERO, size=(rows, K)).astype(np.float32)
    g0 = rng.choice(NONZERO, size=(M, K)).astype(np.float32)
    want = g0 + dz.astype(np.float64).T @ a.astype(np.float64)
    terms = np.abs(g0) + np.abs(dz).astype(np.float64).T @ np.abs(a).astype(np.float64)
    return dz, a, g0, want, terms


# (S, A, hidden, dtypes, hybrid): hybrid = the bf16 forward chain's mask bits without a backward chain
E2E_NETS = [(6, 2, (96, 96), ("bf16", "f32"), False), (5, 1, (128, 64), ("bf16", "f32"), False), (10, 3, (32,), ("bf16", "f32"), False),
            (12, 8, (40, 24, 8), ("bf16", "f32"), False), (32, 12, (96, 96), ("bf16", "f32"), False),
            (20, 4, (64, 64, 64), ("bf16", "f32"), False),
            (5, 1, (256,), ("bf16",), True), (10, 2, (128, 128), ("bf16",), True), (20, 4, (128,) * 7, ("bf16",), True)]
E2E_ROWS = [1, 255, 8193]

# widths around tg_relu_bwd_bias's and tg_head_bwd_relu_bias's limits (1024 fp32 / 2048 bf16 below the top hidden layer; 2048 on top)
LIMIT_WIDTHS = [1024, 1032, 2048, 2056]


def width_ok(widths, bf16, out_dim=1):
    """What mlp.supports() must answer for hidden widths `widths` (multiples of 8), restated from the kernels' argument checks."""
    relu = 2048 if bf16 else 1024
    top = 2048 if out_dim <= 8 else relu
    return widths[-1] <= top and all(w <= relu for w in widths[:-1])
