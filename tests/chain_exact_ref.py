"""Exact CPU reference (numpy, no device) for the three kernels of the bf16 chain learner -- tg_mlp_forward_chain[_ex]
(csrc/mlp_fwd_chain.hip), tg_mlp_backward_chain[_w0|_ex] (csrc/mlp_bwd_chain.hip) and tg_mlp_weight_grad[_ex] (csrc/mlp_dw.hip) -- the
yardstick of test_chain_exact_cpu.py (the cases against their own conditions, planted wrong kernels against the reference) and of
test_chain_exact_gpu.py (the kernels, bit for bit).

INTEGER NETS (make_net).  First layer H x S: one +1 and one -1 per row in distinct columns (S = 1: one +-1).  Every hidden-to-hidden
layer is P_a - P_b for two permutation matrices that share no position: row i (block bi = i / 32, o = i % 32) has its +1 in column
block (bi + o) % (H / 32) and its -1 in the next one, at places drawn per column block -- so every row and column holds one +1 and one
-1 AND every 32 x 32 tile holds a nonzero (condition d) by construction.  Hidden biases and head weights from {-1, 0, 1}, head bias in
{-3 .. 3}, inputs integers |x| <= 3, dOut from {-1, 0, 1} in columns < A.  Then |a_l| <= 2 |a_{l-1}| + 1 and |dZ_below| <= 2 |dZ_above|,
every product and partial sum is an integer below 2^24 (exact in fp32 in ANY order), every stored bf16 value an integer below 257: the
kernels' outputs are one determined bit pattern each.  The reference is float64 BLAS, exact on these integers.

CONDITIONS, asserted by forward_ref / backward_ref / dw_ref / make_net on every unmutated case (a failing case is a broken test):
  (a) every activation and dZ equals its bf16 rounding (round_int() is the identity on it);
  (b) sum |terms| < 2^24 for every fp32 sum (pre-activations, head output, gradient elements, bias sums, slab sums);
  (c) every layer has >= 25 % nonzero activations;
  (d) every 32 x 32 tile of every weight matrix and every 32-row x 32-column block of every weight-gradient operand holds a nonzero.

ROUNDING PROBES (probe=True): the exact integer is NOT representable.  Forward: first-layer biases of 300 +- 1 on even and 600 +- 1 on
odd features: pre-activations are integers in (256, 512) -- the odd ones exact bf16 ties (spacing 2) -- and in (512, 1024) (spacing 4:
v % 4 == 2 ties, odd v inexact non-ties); the second layer consumes the ROUNDED values (differences of two of them, again beyond
256).  Backward: dOut from {+-128, +-1}, A = 4: dZ_top holds 257, 385 (ties), 513 (non-tie), ...  round_int() rounds half to even at
the bf16 spacing 2^(e - 8); (a) becomes "exactly one RNE per stored value", and the probes assert >= 100 ties and >= 100 inexact
non-ties (rounding_stats).

MUTANTS (`mutant=`): reference variants a correct kernel must not match -- MUTANTS below; mutants_for() says which apply to a case.

Layouts restated from include/trajopt_grpo_hip.h: the ReLU mask words (mask_places / pack_mask), TG_LAYOUT_PANEL (panel_chunks /
to_panel / from_panel).  Launch shapes restated from the host code of the three files: 256 rows per workgroup round and one workgroup
per CU (rows_of), 32-row stages, ring depths (ring_depth) and the split of the workgroups between jobs (dw_plan) of csrc/mlp_dw.hip."""
import functools
from types import SimpleNamespace as NS

import numpy as np

import per_layer_ref as P

G = P.G
CUS = 256                                   # the MI355X; the GPU module reads the real count from the library
ROUND, STAGE = 256, 32                      # rows per workgroup round of the chain kernels / per stage of the weight-gradient kernel
HH, HX, DH, HR, RH = range(5)
KIND = ["HH", "HX", "DH", "HR", "RH"]
PANEL_P, PANEL_Q = 1, 2
NAN = {np.dtype(np.uint16): 0x7FC0, np.dtype(np.uint32): 0x7FC00000, np.dtype(np.uint64): 0x7FF8000000000000}
TWO24 = float(2 ** 24)
MUTANTS = ["drop_last_row", "double_last_row", "pad_row", "swap_features", "skip_kblock", "mask_neighbour", "truncate", "half_away",
           "skip_slab", "extra_slab"]
ROUND_MODE = {"truncate": "truncate", "half_away": "half_away"}


def rows_of(spec, blocks=CUS):
    """A row count, or (k, d) = k rounds of EVERY workgroup plus d rows: blocks * 256 * k + d."""
    return spec if isinstance(spec, int) else blocks * ROUND * spec[0] + spec[1]


def pad32(rows):
    return -(-rows // 32) * 32


def nan_words(n, dtype):
    return np.full(int(n), NAN[np.dtype(dtype)], dtype=dtype)


def guarded(bits):
    bits = np.asarray(bits).reshape(-1)
    g = nan_words(G, bits.dtype)
    return np.concatenate([g, bits, g])


def f32_bits(v):
    return np.ascontiguousarray(np.asarray(v, dtype=np.float64) + 0.0, dtype=np.float32).view(np.uint32)


def bf16_bits(v):
    """Bit patterns of values that ARE bf16 values (asserted: the low half of the fp32 pattern is zero)."""
    u = np.ascontiguousarray(np.asarray(v, dtype=np.float64) + 0.0, dtype=np.float32).view(np.uint32)
    assert not (u & np.uint32(0xFFFF)).any(), "not a bf16 value"
    return (u >> np.uint32(16)).astype(np.uint16)


# ----------------------------------------------------------------------------------------------------------------------------------
# rounding
# ----------------------------------------------------------------------------------------------------------------------------------
def _spacing(v):
    _, e = np.frexp(np.asarray(v, dtype=np.float64))
    return np.exp2(np.maximum(e - 8, 0).astype(np.float64))            # bf16 keeps 8 significant bits; integers: never below 1


def round_int(v, mode="rne"):
    """Integers (f64) -> the bf16 value of one rounding: half to even at the bf16 spacing (2 in [256, 512), 4 in [512, 1024), ...);
    "truncate" / "half_away": the two wrong conversions."""
    v = np.asarray(v, dtype=np.float64)
    if v.size == 0 or float(np.abs(v).max()) <= 256:                   # integers up to 256 are bf16 values
        return v + 0.0
    s = _spacing(v)
    q = v / s
    r = np.rint(q) if mode == "rne" else np.trunc(q) if mode == "truncate" else np.sign(q) * np.floor(np.abs(q) + 0.5)
    return r * s + 0.0


def rounding_stats(v):
    """-> (exact ties, inexact non-ties) among the values about to be rounded."""
    if np.size(v) == 0 or float(np.abs(v).max()) <= 256:
        return 0, 0
    q = np.abs(np.asarray(v, dtype=np.float64)) / _spacing(v)
    frac = q - np.floor(q)
    return int((frac == 0.5).sum()), int(((frac != 0) & (frac != 0.5)).sum())


# ----------------------------------------------------------------------------------------------------------------------------------
# layouts
# ----------------------------------------------------------------------------------------------------------------------------------
def mask_places(H):
    """(word, bit) of feature f = 32 mt + 16 h + r: bit (mt & 1) 8 + (r >> 1) + 16 (r & 1) of word h (H / 64) + (mt >> 1)."""
    f = np.arange(H)
    mt, h, r = f >> 5, (f >> 4) & 1, f & 15
    return h * (H // 64) + (mt >> 1), (mt & 1) * 8 + (r >> 1) + 16 * (r & 1)


def pack_mask(mask):
    """bool [rows][H] -> uint32 [rows][H / 32]: the features in (word, bit) order, 32 per word, least significant bit first."""
    rows, H = mask.shape
    word, bit = mask_places(H)
    order = np.lexsort((bit, word))
    by = np.packbits(np.ascontiguousarray(mask[:, order]).reshape(rows, H // 32, 32), axis=2, bitorder="little")
    return np.ascontiguousarray(by).view("<u4").reshape(rows, H // 32).astype(np.uint32)


def panel_chunks(rows, H):
    """[rows][H / 8]: index (in 16-byte units) of chunk c of row r -- the header's byte formula over 16."""
    r, c = np.arange(rows)[:, None], np.arange(H // 8)[None, :]
    return ((r // 32) * (64 * H) + (r % 32 // 4) * (H // 32 * 256) + (c // 4) * 256 + (r % 4) * 64 + (c % 4) * 16) // 16


def to_panel(bits, pad=None):
    """Row-major patterns [rows][H] -> the panel-order image, flat [pad32(rows) H]; the pad rows of the last tile hold `pad` ([H]; None:
    copies of the last row, as the producers write them)."""
    rows, H = bits.shape
    full = np.concatenate([bits, np.broadcast_to(bits[-1] if pad is None else pad, (pad32(rows) - rows, H))]).astype(bits.dtype)
    out = np.empty((pad32(rows) * H // 8, 8), dtype=bits.dtype)
    out[panel_chunks(pad32(rows), H).reshape(-1)] = full.reshape(-1, 8)
    return out.reshape(-1)


def from_panel(flat, rows, H):
    return np.asarray(flat).reshape(-1, 8)[panel_chunks(rows, H).reshape(-1)].reshape(rows, H)


def tiles_nonzero(m):
    """Condition (d): every 32 x 32 block (the last ones ragged) of a matrix holds a nonzero."""
    m = np.asarray(m) != 0
    R, C = -(-m.shape[0] // 32), -(-m.shape[1] // 32)
    full = np.zeros((R * 32, C * 32), dtype=bool)
    full[:m.shape[0], :m.shape[1]] = m
    return bool(full.reshape(R, 32, C, 32).any(axis=(1, 3)).all())


# ----------------------------------------------------------------------------------------------------------------------------------
# nets and inputs
# ----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def make_net(S, A, H, nh, seed=0, probe=False):
    """-> W [nh] ([H][S], then [H][H], [out][in]), b int [nh][H], Wh [A][H], bh [A]."""
    rng = np.random.default_rng([21, S, A, H, nh, seed, int(probe)])
    W0 = np.zeros((H, S))
    i = np.arange(H)
    c1 = rng.integers(0, S, size=H)
    W0[i, c1] = rng.choice([-1.0, 1.0], size=H) if S == 1 else 1.0
    if S > 1:
        W0[i, (c1 + 1 + rng.integers(0, S - 1, size=H)) % S] = -1.0
    W, nb = [W0], H // 32
    bi, o = i // 32, i % 32

    def perm(shift):
        cb = (bi + o + shift) % nb
        sig = np.stack([rng.permutation(32) for _ in range(nb)])
        p = cb * 32 + sig[cb, (o // nb) * nb + bi]
        assert np.array_equal(np.sort(p), i)
        return p

    for _ in range(nh - 1):
        m = np.zeros((H, H))
        m[i, perm(0)] = 1.0
        m[i, perm(1)] = -1.0
        assert (np.abs(m).sum(0) == 2).all() and (np.abs(m).sum(1) == 2).all() and (m.sum(0) == 0).all() and (m.sum(1) == 0).all()
        W.append(m)
    b = rng.integers(-1, 2, size=(nh, H)).astype(np.float64)
    if probe:
        b[0] += np.where(i % 2 == 0, 300.0, 600.0)
    Wh = rng.integers(-1, 2, size=(A, H)).astype(np.float64)
    bh = rng.integers(-3, 4, size=A).astype(np.float64)
    assert all(tiles_nonzero(m) for m in W) and tiles_nonzero(Wh), "condition (d): an empty 32 x 32 weight tile"
    return NS(S=S, A=A, H=H, nh=nh, W=W, b=b, Wh=Wh, bh=bh, probe=probe)


def make_x(S, rows, seed=0):
    """-> integers [rows][32]: |x| <= 3 in columns < S, zeros, and (S < 32) the ones column 31 that prepare_input() writes."""
    rng = np.random.default_rng([22, S, rows, seed])
    x = np.zeros((rows, 32))
    x[:, :S] = rng.integers(-3, 4, size=(rows, S))
    if S < 32:
        x[:, 31] = 1.0
    return x


def make_dout(A, rows, seed=0, probe=False, wide=False):
    """-> integers [rows][8], zero in columns >= A: {-1, 0, 1} (probe: {+-128, +-1}; wide: {-3 .. 3}, a weight-gradient operand)."""
    rng = np.random.default_rng([23, A, rows, seed, int(probe)])
    d = np.zeros((rows, 8))
    d[:, :A] = (rng.choice([-128.0, -1.0, 1.0, 128.0], size=(rows, A)) if probe else
                rng.integers(-3, 4, size=(rows, A)) if wide else rng.integers(-1, 2, size=(rows, A)))
    if not wide and not probe:                                           # the last row counts: a dropped or doubled one must show
        d[-1, :A] = rng.choice([-1.0, 1.0], size=A)
    return d


def _swap01(v):
    """Features 0 and 1 of every 32-feature block change places."""
    v = v.copy()
    v[:, 0::32], v[:, 1::32] = v[:, 1::32].copy(), v[:, 0::32].copy()
    return v


# ----------------------------------------------------------------------------------------------------------------------------------
# forward chain
# ----------------------------------------------------------------------------------------------------------------------------------
def forward_ref(net, x, mutant=None):
    """-> acts [nh] (f64 [rows][H], the STORED values), masks [nh] (a > 0), out f64 [rows][A], ties / inexact (rounding_stats of all
    layers).  Mutants that change values: skip_kblock (input features 32..63 of layer min(1, nh), the head when nh == 1),
    swap_features (stored addresses only: not what the next layer consumes), mask_neighbour, truncate / half_away."""
    mode = ROUND_MODE.get(mutant, "rne")
    a, acts, masks, ties, inexact = x[:, :net.S], [], [], 0, 0
    for l in range(net.nh):
        W = net.W[l]
        z = a @ W.T + net.b[l]
        if mutant == "skip_kblock" and l == 1:
            z = z - a[:, 32:64] @ W[:, 32:64].T
        r = np.maximum(z, 0.0) + 0.0
        t, n = rounding_stats(r)
        ties, inexact = ties + t, inexact + n
        a = round_int(r, mode)
        if mutant is None:
            assert float((np.abs(x[:, :net.S] if l == 0 else acts[-1]) @ np.abs(W).T + np.abs(net.b[l])).max()) < TWO24, "condition (b)"
            assert net.probe or np.array_equal(a, r), "condition (a): an activation is not a bf16 value"
            assert float((a != 0).mean()) >= 0.25, f"condition (c): layer {l} has {float((a != 0).mean()):.2f} alive"
        acts.append(a)
        masks.append(a > 0)
    out = a @ net.Wh.T + net.bh
    if mutant == "skip_kblock" and net.nh == 1:
        out = out - a[:, 32:64] @ net.Wh[:, 32:64].T
    if mutant is None:
        assert float((np.abs(a) @ np.abs(net.Wh).T + np.abs(net.bh)).max()) < TWO24, "condition (b)"
    if mutant == "mask_neighbour":
        masks = [np.roll(m, 1, axis=1) for m in masks]
    stored = [_swap01(v) for v in acts] if mutant == "swap_features" else acts
    return NS(acts=acts, stored=stored, masks=masks, out=out, ties=ties, inexact=inexact)


def _rows_image(vals, panel, as_bits, drop_last):
    bits = as_bits(vals)
    if drop_last:
        bits = bits.copy()
        bits[-1] = NAN[bits.dtype]
    return guarded(to_panel(bits) if panel else bits)


def forward_image(net, fwd, out_cols, panel=False, variant=None, mutant=None):
    """name -> guarded patterns of every buffer the test allocates (NaN before the launch): act{l} / mask{l} / out.  variant: no_a0
    (d_acts[0] NULL: masks still written), no_acts (d_acts and d_masks NULL), no_masks (d_masks NULL)."""
    rows, H = fwd.out.shape[0], net.H
    drop = mutant == "drop_last_row"
    img = {}
    for l in range(net.nh):
        n_act = (pad32(rows) if panel else rows) * H
        stored = variant != "no_acts" and not (variant == "no_a0" and l == 0)
        img[f"act{l}"] = _rows_image(fwd.stored[l], panel, bf16_bits, drop) if stored else guarded(nan_words(n_act, np.uint16))
        img[f"mask{l}"] = (_rows_image(fwd.masks[l], False, pack_mask, drop) if variant not in ("no_acts", "no_masks") else
                           guarded(nan_words(rows * H // 32, np.uint32)))
    out = np.zeros((rows, out_cols))
    out[:, :net.A] = fwd.out
    img["out"] = _rows_image(out, False, f32_bits, drop)
    return img


# ----------------------------------------------------------------------------------------------------------------------------------
# backward chain
# ----------------------------------------------------------------------------------------------------------------------------------
def backward_ref(net, masks, dout, x=None, mutant=None):
    """masks [nh] bottom layer first (forward_ref's), dout [rows][8], x [rows][32] -> dz [nh] TOP layer first (f64, the stored values),
    colsum [nh][H], w0 [H][32] = dZ_bottom^T x (x given).  skip_kblock: features 32..63 of the layer above, in the first
    hidden-to-hidden product."""
    mode = ROUND_MODE.get(mutant, "rne")
    nh, rows = net.nh, dout.shape[0]
    above, dz, ties, inexact = dout[:, :net.A], [], 0, 0
    for j in range(nh):
        i = nh - 1 - j
        W = net.Wh if j == 0 else net.W[i + 1]
        v = above @ W
        if mutant == "skip_kblock" and j == 1:
            v = v - above[:, 32:64] @ W[32:64]
        m = np.roll(masks[i], 1, axis=1) if mutant == "mask_neighbour" else masks[i]
        v = np.where(m, v, 0.0) + 0.0
        t, n = rounding_stats(v)
        ties, inexact = ties + t, inexact + n
        r = round_int(v, mode)
        if mutant is None:
            assert float((np.abs(above) @ np.abs(W)).max()) < TWO24, "condition (b)"
            assert net.probe or np.array_equal(r, v), "condition (a): a dZ is not a bf16 value"
        dz.append(r)
        above = r
    w = np.ones(rows)
    if mutant == "drop_last_row":
        w[-1] = 0.0
    if mutant == "double_last_row":
        w[-1] = 2.0
    colsum = np.stack([(z * w[:, None]).sum(0) for z in dz])
    w0 = None if x is None else (dz[-1] * w[:, None]).T @ x
    if mutant is None:
        assert float(np.stack([np.abs(z).sum(0) for z in dz]).max()) < TWO24, "condition (b)"
        assert x is None or float((np.abs(dz[-1]).T @ np.abs(x)).max()) < TWO24, "condition (b)"
    stored = [_swap01(z) for z in dz] if mutant == "swap_features" else dz
    return NS(dz=dz, stored=stored, colsum=colsum, w0=w0, ties=ties, inexact=inexact)


BWD_MODES = ["partial", "lean", "w0", "panel", "panel_w0"]


def backward_image(net, bwd, mode, blocks=CUS, mutant=None):
    """mode: partial (tg_mlp_backward_chain with column sums), lean (d_dz[0] NULL, no sums), w0 (tg_mlp_backward_chain_w0: top and
    bottom dZ NULL), panel / panel_w0 (tg_mlp_backward_chain_ex in panel order: everything stored / as w0).  -> dz{j}; colsum (the
    partial rows added over the workgroups in order); w0sum (the *n_slabs slabs added in order: [H][32], columns S..30 zero, 31 = db0),
    w0rest (the slabs past *n_slabs and the guard: untouched), n_slabs."""
    rows, H, nh = bwd.dz[0].shape[0], net.H, net.nh
    panel, fused = mode.startswith("panel"), mode.endswith("w0")
    img = {}
    for j in range(nh):
        n = (pad32(rows) if panel else rows) * H
        unwritten = (j == 0 and mode in ("lean", "w0", "panel_w0")) or (j == nh - 1 and fused)
        img[f"dz{j}"] = guarded(nan_words(n, np.uint16)) if unwritten else _rows_image(bwd.stored[j], panel, bf16_bits, mutant == "drop_last_row")
    if mode == "partial":
        img["colsum"] = f32_bits(bwd.colsum).reshape(-1)
        img["partial_guards"] = nan_words(2 * G, np.uint32)
    if fused:
        n_slabs = 2 * min(blocks, -(-rows // ROUND))
        assert mutant is not None or not bwd.w0[:, net.S:31].any()
        img["w0sum"] = f32_bits(bwd.w0).reshape(-1)
        img["w0rest"] = nan_words((2 * blocks - n_slabs) * H * 32 + G, np.uint32)
        img["w0front"] = nan_words(G, np.uint32)
        img["n_slabs"] = np.array([n_slabs], dtype=np.uint32)
    return img


# ----------------------------------------------------------------------------------------------------------------------------------
# weight gradient: the host code's launch shape
# ----------------------------------------------------------------------------------------------------------------------------------
ROW_COST_PCT = [100, 100, 100, 260, 300]


def row_cost(H, kind):
    return {HH: 4 * H, HX: 2 * H + 64, HR: 2 * H + 64, RH: 2 * H + 16 + H // 8, DH: 2 * H + 16}[kind] * ROW_COST_PCT[kind]


def ring_depth(H, kind):
    """DwRing<H, KIND>::D: slots of the LDS ring (160 KiB less 16 zero bytes; HR / RH keep two recomputed tiles behind it)."""
    panel = 64 * H
    slot = 2 * panel if kind == HH else panel + 1024 if kind == DH else panel + 2048
    return min(8, (160 * 1024 - 16 - (2 * panel if kind in (HR, RH) else 0)) // slot)


def dw_plan(H, kinds, rows, cus=CUS):
    """tg_mlp_weight_grad_ex's split, restated: per job NS(alloc, cap, n_blocks, stages = the most stages one workgroup walks, ring)."""
    cost = [row_cost(H, k) for k in kinds]
    wsum = sum(cost)
    n_st = -(-rows // STAGE)
    cap = 1 if n_st < 4 else min(n_st // 4, 1 << 20)
    alloc, rem = [], []
    for c in cost:
        a, r = divmod(c * cus, wsum)
        if a < 1:
            a, r = 1, 0
        alloc.append(a)
        rem.append(r)
    used = sum(alloc)
    while used < cus:
        best = max(range(len(kinds)), key=lambda j: (rem[j], -j))
        if rem[best] == 0:
            break
        alloc[best] += 1
        rem[best] = 0
        used += 1
    return [NS(kind=k, alloc=a, cap=cap, n_blocks=min(a, cap), stages=-(-n_st // min(a, cap)), ring=ring_depth(H, k), n_st=n_st)
            for k, a in zip(kinds, alloc)]


def binding_rows(H, kinds, cus=CUS):
    """Rows at which the allocation (not cap) limits every narrow job's workgroups and each of them walks 8 or 9 stages, the last
    stage partial: n_st = 8 alloc + alloc / 2 of the narrow job with the FEWEST workgroups."""
    plan = dw_plan(H, kinds, 1 << 22, cus)
    a = min(p.alloc for p in plan if p.kind != HH)
    return STAGE * (8 * a + a // 2) - 5


# ----------------------------------------------------------------------------------------------------------------------------------
# weight gradient: operands and reference
# ----------------------------------------------------------------------------------------------------------------------------------
WIDE = {HH: PANEL_P | PANEL_Q, HX: PANEL_P, HR: PANEL_P, DH: PANEL_Q, RH: PANEL_Q}      # the layout bits a kind may carry
WINDOWS = ["full", "m", "n", "ld", "one"]


def _window(kind, H, code, k):
    M, N = (8 if kind == DH else H), (32 if kind == HX else H)
    if kind == DH:                                                   # m_out runs 1..8 with the case / job number
        m = 1 + k % 8
        return {"full": (m, N, N), "m": (m, N, N), "n": (m, N - 5, N - 5), "ld": (m, N, N + 3), "one": (1, 1, 1)}[code]
    return {"full": (M, N, N), "m": (M - 3, N, N), "n": (M, N - 5, N - 5), "ld": (M, N, N + 3), "one": (1, 1, 1)}[code]


def _ints(rng, rows, cols):
    return rng.integers(-3, 4, size=(rows, cols)).astype(np.float64)


@functools.lru_cache(maxsize=2)
def dw_inputs(H, rows, jobs, seed=0):
    """jobs: ((kind, layout bits, window code), ...).  -> NS(net, x, jobs = [NS(kind, layout, p / q / aux = the DEVICE operands as
    patterns, Pe / Qe = the effective operands f64, pad_p / pad_q = what a pad row of the last tile holds, window, w_off, b_off)],
    bucket).  Operands are arbitrary integers |v| <= 3; HR's Q is the net input x (Qe = relu(W0 x + b0)), RH's P is dOut (Pe = (dOut .
    W_head) * mask, mask bits built here).  Panel-order operands carry +-3 in their pad rows."""
    rng = np.random.default_rng([24, H, rows, seed, len(jobs)])
    net = make_net(20, 4 if H == 256 else 8, H, 3, seed=seed)
    x = make_x(20, rows, seed=seed + 1)
    a0 = np.maximum(x[:, :20] @ net.W[0].T + net.b[0], 0.0)
    out, off = [], 3
    pad3 = np.where(np.arange(H) % 2 == 0, 3.0, -3.0)
    for k, (kind, layout, code) in enumerate(jobs):
        assert layout & ~WIDE[kind] == 0
        j = NS(kind=kind, layout=layout, aux=None, window=_window(kind, H, code, k + rows + rows // 32))
        wide_p, wide_q = kind in (HH, HX, HR), kind in (HH, DH, RH)
        Pd = make_dout(net.A, rows, seed=seed + 10 + k, wide=True) if kind == RH else _ints(rng, rows, H if wide_p else 8)
        Qd = x if kind == HR else _ints(rng, rows, H if wide_q else 32)
        j.Pe, j.Qe = Pd, (a0 if kind == HR else Qd)
        if kind == RH:
            j.mask = rng.random((rows, H)) < 0.5
            j.aux = pack_mask(j.mask)
        j.Pd, j.Qd = Pd, Qd
        j.pad_p = pad3 if layout & PANEL_P else None
        j.pad_q = -pad3 if layout & PANEL_Q else None
        j.p = to_panel(bf16_bits(Pd), bf16_bits(pad3)) if layout & PANEL_P else bf16_bits(Pd).reshape(-1)
        j.q = to_panel(bf16_bits(Qd), bf16_bits(-pad3)) if layout & PANEL_Q else bf16_bits(Qd).reshape(-1)
        m_out, n_out, ld = j.window
        j.w_off = off
        off += (m_out - 1) * ld + n_out + 2
        j.b_off = None if (kind == DH or k % 5 == 4) else off
        off += 0 if j.b_off is None else m_out + 3
        out.append(j)
    bucket = rng.choice(P.NONZERO, size=off + 3)
    return NS(H=H, rows=rows, net=net, x=x, jobs=out, bucket=bucket)


def _effective_p(inp, j, mutant):
    if j.kind != RH:
        return j.Pe
    m = np.roll(j.mask, 1, axis=1) if mutant == "mask_neighbour" else j.mask
    return np.where(m, j.Pd[:, :inp.net.A] @ inp.net.Wh, 0.0) + 0.0


def dw_ref(inp, mutant=None):
    """-> (guarded bucket image, per job (dW, db) f64).  Row mutants weigh rows: drop_last_row / double_last_row / skip_kblock (the
    second 32-row stage) / pad_row (row `rows` of the last tile counted: the pad row of a panel-order operand, the re-read last row
    of any other); swap_features: columns 0 / 1 of every 32-column block of Q."""
    rows = inp.rows
    w = np.ones(rows)
    if mutant == "drop_last_row":
        w[-1] = 0.0
    if mutant == "double_last_row":
        w[-1] = 2.0
    if mutant == "skip_kblock":
        w[32:64] = 0.0
    bucket = inp.bucket.copy()
    grads = []
    for j in inp.jobs:
        Pe, Qe = _effective_p(inp, j, mutant), j.Qe
        if mutant is None:
            assert np.array_equal(round_int(Pe), Pe) and np.array_equal(round_int(Qe), Qe), "condition (a)"
            assert tiles_nonzero(Pe) and tiles_nonzero(Qe), "condition (d): an operand block without a nonzero"
            assert float((np.abs(Pe).T @ np.abs(Qe)).max()) + 3 < TWO24, "condition (b)"
        if mutant == "swap_features":
            Qe = _swap01(Qe)
        dW, db = (Pe * w[:, None]).T @ Qe, (Pe * w[:, None]).sum(0)
        if mutant == "pad_row":
            pp, pq = (Pe[-1] if j.pad_p is None else j.pad_p), (Qe[-1] if j.pad_q is None else j.pad_q)
            dW, db = dW + np.outer(pp, pq), db + pp
        m_out, n_out, ld = j.window
        idx = (j.w_off + np.arange(m_out)[:, None] * ld + np.arange(n_out)[None, :]).reshape(-1)
        bucket[idx] += dW[:m_out, :n_out].reshape(-1)
        if j.b_off is not None:
            bucket[j.b_off:j.b_off + m_out] += db[:m_out]
        grads.append((dW, db))
    return guarded(f32_bits(bucket)), grads


# ----------------------------------------------------------------------------------------------------------------------------------
# tg_mlp_weight_grad_ex's riders
# ----------------------------------------------------------------------------------------------------------------------------------
# (n_slabs, m_out, n_out, row_pitch, slab_stride, grad_ld); lanes per element: 1 up to 96 slabs, 32 above; the four-way unrolled slab
# loop runs n_slabs / (4 lanes) times and leaves n_slabs % (4 lanes) to the remainder loop
RIDER_SETS = {
    "none": (),
    "one": ((0, 5, 7, 9, 50, 11),),                                       # nothing to add; 35 elements: off a multiple of 64
    "two": ((1, 3, 50, 64, 200, 70), (3, 128, 32, 32, 4096, 32)),        # remainder only; row_pitch > n_out and grad_ld > n_out
    "three": ((4, 16, 16, 16, 256, 16), (5, 4, 33, 40, 160, 33), (96, 8, 8, 8, 64, 8)),     # one unrolled trip; + 1; the last 1-lane count
    "four": ((97, 5, 7, 9, 50, 11), (131, 4, 33, 40, 160, 35), (1024, 4, 33, 33, 132, 33), (0, 1, 1, 1, 1, 1)),  # 32 lanes: 97 = 3 x 32 + 1
}
LOSS_ROWS = {"none": 0, "one": 1, "two": 63, "three": 64, "four": 65, "loss_only": 256}
RIDER_CASES = [("none", None), ("one", 1), ("two", 63), ("three", 64), ("four", 65), ("none", 256), ("two", 0), ("one", None)]


@functools.lru_cache(maxsize=None)
def rider_inputs(name, n_loss_rows, seed=0):
    rng = np.random.default_rng([25, list(RIDER_SETS).index(name), 0 if n_loss_rows is None else n_loss_rows + 1, seed])
    regions, off = [], 2
    for n_slabs, m_out, n_out, pitch, stride, ld in RIDER_SETS[name]:
        assert pitch >= n_out and stride >= (m_out - 1) * pitch + n_out and ld >= n_out
        size = (n_slabs - 1) * stride + (m_out - 1) * pitch + n_out if n_slabs else 0
        regions.append(NS(n_slabs=n_slabs, m_out=m_out, n_out=n_out, pitch=pitch, stride=stride, ld=ld, off=off,
                          slab=rng.choice(P.NONZERO, size=size)))
        off += (m_out - 1) * ld + n_out + 3
    loss = None
    if n_loss_rows is not None:
        loss = NS(work=rng.choice(P.NONZERO, size=(n_loss_rows, 4)), sums=rng.choice(P.NONZERO, size=4))
    return NS(regions=regions, bucket=rng.choice(P.NONZERO, size=off + 2), loss=loss)


def rider_ref(r, mutant=None):
    """-> {"rider_bucket": guarded f32 patterns, "loss_sums": guarded f64 patterns (with a loss rider)}.  skip_slab: the last slab
    left out; extra_slab: slab `n_slabs` read -- the NaN guard behind the slab buffer."""
    bucket = r.bucket.copy()
    for g in r.regions:
        idx = (np.arange(g.m_out)[:, None] * g.pitch + np.arange(g.n_out)[None, :]).reshape(-1)
        n = g.n_slabs - 1 if (mutant == "skip_slab" and g.n_slabs) else g.n_slabs
        s = sum((g.slab[k * g.stride + idx] for k in range(n)), np.zeros(idx.size))
        if mutant is None and g.n_slabs:
            assert float(sum(np.abs(g.slab[k * g.stride + idx]) for k in range(n)).max()) + 3 < TWO24, "condition (b)"
        if mutant == "extra_slab":
            s = s + np.nan
        out = (g.off + np.arange(g.m_out)[:, None] * g.ld + np.arange(g.n_out)[None, :]).reshape(-1)
        bucket[out] += s
    img = {"rider_bucket": guarded(np.ascontiguousarray(bucket, dtype=np.float32).view(np.uint32))}
    if mutant == "extra_slab":
        b = img["rider_bucket"]
        b[(b & 0x7FFFFFFF) > 0x7F800000] = NAN[np.dtype(np.uint32)]
    if r.loss is not None:
        n = r.loss.work.shape[0] - (1 if mutant == "skip_slab" and r.loss.work.shape[0] else 0)
        img["loss_sums"] = guarded(np.ascontiguousarray(r.loss.sums + r.loss.work[:n].sum(0) + 0.0).view(np.uint64))
    return img


# ----------------------------------------------------------------------------------------------------------------------------------
# case tables (shared by test_chain_exact_cpu.py and test_chain_exact_gpu.py)
# ----------------------------------------------------------------------------------------------------------------------------------
SMALL_ROWS = [1, 31, 32, 33, 255, 256, 257]
BIG_ROWS = [(1, -1), (1, 0), (1, 1), (1, 257)]      # the second round of the first workgroup (+-1 row) and of the second workgroup


def _rid(spec):
    return str(spec) if isinstance(spec, int) else f"B{spec[0]}{spec[1]:+d}"


def _fwd(S, A, oc, H, nh, rows, panel=False, variant=None, probe=False):
    tag = f"{S}-{H}x{nh}-{A}o{oc}-r{_rid(rows)}" + ("-panel" if panel else "") + (f"-{variant}" if variant else "") + ("-probe" if probe else "")
    return NS(S=S, A=A, out_cols=oc, H=H, nh=nh, rows=rows, panel=panel, variant=variant, probe=probe, id=tag)


def forward_cases():
    out = []
    for k, rows in enumerate(SMALL_ROWS):                                  # the row sweep on the two learner shapes, both layouts
        for panel in (False, True):
            out += [_fwd(20, 4, 4, 256, 6, rows, panel), _fwd(5, 1, 4, 128, 3, rows, panel)]
    # every depth, input width and output width once more, at the 256-row edge
    out += [_fwd(1, 1, 4, 128, 1, 257), _fwd(32, 12, 16, 256, 2, 257), _fwd(32, 12, 16, 256, 2, 33, True), _fwd(1, 8, 8, 128, 8, 257),
            _fwd(20, 8, 16, 256, 8, 255, True), _fwd(5, 4, 8, 256, 1, 256), _fwd(32, 1, 8, 128, 2, 31, True), _fwd(1, 12, 16, 128, 6, 1),
            _fwd(20, 4, 4, 256, 3, 257), _fwd(5, 8, 8, 128, 3, 256, True)]
    for k, rows in enumerate(BIG_ROWS):                                    # H = 128 x 3 at the large row counts; H = 256 once
        out += [_fwd(5, 1, 4, 128, 3, rows, panel=k % 2 == 1)]
    out += [_fwd(20, 4, 4, 128, 3, (1, 257), True), _fwd(20, 4, 4, 256, 3, (1, 257), True)]
    for variant in ("no_a0", "no_acts", "no_masks"):
        out += [_fwd(20, 4, 4, 256, 6, 257, variant=variant), _fwd(5, 1, 4, 128, 3, (1, 1), variant=variant)]
    out += [_fwd(20, 4, 4, 256, 3, 33, True, variant="no_a0"), _fwd(5, 1, 4, 128, 3, 257, True, variant="no_masks")]
    out += [_fwd(20, 4, 4, 256, 3, 300, probe=True), _fwd(5, 1, 4, 128, 3, 300, True, probe=True)]
    assert {c.H for c in out} == {128, 256} and {c.nh for c in out} == {1, 2, 3, 6, 8} and {c.S for c in out} == {1, 5, 20, 32}
    assert {(c.A, c.out_cols) for c in out} >= {(1, 4), (4, 4), (4, 8), (8, 8), (8, 16), (12, 16), (1, 8)}
    assert len({c.id for c in out}) == len(out)
    return out


def _bwd(S, A, H, nh, rows, modes, probe=False):
    return NS(S=S, A=A, H=H, nh=nh, rows=rows, modes=tuple(modes), probe=probe,
              id=f"{S}-{H}x{nh}-{A}-r{_rid(rows)}-" + "+".join(modes) + ("-probe" if probe else ""))


def backward_cases():
    out = []
    for rows in SMALL_ROWS:
        out += [_bwd(20, 4, 256, 6, rows, BWD_MODES), _bwd(5, 1, 128, 3, rows, BWD_MODES)]
    out += [_bwd(10, 8, 256, 4, 257, BWD_MODES), _bwd(20, 8, 128, 6, 33, BWD_MODES), _bwd(1, 1, 256, 3, 255, BWD_MODES),
            _bwd(20, 4, 128, 4, 256, BWD_MODES)]
    for k, rows in enumerate(BIG_ROWS):
        out += [_bwd(5, 1, 128, 3, rows, [["partial", "w0"], ["lean", "panel_w0"], ["w0", "panel"], ["partial", "panel_w0"]][k])]
    out += [_bwd(20, 4, 256, 3, (1, 257), ["partial", "panel_w0"])]
    out += [_bwd(20, 4, 256, 3, 2000, ["partial", "panel"], probe=True), _bwd(5, 4, 128, 3, 2000, ["partial", "panel"], probe=True)]
    assert {c.H for c in out} == {128, 256} and {c.nh for c in out} == {3, 4, 6} and {c.A for c in out} == {1, 4, 8}
    assert len({c.id for c in out}) == len(out)
    return out


def _set(name, panel):
    """The job sets: `learner3` / `learner5` = what GemmMLP.backward_fused() launches for 3 / 5 hidden layers (RH on top, HH between, HR
    at the bottom; the head and the first layer are formed inside the chain kernels); `eight`: every kind, HH / HX / DH twice."""
    lay = lambda kind: WIDE[kind] if panel else 0
    if name == "learner3":
        kinds = [RH, HR]
    elif name == "learner5":
        kinds = [RH, HH, HH, HR]
    elif name == "eight":
        return tuple((k, l, WINDOWS[i % 5]) for i, (k, l) in enumerate([(HH, 3), (HX, 1), (DH, 2), (HR, 0), (RH, 0), (HH, 0), (HX, 0), (DH, 0)]))
    return tuple((k, lay(k), WINDOWS[i % 5]) for i, k in enumerate(kinds))


DW_SMALL_ROWS = [1, 31, 32, 33, 64, 65, 96, 97, 127, 128, 129, 160, 223, 224, 255, 256, 257, 288]   # n_st 1 1 1 2 2 3 3 4 4 4 5 5 7 7 8 8 9 9
SINGLES = [(HH, 0), (HH, 1), (HH, 2), (HH, 3), (HX, 0), (HX, 1), (DH, 0), (DH, 2), (HR, 0), (HR, 1), (RH, 0), (RH, 2)]


def _dw(H, rows, jobs, name):
    """rows: a count, "bind" (binding_rows() of the job set) or "b<k>" variants resolved by dw_rows()."""
    return NS(H=H, rows=rows, jobs=jobs, id=f"{name}-{H}-r{rows}")


def dw_rows(c, cus=CUS):
    return binding_rows(c.H, [k for k, _, _ in c.jobs], cus) if c.rows == "bind" else c.rows


def dw_cases():
    out = []
    for k, rows in enumerate(DW_SMALL_ROWS):
        out += [_dw(256, rows, _set("learner5", k % 2 == 0), "learner5" + ("-panel" if k % 2 == 0 else "")), _dw(128, rows, _set("eight", None), "eight")]
    for k, (kind, layout) in enumerate(SINGLES):
        out += [_dw(256 if k % 2 == 0 else 128, 97, ((kind, layout, WINDOWS[k % 5]),), f"one-{KIND[kind]}{layout}"),
                _dw(128 if k % 2 == 0 else 256, 1000, ((kind, layout, WINDOWS[(k + 2) % 5]),), f"one-{KIND[kind]}{layout}")]
    out += [_dw(128, 255, _set("learner3", True), "learner3-panel"), _dw(256, 129, _set("learner3", False), "learner3"),
            _dw(256, 257, _set("eight", None), "eight")]
    out += [_dw(128, "bind", _set("eight", None), "eight"), _dw(256, "bind", _set("eight", None), "eight"),
            _dw(256, "bind", _set("learner5", True), "learner5-panel")]
    out += [_dw(256, 70001, _set("learner5", True), "learner5-panel"), _dw(128, 70001, _set("eight", None), "eight")]
    assert len({c.id for c in out}) == len(out)
    return out


def check_dw_table(cus=CUS):
    """What the weight-gradient row counts are for, asserted against the restated host code."""
    cases = dw_cases()
    n_sts = {}
    for c in cases:
        if isinstance(c.rows, int):
            n_sts.setdefault(-(-c.rows // STAGE), set()).add(c.rows % STAGE != 0)
    assert all(n_sts.get(n) == {True, False} for n in (1, 2, 3, 4, 5, 7, 8, 9)), n_sts
    for c in cases:
        plan = dw_plan(c.H, [k for k, _, _ in c.jobs], dw_rows(c, cus), cus)
        assert sum(p.n_blocks for p in plan) <= cus
        if c.rows == "bind":                                           # the allocation binds; 8-9 stages > the 7-8 slots of a narrow ring
            narrow = [p for p in plan if p.kind != HH]
            assert len(plan) > 1 and any(p.n_blocks == p.alloc < p.cap and p.stages == 9 and p.n_st // p.n_blocks == 8 and p.stages > p.ring
                                         for p in narrow), [vars(p) for p in plan]
        if c.rows == 70001:                                            # every workgroup wraps its ring at least three times
            assert all(p.n_blocks == p.alloc < p.cap and p.n_st // p.n_blocks >= 3 * p.ring for p in plan), [vars(p) for p in plan]
    assert any(c.H == 128 and c.rows == "bind" for c in cases) and any(c.H == 256 and c.rows == "bind" for c in cases)
    kinds = {(k, l) for c in cases for k, l, _ in c.jobs}
    assert kinds >= set(SINGLES)
    assert {_window(DH, 128, w, k + dw_rows(c, cus) + dw_rows(c, cus) // 32)[0] for c in cases for k, (kd, _, w) in enumerate(c.jobs) if kd == DH} == set(range(1, 9))


def mutants_for(kind, c=None, rows=None):
    """The mutants that apply to a case.  kind: "fwd" / "bwd" / "dw" / "rider"."""
    if kind == "fwd":
        m = ["drop_last_row", "swap_features", "skip_kblock"] + ([] if c.variant in ("no_acts", "no_masks") else ["mask_neighbour"])
        if c.variant == "no_acts":                                     # only the head output is written
            m = ["drop_last_row", "skip_kblock"]
        return m + (["truncate", "half_away"] if c.probe else [])
    if kind == "bwd":
        m = ["drop_last_row", "swap_features", "skip_kblock", "mask_neighbour"]
        if set(c.modes) & {"partial", "w0", "panel_w0"}:
            m.append("double_last_row")
        return m + (["truncate", "half_away"] if c.probe else [])
    if kind == "dw":
        m = ["drop_last_row", "double_last_row", "swap_features"] + (["pad_row"] if rows % 32 else []) + (["skip_kblock"] if rows > 32 else [])
        return m + (["mask_neighbour"] if any(k == RH for k, _, _ in c.jobs) else [])
    return ["skip_slab", "extra_slab"]
