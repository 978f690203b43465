"""The per-layer learner on the MI355X (run with `-m gpu`): the kernels of csrc/mlp_kernels.hip that GemmMLP._backward_relu runs for
every ReLU net outside the tuned chain shapes, each called directly against tests/per_layer_ref.py, then _dw / _dw_into / _bias_into
and forward(keep=True) + backward() of the whole path.

  1. tg_relu_bwd_bias: bf16 widths 8 / 24 / 96 / 136 / 2048, fp32 widths 4 / 12 / 96 / 1000 / 1024 (tpr = cols / per does not divide
     256 at 24, 96, 136, 12, 1000: idle threads), rows 0, 1, rpp - 1, rpp, rpp + 1, 2048 rpp - 1, 2048 rpp + 1 (the second grid-stride
     trip).  Integer inputs: dZ, every partial row and every guard word bit for bit.  Real inputs: dZ bit for bit (the kernel copies or
     zeroes; activations include +0, -0, -1, the smallest subnormal and the smallest normal), partials within (n - 1) 2^-24 sum |v|.
  2. tg_head_bwd_relu_bias: every act_dim 1..8 on fp32 activations, bf16 activations and bf16 mask bits (all eight <dtype, KA>
     instantiations; act_dim 3, 5, 6, 7 also past the second trip), widths 8 / 40 / 96 / 128 / 256 / 2048 (mask bits: 128 / 256); dout
     and W_head are allocated at exactly rows x act_dim and act_dim x cols elements between NaN guards, so a read of row k >= act_dim
     shows.  The mask-bit form equals the activation form bit for bit.  Real inputs: every element inside per_layer_ref.head_interval()
     (A 2^-23 sum |d||w|, in bf16 one RNE of the ends); the rounding-mode probe stores RNE bit for bit.
  3. tg_dw_finish: n_batches 0 / 1 / 7 / 8 / 9 / 15 / 16 / 17 (the remainder loop), tails 0 .. 4096, five windows (m_out < M, k_out < K,
     grad_ld > k_out, 1 x 1), both dtypes, accumulating into a view of a nonzero bucket; m_out = 0 and tail = 4097 write nothing.
  4. tg_colsum_finish: n_blocks 0 / 1 / 15 / 16 / 17 / 1024 / 2049, 1..8 vectors, widths 1 .. 2048 (n_vec x width off a multiple of 64).
  5. tg_head_prep: both dtypes, act_dim 1..8, out_pad 8 / 16, rows up to 524,291 (the third grid-stride trip).
  6. GemmMLP._dw / _dw_into (both splits) and _bias_into's torch fall-back, exact on integers.
  7. forward(keep=True) + backward() of nine nets (six per-layer nets in both dtypes, three bf16 hybrids: the forward chain's mask bits
     without a backward chain) at 1, 255 and 8,193 rows against fp64, from the path's own compute-dtype weights and the masks of its own
     stored activations.  DERIVED: a stored activation is one rounding (2^-8 bf16, 2^-24 fp32) of an fp32 sum of K + 1 terms, (K + 1)
     2^-24 sum |terms| from its fp64 value; a dZ carries the bound E of the layer above through |W|, the same accumulation term and one
     output rounding; a gradient carries E through the |activations| (|E|^T |A|, column sums of E).  CONVENTION (the project's
     existing row-sum slack, not derived): 2e-5 (max |reference| + 1e-3) max(1, sqrt(rows / 1000)) for the fp32 sums over rows.
     The top hidden layer's dZ is formed from the head's fp32 MASTER weights and the fp32 dout (tg_head_bwd_relu_bias's contract, nets
     with <= 8 outputs), not from the bf16 copies the forward pass multiplied by: the reference follows the path.
  8. mlp.supports() turns away nets wider than these kernels take (found by reading: an fp32 20-1536-1536-4 policy got a GemmMLP and
     raised inside learn()); an fp32 5-1032-1032-1 GRPO learn() completes on torch autograd.  That gap is the one defect this module
     found; the five kernels passed every case above as they stood.  No bound here was fitted to a measurement: the worst figures seen
     were 0.997 of the bound (one fp32 addition of two values, one bf16 rounding), most far below.

Every output and partial buffer is NaN before a launch, every buffer sits between 64 NaN guard words, gradient targets are views into
a nonzero bucket.  Every launch is repeated and must return the same bits.  Each test prints its worst error over its bound."""
import math

import numpy as np
import pytest
import torch

import per_layer_ref as P
import row_kernels_ref as RK

pytestmark = pytest.mark.gpu
G = P.G


@pytest.fixture(scope="module")
def tg():
    import trajopt_grpo_amd as tg
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return tg


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


class _Buf:
    """Bit patterns between NaN guards on the device: .ptr = the first word after the front guard; .back() = everything, as patterns."""

    def __init__(self, bits, dev, after=G):
        bits = np.ascontiguousarray(bits).reshape(-1)
        self.bf16 = bits.dtype == np.uint16
        whole = np.concatenate([P.nan_bits(G, self.bf16), bits, P.nan_bits(after, self.bf16)])
        self.n, self.size = bits.size, 2 if self.bf16 else 4
        self.whole = torch.from_numpy(whole.view(np.int16 if self.bf16 else np.int32)).to(dev)
        self.ptr = self.whole.data_ptr() + G * self.size
        assert self.ptr % 16 == 0

    def view(self, *shape):
        return self.whole[G:G + self.n].view(torch.bfloat16 if self.bf16 else torch.float32).view(*shape)

    def back(self):
        return self.whole.cpu().numpy().view(np.uint16 if self.bf16 else np.uint32)


def _nan(n, bf16, dev):
    return _Buf(P.nan_bits(n, bf16), dev)


def _twice(run):
    """Run a launch twice on fresh buffers: the same bits."""
    a, b = run(), run()
    for k in a:
        assert np.array_equal(a[k], b[k]), f"{k}: a repeated launch differs"
    return a


# --------------------------------------------------------------------------------------------------------------------------------
# 1. tg_relu_bwd_bias
# --------------------------------------------------------------------------------------------------------------------------------
def _run_relu(N, x, dev):
    dA, a, part = _Buf(x.dA_bits, dev), _Buf(x.a_bits, dev), _nan(P.BLOCKS * x.cols, False, dev)
    assert N.load().tg_relu_bwd_bias_blocks() == P.BLOCKS
    N.check(N.load().tg_relu_bwd_bias(dA.ptr, a.ptr, x.rows, x.cols, int(x.bf16), part.ptr, N.stream_ptr(dev)), "tg_relu_bwd_bias")
    torch.cuda.synchronize()
    return {"dz": dA.back(), "partial": part.back()}


RELU = P.relu_cases()


@pytest.mark.parametrize("c", RELU, ids=[c.id for c in RELU])
def test_relu_bwd_bias_is_exact_on_integers(tg, dev, c):
    x = P.relu_inputs(c.bf16, c.cols, c.rows)
    ref = P.relu_ref(x)
    P.assert_exact(ref.abs64)
    P.check_image(_twice(lambda: _run_relu(tg._native, x, dev)), P.relu_image(ref), c.id)
    print(f"{c.id}: rpp {x.rpp}, bitwise")


@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "f32"])
def test_relu_bwd_bias_on_real_values(tg, dev, bf16):
    """dZ bit for bit where(a > 0, dA, +0); the partial rows within the summation bound of what was written."""
    worst = 0.0
    for cols in P.RELU_COLS[bf16]:
        rp = P.rpp_of(cols, P.per_of(bf16))
        for rows in (rp + 1, P.BLOCKS * rp + 1):
            x = P.relu_inputs(bf16, cols, rows, real=True)
            ref = P.relu_ref(x)
            got = _twice(lambda: _run_relu(tg._native, x, dev))
            P.check_image({"dz": got["dz"]}, {"dz": P.guarded(ref.dz_bits)}, f"{cols} x {rows}")
            assert np.array_equal(got["partial"][:G], P.nan_bits(G, False)) and np.array_equal(got["partial"][-G:], P.nan_bits(G, False))
            worst = max(worst, P.check_partial_real(got["partial"][G:-G], ref.dz_bits, rp, P.BLOCKS, f"{cols} x {rows}"))
    print(f"relu_bwd_bias {'bf16' if bf16 else 'f32'}: worst partial error / bound {worst:.3f}")


# --------------------------------------------------------------------------------------------------------------------------------
# 2. tg_head_bwd_relu_bias
# --------------------------------------------------------------------------------------------------------------------------------
def _run_head(N, x, dev, form=None):
    form = form or x.form
    dout = _Buf(RK.f32_bits(x.dout), dev)                           # exactly rows x a_dim floats, then NaN
    W = _Buf(RK.f32_bits(x.W), dev, after=8 * x.cols + G)            # exactly a_dim x cols floats, then NaN
    act = _Buf(x.a_bits, dev) if form != "bits" else None
    bits = _Buf(P.pack_mask_bits(x.mask), dev) if form == "bits" else None
    dz, part = _nan(x.rows * x.cols, x.bf16, dev), _nan(P.BLOCKS * x.cols, False, dev)
    N.check(N.load().tg_head_bwd_relu_bias(dout.ptr, x.a_dim, W.ptr, act.ptr if act else None, bits.ptr if bits else None, dz.ptr, x.rows,
                                           x.cols, int(x.bf16), part.ptr, N.stream_ptr(dev)), "tg_head_bwd_relu_bias")
    torch.cuda.synchronize()
    return {"dz": dz.back(), "partial": part.back()}


HEAD = P.head_cases()


@pytest.mark.parametrize("c", HEAD, ids=[c.id for c in HEAD])
def test_head_bwd_relu_bias_is_exact_on_integers(tg, dev, c):
    x = P.head_inputs(c.form, c.cols, c.rows, c.a_dim)
    ref = P.head_ref(x)
    P.assert_exact(ref.abs64, ref.absv)
    got = _twice(lambda: _run_head(tg._native, x, dev))
    P.check_image(got, P.head_image(ref), c.id)
    if c.form == "bits":                                            # the activation form on the same mask: the same bits
        P.check_image(_run_head(tg._native, x, dev, form="bf16"), got, c.id + " activation form")
    print(f"{c.id}: rpp {x.rpp}, KA {P.ka_of(c.a_dim)}, bitwise")


@pytest.mark.parametrize("form", ["f32", "bf16", "bits"])
def test_head_bwd_relu_bias_on_real_values(tg, dev, form):
    shapes = [(128, 17, 5), (256, P.BLOCKS * 8 + 1, 6), (128, 3, 1)] if form == "bits" else \
        [(40, 52, 3), (96, P.BLOCKS * 21 + 1, 7), (2048, 3, 8), (128, 17, 5), (8, 257, 2), (256, 9, 4), (40, 1, 1), (96, 22, 6)]
    worst, worst_p = 0.0, 0.0
    for cols, rows, a_dim in shapes:
        x = P.head_inputs(form, cols, rows, a_dim, real=True)
        ref = P.head_ref(x)
        got = _twice(lambda: _run_head(tg._native, x, dev))
        dz = got["dz"][G:-G].reshape(rows, cols)
        worst = max(worst, P.check_head_real(dz, x, ref, f"{form} {cols} x {rows} A {a_dim}"))
        worst_p = max(worst_p, P.check_partial_real(got["partial"][G:-G], dz, x.rpp, P.BLOCKS, f"{form} {cols} x {rows}"))
        for k in ("dz", "partial"):
            nan = P.nan_bits(G, got[k].dtype == np.uint16)
            assert np.array_equal(got[k][:G], nan) and np.array_equal(got[k][-G:], nan)
        if form == "bits":
            P.check_image(_run_head(tg._native, x, dev, form="bf16"), got, "activation form")
    print(f"head_bwd_relu_bias {form}: worst error / (A 2^-23 sum|d||w| + storage rounding) {worst:.3f}, worst partial error / bound {worst_p:.3f}")


@pytest.mark.parametrize("form", ["bf16", "bits", "f32"])
def test_head_bwd_relu_bias_rounds_to_nearest_even(tg, dev, form):
    """A = 1, dout = 1: the product IS the weight.  Weights at, just below and just above the fp32 midpoints of bf16 neighbours."""
    W, want = P.rne_probe()
    cols = 128 if form == "bits" else 96
    Wp = np.ones((1, cols), np.float32)
    Wp[0, :96] = W[0]
    x = P.head_inputs(form, cols, 3, 1)
    x = type(x)(**{**vars(x), "dout": np.ones((3, 1), np.float32), "W": Wp, "mask": np.ones((3, cols), bool),
                   "a_bits": np.full((3, cols), P.POS_BITS[form != "f32"][0])})
    got = _run_head(tg._native, x, dev)["dz"][G:-G].reshape(3, cols)
    for r in range(3):
        assert np.array_equal(got[r, :96], want if form != "f32" else RK.f32_bits(W[0])), (form, r)
    print(f"rounding probe {form}: 96 values x 3 rows, bitwise")


# --------------------------------------------------------------------------------------------------------------------------------
# 3. tg_dw_finish
# --------------------------------------------------------------------------------------------------------------------------------
def _run_dw(N, x, bf16, dev, window=None, tail=None, null_inputs=False):
    M, K, m_out, k_out, ld = window or x.window
    tail = x.tail if tail is None else tail
    bucket, part = _Buf(RK.f32_bits(x.bucket), dev), _Buf(RK.f32_bits(x.partial), dev)
    dz, a = _Buf(P.to_bits(x.dz_tail, bf16), dev), _Buf(P.to_bits(x.a_tail, bf16), dev)
    rc = N.load().tg_dw_finish(None if (null_inputs and x.n_batches == 0) else part.ptr, x.n_batches, M, K,
                               None if (null_inputs and tail == 0) else dz.ptr, None if (null_inputs and tail == 0) else a.ptr, tail, int(bf16),
                               bucket.ptr + 4 * P.DW_OFFSET, ld, m_out, k_out, N.stream_ptr(dev))
    torch.cuda.synchronize()
    return rc, {"bucket": bucket.back()}


@pytest.mark.parametrize("window", P.DW_WINDOWS, ids=["x".join(map(str, w)) for w in P.DW_WINDOWS])
@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "f32"])
def test_dw_finish_is_exact_on_integers(tg, dev, bf16, window):
    N = tg._native
    pairs = P.dw_pairs(window)
    for nb, tail in pairs:
        x = P.dw_inputs(window, nb, tail)
        want, terms = P.dw_ref(x)
        P.assert_exact(terms)
        rc, got = _run_dw(N, x, bf16, dev, null_inputs=(nb + tail) % 2 == 0)
        N.check(rc, "tg_dw_finish")
        P.check_image(got, want, f"{window} n_batches {nb} tail {tail}")
    x = P.dw_inputs(window, 9, 9)
    untouched = {"bucket": P.guarded(RK.f32_bits(x.bucket))}
    M, K, m_out, k_out, ld = window
    rc, got = _run_dw(N, x, bf16, dev, window=(M, K, 0, k_out, ld))  # an empty window: nothing is written
    N.check(rc, "tg_dw_finish")
    P.check_image(got, untouched, "m_out 0")
    rc, got = _run_dw(N, x, bf16, dev, tail=4097)                    # a tail beyond the ABI's 4,096 rows: refused before any launch
    assert rc == N.TG_ERR_ARG and b"tail" in N.load().tg_last_error()
    P.check_image(got, untouched, "tail 4097")
    print(f"dw_finish {window} {'bf16' if bf16 else 'f32'}: {len(pairs)} (n_batches, tail) pairs, bitwise")


# --------------------------------------------------------------------------------------------------------------------------------
# 4. tg_colsum_finish
# --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_blocks", P.CS_BLOCKS)
def test_colsum_finish_is_exact_on_integers(tg, dev, n_blocks):
    N = tg._native
    mine = [c for c in P.colsum_cases() if c[0] == n_blocks]
    assert len(mine) == len(P.CS_WIDTHS)
    for nb, nv, w in mine:
        x = P.colsum_inputs(nb, nv, w)
        want, terms = P.colsum_ref(x)
        P.assert_exact(terms)

        def run():
            bucket, part = _Buf(RK.f32_bits(x.bucket), dev), _Buf(RK.f32_bits(x.partial), dev)
            ptrs = (N.C.c_void_p * nv)(*[bucket.ptr + 4 * o for o in x.offs])
            N.check(N.load().tg_colsum_finish(part.ptr, nb, nv, w, ptrs, N.stream_ptr(dev)), "tg_colsum_finish")
            torch.cuda.synchronize()
            return {"bucket": bucket.back()}
        P.check_image(_twice(run), want, f"n_blocks {nb} n_vec {nv} width {w}")
    print(f"colsum_finish n_blocks {n_blocks}: {[(nv, w) for _, nv, w in mine]}, bitwise")


# --------------------------------------------------------------------------------------------------------------------------------
# 5. tg_head_prep
# --------------------------------------------------------------------------------------------------------------------------------
def _run_prep(N, dout, pad, bf16, dev):
    rows, a_dim = dout.shape
    d, dz, part = _Buf(RK.f32_bits(dout), dev), _nan(rows * pad, bf16, dev), _nan(P.PREP_BLOCKS * a_dim, False, dev)
    assert N.load().tg_head_prep_blocks() == P.PREP_BLOCKS
    N.check(N.load().tg_head_prep(d.ptr, rows, a_dim, pad, int(bf16), dz.ptr, part.ptr, N.stream_ptr(dev)), "tg_head_prep")
    torch.cuda.synchronize()
    return {"dz": dz.back(), "partial": part.back()}


@pytest.mark.parametrize("rows", P.PREP_ROWS)
@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "f32"])
def test_head_prep_is_exact(tg, dev, bf16, rows):
    N = tg._native
    worst, n = 0.0, 0
    for bf, r, a_dim, pad in P.prep_cases():
        if (bf, r) != (bf16, rows):
            continue
        dout = P.prep_inputs(rows, a_dim)
        ref = P.prep_ref(dout, pad, bf16)
        P.assert_exact(ref.abs64)
        P.check_image(_twice(lambda: _run_prep(N, dout, pad, bf16, dev)), P.prep_image(ref), f"rows {rows} A {a_dim} pad {pad}")
        n += 1
        if a_dim in (3, 8) and rows in (257, 262145):               # real values: dZ is ONE rounding (bit for bit), the partials within the bound
            dout = P.prep_inputs(rows, a_dim, real=True)
            ref = P.prep_ref(dout, pad, bf16)
            got = _run_prep(N, dout, pad, bf16, dev)
            P.check_image({"dz": got["dz"]}, {"dz": P.guarded(ref.dz_bits)}, f"real rows {rows} A {a_dim}")
            worst = max(worst, P.check_partial_real(got["partial"][G:-G], RK.f32_bits(dout), P.THREADS, P.PREP_BLOCKS))
    print(f"head_prep {'bf16' if bf16 else 'f32'} rows {rows}: {n} cases bitwise, worst real partial error / bound {worst:.3f}")


# --------------------------------------------------------------------------------------------------------------------------------
# 6. GemmMLP._dw, _dw_into, _bias_into
# --------------------------------------------------------------------------------------------------------------------------------
def _small_mlp(tg, dev, cd):
    return tg.mlp.GemmMLP(tg.NeuralNetwork(20, 4, (64, 64), "ReLU").to(dev), cd)


def _check_dw(m, cd, rows, M, K, dev):
    dz, a, g0, want, terms = P.dw_gemm_inputs(rows, M, K)
    P.assert_exact(terms)
    dz_d, a_d = torch.from_numpy(dz).to(dev).to(cd), torch.from_numpy(a).to(dev).to(cd)
    got = m._dw(dz_d, a_d)
    assert got.dtype == torch.float32 and np.array_equal(got.double().cpu().numpy(), want - g0), ("_dw", rows, M, K)
    for mo, ko in ((M, K), (M - M // 4, K - 3)):                     # the whole product and a window of it
        bucket0 = np.concatenate([P.NONZERO[np.arange(5) % 6], g0[:mo, :ko].reshape(-1), P.NONZERO[np.arange(3) % 6]]).astype(np.float32)
        outs = []
        for _ in range(2):
            bucket = torch.from_numpy(bucket0.copy()).to(dev)
            m._dw_into(bucket[5:5 + mo * ko].view(mo, ko), dz_d, a_d)
            outs.append(bucket.cpu().numpy())
        w = bucket0.astype(np.float64)
        w[5:5 + mo * ko] = want[:mo, :ko].reshape(-1)
        assert np.array_equal(outs[0].astype(np.float64), w) and np.array_equal(outs[0], outs[1]), ("_dw_into", rows, M, K, mo, ko)


@pytest.mark.parametrize("cdn", ["bf16", "f32"])
def test_dw_and_dw_into_are_exact_on_integers(tg, dev, cdn):
    cd = torch.bfloat16 if cdn == "bf16" else torch.float32
    m = _small_mlp(tg, dev, cd)
    for M, K in P.DW_GEMM_SHAPES:
        for rows in P.DW_GEMM_ROWS:
            _check_dw(m, cd, rows, M, K, dev)
    print(f"_dw / _dw_into {cdn}: {len(P.DW_GEMM_SHAPES) * len(P.DW_GEMM_ROWS)} cases, bitwise")


@pytest.mark.parametrize("rows", P.DW_SPLIT_ROWS)
def test_dw_split_path_is_exact_on_integers(tg, dev, rows):
    """>= 2^19 rows: 128 batches of rows / 128 rows and tg_dw_finish with n_batches = 128 and a tail of 0 or 127 rows."""
    _check_dw(_small_mlp(tg, dev, torch.bfloat16), torch.bfloat16, rows, 64, 64, dev)
    print(f"_dw / _dw_into split path, {rows} rows (tail {rows - 128 * (rows // 128)}): bitwise")


def test_bias_into_fallback_equals_the_kernel_path(tg, dev):
    """A non-contiguous gradient, or more than 8 vectors, takes torch; the same partials through tg_colsum_finish: the same integers."""
    m = _small_mlp(tg, dev, torch.float32)
    for nb, nv, w in ((2048, 3, 96), (17, 9, 40), (1024, 8, 65)):
        rng = np.random.default_rng([18, nb, nv, w])
        part = rng.choice(P.NONZERO, size=(nb, nv, w)).astype(np.float32)
        g0 = rng.choice(P.NONZERO, size=(nv, w)).astype(np.float32)
        want = g0.astype(np.float64) + part.astype(np.float64).sum(0)
        P.assert_exact(np.abs(g0) + np.abs(part).sum(0))
        part_d = torch.from_numpy(part).to(dev)
        strided = torch.from_numpy(np.repeat(g0, 2, axis=1)).to(dev)        # every second element: not contiguous
        grads = [strided[v, ::2] for v in range(nv)]
        assert not grads[0].is_contiguous() or w == 1
        m._bias_into(grads, part_d)
        assert np.array_equal(strided[:, ::2].double().cpu().numpy(), want) and np.array_equal(strided[:, 1::2].cpu().numpy(), g0)
        if nv <= 8:
            dense = torch.from_numpy(g0.copy()).to(dev)
            m._bias_into([dense[v] for v in range(nv)], part_d)
            assert np.array_equal(dense.double().cpu().numpy(), want)
    print("_bias_into: torch fall-back == tg_colsum_finish, bitwise")


# --------------------------------------------------------------------------------------------------------------------------------
# 7. forward(keep=True) + backward() against fp64
# --------------------------------------------------------------------------------------------------------------------------------
E2E = [(i, d) for i, n in enumerate(P.E2E_NETS) for d in n[3]]


def _conv(ref, rows):
    """The project's row-sum convention (test_backward_chain_kernel_matches_fp64): not derived."""
    return 2e-5 * (float(ref.abs().max()) + 1e-3) * max(1.0, math.sqrt(rows / 1000))


@pytest.mark.parametrize("rows", P.E2E_ROWS)
@pytest.mark.parametrize("net_i,cdn", E2E, ids=[f"{P.E2E_NETS[i][0]}-{'x'.join(map(str, P.E2E_NETS[i][2]))}-{P.E2E_NETS[i][1]}-{d}" for i, d in E2E])
def test_per_layer_forward_backward_matches_fp64(tg, dev, net_i, cdn, rows):
    S, A, hidden, _, hybrid = P.E2E_NETS[net_i]
    bf = cdn == "bf16"
    cd = torch.bfloat16 if bf else torch.float32
    u = 2.0 ** -8 if bf else 2.0 ** -24
    torch.manual_seed(1000 * net_i + rows + int(bf))
    net = tg.NeuralNetwork(S, A, hidden, "ReLU").to(dev)
    m = tg.mlp.GemmMLP(net, cd)
    if m._f32 is not None:                                          # the fp32 chain learner's shape: back to the per-layer path
        assert (hidden, cd) == ((64, 64, 64), torch.float32) and m.disable_f32_chain()
    assert m._f32 is None and m._bchain is None and (m._chain is not None) == hybrid, "the routing changed: this case no longer runs the per-layer path"
    if bf and hidden == (64, 64, 64):
        assert m._dxfrag[1] is not None and m._dxfrag[2] is not None, "tg_dx_relu_bias (64 x 64) not selected"
    lin, L = m.linears, len(m.linears)
    X, g = torch.randn(rows, S, device=dev), torch.randn(rows, A, device=dev)
    xp = m.prepare_input(X)

    def run():
        for p in net.parameters():
            p.grad = torch.zeros_like(p)
        m.forward(xp, keep=True)
        assert (m._bits is not None) == hybrid and not m._chain_backward_ok() and all(a is not None for a in m._acts)
        acts = [a.clone() for a in m._acts]
        bits = None if m._bits is None else [None if b is None else b.clone() for b in m._bits]
        m.backward(g)
        torch.cuda.synchronize()
        return acts, bits, [(l.weight.grad.clone(), l.bias.grad.clone()) for l in lin]

    acts, bits, got = run()
    acts2, _, got2 = run()
    assert all(torch.equal(a, b) for a, b in zip(acts, acts2)) and all(torch.equal(x, y) for p, q in zip(got, got2) for x, y in zip(p, q))
    worst = {"act": 0.0, "dW": 0.0, "db": 0.0}

    def hold(kind, name, value, ref, bound):
        err = (value.double() - ref).abs()
        assert bool((err <= bound).all()), (name, float(err.max()), float((err / bound).max()))
        worst[kind] = max(worst[kind], float((err / bound).max()))

    Wc = [l.weight.detach().to(cd).double() for l in lin]
    # ---- stored activations: one rounding of the fp64 value of their own input ----
    for i in range(L - 1):
        a_prev = acts[i][:, :lin[i].in_features].double()
        b = (lin[i].bias.detach() if hybrid else m.b[i]).double()     # (the forward chain adds the fp32 bias, the GEMM epilogue the rounded one)
        z = a_prev @ Wc[i].t() + b
        acc = (lin[i].in_features + 1) * 2.0 ** -24 * (a_prev.abs() @ Wc[i].abs().t() + b.abs())
        hold("act", f"activation {i}", acts[i + 1], torch.relu(z), acc + u * (z.abs() + acc) + 1e-300)
    masks = [a > 0 for a in acts[1:]]
    if hybrid:
        for i in range(L - 1):
            assert np.array_equal(bits[i + 1].cpu().numpy().view(np.uint32), P.pack_mask_bits(masks[i].cpu().numpy())), f"mask bits {i}"
    # ---- gradients, with the bound E on each dZ carried down beside the reference ----
    g64 = g.double()
    dzh = g.to(cd).double()                                           # tg_head_prep's one rounding (held bit for bit above)
    hold("db", "head bias", got[L - 1][1], g64.sum(0), _conv(g64.sum(0), rows))
    refW = dzh.t() @ acts[L - 1].double()
    hold("dW", "head weight", got[L - 1][0], refW, _conv(refW, rows))
    if A <= 8:                                                        # tg_head_bwd_relu_bias: fp32 dout x the fp32 master weights
        Wh = lin[-1].weight.detach().double()
        ref, acc = g64 @ Wh, A * 2.0 ** -23 * (g64.abs() @ Wh.abs())
    else:                                                             # GEMM of the padded compute-dtype dZ and weights
        ref, acc = dzh @ Wc[-1], (m.out_pad + 1) * 2.0 ** -24 * (dzh.abs() @ Wc[-1].abs())
    for i in range(L - 2, -1, -1):
        E = (acc + u * (ref.abs() + acc)) * masks[i]
        ref = ref * masks[i]
        hold("db", f"bias {i}", got[i][1], ref.sum(0), E.sum(0) + _conv(ref.sum(0), rows))
        a_in = acts[i][:, :lin[i].in_features].double()
        refW = ref.t() @ a_in
        hold("dW", f"weight {i}", got[i][0], refW, E.t() @ a_in.abs() + _conv(refW, rows))
        if i > 0:
            acc = E @ Wc[i].abs() + (lin[i].out_features + 1) * 2.0 ** -24 * ((ref.abs() + E) @ Wc[i].abs())
            ref = ref @ Wc[i]
    print(f"{S}-{hidden}-{A} {cdn} rows {rows}: worst error / bound: activations {worst['act']:.3f}, dW {worst['dW']:.3f}, db {worst['db']:.3f}")


# --------------------------------------------------------------------------------------------------------------------------------
# 8. a net wider than the kernels take stays on torch autograd
# --------------------------------------------------------------------------------------------------------------------------------
def test_too_wide_fp32_net_learns_on_autograd(tg, dev):
    torch.manual_seed(7)
    pol = tg.GaussianActor_NeuralNetwork(5, 1, (1032, 1032), cov=0.5, device=dev)
    assert not tg.mlp.supports(pol.actor, torch.float32) and tg.mlp.supports(pol.actor, torch.bfloat16)
    mgr = tg.RolloutManager(lambda: tg.CartPole(max_steps=8), pol, num_workers=2, num_episodes_per_worker=4, seed=8)
    buf = tg.Rollout_Buffer(mgr)
    buf.sample()
    algo = tg.GRPO(epsilon=0.15, beta=0.5, gamma=0.5, policy=pol, optimizer=torch.optim.Adam(pol.parameters(), lr=3e-4), updates_per_iter=2)
    before = [p.detach().clone() for p in pol.parameters()]
    algo.learn(buf)
    assert algo._mlp(pol.actor) is None, "a 1032-wide fp32 net got a GemmMLP"
    assert np.isfinite(algo.last_stats["J"]).all() and any(not torch.equal(a, b) for a, b in zip(before, pol.parameters()))
