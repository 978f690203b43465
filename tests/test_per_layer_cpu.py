"""CPU: the yardstick of test_per_layer_gpu.py checked without a GPU.  (1) tests/per_layer_ref.py's restatements of tg_relu_bwd_bias,
tg_head_bwd_relu_bias, tg_dw_finish, tg_colsum_finish and tg_head_prep agree with torch's own CPU operations on every case of the GPU
module's tables, and the integer builders keep sum |terms| < 2^24 on every one of them; (2) the checkers reject planted wrong kernels
on the GPU module's own inputs; (3) mlp.supports() against the per-layer kernels' width limits."""
import numpy as np
import pytest
import torch

import per_layer_ref as P
import row_kernels_ref as RK


def _t(bits):
    """Bit patterns -> a torch CPU tensor of the dtype they encode."""
    bits = np.ascontiguousarray(bits)
    return torch.from_numpy(bits.view(np.int16)).view(torch.bfloat16) if bits.dtype == np.uint16 else torch.from_numpy(bits.view(np.float32))


def _b(t):
    """A torch CPU tensor -> its bit patterns."""
    return t.contiguous().view(torch.int16).numpy().view(np.uint16) if t.dtype == torch.bfloat16 else t.contiguous().numpy().view(np.uint32)


def _rejected(got, want, tag):
    with pytest.raises(AssertionError):
        P.check_image(got, want, tag)


# --------------------------------------------------------------------------------------------------------------------------------
# 1. restatements against torch, exactness of the integer builders
# --------------------------------------------------------------------------------------------------------------------------------
def test_tables_hold_what_they_are_for():
    for bf in (True, False):
        per = P.per_of(bf)
        assert any(256 % (c // per) for c in P.RELU_COLS[bf]), "no width with idle threads"
        assert max(P.RELU_COLS[bf]) == 256 * per and min(P.RELU_COLS[bf]) == per
        for c in P.RELU_COLS[bf]:
            rc = P.row_counts(c, per)
            assert {0, 1, P.rpp_of(c, per) + 1, 2048 * P.rpp_of(c, per) + 1} <= set(rc) and max(rc) * c <= P.MAX_ELEMS
    assert P.rpp_of(136, 8) == 15 and P.rpp_of(40, 8) == 51 and P.rpp_of(1000, 4) == 1 and P.rpp_of(24, 8) == 85
    cases = P.head_cases()
    assert all(c.rows * c.cols <= P.MAX_ELEMS for c in cases)
    for form in ("f32", "bf16", "bits"):
        mine = [c for c in cases if c.form == form]
        assert {c.a_dim for c in mine} == set(range(1, 9)) and {c.cols for c in mine} == set(P.HEAD_COLS[form])
        assert {c.a_dim for c in mine if c.rows > 2048 * P.rpp_of(c.cols, 8)} >= {3, 5, 6, 7}
    for w in P.DW_WINDOWS:
        pairs = P.dw_pairs(w)
        assert {nb for nb, _ in pairs} == set(P.DW_BATCHES) and {t for _, t in pairs} == set(P.DW_TAILS)
    assert len(P.dw_pairs(P.DW_WINDOWS[0])) == len(P.DW_BATCHES) * len(P.DW_TAILS)
    cs = P.colsum_cases()
    assert {(nb, w) for nb, _, w in cs} == {(nb, w) for nb in P.CS_BLOCKS for w in P.CS_WIDTHS}
    assert all(nb * nv * w <= P.MAX_ELEMS for nb, nv, w in cs)
    pc = P.prep_cases()
    assert {(bf, r, a) for bf, r, a, _ in pc} == {(bf, r, a) for bf in (True, False) for r in P.PREP_ROWS for a in range(1, 9)}
    assert {(r, pad) for _, r, _, pad in pc} == {(r, pad) for r in P.PREP_ROWS for pad in (8, 16)}
    assert P.PREP_ROWS[-1] > 2 * P.PREP_BLOCKS * 256 and P.PREP_ROWS[-2] == P.PREP_BLOCKS * 256 + 1


def test_mask_bit_layout_is_the_documented_one():
    rng = np.random.default_rng(0)
    for cols in (128, 256):
        mask = rng.random((5, cols)) < 0.5
        words = P.pack_mask_bits(mask)
        assert words.shape == (5, cols // 32) and np.array_equal(P.unpack_mask_bits(words, cols), mask)
        for f in range(cols):                                      # feature 32 mt + 16 h + r -> bit (mt & 1) 8 + (r >> 1) + 16 (r & 1) of word h (cols / 64) + (mt >> 1)
            mt, h, r = f >> 5, (f >> 4) & 1, f & 15
            one = np.zeros((1, cols), dtype=bool)
            one[0, f] = True
            w = P.pack_mask_bits(one)[0]
            want = np.zeros(cols // 32, dtype=np.uint32)
            want[h * (cols // 64) + (mt >> 1)] = np.uint32(1) << np.uint32((mt & 1) * 8 + (r >> 1) + 16 * (r & 1))
            assert np.array_equal(w, want), (cols, f)
        assert not np.array_equal(P.unpack_mask_bits(words, cols, "halves_swapped"), mask)


RELU = P.relu_cases()


@pytest.mark.parametrize("c", RELU, ids=[c.id for c in RELU])
def test_relu_bwd_restatement_matches_torch_and_is_exact(c):
    x = P.relu_inputs(c.bf16, c.cols, c.rows)
    ref = P.relu_ref(x)
    a, dA = _t(x.a_bits), _t(x.dA_bits)
    want = torch.where(a > 0, dA, torch.zeros_like(dA))
    assert np.array_equal(_b(want), ref.dz_bits) and np.array_equal(x.mask, (a > 0).numpy())
    assert np.array_equal(ref.p64.sum(0), want.double().sum(0).numpy()) and ref.n.sum() == c.rows
    P.assert_exact(ref.abs64)
    assert np.array_equal(P.from_bits(ref.partial_bits).astype(np.float64), ref.p64)
    if c.rows:
        # every row has a nonzero passed and a nonzero masked entry in every thread's column group
        per = P.per_of(c.bf16)
        v = P.from_bits(x.dA_bits).reshape(c.rows, c.cols // per, per)
        m = x.mask.reshape(c.rows, c.cols // per, per)
        assert bool(((v != 0) & m).any(2).all()) and bool(((v != 0) & ~m).any(2).all())
    if c.rows * c.cols >= 4096:
        for table in (P.POS_BITS[c.bf16], P.NEG_BITS[c.bf16]):
            assert all(bool((x.a_bits == b).any()) for b in table), "a special activation value is missing"


HEAD = P.head_cases()


@pytest.mark.parametrize("c", HEAD, ids=[c.id for c in HEAD])
def test_head_bwd_restatement_matches_torch_and_is_exact(c):
    x = P.head_inputs(c.form, c.cols, c.rows, c.a_dim)
    ref = P.head_ref(x)
    v = torch.from_numpy(x.dout).double() @ torch.from_numpy(x.W).double()
    m = torch.from_numpy(x.mask)
    assert np.array_equal(x.mask, (_t(x.a_bits) > 0).numpy())
    want = torch.where(m, v, torch.zeros_like(v)).to(torch.bfloat16 if c.bf16 else torch.float32)
    assert np.array_equal(_b(want), ref.dz_bits)
    assert np.array_equal(want.double().numpy(), torch.where(m, v, torch.zeros_like(v)).numpy()), "a rounding was not exact"
    P.assert_exact(ref.abs64, ref.absv)
    assert float(ref.absv.max(initial=0)) <= 256 and np.array_equal(ref.p64.sum(0), want.double().sum(0).numpy())
    if c.form == "bits":
        assert np.array_equal(P.unpack_mask_bits(P.pack_mask_bits(x.mask), c.cols), x.mask)


@pytest.mark.parametrize("window", P.DW_WINDOWS, ids=[str(w) for w in P.DW_WINDOWS])
def test_dw_finish_restatement_matches_torch_and_is_exact(window):
    M, K, m_out, k_out, ld = window
    for nb, tail in P.dw_pairs(window):
        x = P.dw_inputs(window, nb, tail)
        img, terms = P.dw_ref(x)
        P.assert_exact(terms)
        bucket = torch.from_numpy(x.bucket.copy()).double()
        grad = torch.as_strided(bucket, (m_out, k_out), (ld, 1), P.DW_OFFSET)
        grad += (torch.from_numpy(x.partial).double().sum(0) + torch.from_numpy(x.dz_tail).double().t() @ torch.from_numpy(x.a_tail).double())[:m_out, :k_out]
        assert np.array_equal(img["bucket"][P.G:-P.G], RK.f32_bits(bucket.float().numpy())), (nb, tail)
        assert np.array_equal(bucket.float().double().numpy(), bucket.numpy())


def test_colsum_finish_restatement_matches_torch_and_is_exact():
    for nb, nv, w in P.colsum_cases():
        x = P.colsum_inputs(nb, nv, w)
        img, terms = P.colsum_ref(x)
        P.assert_exact(terms)
        bucket = torch.from_numpy(x.bucket.copy()).double()
        s = torch.from_numpy(x.partial).double().sum(0)
        for v, o in enumerate(x.offs):
            bucket[o:o + w] += s[v]
        assert np.array_equal(img["bucket"][P.G:-P.G], RK.f32_bits(bucket.float().numpy())), (nb, nv, w)


@pytest.mark.parametrize("rows", P.PREP_ROWS)
def test_head_prep_restatement_matches_torch_and_is_exact(rows):
    for bf, r, a_dim, pad in P.prep_cases():
        if r != rows:
            continue
        for real in ((False, True) if a_dim in (3, 8) and rows in (257, 262145) else (False,)):
            dout = P.prep_inputs(rows, a_dim, real)
            ref = P.prep_ref(dout, pad, bf)
            want = torch.zeros(rows, pad, dtype=torch.bfloat16 if bf else torch.float32)
            want[:, :a_dim] = torch.from_numpy(dout)
            assert np.array_equal(_b(want), ref.dz_bits)
            assert np.array_equal(ref.p64.sum(0), torch.from_numpy(dout).double().sum(0).numpy()) or real
            if not real:
                P.assert_exact(ref.abs64)


def test_dw_gemm_inputs_are_exact():
    for rows in P.DW_GEMM_ROWS:
        for M, K in P.DW_GEMM_SHAPES:
            P.assert_exact(P.dw_gemm_inputs(rows, M, K)[4])
    for rows in P.DW_SPLIT_ROWS:
        dz, a, g0, want, terms = P.dw_gemm_inputs(rows, 64, 64)
        P.assert_exact(terms)
        assert rows >= 128 * 4096 and (rows - 128 * (rows // 128)) in (0, 127)
        assert np.array_equal(want, g0 + (torch.from_numpy(dz).double().t() @ torch.from_numpy(a).double()).numpy())


# --------------------------------------------------------------------------------------------------------------------------------
# 2. planted wrong kernels
# --------------------------------------------------------------------------------------------------------------------------------
def test_checkers_reject_wrong_relu_bwd_kernels():
    for bf, cols in ((True, 136), (False, 12)):
        per = P.per_of(bf)
        rp = P.rpp_of(cols, per)
        for rows, mutants in ((rp + 1, ("drop_last_row", "mask_shift", "neg_zero_positive", "partial_unwritten", "guard_overwrite")),
                              (2048 * rp + 1, ("drop_last_row", "drop_wrap_row", "mask_shift", "neg_zero_positive")),
                              (1, ("drop_last_row", "partial_unwritten"))):
            x = P.relu_inputs(bf, cols, rows)
            good = P.relu_image(P.relu_ref(x))
            P.check_image(good, P.relu_image(P.relu_ref(x)))
            for mu in mutants:
                _rejected(P.relu_image(P.relu_ref(x, mu), mu), good, f"{bf} {cols} {rows} {mu}")


def test_checkers_reject_wrong_head_bwd_kernels():
    for form, cols, a_dim in (("f32", 40, 3), ("bf16", 96, 5), ("bits", 128, 3), ("bits", 256, 5), ("f32", 8, 7), ("bf16", 40, 6)):
        rp = P.rpp_of(cols, 8)
        for rows in (1, rp + 1, 2048 * rp + 1):
            x = P.head_inputs(form, cols, rows, a_dim)
            good = P.head_image(P.head_ref(x))
            mutants = ["drop_last_row", "guard_overwrite", "w_leak"]
            if rows <= rp + 1:                                      # most blocks own no rows
                mutants += ["partial_unwritten"]
            if rows > 1:
                mutants += ["dout_stride_ka"]
            if rows > 2048 * rp:
                mutants += ["drop_wrap_row"]
            mutants += ["halves_swapped"] if form == "bits" else ["mask_shift", "neg_zero_positive"]
            for mu in mutants:
                _rejected(P.head_image(P.head_ref(x, mu), mu), good, f"{form} {cols} {a_dim} {rows} {mu}")


def test_rounding_probe_and_real_checker_reject_truncation():
    W, want = P.rne_probe()
    x = P.head_inputs("bf16", 96, 3, 1)
    x = type(x)(**{**vars(x), "dout": np.ones((3, 1), np.float32), "W": W, "a_bits": np.full((3, 96), 0x3F80, np.uint16), "mask": np.ones((3, 96), bool)})
    good = P.head_ref(x)
    assert np.array_equal(good.dz_bits, np.broadcast_to(want, (3, 96)))
    assert not np.array_equal(P.head_ref(x, "bf16_truncate").dz_bits, good.dz_bits)
    # real-valued inputs: RNE passes the interval check, truncation (an error of up to one whole bf16 step) does not
    xr = P.head_inputs("bf16", 96, 257, 5, real=True)
    ref = P.head_ref(xr)
    assert P.check_head_real(ref.dz_bits, xr, ref) <= 1.0
    with pytest.raises(AssertionError):
        P.check_head_real(P.head_ref(xr, "bf16_truncate").dz_bits, xr, ref)
    for form in ("f32", "bf16"):                                  # a product formed in fp32 in either contraction order stays inside
        xr = P.head_inputs(form, 40, 52, 7, real=True)
        ref = P.head_ref(xr)
        s = np.zeros((52, 40), np.float32)
        for k in range(7):
            s = (s + (xr.dout[:, k:k + 1] * xr.W[k:k + 1, :]).astype(np.float32)).astype(np.float32)
        got = np.where(ref.mask, P.to_bits(s, xr.bf16), 0).astype(ref.dz_bits.dtype)
        assert P.check_head_real(got, xr, ref) <= 1.0
    # a partial row that lost a value is outside the summation bound
    xr = P.relu_inputs(True, 24, 86, real=True)
    ref = P.relu_ref(xr)
    assert P.check_partial_real(ref.partial_bits, ref.dz_bits, xr.rpp, P.BLOCKS) <= 1.0
    with pytest.raises(AssertionError):
        P.check_partial_real(P.relu_ref(xr, "drop_last_row").partial_bits, ref.dz_bits, xr.rpp, P.BLOCKS)


def test_checkers_reject_wrong_dw_finish_and_colsum_kernels():
    w = P.DW_WINDOWS[3]
    for nb, tail, mutants in ((9, 9, ("drop_remainder", "drop_tail_last", "overwrite", "guard_overwrite")), (7, 1, ("drop_remainder", "drop_tail_last")),
                              (17, 4096, ("drop_remainder", "drop_tail_last")), (0, 0, ("overwrite",))):
        x = P.dw_inputs(w, nb, tail)
        good, _ = P.dw_ref(x)
        for mu in mutants:
            _rejected(P.dw_ref(x, mu)[0], good, f"dw {nb} {tail} {mu}")
    for nb, nv, width in ((17, 3, 65), (0, 2, 3), (1, 8, 1)):
        x = P.colsum_inputs(nb, nv, width)
        good, _ = P.colsum_ref(x)
        for mu in ("overwrite", "guard_overwrite"):
            _rejected(P.colsum_ref(x, mu)[0], good, f"colsum {nb} {nv} {width} {mu}")


def test_checkers_reject_wrong_head_prep_kernels():
    for bf in (True, False):
        for rows in (1, 257, 262145):
            dout = P.prep_inputs(rows, 5)
            good = P.prep_image(P.prep_ref(dout, 16, bf))
            for mu in ("drop_last_row", "pad_unwritten") + (("partial_unwritten",) if rows < 262144 else ("drop_wrap_row",)):
                mutant = P.prep_ref(dout, 16, bf, mu)
                if mu == "drop_wrap_row":                          # the first row of the second grid-stride trip
                    keep = np.ones(rows, bool)
                    keep[P.PREP_BLOCKS * 256] = False
                    mutant.dz_bits[~keep] = P.NAN16 if bf else P.NAN32
                _rejected(P.prep_image(mutant), good, f"prep {bf} {rows} {mu}")
    dout = P.prep_inputs(257, 3, real=True)
    _rejected(P.prep_image(P.prep_ref(dout, 8, True, "bf16_truncate")), P.prep_image(P.prep_ref(dout, 8, True)), "prep truncate")


# --------------------------------------------------------------------------------------------------------------------------------
# 3. supports() and the kernels' width limits
# --------------------------------------------------------------------------------------------------------------------------------
def test_a_net_turned_away_for_its_width_is_logged_once(caplog):
    import logging
    import trajopt_grpo_amd as tg
    with torch.device("meta"):
        wide, fine = tg.NeuralNetwork(7, 3, (1040, 16), "ReLU"), tg.NeuralNetwork(7, 3, (16, 1040), "ReLU")
    with caplog.at_level(logging.INFO, logger="trajopt_grpo_amd"):
        for _ in range(2):
            tg.mlp.log_too_wide(wide, torch.float32)
            tg.mlp.log_too_wide(fine, torch.float32)                # (supported: the top hidden layer may be 2048 wide)
            tg.mlp.log_too_wide(wide, torch.bfloat16)
    lines = [r.getMessage() for r in caplog.records if "torch autograd" in r.getMessage()]
    assert len(lines) == 1 and lines[0].startswith("7-1040-16-3 float32") and "1024" in lines[0] and "2048" in lines[0]


def test_supports_follows_the_per_layer_kernels_width_limits():
    import trajopt_grpo_amd as tg
    M, lib = tg.mlp, tg._native.load()
    assert (lib.tg_relu_bwd_bias_max_cols(1), lib.tg_relu_bwd_bias_max_cols(0), lib.tg_head_bwd_relu_bias_max_cols()) == (2048, 1024, 2048)
    assert M.per_layer_width_limits(torch.bfloat16, 1) == (2048, 2048) and M.per_layer_width_limits(torch.float32, 8) == (1024, 2048)
    assert M.per_layer_width_limits(torch.float32, 12) == (1024, 1024)
    seen = set()
    for cd, bf in ((torch.bfloat16, True), (torch.float32, False)):
        for n_hidden in (1, 2, 3):
            for top in P.LIMIT_WIDTHS:
                for below in (P.LIMIT_WIDTHS if n_hidden > 1 else [8]):
                    widths = (8,) * max(n_hidden - 2, 0) + ((below,) if n_hidden > 1 else ()) + (top,)
                    for order in ({widths, widths[::-1]} if n_hidden == 3 else {widths}):
                        with torch.device("meta"):
                            net = tg.NeuralNetwork(5, 1, order, "ReLU")
                        want = P.width_ok(order, bf)
                        assert M.supports(net, cd) is want, (cd, order)
                        seen.add(want)
    assert seen == {True, False}
    with torch.device("meta"):
        wide_head, odd = tg.NeuralNetwork(5, 12, (8, 1032), "ReLU"), tg.NeuralNetwork(5, 1, (12,), "ReLU")
    assert M.supports(wide_head, torch.bfloat16) and not M.supports(wide_head, torch.float32) and P.width_ok((8, 1032), False, 12) is False
    assert not M.supports(odd, torch.bfloat16)
    # the default compute dtype is float32, the stricter of the two
    with torch.device("meta"):
        net = tg.NeuralNetwork(20, 4, (1536, 1536), "ReLU")
    assert not M.supports(net) and M.supports(net, torch.bfloat16)
