"""tests/chain_exact_ref.py against itself, without a device: every case test_chain_exact_gpu.py runs meets conditions (a)-(d) (the
reference functions assert them), every planted wrong kernel (`mutant=`) gives another image than the reference on every case it
applies to, the layout restatements round-trip and agree with the older helpers, the rounding helper agrees with torch, and the
weight-gradient row counts reach the launch edges they are named for (check_dw_table, on the restated host code)."""
import functools

import numpy as np
import pytest
import torch

import chain_exact_ref as R
import per_layer_ref as P
import row_kernels_ref as RK

FWD, BWD, DW = R.forward_cases(), R.backward_cases(), R.dw_cases()


def _differs(a, b):
    assert set(a) == set(b)
    return any(not np.array_equal(a[k], b[k]) for k in a)


def _forward(c, mutant=None):
    rows = R.rows_of(c.rows)
    net = R.make_net(c.S, c.A, c.H, c.nh, probe=c.probe)
    fwd = R.forward_ref(net, R.make_x(c.S, rows), mutant)
    return net, fwd, R.forward_image(net, fwd, c.out_cols, c.panel, c.variant, mutant)


@pytest.mark.parametrize("c", FWD, ids=[c.id for c in FWD])
def test_forward_cases_meet_the_conditions_and_see_every_mutant(c):
    net, fwd, img = _forward(c)
    rows = R.rows_of(c.rows)
    assert img["out"].size == rows * c.out_cols + 2 * R.G
    if c.probe:
        assert fwd.ties >= 100 and fwd.inexact >= 100, (fwd.ties, fwd.inexact)
        assert any(not np.array_equal(a, np.rint(a)) or float(a.max()) > 256 for a in fwd.acts)
    else:
        assert fwd.ties == 0 and fwd.inexact == 0 and max(float(a.max()) for a in fwd.acts) <= 256
    for m in R.mutants_for("fwd", c):
        assert _differs(img, _forward(c, m)[2]), f"{c.id} cannot see {m}"


@functools.lru_cache(maxsize=1)
def _masks(S, A, H, nh, probe, rows):
    return R.forward_ref(R.make_net(S, A, H, nh, probe=probe), R.make_x(S, rows)).masks


def _backward(c, mutant=None):
    rows = R.rows_of(c.rows)
    net = R.make_net(c.S, c.A, c.H, c.nh, probe=c.probe)
    x = R.make_x(c.S, rows)
    masks = _masks(c.S, c.A, c.H, c.nh, c.probe, rows)
    bwd = R.backward_ref(net, masks, R.make_dout(c.A, rows, probe=c.probe), x, mutant)
    return net, bwd, {m: R.backward_image(net, bwd, m, mutant=mutant) for m in c.modes}


@pytest.mark.parametrize("c", BWD, ids=[c.id for c in BWD])
def test_backward_cases_meet_the_conditions_and_see_every_mutant(c):
    net, bwd, imgs = _backward(c)
    if c.probe:
        assert bwd.ties >= 100 and bwd.inexact >= 100, (bwd.ties, bwd.inexact)
    else:
        assert bwd.ties == 0 and bwd.inexact == 0 and max(float(np.abs(z).max()) for z in bwd.dz) <= 256
    assert all(np.abs(z).any() for z in bwd.dz)
    for m in R.mutants_for("bwd", c):
        mut = _backward(c, m)[2]
        for mode in c.modes:
            if m == "double_last_row" and mode not in ("partial", "w0", "panel_w0"):
                continue
            assert _differs(imgs[mode], mut[mode]), f"{c.id} ({mode}) cannot see {m}"


@pytest.mark.parametrize("c", DW, ids=[c.id for c in DW])
def test_weight_gradient_cases_meet_the_conditions_and_see_every_mutant(c):
    rows = R.dw_rows(c)
    inp = R.dw_inputs(c.H, rows, c.jobs)
    img, grads = R.dw_ref(inp)
    assert all(np.abs(dW).any() for dW, _ in grads)
    for j in inp.jobs:                                               # the operands hold exactly their documented element counts
        wide_p, wide_q = j.kind in (R.HH, R.HX, R.HR), j.kind in (R.HH, R.DH, R.RH)
        assert j.p.size == (R.pad32(rows) if j.layout & R.PANEL_P else rows) * (c.H if wide_p else 8)
        assert j.q.size == (R.pad32(rows) if j.layout & R.PANEL_Q else rows) * (c.H if wide_q else 32)
    for m in R.mutants_for("dw", c, rows):
        assert not np.array_equal(img, R.dw_ref(inp, m)[0]), f"{c.id} cannot see {m}"


def test_weight_gradient_row_counts_reach_their_edges():
    R.check_dw_table()
    R.check_dw_table(cus=304)                                        # (another CU count: the table is not tuned to 256)
    assert [R.ring_depth(256, k) for k in range(5)] == [4, 8, 8, 7, 7] and [R.ring_depth(128, k) for k in range(5)] == [8] * 5


@pytest.mark.parametrize("name,n_loss", R.RIDER_CASES)
def test_rider_cases_see_their_mutants(name, n_loss):
    r = R.rider_inputs(name, n_loss)
    img = R.rider_ref(r)
    if any(g.n_slabs for g in r.regions) or (r.loss is not None and n_loss):
        assert _differs(img, R.rider_ref(r, "skip_slab"))
    if r.regions:
        assert _differs(img, R.rider_ref(r, "extra_slab"))


def test_rider_table_covers_the_issue():
    sets = [g for name, _ in R.RIDER_CASES for g in R.RIDER_SETS[name]]
    assert {g[0] for g in sets} == {0, 1, 3, 4, 5, 96, 97, 131, 1024}
    assert {len(R.RIDER_SETS[name]) for name, _ in R.RIDER_CASES} == {0, 1, 2, 3, 4}
    assert any((g[1] * g[2]) % 64 for g in sets) and any(g[3] > g[2] and g[5] > g[2] for g in sets)
    assert {n for _, n in R.RIDER_CASES if n is not None} == {0, 1, 63, 64, 65, 256}


@pytest.mark.parametrize("H", [128, 256])
@pytest.mark.parametrize("rows", [1, 31, 32, 33, 100])
def test_panel_formula_round_trips(H, rows):
    rng = np.random.default_rng(rows + H)
    bits = rng.integers(0, 2 ** 16, size=(rows, H)).astype(np.uint16)
    flat = R.to_panel(bits)
    assert flat.size == R.pad32(rows) * H and np.array_equal(R.from_panel(flat, rows, H), bits)
    full = R.from_panel(flat, R.pad32(rows), H)
    assert np.array_equal(full[rows:], np.broadcast_to(bits[-1], (R.pad32(rows) - rows, H)))
    idx = R.panel_chunks(R.pad32(rows), H).reshape(-1)
    assert np.array_equal(np.sort(idx), np.arange(idx.size))        # a permutation of the whole tiles
    # a 32-row tile is 64 H contiguous bytes, and 4 rows x 4 chunks make one 256-byte run
    assert idx.reshape(-1, 32, H // 8)[0].max() == 32 * H // 8 - 1
    pad = np.full(H, 7, dtype=np.uint16)
    assert np.array_equal(R.from_panel(R.to_panel(bits, pad), R.pad32(rows), H)[rows:], np.broadcast_to(pad, (R.pad32(rows) - rows, H)))


@pytest.mark.parametrize("H", [128, 256])
def test_mask_packer_agrees_with_the_per_layer_helper(H):
    rng = np.random.default_rng(H)
    mask = rng.random((77, H)) < 0.5
    assert np.array_equal(R.pack_mask(mask), P.pack_mask_bits(mask))
    one = np.zeros((H, H), dtype=bool)
    one[np.arange(H), np.arange(H)] = True                           # feature f alone: exactly the documented bit of the documented word
    word, bit = R.mask_places(H)
    got = R.pack_mask(one)
    assert all(got[f, word[f]] == 1 << bit[f] and np.count_nonzero(got[f]) == 1 for f in range(H))


def test_rounding_helper_agrees_with_torch():
    probes = [np.arange(-70000, 70001, dtype=np.float64)]
    for c in [c for c in FWD if c.probe]:
        net = R.make_net(c.S, c.A, c.H, c.nh, probe=True)
        x = R.make_x(c.S, R.rows_of(c.rows))
        a0 = np.maximum(x[:, :c.S] @ net.W[0].T + net.b[0], 0.0)
        probes += [a0.reshape(-1), np.maximum(R.round_int(a0) @ net.W[1].T + net.b[1], 0.0).reshape(-1)]
    for c in [c for c in BWD if c.probe]:
        net = R.make_net(c.S, c.A, c.H, c.nh, probe=True)
        probes.append((R.make_dout(c.A, R.rows_of(c.rows), probe=True)[:, :c.A] @ net.Wh).reshape(-1))
    v = np.concatenate(probes)
    want = torch.from_numpy(v.astype(np.float32)).to(torch.bfloat16).to(torch.float64).numpy()
    assert np.array_equal(R.round_int(v), want)
    assert np.array_equal(R.round_int(v), P.from_bits(RK.bf16_bits(v.astype(np.float32))).astype(np.float64))
    assert np.array_equal(R.round_int(v, "truncate"), P.from_bits(RK.bf16_bits(v.astype(np.float32), truncate=True)).astype(np.float64))
    assert np.array_equal(R.bf16_bits(want), P.to_bits(want, True))   # the pattern helper against the older one, on every rounded value
    ties, inexact = R.rounding_stats(v)
    assert ties > 100 and inexact > 100
    assert R.round_int(257.0) == 256 and R.round_int(259.0) == 260 and R.round_int(514.0) == 512 and R.round_int(518.0) == 520
    assert R.round_int(257.0, "half_away") == 258 and R.round_int(-257.0, "half_away") == -258 and R.round_int(259.0, "truncate") == 258
    assert R.round_int(513.0) == 512 and R.round_int(515.0) == 516 and R.round_int(-515.0, "truncate") == -512


def test_images_carry_their_guards_and_nan_prefill():
    c = next(c for c in FWD if c.variant == "no_a0" and not c.panel and isinstance(c.rows, int))
    net, fwd, img = _forward(c)
    assert np.array_equal(img["act0"], R.guarded(R.nan_words(257 * c.H, np.uint16)))
    assert not np.array_equal(img["mask0"], R.guarded(R.nan_words(257 * c.H // 32, np.uint32)))
    for v in img.values():
        assert np.array_equal(v[:R.G], R.nan_words(R.G, v.dtype)) and np.array_equal(v[-R.G:], R.nan_words(R.G, v.dtype))
    assert np.array_equal(img["out"][R.G:-R.G].view(np.float32).reshape(257, c.out_cols)[:, :c.A], fwd.out.astype(np.float32))
