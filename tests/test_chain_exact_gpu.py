"""The three kernels of the bf16 chain learner on the MI355X (run with `-m gpu`), bit for bit against tests/chain_exact_ref.py:
tg_mlp_forward_chain[_ex], tg_mlp_backward_chain[_w0|_ex] and tg_mlp_weight_grad[_ex], each called through the C ABI on INTEGER nets,
whose every product, partial sum and stored bf16 value is exact in any order (conditions (a)-(d) of the reference, asserted per case):
the kernel's output is one determined bit pattern, and a dropped, doubled or mis-addressed row, feature, k-block, pad row or slab is a
bit mismatch.  The rounding probes push the same nets past 256, where odd integers are exact bf16 ties: round-to-nearest-even is the
only conversion that matches.  There is no tolerance anywhere in this module.

Every input buffer holds exactly its documented element count between 64 NaN guard words (the weight streams are copies of
mlp.FragmentStream's, the recompute kinds get exactly the first block, 32 H elements); every output buffer is NaN between guards before a
launch; every gradient target is a window into a bucket of nonzero integers; every launch runs twice on fresh buffers and must return
the same bits; the comparison is per_layer_ref.check_image: the whole buffer, guards included.  Sizes that depend on the device come
from the library: tg_mlp_forward_chain_blocks(), tg_mlp_backward_chain_blocks(), tg_mlp_weight_grad_workspace() (one H x H + H slab
per CU: the CU count the host code splits between the jobs).

WHICH ROW COUNT REACHES WHICH EDGE

Forward and backward chain (chain_launch / launch_bwd_chain: a workgroup of 8 waves takes a ROUND of 8 x 32 = 256 rows, round r goes
to workgroup r % grid, grid = min(blocks, ceil(rows / 256))):
  1                 one row: 31 clamped tail rows in the only wave that works
  31 / 32 / 33      the 32-row tile of a wave (and of the panel-order layout: 31 and 33 leave pad rows, copies of the last row)
  255 / 256 / 257   the round: one workgroup with a ragged last wave / exactly full / a second workgroup with one row
  B - 1, B, B + 1   B = blocks x 256: every workgroup has one full round (the last one short by a row) / workgroup 0 starts its SECOND
                    round with one row: the prefetch of round + grid, the ring carried across rounds
  B + 257           workgroup 0's second round is full and workgroup 1 starts its second round with one row
The large counts run H = 128 x 3 layers; H = 256 x 3 once per kernel (B + 257).  Shapes: H 128 / 256, 1 / 2 / 3 / 6 / 8 hidden layers
forward (3 / 4 / 6 backward), S 1 / 5 / 20 / 32, A 1 / 4 / 8 / 12 with out_cols 4 / 8 / 16.

Weight gradient (tg_mlp_weight_grad_ex: stages of kDwStageRows = 32 rows, n_st = ceil(rows / 32); cap = 1 below 4 stages, else
n_st / 4; a job gets alloc = its share of the CUs by dw_row_cost and runs min(alloc, cap) workgroups, workgroup w of a job walking
stages w, w + n, ...; ring depths DwRing::D: HH 4 slots at H = 256, HR / RH 7, HX / DH 8, everything 8 at H = 128):
  1, 31 | 32        n_st = 1, partial | full: one workgroup, the masked last-stage instantiation alone
  33 | 64           n_st = 2          65 | 96    n_st = 3: two / three stages in ONE workgroup (cap = 1), fewer than the ring's prologue
  97, 127 | 128     n_st = 4: cap = n_st / 4 first applies (still 1)
  129 | 160         n_st = 5          223 | 224  n_st = 7
  255 | 256         n_st = 8: cap = 2, two workgroups per job, 4 stages each
  257 | 288         n_st = 9: 5 and 4 stages
  97 / 1000         every kind alone in every legal layout (cap binds: 1 and 8 workgroups)
  "bind"            chain_exact_ref.binding_rows(): n_st = 8.5 x the smallest narrow job's alloc, less 5 rows -- alloc < cap, so the
                    ALLOCATION limits the job and its workgroups walk 8 or 9 stages, more than the 7-8 slots of the narrow rings (the
                    ring wraps); run on the 8-job set at both widths and on the learner's 5-layer set
  70,001            n_st = 2,188, cap = 547 > every alloc: each workgroup walks >= 3 ring depths (27-122 stages), ragged last stage
check_dw_table() asserts all of this on the restated host code with the CU count read from the library.  Job sets: one job; the
learner's sets for 3 and 5 hidden layers (RH, HH.., HR: what GemmMLP.backward_fused launches); 8 jobs (every kind, HH / HX / DH twice).
Windows cycle through full, m_out < M, n_out < N, wgrad_ld > n_out and 1 x 1; DH's m_out runs 1..8.  Panel-order operands carry +-3 in
their pad rows (the contract multiplies them by zero; NaN there would be a broken case).

Riders (dw_finish_all_kernel): n_slabs 0 / 1 / 3 (remainder loop only) / 4 (one unrolled trip) / 5 / 96 (the last one-lane count) /
97 / 131 / 1024 (32 lanes per element, > 96 slabs), 1-4 regions, 35 and 132 elements (off a multiple of 64), row_pitch > n_out with
grad_ld > n_out; the f64 loss rider with 0 / 1 / 63 / 64 / 65 / 256 rows onto nonzero sums.  The job's own gradient is compared with
the same image in every rider case: the riders' presence does not change it."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import chain_exact_ref as R
import per_layer_ref as P

pytestmark = pytest.mark.gpu
G = R.G
_SIGNED = {2: np.int16, 4: np.int32, 8: np.int64}
FWD, BWD, DW = R.forward_cases(), R.backward_cases(), R.dw_cases()


@pytest.fixture(scope="module")
def tg():
    import trajopt_grpo_amd as tg
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return tg


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


class _Buf:
    """Patterns between NaN guards on the device: .ptr = the first word behind the front guard; .back() = everything, as patterns."""

    def __init__(self, bits, dev):
        bits = np.ascontiguousarray(bits).reshape(-1)
        self.dtype, self.n = bits.dtype, bits.size
        self.whole = torch.from_numpy(R.guarded(bits).view(_SIGNED[bits.dtype.itemsize])).to(dev)
        self.ptr = self.whole.data_ptr() + G * bits.dtype.itemsize
        assert self.ptr % 16 == 0

    def back(self):
        return self.whole.cpu().numpy().view(self.dtype)


def _nan(n, dtype, dev):
    return _Buf(R.nan_words(n, dtype), dev)


def _ptrs(items):
    return (C.c_void_p * len(items))(*items)


def _twice(run):
    a, b = run(), run()
    for k in a:
        assert np.array_equal(a[k], b[k]), f"{k}: a repeated launch differs"
    return a


@functools.lru_cache(maxsize=None)
def _streams(S, A, H, nh, seed=0, probe=False):
    """The net's weight streams as mlp.FragmentStream builds them, copied back as patterns: forward stream, bias table f32
    [nh + 1][H], backward (transposed) stream."""
    import trajopt_grpo_amd as tg
    from trajopt_grpo_amd import mlp as M
    net = R.make_net(S, A, H, nh, seed, probe)
    dev = torch.device("cuda", 0)
    tnet = tg.NeuralNetwork(S, A, (H,) * nh, "ReLU").to(dev)
    lin = [m for m in tnet.network if isinstance(m, torch.nn.Linear)]
    with torch.no_grad():
        for l, (W, b) in zip(lin, list(zip(net.W, net.b)) + [(net.Wh, net.bh)]):
            l.weight.copy_(torch.from_numpy(np.ascontiguousarray(W, dtype=np.float32)))
            l.bias.copy_(torch.from_numpy(np.ascontiguousarray(b, dtype=np.float32)))
    fs = M.FragmentStream(tnet, H, layout="chain")
    bs = M.FragmentStream(tnet, H, layout="chain", transposed=True)
    torch.cuda.synchronize()
    u16 = lambda t: t.detach().contiguous().view(torch.int16).cpu().numpy().view(np.uint16).reshape(-1)
    bias = fs.bias.detach().contiguous().cpu().numpy().view(np.uint32).reshape(-1)
    assert bias.size == (nh + 1) * H
    return R.NS(net=net, fwd=u16(fs.stream), bias=bias, bwd=u16(bs.stream))


# --------------------------------------------------------------------------------------------------------------------------------
# forward chain
# --------------------------------------------------------------------------------------------------------------------------------
def _run_forward(N, dev, c, rows, st, x_bits, entry):
    lib, H, nh = N.load(), c.H, c.nh
    x, w, b = _Buf(x_bits, dev), _Buf(st.fwd, dev), _Buf(st.bias, dev)
    acts = [_nan((R.pad32(rows) if c.panel else rows) * H, np.uint16, dev) for _ in range(nh)]
    masks = [_nan(rows * H // 32, np.uint32, dev) for _ in range(nh)]
    out = _nan(rows * c.out_cols, np.uint32, dev)
    a_ptrs = None if c.variant == "no_acts" else _ptrs([None if (c.variant == "no_a0" and l == 0) else acts[l].ptr for l in range(nh)])
    m_ptrs = None if c.variant in ("no_acts", "no_masks") else _ptrs([m.ptr for m in masks])
    if entry == "plain":
        N.check(lib.tg_mlp_forward_chain(x.ptr, w.ptr, b.ptr, H, nh, rows, a_ptrs, m_ptrs, out.ptr, c.out_cols, N.stream_ptr(dev)), "forward")
    else:
        N.check(lib.tg_mlp_forward_chain_ex(x.ptr, w.ptr, b.ptr, H, nh, rows, a_ptrs, m_ptrs, out.ptr, c.out_cols,
                                            N.TG_LAYOUT_PANEL if c.panel else N.TG_LAYOUT_ROWS, N.stream_ptr(dev)), "forward_ex")
    torch.cuda.synchronize()
    got = {f"act{l}": acts[l].back() for l in range(nh)}
    got.update({f"mask{l}": masks[l].back() for l in range(nh)})
    got["out"] = out.back()
    return got


@pytest.mark.parametrize("c", FWD, ids=[c.id for c in FWD])
def test_forward_chain_is_exact(tg, dev, c):
    """Stored activations (row-major, or panel order through the header formula with the pad rows copies of the last row), mask words
    and the head output with its padded columns; the variants leave everything else unchanged; the probes pin round-to-nearest-even."""
    N = tg._native
    rows = R.rows_of(c.rows, N.load().tg_mlp_forward_chain_blocks())
    st = _streams(c.S, c.A, c.H, c.nh, 0, c.probe)
    x = R.make_x(c.S, rows)
    fwd = R.forward_ref(st.net, x)
    assert not c.probe or (fwd.ties >= 100 and fwd.inexact >= 100)
    want = R.forward_image(st.net, fwd, c.out_cols, c.panel, c.variant)
    x_bits = R.bf16_bits(x)
    entries = ["ex", "ex"] if c.panel else ["plain", "ex"]           # row-major: the plain entry point, then _ex with TG_LAYOUT_ROWS
    it = iter(entries)
    got = _twice(lambda: _run_forward(N, dev, c, rows, st, x_bits, next(it)))
    P.check_image(got, want, c.id)
    print(f"fwd {c.id} rows {rows}: {len(want)} buffers, bitwise" + (f" ({fwd.ties} ties, {fwd.inexact} inexact)" if c.probe else ""))


# --------------------------------------------------------------------------------------------------------------------------------
# backward chain
# --------------------------------------------------------------------------------------------------------------------------------
def _run_backward(N, dev, c, rows, st, mode, dout_bits, mask_bits, x_bits, blocks):
    lib, H, nh = N.load(), c.H, c.nh
    panel, fused = mode.startswith("panel"), mode.endswith("w0")
    dout, w = _Buf(dout_bits, dev), _Buf(st.bwd, dev)
    masks = [_Buf(m, dev) for m in mask_bits]                        # bottom layer first; the kernel takes the TOP layer first
    m_ptrs = _ptrs([masks[nh - 1 - j].ptr for j in range(nh)])
    dz = [_nan((R.pad32(rows) if panel else rows) * H, np.uint16, dev) for _ in range(nh)]
    skip = {0} if mode == "lean" else ({0, nh - 1} if fused else set())
    d_ptrs = _ptrs([None if j in skip else dz[j].ptr for j in range(nh)])
    got, s = {}, N.stream_ptr(dev)
    x = slabs = partial = None
    n_slabs = C.c_int32(-1)
    if fused:
        x, slabs = _Buf(x_bits, dev), _nan(2 * blocks * H * 32, np.uint32, dev)
    if mode == "partial":
        partial = _nan(blocks * nh * H, np.uint32, dev)
        N.check(lib.tg_mlp_backward_chain(dout.ptr, w.ptr, H, nh, rows, d_ptrs, m_ptrs, partial.ptr, s), mode)
    elif mode == "lean":
        N.check(lib.tg_mlp_backward_chain(dout.ptr, w.ptr, H, nh, rows, d_ptrs, m_ptrs, None, s), mode)
    elif mode == "w0":
        N.check(lib.tg_mlp_backward_chain_w0(dout.ptr, w.ptr, H, nh, rows, d_ptrs, m_ptrs, x.ptr, slabs.ptr, slabs.n, C.byref(n_slabs), s), mode)
    else:
        N.check(lib.tg_mlp_backward_chain_ex(dout.ptr, w.ptr, H, nh, rows, d_ptrs, m_ptrs, x.ptr if fused else None, slabs.ptr if fused else None,
                                             slabs.n if fused else 0, C.byref(n_slabs), N.TG_LAYOUT_PANEL, s), mode)
    torch.cuda.synchronize()
    for j in range(nh):
        got[f"dz{j}"] = dz[j].back()
    if partial is not None:
        whole = partial.back()
        part = whole[G:-G].view(np.float32).reshape(blocks, nh, H)
        acc = np.zeros((nh, H), dtype=np.float32)
        for b in range(blocks):                                      # the caller's sum over the workgroups, in order, in fp32
            acc = acc + part[b]
        got["colsum"] = acc.view(np.uint32).reshape(-1)
        got["partial_guards"] = np.concatenate([whole[:G], whole[-G:]])
    if fused:
        whole, n = slabs.back(), n_slabs.value
        assert 0 <= n <= 2 * blocks
        acc = np.zeros(H * 32, dtype=np.float32)
        for k in range(n):
            acc = acc + whole[G + k * H * 32:G + (k + 1) * H * 32].view(np.float32)
        got["w0sum"], got["w0rest"], got["w0front"] = acc.view(np.uint32), whole[G + n * H * 32:], whole[:G]
        got["n_slabs"] = np.array([n], dtype=np.uint32)
    return got


@pytest.mark.parametrize("c", BWD, ids=[c.id for c in BWD])
def test_backward_chain_is_exact(tg, dev, c):
    """Every layer's dZ (masked entries +0), from mask bits built on the host; the column sums added over the workgroups in order; d_dz[0]
    = NULL leaves the other layers unchanged; _w0: the sum of the *n_slabs slabs = dZ_bottom^T [x | 1] with columns S..30 exactly
    zero and the top and bottom dZ unwritten; _ex: the same in panel order."""
    N = tg._native
    blocks = N.load().tg_mlp_backward_chain_blocks()
    rows = R.rows_of(c.rows, blocks)
    st = _streams(c.S, c.A, c.H, c.nh, 0, c.probe)
    x = R.make_x(c.S, rows)
    masks = R.forward_ref(st.net, x).masks
    dout = R.make_dout(c.A, rows, probe=c.probe)
    bwd = R.backward_ref(st.net, masks, dout, x)
    assert not c.probe or (bwd.ties >= 100 and bwd.inexact >= 100)
    for j, z in enumerate(bwd.dz):
        assert not R.bf16_bits(z)[~masks[c.nh - 1 - j]].any()          # masked entries are +0 in the reference image
    dout_bits, x_bits, mask_bits = R.bf16_bits(dout), R.bf16_bits(x), [R.pack_mask(m) for m in masks]
    n = 0
    for mode in c.modes:
        want = R.backward_image(st.net, bwd, mode, blocks)
        got = _twice(lambda: _run_backward(N, dev, c, rows, st, mode, dout_bits, mask_bits, x_bits, blocks))
        P.check_image(got, want, f"{c.id} [{mode}]")
        n += len(want)
    print(f"bwd {c.id} rows {rows}: {n} buffers over {len(c.modes)} entry points, bitwise" + (f" ({bwd.ties} ties, {bwd.inexact} inexact)" if c.probe else ""))


# --------------------------------------------------------------------------------------------------------------------------------
# weight gradient
# --------------------------------------------------------------------------------------------------------------------------------
def _cus(N, H):
    return N.load().tg_mlp_weight_grad_workspace(H) // ((H * H + H) * 4)


def _run_dw(N, dev, inp, st, rider=None, entry="ex"):
    lib, H = N.load(), inp.H
    keep = []

    def buf(bits):
        keep.append(_Buf(bits, dev))
        return keep[-1]

    bucket = buf(R.f32_bits(inp.bucket))
    jobs = (N.DwJob * len(inp.jobs))()
    for slot, j in zip(jobs, inp.jobs):
        m_out, n_out, ld = j.window
        slot.d_p, slot.d_q = buf(j.p).ptr, buf(j.q).ptr
        slot.d_aux = buf(j.aux).ptr if j.aux is not None else None
        slot.d_wgrad = bucket.ptr + 4 * j.w_off
        slot.d_bgrad = None if j.b_off is None else bucket.ptr + 4 * j.b_off
        slot.wgrad_ld, slot.kind, slot.m_out, slot.n_out, slot.layout = ld, j.kind, m_out, n_out, j.layout
    ws_bytes = lib.tg_mlp_weight_grad_workspace(H)
    ws = _nan(ws_bytes // 4, np.uint32, dev)
    w0, b0, wh = buf(st.fwd[:32 * H]), buf(st.bias[:H]), buf(st.bwd[:32 * H])      # exactly the first block of either stream, b0 [H]
    s = N.stream_ptr(dev)
    got = {}
    if entry == "plain":
        N.check(lib.tg_mlp_weight_grad(H, jobs, len(inp.jobs), inp.rows, w0.ptr, b0.ptr, wh.ptr, ws.ptr, ws_bytes, s), "weight_grad")
    else:
        regions = rider.regions if rider else []
        ex = (N.SlabSum * max(len(regions), 1))()
        rb = buf(R.f32_bits(rider.bucket)) if rider else None
        for slot, g in zip(ex, regions):
            slot.d_slab, slot.slab_stride, slot.n_slabs, slot.row_pitch = buf(R.f32_bits(g.slab)).ptr, g.stride, g.n_slabs, g.pitch
            slot.d_grad, slot.grad_ld, slot.m_out, slot.n_out = rb.ptr + 4 * g.off, g.ld, g.m_out, g.n_out
        loss = rider.loss if rider else None
        lw = buf(np.ascontiguousarray(loss.work).view(np.uint64)) if loss else None
        ls = buf(np.ascontiguousarray(loss.sums).view(np.uint64)) if loss else None
        N.check(lib.tg_mlp_weight_grad_ex(H, jobs, len(inp.jobs), inp.rows, w0.ptr, b0.ptr, wh.ptr, ws.ptr, ws_bytes, ex, len(regions),
                                          lw.ptr if loss else None, loss.work.shape[0] if loss else 0, ls.ptr if loss else None, s), "weight_grad_ex")
        torch.cuda.synchronize()
        if rider:
            got["rider_bucket"] = rb.back()
        if loss:
            got["loss_sums"] = ls.back()
    torch.cuda.synchronize()
    got["bucket"] = bucket.back()
    whole = ws.back()
    got["workspace_guards"] = np.concatenate([whole[:G], whole[-G:]])
    return got


def test_weight_gradient_table_reaches_its_edges_on_this_device(tg):
    for H in (128, 256):
        assert _cus(tg._native, H) == tg._native.load().tg_mlp_forward_chain_blocks()
    R.check_dw_table(_cus(tg._native, 256))


@pytest.mark.parametrize("c", DW, ids=[c.id for c in DW])
def test_weight_gradient_is_exact(tg, dev, c):
    """Every job's dW and db accumulated into its window of the nonzero bucket, the rest of the bucket and the guards untouched."""
    N = tg._native
    cus = _cus(N, c.H)
    rows = R.dw_rows(c, cus)
    inp = R.dw_inputs(c.H, rows, c.jobs)
    st = _streams(inp.net.S, inp.net.A, c.H, inp.net.nh, 0, False)
    want = {"bucket": R.dw_ref(inp)[0], "workspace_guards": R.nan_words(2 * G, np.uint32)}
    it = iter(["plain", "ex"])
    got = _twice(lambda: _run_dw(N, dev, inp, st, entry=next(it)))
    P.check_image(got, want, c.id)
    plan = R.dw_plan(c.H, [k for k, _, _ in c.jobs], rows, cus)
    print(f"dw {c.id} rows {rows}: {len(c.jobs)} jobs, n_st {plan[0].n_st}, workgroups {[p.n_blocks for p in plan]}, "
          f"stages {[p.stages for p in plan]}, rings {[p.ring for p in plan]}: bucket bitwise")


@pytest.mark.parametrize("name,n_loss", R.RIDER_CASES)
def test_weight_gradient_riders_are_exact(tg, dev, name, n_loss):
    """tg_slab_sum regions and the f64 loss rider on the second launch of a one-job launch: every region's window, the loss sums, and
    the job's own gradient -- the same image whatever rides along."""
    N = tg._native
    jobs = ((R.DH, 0, "ld"),)
    inp = R.dw_inputs(128, 33, jobs)
    st = _streams(inp.net.S, inp.net.A, 128, inp.net.nh, 0, False)
    rider = R.rider_inputs(name, n_loss)
    want = dict(R.rider_ref(rider), bucket=R.dw_ref(inp)[0], workspace_guards=R.nan_words(2 * G, np.uint32))
    got = _twice(lambda: _run_dw(N, dev, inp, st, rider=rider))
    P.check_image(got, want, f"{name}-{n_loss}")
    print(f"riders {name} ({[g.n_slabs for g in rider.regions]} slabs), loss rows {n_loss}: {len(want)} buffers, bitwise")

