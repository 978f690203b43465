"""The bf16 chain learner's kernels at the depth it trains at (H = 256, 5 hidden layers, panel order), on the MI355X (run with
`-m gpu`).

The depth-specialised backward chain, mlp_bwd_chain_kernel<..., NL = 5> behind tg_mlp_backward_chain_ex with the first layer's gradient
inside (chain_exact_ref's mode panel_w0, the one the learner launches), against
  (a) its run-time-depth twin through the process-wide switch tg_chain_depth_kernels -- every buffer the pass writes, bit for bit,
      guards included: the specialisation renames registers and folds addresses, it must not change one stored bit;
  (b) tests/chain_exact_ref.py on its integer nets (every product and partial sum exact in any order, see there) at 257 rows and at
      B + 1 rows.
The forward pass with the loss head (tg_mlp_forward_chain_loss_ex, which has no specialised form) against the same reference at the
same depth and row counts: test_chain_exact_gpu.py pins the forward chain at 1 / 2 / 3 / 6 / 8 hidden layers and the backward chain
at 3 / 4 / 6 -- the depth the learner runs was pinned by no case.
There is no tolerance in this module.  Conventions of test_chain_exact_gpu.py: every input sits between 64 NaN guard words, every
output is NaN between guards before a launch, every launch runs twice on fresh buffers, whole buffers are compared.

ROW COUNTS of the backward chain (B = tg_mlp_backward_chain_blocks() x 256 rows: one round of every workgroup):
  1, 33, 257       one row / a ragged second 32-row tile / a second workgroup with one row
  B + 1            the second round of the first workgroup: the ring carried across rounds at its constant slots (33 blocks, 3 slots)
  2 B + 1          the third round
  3 B - 31         three full rounds of every workgroup but the last, whose third round ends in a ragged tile
The forward pass runs all three heads: actor (kind 0), actor writing logp_old (kind 2: d_logp_old_out) and critic (kind 1)."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import chain_exact_ref as R
import per_layer_ref as P
from test_chain_exact_gpu import _Buf, _nan, _ptrs, _streams

pytestmark = pytest.mark.gpu
G = R.G
S, H, NH = 20, 256, 5
ROW_SPECS = [1, 33, 257, (1, 1), (2, 1), (3, -31)]
REF_ROWS = (257, (1, 1))                    # comparison (b)
HEADS = [("actor", 0, 4), ("actor_logp_out", 2, 4), ("critic", 1, 1)]


@pytest.fixture(scope="module")
def tg():
    import trajopt_grpo_amd as tg
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return tg


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture()
def switch(tg):
    """Sets the native switch; puts back what it found."""
    lib = tg._native.load()
    before = lib.tg_chain_depth_kernels(1)
    yield lambda on: lib.tg_chain_depth_kernels(int(on))
    lib.tg_chain_depth_kernels(before)


def _rid(spec):
    return str(spec) if isinstance(spec, int) else f"B{spec[0]}{spec[1]:+d}"


def _same(a, b, tag):
    """Whole device buffers, guards included, bit for bit (compared on the device: the large cases hold 100 MB each)."""
    assert set(a) == set(b)
    for k in a:
        assert a[k].whole.dtype == b[k].whole.dtype and torch.equal(a[k].whole, b[k].whole), f"{tag}: {k} differs"


@functools.lru_cache(maxsize=1)
def _reference(A, rows):
    """chain_exact_ref's forward pass of the 20-256x5-A integer net at `rows` rows (its conditions asserted inside), shared by the
    cases that follow each other at one row count and left unchanged."""
    x = R.make_x(S, rows)
    return R.NS(x=x, fwd=R.forward_ref(_streams(S, A, H, NH).net, x))


# --------------------------------------------------------------------------------------------------------------------------------
# forward chain with the loss head
# --------------------------------------------------------------------------------------------------------------------------------
def _loss_inputs(kind, A, rows):
    rng = np.random.default_rng([31, kind, A, rows])
    f32 = lambda v: np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)
    return R.NS(act=f32(rng.normal(size=(rows, A))), logp_old=f32(-1.0 - 0.5 * rng.random(rows)), adv=f32(rng.normal(size=rows)),
                ret=f32(rng.normal(size=rows)))


def _run_forward_loss(N, dev, kind, A, rows, st, x_bits, inp, blocks):
    lib = N.load()
    x, w, b = _Buf(x_bits, dev), _Buf(st.fwd, dev), _Buf(st.bias, dev)
    out = {}
    for l in range(1, NH - 1):                                       # the first activation is recomputed, the top one never written
        out[f"act{l}"] = _nan(R.pad32(rows) * H, np.uint16, dev)
    for l in range(NH):
        out[f"mask{l}"] = _nan(rows * H // 32, np.uint32, dev)
    out["dout8"] = _nan(rows * 8, np.uint16, dev)
    out["head_slabs"] = _nan(blocks * 4 * 16 * H, np.uint32, dev)
    out["work"] = _nan(blocks * 4, np.uint64, dev)
    out["bias_partial"] = _nan(blocks * 4, np.uint32, dev)
    keep = [_Buf(inp.act, dev), _Buf(inp.adv, dev), _Buf(inp.ret, dev)]
    a = N.ChainLoss()
    a.kind, a.act_dim = (1 if kind == 1 else 0), A
    a.norm_mean, a.norm_inv, a.epsilon = 0.1, 1.3, 0.2
    a.surr_coef, a.critic_coef, a.kl_coef = -1.0 / rows, 0.5 / rows, 0.5 / rows
    for k in range(4):
        a.var[k] = 0.3
    if kind == 1:
        a.d_ret = keep[2].ptr
    else:
        a.d_act, a.act_row_stride, a.act_col_stride, a.d_adv = keep[0].ptr, A, 1, keep[1].ptr
        if kind == 2:
            out["logp_old"] = _nan(rows, np.uint32, dev)
            a.d_logp_old_out = out["logp_old"].ptr
        else:
            keep.append(_Buf(inp.logp_old, dev))
            a.d_logp_old = keep[-1].ptr
    a.d_dout8, a.d_head_slabs, a.d_work, a.d_bias_partial = out["dout8"].ptr, out["head_slabs"].ptr, out["work"].ptr, out["bias_partial"].ptr
    a_ptrs = _ptrs([None] + [out[f"act{l}"].ptr for l in range(1, NH - 1)] + [None])
    m_ptrs = _ptrs([out[f"mask{l}"].ptr for l in range(NH)])
    N.check(lib.tg_mlp_forward_chain_loss_ex(x.ptr, w.ptr, b.ptr, H, NH, rows, a_ptrs, m_ptrs, C.byref(a), None, None, N.TG_LAYOUT_PANEL,
                                             N.stream_ptr(dev)), "tg_mlp_forward_chain_loss_ex")
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("head", HEADS, ids=[h[0] for h in HEADS])
@pytest.mark.parametrize("spec", REF_ROWS, ids=[_rid(s) for s in REF_ROWS])
def test_forward_loss_pass_at_the_learner_depth_against_reference(tg, dev, spec, head):
    """Stored activations (panel order) and mask words of the loss-head pass at 5 hidden layers against chain_exact_ref; dout8, the
    head's weight-gradient slabs, loss sums and bias partials (and logp_old for kind 2) the same bits from a repeated launch, and
    the head's count of rows."""
    N = tg._native
    _, kind, A = head
    blocks = N.load().tg_mlp_forward_chain_blocks()
    rows = R.rows_of(spec, blocks)
    st = _streams(S, A, H, NH)
    ref = _reference(A, rows)
    x_bits = R.bf16_bits(ref.x)
    inp = _loss_inputs(kind, A, rows)
    got = _run_forward_loss(N, dev, kind, A, rows, st, x_bits, inp, blocks)
    _same(got, _run_forward_loss(N, dev, kind, A, rows, st, x_bits, inp, blocks), f"{head[0]} r{_rid(spec)}: a repeated launch")
    grid = min(blocks, -(-rows // R.ROUND))
    work = got["work"].back()[G:-G].view(np.float64).reshape(blocks, 4)
    assert float(work[:grid, 3].sum()) == rows, "the loss head's row count"
    img = R.forward_image(st.net, ref.fwd, 4, panel=True)
    names = [f"act{l}" for l in range(1, NH - 1)] + [f"mask{l}" for l in range(NH)]
    P.check_image({k: got[k].back() for k in names}, {k: img[k] for k in names}, f"{head[0]} r{_rid(spec)}")
    print(f"fwd {head[0]} rows {rows}: {len(names)} buffers == reference, {len(got)} buffers repeatable")


# --------------------------------------------------------------------------------------------------------------------------------
# backward chain with the first layer's gradient (the product's mode, chain_exact_ref's "panel_w0")
# --------------------------------------------------------------------------------------------------------------------------------
def _run_backward_w0(N, dev, rows, st, dout_bits, mask_bits, x_bits, blocks):
    lib = N.load()
    dout, w, x = _Buf(dout_bits, dev), _Buf(st.bwd, dev), _Buf(x_bits, dev)
    masks = [_Buf(m, dev) for m in mask_bits]                        # bottom layer first; the kernel takes the TOP layer first
    out = {f"dz{j}": _nan(R.pad32(rows) * H, np.uint16, dev) for j in range(NH)}
    out["slabs"] = _nan(2 * blocks * H * 32, np.uint32, dev)
    n_slabs = C.c_int32(-1)
    d_ptrs = _ptrs([None if j in (0, NH - 1) else out[f"dz{j}"].ptr for j in range(NH)])
    N.check(lib.tg_mlp_backward_chain_ex(dout.ptr, w.ptr, H, NH, rows, d_ptrs, _ptrs([masks[NH - 1 - j].ptr for j in range(NH)]), x.ptr,
                                         out["slabs"].ptr, out["slabs"].n, C.byref(n_slabs), N.TG_LAYOUT_PANEL, N.stream_ptr(dev)),
            "tg_mlp_backward_chain_ex")
    torch.cuda.synchronize()
    return out, n_slabs.value


def _w0_image(out, n, blocks):
    """The buffers of chain_exact_ref.backward_image(mode="panel_w0") from a run's device buffers."""
    got = {f"dz{j}": out[f"dz{j}"].back() for j in range(NH)}
    whole = out["slabs"].back()
    acc = np.zeros(H * 32, dtype=np.float32)
    for k in range(n):                                               # the caller's sum over the slabs, in order, in fp32
        acc = acc + whole[G + k * H * 32:G + (k + 1) * H * 32].view(np.float32)
    got["w0sum"], got["w0rest"], got["w0front"] = acc.view(np.uint32), whole[G + n * H * 32:], whole[:G]
    got["n_slabs"] = np.array([n], dtype=np.uint32)
    return got


@pytest.mark.parametrize("spec", ROW_SPECS, ids=[_rid(s) for s in ROW_SPECS])
def test_backward_specialised_against_generic_and_reference(tg, dev, switch, spec):
    """Every stored dZ (panel order; top and bottom unwritten) and the first layer's gradient slabs: NL = 5 against the run-time depth,
    each launched twice; at REF_ROWS both against chain_exact_ref's panel_w0 image."""
    N = tg._native
    A = 4
    blocks = N.load().tg_mlp_backward_chain_blocks()
    rows = R.rows_of(spec, blocks)
    st = _streams(S, A, H, NH)
    dout = R.make_dout(A, rows)
    if spec in REF_ROWS:
        ref = _reference(A, rows)
        x, masks = ref.x, ref.fwd.masks
    else:                                                            # (the twin comparison alone: any mask bits will do)
        rng = np.random.default_rng([32, rows])
        x, masks = R.make_x(S, rows), [rng.random((rows, H)) < 0.6 for _ in range(NH)]
    dout_bits, x_bits, mask_bits = R.bf16_bits(dout), R.bf16_bits(x), [R.pack_mask(m) for m in masks]
    got = {}
    for on in (True, False):
        switch(on)
        first, n1 = _run_backward_w0(N, dev, rows, st, dout_bits, mask_bits, x_bits, blocks)
        second, n2 = _run_backward_w0(N, dev, rows, st, dout_bits, mask_bits, x_bits, blocks)
        assert n1 == n2 == 2 * min(blocks, -(-rows // R.ROUND))
        _same(first, second, f"bwd r{_rid(spec)} depth kernels {on}: a repeated launch")
        got[on] = (first, n1)
        del second
    _same(got[True][0], got[False][0], f"bwd r{_rid(spec)}: specialised against generic")
    if spec in REF_ROWS:
        want = R.backward_image(st.net, R.backward_ref(st.net, masks, dout, x), "panel_w0", blocks)
        for on in (True, False):
            P.check_image(_w0_image(*got[on], blocks), want, f"bwd r{_rid(spec)} depth kernels {on}")
    print(f"bwd rows {rows}: {len(got[True][0])} buffers, specialised == generic bitwise" + (", both == reference" if spec in REF_ROWS else ""))


# --------------------------------------------------------------------------------------------------------------------------------
# learn()
# --------------------------------------------------------------------------------------------------------------------------------
def test_learn_is_bit_identical_with_the_depth_kernels_off(tg, dev, monkeypatch):
    """PPO 20-256x5-{4,1} bf16, three updates over two chunks: GemmMLP.depth_kernels on against off -- post-update weights and
    last_stats bit-identical."""
    T = 32
    monkeypatch.setenv("TG_CHUNK_ROWS", "8192")
    torch.manual_seed(12)
    pol0 = tg.GaussianActorCritic_NeuralNetwork(20, 4, (256,) * 5, cov=0.3, device=dev)
    lib = tg._native.load()
    before = lib.tg_chain_depth_kernels(1)

    def run(on):
        pol = copy.deepcopy(pol0)
        mgr = tg.RolloutManager(lambda: tg.QuadPole(max_steps=T), pol, num_workers=8, num_episodes_per_worker=75, seed=5,
                                compute_dtype=torch.bfloat16)
        buf = tg.Rollout_Buffer(mgr)
        buf.sample()
        algo = tg.PPO(epsilon=0.2, policy=pol, optimizer=torch.optim.Adam(pol.parameters(), lr=3e-4), ref_model=None,
                      updates_per_iter=3, gamma=0.999, batch_size=None, autocast_dtype=torch.bfloat16)
        assert algo.chunk_rows == 8192
        mlps = [algo._mlp(pol.actor), algo._mlp(pol.critic)]
        for m in mlps:
            assert m._chain is not None and m._bchain is not None and m.panel_order and m.depth_kernels
            m.depth_kernels = on
        algo.learn(buf)
        torch.cuda.synchronize()
        assert all(m._dw_ws is not None for m in mlps), "chain kernels not selected"
        assert int(buf.group_masks.sum()) > 8192, "one chunk only"
        assert lib.tg_chain_depth_kernels(int(on)) == int(on), "GemmMLP.depth_kernels did not reach the native switch"
        return [p.detach().clone() for p in pol.parameters()], copy.deepcopy(algo.last_stats)

    try:
        (w_on, s_on), (w_off, s_off) = run(True), run(False)
    finally:
        lib.tg_chain_depth_kernels(before)
    assert any(not torch.equal(a, b) for a, b in zip(w_on, pol0.parameters()))
    assert all(torch.equal(a, b) for a, b in zip(w_on, w_off))
    assert set(s_on) == set(s_off)
    for k in s_on:
        assert np.asarray(s_on[k], dtype=np.float64).tobytes() == np.asarray(s_off[k], dtype=np.float64).tobytes(), k
