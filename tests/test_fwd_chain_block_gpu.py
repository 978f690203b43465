"""The block-structured forward chain of the bf16 learner (mlp_fwd_chain_kernel<..., kBlk>: H = 256, plain loss head, panel order,
the depth at run time) on the MI355X (run with `-m gpu`), behind tg_mlp_forward_chain_loss_ex and the process-wide switch
tg_chain_fwd_kernels, against
  (a) its run-time twin through the switch -- every buffer the pass writes (stored activations, all mask-bit planes, dout8, the head's
      weight-gradient slabs, loss sums, bias partials, logp_old), bit for bit, guards included: the specialisation renames registers
      and folds addresses, it must not change one stored bit;
  (b) tests/chain_exact_ref.py on its integer nets (every product and partial sum exact in any order, see there) at 257 rows and at
      B + 1 rows, with the switch explicitly on;
  (c) a PPO learn() over two chunks, GemmMLP.fwd_depth_kernels on against off.
There is no tolerance in this module.  Conventions of test_chain_exact_gpu.py: every input sits between 64 NaN guard words, every
output is NaN between guards before a launch, every launch runs twice on fresh buffers, whole buffers are compared.

ROW COUNTS (B = tg_mlp_forward_chain_blocks() x 256 rows: one round of every workgroup):
  1, 33, 257       one row / a ragged second 32-row tile / a second workgroup with one row
  B + 1            the second round of the first workgroup: a round of 8 n + 2 blocks turns the ring of 4 slots by half a ring, so the
                   second round runs on the swapped pair of slot bases
  2 B + 1          the third round, back on the first round's slots
  3 B - 31         three full rounds of every workgroup but the last, whose third round ends in a ragged tile
DEPTHS: 5 hidden layers (the learner's), 4, and 3 -- the smallest the entry point takes: the first and the top H x H layer next to
each other, the rolled loop over the middle layers never entered (4: entered once, 5: twice).
HEADS: actor (kind 0), actor writing logp_old (kind 2: d_logp_old_out) and critic (kind 1)."""
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
S, H = 20, 256
DEPTHS = [5, 4, 3]
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
    before = lib.tg_chain_fwd_kernels(1)
    yield lambda on: lib.tg_chain_fwd_kernels(int(on))
    lib.tg_chain_fwd_kernels(before)


def _rid(spec):
    return str(spec) if isinstance(spec, int) else f"B{spec[0]}{spec[1]:+d}"


def _same(a, b, tag):
    """Whole device buffers, guards included, bit for bit (compared on the device: the large cases hold 100 MB each)."""
    assert set(a) == set(b)
    for k in a:
        assert a[k].whole.dtype == b[k].whole.dtype and torch.equal(a[k].whole, b[k].whole), f"{tag}: {k} differs"


def _no_nan_left(out, tag):
    """Every word between the guards was written: a buffer still holding its NaN fill equals itself in both arms."""
    for k, b in out.items():
        fill = R.nan_words(1, b.dtype)[0]
        body = b.whole[G:G + b.n]
        assert not bool((body == int(fill.view({2: np.int16, 4: np.int32, 8: np.int64}[b.dtype.itemsize]))).all()), f"{tag}: {k} was never written"


@functools.lru_cache(maxsize=1)
def _reference(A, nh, rows):
    """chain_exact_ref's forward pass of the 20-256 x nh-A integer net at `rows` rows (its conditions asserted inside), shared by the
    cases that follow each other at one shape and left unchanged."""
    x = R.make_x(S, rows)
    return R.NS(x=x, fwd=R.forward_ref(_streams(S, A, H, nh).net, x))


def _loss_inputs(kind, A, rows):
    rng = np.random.default_rng([41, kind, A, rows])
    f32 = lambda v: np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)
    return R.NS(act=f32(rng.normal(size=(rows, A))), logp_old=f32(-1.0 - 0.5 * rng.random(rows)), adv=f32(rng.normal(size=rows)),
                ret=f32(rng.normal(size=rows)))


def _run_forward_loss(N, dev, nh, kind, A, rows, st, x_bits, inp, blocks):
    lib = N.load()
    x, w, b = _Buf(x_bits, dev), _Buf(st.fwd, dev), _Buf(st.bias, dev)
    out = {}
    for l in range(1, nh - 1):                                       # the first activation is recomputed, the top one never written
        out[f"act{l}"] = _nan(R.pad32(rows) * H, np.uint16, dev)
    for l in range(nh):
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
    a_ptrs = _ptrs([None] + [out[f"act{l}"].ptr for l in range(1, nh - 1)] + [None])
    m_ptrs = _ptrs([out[f"mask{l}"].ptr for l in range(nh)])
    N.check(lib.tg_mlp_forward_chain_loss_ex(x.ptr, w.ptr, b.ptr, H, nh, rows, a_ptrs, m_ptrs, C.byref(a), None, None, N.TG_LAYOUT_PANEL,
                                             N.stream_ptr(dev)), "tg_mlp_forward_chain_loss_ex")
    torch.cuda.synchronize()
    return out


def _row_count(got, blocks, rows):
    grid = min(blocks, -(-rows // R.ROUND))
    work = got["work"].back()[G:-G].view(np.float64).reshape(blocks, 4)
    return float(work[:grid, 3].sum())


# --------------------------------------------------------------------------------------------------------------------------------
# (a) the twin through the switch
# --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("head", HEADS, ids=[h[0] for h in HEADS])
@pytest.mark.parametrize("spec", ROW_SPECS, ids=[_rid(s) for s in ROW_SPECS])
@pytest.mark.parametrize("nh", DEPTHS, ids=[f"nh{n}" for n in DEPTHS])
def test_block_structured_pass_equals_its_run_time_twin(tg, dev, switch, nh, spec, head):
    """Every buffer of the loss-head pass, the switch on against off, each launched twice on fresh buffers."""
    N = tg._native
    _, kind, A = head
    blocks = N.load().tg_mlp_forward_chain_blocks()
    rows = R.rows_of(spec, blocks)
    st = _streams(S, A, H, nh)
    x_bits = R.bf16_bits(R.make_x(S, rows))
    inp = _loss_inputs(kind, A, rows)
    tag = f"{head[0]} nh{nh} r{_rid(spec)}"
    got = {}
    for on in (True, False):
        switch(on)
        first = _run_forward_loss(N, dev, nh, kind, A, rows, st, x_bits, inp, blocks)
        second = _run_forward_loss(N, dev, nh, kind, A, rows, st, x_bits, inp, blocks)
        _same(first, second, f"{tag} switch {on}: a repeated launch")
        del second
        assert _row_count(first, blocks, rows) == rows, f"{tag} switch {on}: the loss head's row count"
        _no_nan_left(first, f"{tag} switch {on}")
        got[on] = first
    _same(got[True], got[False], f"{tag}: block-structured against run-time")
    print(f"fwd {tag} rows {rows}: {len(got[True])} buffers, block-structured == run-time bitwise")


# --------------------------------------------------------------------------------------------------------------------------------
# (b) against chain_exact_ref, the switch on
# --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("head", HEADS, ids=[h[0] for h in HEADS])
@pytest.mark.parametrize("spec", REF_ROWS, ids=[_rid(s) for s in REF_ROWS])
@pytest.mark.parametrize("nh", DEPTHS, ids=[f"nh{n}" for n in DEPTHS])
def test_block_structured_pass_against_reference(tg, dev, switch, nh, spec, head):
    """Stored activations (panel order) and mask words against chain_exact_ref with the switch on; the other buffers the same bits
    from a repeated launch, and the head's count of rows."""
    N = tg._native
    _, kind, A = head
    blocks = N.load().tg_mlp_forward_chain_blocks()
    rows = R.rows_of(spec, blocks)
    st = _streams(S, A, H, nh)
    ref = _reference(A, nh, rows)
    x_bits = R.bf16_bits(ref.x)
    inp = _loss_inputs(kind, A, rows)
    tag = f"{head[0]} nh{nh} r{_rid(spec)}"
    assert switch(True) in (0, 1)
    got = _run_forward_loss(N, dev, nh, kind, A, rows, st, x_bits, inp, blocks)
    _same(got, _run_forward_loss(N, dev, nh, kind, A, rows, st, x_bits, inp, blocks), f"{tag}: a repeated launch")
    assert N.load().tg_chain_fwd_kernels(1) == 1, "the switch was not on during the launches"
    assert _row_count(got, blocks, rows) == rows, "the loss head's row count"
    img = R.forward_image(st.net, ref.fwd, 4, panel=True)
    names = [f"act{l}" for l in range(1, nh - 1)] + [f"mask{l}" for l in range(nh)]
    P.check_image({k: got[k].back() for k in names}, {k: img[k] for k in names}, tag)
    print(f"fwd {tag} rows {rows}: {len(names)} buffers == reference, {len(got)} buffers repeatable")


# --------------------------------------------------------------------------------------------------------------------------------
# (c) learn()
# --------------------------------------------------------------------------------------------------------------------------------
def test_learn_is_bit_identical_with_the_forward_kernel_off(tg, dev, monkeypatch):
    """PPO 20-256x5-{4,1} bf16, three updates over two chunks: GemmMLP.fwd_depth_kernels on against off -- post-update weights and
    last_stats bit-identical."""
    T = 32
    monkeypatch.setenv("TG_CHUNK_ROWS", "8192")
    torch.manual_seed(12)
    pol0 = tg.GaussianActorCritic_NeuralNetwork(20, 4, (256,) * 5, cov=0.3, device=dev)
    lib = tg._native.load()
    before = lib.tg_chain_fwd_kernels(1)

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
            assert m._chain is not None and m._bchain is not None and m.panel_order and m.fwd_depth_kernels
            m.fwd_depth_kernels = on
        algo.learn(buf)
        torch.cuda.synchronize()
        assert all(m._dw_ws is not None for m in mlps), "chain kernels not selected"
        assert int(buf.group_masks.sum()) > 8192, "one chunk only"
        assert lib.tg_chain_fwd_kernels(int(on)) == int(on), "GemmMLP.fwd_depth_kernels did not reach the native switch"
        return [p.detach().clone() for p in pol.parameters()], copy.deepcopy(algo.last_stats)

    try:
        (w_on, s_on), (w_off, s_off) = run(True), run(False)
    finally:
        lib.tg_chain_fwd_kernels(before)
    assert any(not torch.equal(a, b) for a, b in zip(w_on, pol0.parameters()))
    assert all(torch.equal(a, b) for a, b in zip(w_on, w_off))
    assert set(s_on) == set(s_off)
    for k in s_on:
        assert np.asarray(s_on[k], dtype=np.float64).tobytes() == np.asarray(s_off[k], dtype=np.float64).tobytes(), k
