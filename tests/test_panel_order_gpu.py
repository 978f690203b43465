"""Panel order (include/trajopt_grpo_hip.h TG_LAYOUT_PANEL): the bf16 chain learner's internal activations and dZ stored as the
weight-gradient kernel's own panel image.  Only addresses differ from the row-major form, so everything here is bit-for-bit:
the producers' buffers un-permuted on the host with the layout formula, the weight gradients and loss sums on either kind of
operand, and the weights after a PPO learn() with the path on and forced off."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(20, 4, (256,) * 5), (20, 1, (256,) * 5), (20, 4, (128,) * 5)]      # (H = 128: the chain path takes it)
# one row / the 32-row tile edge / the 256-row workgroup-round edge / several rounds and a ragged tail
ROWS = [1, 31, 32, 33, 255, 256, 257, 8 * 32 * 3 + 5]


@pytest.fixture(scope="module")
def tg():
    import trajopt_grpo_amd as tg
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return tg


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def pad32(rows):
    return (rows + 31) // 32 * 32


def chunk_index(rows, H):
    """Index of the 16-byte chunk c of row r in a panel-order buffer, [rows][H / 8] -- THE layout formula, in 16-byte units."""
    r = torch.arange(rows).view(-1, 1)
    c = torch.arange(H // 8).view(1, -1)
    off = (r // 32) * (64 * H) + (r % 32 // 4) * (H // 32 * 256) + (c // 4) * 256 + (r % 4) * 64 + (c % 4) * 16
    return off // 16


def from_panel(buf, rows, H):
    """Row-major int16 [rows][H] view of the valid rows of a panel-order bf16 buffer [pad32(rows)][H]."""
    chunks = buf.detach().cpu().view(torch.int16).reshape(-1, 8)
    return chunks[chunk_index(rows, H).reshape(-1)].reshape(rows, H)


def to_panel(t, H):
    """Panel-order copy of a row-major bf16 [rows][H] tensor; pad rows zero."""
    rows = t.shape[0]
    out = torch.zeros(pad32(rows) * H // 8, 8, dtype=torch.int16)
    out[chunk_index(rows, H).reshape(-1)] = t.detach().cpu().view(torch.int16).reshape(-1, 8)
    return out.view(torch.bfloat16).reshape(pad32(rows), H).to(t.device)


def bits_of(t):
    return t.detach().cpu().view(torch.int16)


_STORED = {}


def stored(tg, dev, shape, rows):
    """The storing forward pass and the backward chain of one net in both layouts, computed once per (shape, rows) and left
    unchanged: {"fwd": {skip_a0: (row-major acts, panel acts, mask bits, outputs)}, "bwd": {fuse0: (row-major dZ, panel dZ, slabs)}}."""
    key = (shape, rows)
    if key in _STORED:
        return _STORED[key]
    from trajopt_grpo_amd import mlp as M, _native as N
    S, A, hidden = shape
    H, nh = hidden[0], len(hidden)
    torch.manual_seed(rows + H + A)
    net = tg.NeuralNetwork(S, A, hidden, "ReLU").to(dev)
    mlp = M.GemmMLP(net, torch.bfloat16)
    lib = N.load()
    xp = mlp.prepare_input(torch.randn(rows, S, device=dev))
    mlp._fresh("chain")
    mlp._fresh("bchain")
    st = N.stream_ptr(dev)
    res = {"net": net, "mlp": mlp, "xp": xp, "fwd": {}, "bwd": {}}
    for skip_a0 in (False, True):
        runs = []
        for layout in (N.TG_LAYOUT_ROWS, N.TG_LAYOUT_PANEL):
            n_rows = pad32(rows) if layout == N.TG_LAYOUT_PANEL else rows
            acts = [None if (skip_a0 and i == 0) else torch.full((n_rows, H), 7.0, dtype=torch.bfloat16, device=dev) for i in range(nh)]
            bits = [torch.zeros(rows, H // 32, dtype=torch.int32, device=dev) for _ in range(nh)]
            out = torch.zeros(rows, 4, dtype=torch.float32, device=dev)
            ptrs = (N.C.c_void_p * nh)(*[N.ptr(t) or None for t in acts])
            mptrs = (N.C.c_void_p * nh)(*[t.data_ptr() for t in bits])
            N.check(lib.tg_mlp_forward_chain_ex(xp.data_ptr(), mlp._chain.stream.data_ptr(), mlp._chain.bias.data_ptr(), H, nh, rows, ptrs,
                                                mptrs, out.data_ptr(), 4, layout, st), "tg_mlp_forward_chain_ex")
            runs.append((acts, bits, out))
        torch.cuda.synchronize()
        res["fwd"][skip_a0] = runs
    bits = res["fwd"][False][0][1]
    dzh = torch.zeros(rows, 8, dtype=torch.bfloat16, device=dev)
    dzh[:, :A] = torch.randn(rows, A, device=dev).bfloat16()
    res["dzh"] = dzh
    m_ptrs = (N.C.c_void_p * nh)(*[bits[nh - 1 - j].data_ptr() for j in range(nh)])
    for fuse0 in (False, True):                      # (False: the top layer's dZ is stored too, True: it is left to kind RH)
        runs = []
        for layout in (N.TG_LAYOUT_ROWS, N.TG_LAYOUT_PANEL):
            n_rows = pad32(rows) if layout == N.TG_LAYOUT_PANEL else rows
            dzs = [torch.full((n_rows, H), 7.0, dtype=torch.bfloat16, device=dev) for _ in range(nh)]
            live = [not (fuse0 and j in (0, nh - 1)) for j in range(nh)]
            ptrs = (N.C.c_void_p * nh)(*[(t.data_ptr() if keep else None) for t, keep in zip(dzs, live)])
            slabs = torch.zeros(2 * lib.tg_mlp_backward_chain_blocks() * H * 32, dtype=torch.float32, device=dev)
            n_slabs = N.C.c_int32(0)
            N.check(lib.tg_mlp_backward_chain_ex(dzh.data_ptr(), mlp._bchain.stream.data_ptr(), H, nh, rows, ptrs, m_ptrs,
                                                 xp.data_ptr() if fuse0 else None, slabs.data_ptr(), slabs.numel(), N.C.byref(n_slabs),
                                                 layout, st), "tg_mlp_backward_chain_ex")
            runs.append(([t if keep else None for t, keep in zip(dzs, live)], slabs[:n_slabs.value * H * 32]))
        torch.cuda.synchronize()
        res["bwd"][fuse0] = runs
    _STORED[key] = res
    return res


def check_panel(row_major, panel, rows, H):
    """The valid rows un-permute to the row-major buffer; the pad rows of the last tile hold copies of the last row."""
    assert torch.equal(from_panel(panel, rows, H), bits_of(row_major))
    if pad32(rows) > rows:
        full = from_panel(panel, pad32(rows), H)
        assert torch.equal(full[rows:], full[rows - 1:rows].expand(pad32(rows) - rows, H))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("rows", ROWS)
def test_layout_round_trip(tg, dev, shape, rows):
    """The storing forward pass and the backward chain write the same bytes in both layouts: the panel-order buffers, un-permuted
    on the host with the layout formula, are bit-equal to the row-major ones (last valid row included, pad rows excluded);
    everything else the passes write (mask bits, outputs, first-layer slabs) does not depend on the layout."""
    H = shape[2][0]
    res = stored(tg, dev, shape, rows)
    for skip_a0, ((acts_r, bits_r, out_r), (acts_p, bits_p, out_p)) in res["fwd"].items():
        assert torch.equal(out_r, out_p) and all(torch.equal(a, b) for a, b in zip(bits_r, bits_p))
        assert (acts_r[0] is None) == skip_a0
        for a_r, a_p in zip(acts_r, acts_p):
            if a_r is not None:
                check_panel(a_r, a_p, rows, H)
    for a, b in zip(res["fwd"][False][0][0][1:], res["fwd"][True][0][0][1:]):
        assert torch.equal(a, b)
    for fuse0, ((dz_r, slabs_r), (dz_p, slabs_p)) in res["bwd"].items():
        assert torch.equal(slabs_r, slabs_p) and (slabs_r.numel() > 0) == fuse0
        n = 0
        for z_r, z_p in zip(dz_r, dz_p):
            if z_r is not None:
                check_panel(z_r, z_p, rows, H)
                n += 1
        assert n == (len(dz_r) - 2 if fuse0 else len(dz_r))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("rows", ROWS)
def test_weight_gradients_and_sums(tg, dev, shape, rows):
    """tg_mlp_weight_grad on panel-order operands against row-major operands: the learner's job set (RH, HH.., HR) with every
    [rows][H] operand in panel order -- as the producers wrote it, and as a host permutation with zero pad rows -- gives
    bit-equal weight and bias gradients; then forward_loss() + backward_fused() with the path on and forced off: bit-equal
    gradients and loss sums."""
    from trajopt_grpo_amd import mlp as M, _native as N
    S, A, hidden = shape
    H, nh = hidden[0], len(hidden)
    res = stored(tg, dev, shape, rows)
    mlp, xp, dzh = res["mlp"], res["xp"], res["dzh"]
    (acts_r, bits, _), (acts_p, _, _) = res["fwd"][True]
    (dz_r, _), (dz_p, _) = res["bwd"][False]
    ws = M.weight_grad_workspace(H, dev)

    def grads(acts, dzs, lp, lq):
        out, jobs = [], []
        for j in range(nh - 1):                                  # chain order: dZ j belongs to hidden layer nh - 1 - j, whose input is
            i = nh - 1 - j                                       # the stored activation i - 1
            w, b = torch.zeros(H, H, device=dev), torch.zeros(H, device=dev)
            out += [w, b]
            if j == 0:
                jobs.append((N.TG_DW_RH, dzh, acts[i - 1], w, b, bits[nh - 1], lq))
            elif i == 1:
                jobs.append((N.TG_DW_HR, dzs[j], xp, w, b, None, lp))
            else:
                jobs.append((N.TG_DW_HH, dzs[j], acts[i - 1], w, b, None, lp | lq))
        M.weight_grad(H, jobs, rows, ws, mlp._chain.stream, mlp._chain.bias[0], mlp._bchain.stream)
        torch.cuda.synchronize()
        return out

    want = grads(acts_r, dz_r, 0, 0)
    assert all(float(g.abs().max()) > 0 for g in want)
    for name, got in (("producers' buffers", grads(acts_p, dz_p, N.DW_P_PANEL, N.DW_Q_PANEL)),
                      ("dZ alone", grads(acts_r, dz_p, N.DW_P_PANEL, 0)),
                      ("host permutation", grads([None if a is None else to_panel(a, H) for a in acts_r],
                                                 [to_panel(z, H) for z in dz_r], N.DW_P_PANEL, N.DW_Q_PANEL))):
        assert all(torch.equal(a, b) for a, b in zip(want, got)), name

    net = res["net"]
    torch.manual_seed(rows)
    act = torch.randn(rows, A, device=dev)
    lpo = (-0.5 * torch.rand(rows, device=dev) - 1.0).contiguous()
    adv, ret = torch.randn(rows, device=dev), torch.randn(rows, device=dev)

    def update(panel, kind):
        m = M.GemmMLP(net, torch.bfloat16)
        m.panel_order = panel
        for p in net.parameters():
            p.grad = torch.zeros_like(p)
        sums = torch.zeros(4, dtype=torch.float64, device=dev)
        if kind == 0:
            m.forward_loss(xp, 0, act=act, logp_old=lpo, adv=adv, norm=[0.1, 1.3], var=torch.full((A,), 0.3), epsilon=0.2,
                           surr_coef=-1.0 / rows, kl_coef=0.5 / rows, sums_out=sums)
        else:
            m.forward_loss(xp, 1, ret=ret, norm=[-0.2, 0.7], critic_coef=0.5 / rows, sums_out=sums)
        assert m._acts_panel == (panel and M.PANEL_ORDER_HEAD_PASS)
        m.backward_fused()
        torch.cuda.synchronize()
        return [p.grad.clone() for p in net.parameters()] + [sums]

    for kind in ((0, 1) if A == 1 else (0,)):
        a, b = update(True, kind), update(False, kind)
        assert all(torch.equal(x, y) for x, y in zip(a, b)) and float(a[-1][3]) == rows


def test_learn_is_bit_identical_with_the_panel_path_forced_off(tg, dev):
    """One PPO learn() with two updates and a small chunk_rows on the bf16 chain learner, panel order on, and again with
    GemmMLP.panel_order forced off on both nets: bit-equal post-update weights."""
    T = 48
    torch.manual_seed(11)
    pol0 = tg.GaussianActorCritic_NeuralNetwork(20, 4, (256,) * 5, cov=0.3, device=dev)

    def run(panel):
        pol = copy.deepcopy(pol0)
        mgr = tg.RolloutManager(lambda: tg.QuadPole(max_steps=T), pol, num_workers=8, num_episodes_per_worker=16, seed=5,
                                compute_dtype=torch.bfloat16)
        buf = tg.Rollout_Buffer(mgr)
        buf.sample()
        algo = tg.PPO(epsilon=0.2, policy=pol, optimizer=torch.optim.Adam(pol.parameters(), lr=3e-4), ref_model=None,
                      updates_per_iter=2, gamma=0.999, batch_size=None, autocast_dtype=torch.bfloat16, chunk_rows=1000)
        mlps = [algo._mlp(pol.actor), algo._mlp(pol.critic)]
        for m in mlps:
            assert m._chain is not None and m._bchain is not None and m.panel_order
            m.panel_order = panel
        algo.learn(buf)
        torch.cuda.synchronize()
        assert all(m._dw_ws is not None for m in mlps), "chain kernels not selected"
        return [p.detach().clone() for p in pol.parameters()], [p.detach().clone() for p in pol0.parameters()]

    on, start = run(True)
    off, _ = run(False)
    assert any(not torch.equal(a, b) for a, b in zip(on, start))
    assert all(torch.equal(a, b) for a, b in zip(on, off))
