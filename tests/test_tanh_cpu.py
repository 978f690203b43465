"""Tanh hidden activations on the fp32 hot path, host side (no GPU): the `_act` entry points of the C ABI, their refusals (checked
before anything is launched: the pointers below are never dereferenced), the shape predicates and GemmMLP's refusal to run a Tanh
net on a ReLU-only path."""
import ctypes as C

import pytest
import torch

import trajopt_grpo_amd as tg
from trajopt_grpo_amd import mlp as M

N = tg._native
ACT_ENTRIES = ["tg_mlp_f32_forward_act", "tg_mlp_f32_forward_backward_act", "tg_fused_rollout_f32_act"]
FAKE = 256


def test_act_entry_points_are_exported_and_the_abi_is_13():
    lib = N.load()
    for name in ACT_ENTRIES:
        assert name in N.SIGNATURES and hasattr(lib, name), name
    assert (N.TG_ACT_RELU, N.TG_ACT_TANH) == (0, 1)
    assert lib.tg_abi_version() == N.ABI_VERSION == 13


def _loss():
    a = N.ChainLoss()
    a.kind, a.act_dim = 0, 1
    a.d_act, a.act_row_stride, a.act_col_stride = FAKE, 1, 1
    a.d_logp_old, a.d_adv, a.d_dout8, a.d_work = FAKE, FAKE, FAKE, FAKE
    return a


def _fwd_bwd(activation, acts, dzs, mask=None, hidden=128, n_hidden=3, ref=None):
    lib = N.load()
    arr_a = (C.c_void_p * 4)(*acts)
    arr_z = (C.c_void_p * 4)(*dzs)
    loss = _loss()
    return lib.tg_mlp_f32_forward_backward_act(FAKE, 8, FAKE, hidden, n_hidden, 100, arr_a, arr_z, mask, C.byref(loss),
                                               C.byref(ref) if ref is not None else None, activation, None)


def test_forward_backward_act_refusals():
    lib = N.load()
    full = [FAKE] * 4
    assert _fwd_bwd(7, full, full) < 0 and b"unknown activation 7" in lib.tg_last_error()
    assert _fwd_bwd(-1, full, full) < 0 and b"unknown activation" in lib.tg_last_error()
    # Tanh: no mask bits, every activation and dZ stored (a mask bit cannot stand for 1 - a^2: nothing is rebuilt)
    assert _fwd_bwd(N.TG_ACT_TANH, full, full, mask=FAKE) < 0 and b"d_top_maskbits must be NULL" in lib.tg_last_error()
    for l in range(3):
        holes = [None if i == l else FAKE for i in range(4)]
        assert _fwd_bwd(N.TG_ACT_TANH, holes, full) < 0 and b"buffer %d is null" % l in lib.tg_last_error()
        assert _fwd_bwd(N.TG_ACT_TANH, full, holes) < 0 and b"buffer %d is null" % l in lib.tg_last_error()
    # ... what the plain entries refuse, with either activation
    for act in (N.TG_ACT_RELU, N.TG_ACT_TANH):
        assert _fwd_bwd(act, full, full, hidden=96) < 0 and b"hidden width 96" in lib.tg_last_error()
        assert _fwd_bwd(act, full, full, hidden=256) < 0 and b"hidden width 256" in lib.tg_last_error()
        assert _fwd_bwd(act, full, full, n_hidden=5) < 0 and b"hidden layers" in lib.tg_last_error()
        missing = N.RefPenalty()
        missing.coef = 0.5
        assert _fwd_bwd(act, full, full, ref=missing) < 0 and b"d_logp_ref is null" in lib.tg_last_error()
    # ReLU keeps the plain entry's optional buffers: the first activation and (given mask bits) the top dZ may be left out.  The call
    # gets past the buffer checks, and is refused by the next check (a zero padded input width) instead
    lib2 = N.load()
    arr = (C.c_void_p * 4)(None, FAKE, FAKE, FAKE)
    arr_z = (C.c_void_p * 4)(FAKE, FAKE, None, FAKE)
    loss = _loss()
    loss.act_dim = 5
    assert lib2.tg_mlp_f32_forward_backward_act(FAKE, 8, FAKE, 128, 3, 100, arr, arr_z, FAKE, C.byref(loss), None, N.TG_ACT_RELU, None) < 0
    assert b"5 outputs unsupported" in lib2.tg_last_error()


def test_forward_act_and_rollout_act_refusals():
    lib = N.load()
    assert lib.tg_mlp_f32_forward_act(FAKE, 8, FAKE, 128, 2, 10, FAKE, 2, None) < 0 and b"unknown activation 2" in lib.tg_last_error()
    assert lib.tg_mlp_f32_forward_act(FAKE, 8, FAKE, 96, 2, 10, FAKE, N.TG_ACT_TANH, None) < 0 and b"hidden width 96" in lib.tg_last_error()
    assert lib.tg_mlp_f32_forward_act(FAKE, 8, FAKE, 64, 5, 10, FAKE, N.TG_ACT_TANH, None) < 0 and b"hidden layers" in lib.tg_last_error()
    assert lib.tg_mlp_f32_forward_act(FAKE, 12, FAKE, 64, 2, 10, FAKE, N.TG_ACT_TANH, None) < 0 and b"padded input width" in lib.tg_last_error()
    # rows == 0: accepted, nothing launched
    assert lib.tg_mlp_f32_forward_act(FAKE, 8, FAKE, 64, 2, 0, FAKE, N.TG_ACT_TANH, None) == 0
    sigma = (C.c_float * 1)(0.5)
    p, tr = N.EnvParams(), N.Traj()
    assert lib.tg_fused_rollout_f32_act(C.byref(p), C.byref(tr), FAKE, FAKE, 128, 2, 32, sigma, FAKE, 0, 0, 1, 3, None) < 0
    assert b"unknown activation 3" in lib.tg_last_error()
    assert lib.tg_fused_rollout_f32_act(None, C.byref(tr), FAKE, FAKE, 128, 2, 32, sigma, FAKE, 0, 0, 1, N.TG_ACT_TANH, None) < 0
    assert b"null pointer" in lib.tg_last_error()


COVERED = [(S, A, (H,) * L) for H in (64, 128) for L in (1, 2, 3, 4) for S, A in ((5, 1), (32, 4), (1, 2))]


@pytest.mark.parametrize("S,A,hidden", COVERED, ids=[f"{s}-{h[0]}x{len(h)}-{a}" for s, a, h in COVERED])
def test_predicates_accept_tanh_nets_of_every_covered_shape(S, A, hidden):
    net = tg.NeuralNetwork(S, A, hidden, "Tanh")
    assert M.hidden_activation(net) == "Tanh"
    assert M.f32_chain_supported(net) == hidden[0]
    assert M.fused_rollout_f32_supported(net, S, A, activations=("ReLU", "Tanh")) == hidden[0]
    assert M.fused_rollout_f32_supported(net, S, A) == 0            # (the default keeps tg_fused_rollout_f32's ReLU-only meaning)
    assert not M.supports(net)                                       # the bf16 / per-layer paths stay ReLU-only
    relu = tg.NeuralNetwork(S, A, hidden, "ReLU")
    assert M.hidden_activation(relu) == "ReLU" and M.supports(relu) and M.f32_chain_supported(relu) == hidden[0]


@pytest.mark.parametrize("S,A,hidden,act", [
    (5, 1, (128, 128), ["Tanh", "ReLU"]), (5, 1, (128, 128), ["ReLU", "Tanh"]), (5, 1, (64, 64), "Sigmoid"),
    (5, 1, (256,), "Tanh"), (5, 1, (256, 256), "Tanh"), (5, 1, (96, 96), "Tanh"), (5, 1, (128,) * 5, "Tanh"),
    (33, 1, (128, 128), "Tanh"), (5, 5, (128, 128), "Tanh"), (5, 1, (128, 64), "Tanh"), (5, 1, (32, 32), "Tanh")])
def test_predicates_reject_uncovered_nets(S, A, hidden, act):
    net = tg.NeuralNetwork(S, A, hidden, act)
    mixed_or_other = not isinstance(act, str) or act != "Tanh"
    assert (M.hidden_activation(net) is None) == mixed_or_other
    assert M.f32_chain_supported(net) == 0
    assert M.fused_rollout_f32_supported(net, S, A, activations=("ReLU", "Tanh")) == 0
    assert not M.supports(net)
    with pytest.raises((ValueError, AssertionError)):
        M.GemmMLP(net, torch.float32)


def test_gemm_mlp_takes_a_tanh_net_only_on_the_fp32_chain_learner():
    torch.manual_seed(0)
    net = tg.NeuralNetwork(5, 1, (128, 128), "Tanh")               # (a resident-kernel shape: the chain kernel runs it)
    with pytest.raises(ValueError, match="Tanh net only in float32"):
        M.GemmMLP(net, torch.bfloat16)
    m = M.GemmMLP(net, torch.float32)
    assert m.act == "Tanh" and m._f32 is not None and not m._f32.res and not m._f32.wide and m._f32.act == N.TG_ACT_TANH
    assert m.f32_store_all and m._chain is None and m._bchain is None
    xp = m.prepare_input(torch.randn(7, 5))
    # every ReLU-only method refuses (before anything is launched) instead of applying ReLU
    with pytest.raises(NotImplementedError, match="applies ReLU"):
        m.forward(xp, keep=True)
    with pytest.raises(NotImplementedError, match="ReLU mask"):
        m.backward(torch.zeros(7, 1))
    assert m.disable_f32_chain() is False and m._f32 is not None
    relu = M.GemmMLP(tg.NeuralNetwork(5, 1, (128, 128), "ReLU"), torch.float32)
    assert relu.act == "ReLU" and relu._f32.act == N.TG_ACT_RELU and not relu.f32_store_all
