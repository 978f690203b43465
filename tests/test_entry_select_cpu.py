"""Which native entry point each combination of optional features calls: the selectors of mlp.py, rollout.py and hip_ops.py against
tables written out here (the names, and the kernel-name suffixes of the profiling events, are what bench.py, the profiles and the
call-counting GPU tests key on), and every (name, argument count) against _native.SIGNATURES.  No library is loaded, no device used."""
import ctypes as C
import itertools

import pytest

from trajopt_grpo_amd import _native as N
from trajopt_grpo_amd import hip_ops as K
from trajopt_grpo_amd import mlp as M
from trajopt_grpo_amd import rollout as R

RELU, TANH = N.TG_ACT_RELU, N.TG_ACT_TANH
REF, STD = N.RefPenalty(), N.LearnedStd()


def _fits(name, n_args):
    """`name` is bound, and a call with n_args arguments (the stream included) matches its signature."""
    assert name in N.SIGNATURES, name
    assert n_args == len(N.SIGNATURES[name][1]), (name, n_args, len(N.SIGNATURES[name][1]))


def _is_byref(arg, struct):
    return type(arg) is type(C.byref(struct))


# (machine, act, ref?, std?) -> (entry, arguments after the loss struct, trailing template arguments of the profiled kernel's name)
LOSS = {
    ("bf16", RELU, False, False): ("tg_mlp_forward_chain_loss", "", ""),
    ("bf16", RELU, True, False): ("tg_mlp_forward_chain_loss_ref", "r", ",true"),
    ("bf16", RELU, False, True): ("tg_mlp_forward_chain_loss_std", "0s", ",false,true"),
    ("bf16", RELU, True, True): ("tg_mlp_forward_chain_loss_std", "rs", ",true,true"),
    ("f32", RELU, False, False): ("tg_mlp_f32_forward_backward", "", ">"),
    ("f32", RELU, True, False): ("tg_mlp_f32_forward_backward_ref", "r", ",true>"),
    ("f32", RELU, False, True): ("tg_mlp_f32_forward_backward_act_std", "0sa", ">"),
    ("f32", RELU, True, True): ("tg_mlp_f32_forward_backward_act_std", "rsa", ",true>"),
    ("f32", TANH, False, False): ("tg_mlp_f32_forward_backward_act", "0a", ",false,1>"),
    ("f32", TANH, True, False): ("tg_mlp_f32_forward_backward_act", "ra", ",true,1>"),
    ("f32", TANH, False, True): ("tg_mlp_f32_forward_backward_act_std", "0sa", ",false,1>"),
    ("f32", TANH, True, True): ("tg_mlp_f32_forward_backward_act_std", "rsa", ",true,1>"),
    ("f32w", RELU, False, False): ("tg_mlp_f32w_forward_backward", "", ">"),
    ("f32w", RELU, True, False): ("tg_mlp_f32w_forward_backward_ref", "r", ",true>"),
    ("f32w", RELU, False, True): ("tg_mlp_f32w_forward_backward_std", "0s", ">"),
    ("f32w", RELU, True, True): ("tg_mlp_f32w_forward_backward_std", "rs", ",true>"),
    ("f32r", RELU, False, False): ("tg_mlp_f32r_forward_backward", "", ">"),
    ("f32r", RELU, True, False): ("tg_mlp_f32r_forward_backward_ref", "r", ",true>"),
    ("f32r", RELU, False, True): ("tg_mlp_f32r_forward_backward_std", "0s", ">"),
    ("f32r", RELU, True, True): ("tg_mlp_f32r_forward_backward_std", "rs", ",true>"),
}
# arguments the call sites of GemmMLP.forward_loss() pass ahead of the tail: bf16 (input, stream, bias, H, layers, rows, activations, mask
# bits, loss), f32 (input, in_pad, stream, H, layers, rows, activations, dZ, top mask, loss), f32w (table for H, no top mask), f32r (w0, table)
LOSS_PREFIX = {"bf16": 9, "f32": 10, "f32w": 9, "f32r": 12}


def _check_tail(tail, code, act):
    """code: one letter per tail argument -- r: the reference penalty, 0: NULL in its place, s: the learned log-std, a: the activation."""
    assert len(tail) == len(code)
    for arg, c in zip(tail, code):
        if c == "r":
            assert _is_byref(arg, REF)
        elif c == "s":
            assert _is_byref(arg, STD)
        elif c == "0":
            assert arg is None
        else:
            assert arg == act and isinstance(arg, int)


def test_training_head_entries():
    for machine, act, ref, std in itertools.product(("bf16", "f32", "f32w", "f32r"), (RELU, TANH), (False, True), (False, True)):
        if act == TANH and machine != "f32":
            with pytest.raises(AssertionError):                         # (ReLU-only kernels: never launched with another activation)
                M.loss_entry(machine, act, REF if ref else None, STD if std else None)
            continue
        name, tail, targs = M.loss_entry(machine, act, REF if ref else None, STD if std else None)
        want_name, code, want_targs = LOSS[machine, act, ref, std]
        assert (name, targs) == (want_name, want_targs), (machine, act, ref, std)
        _check_tail(tail, code, act)
        _fits(name, LOSS_PREFIX[machine] + len(tail) + 1)


def test_stand_alone_loss_head_entries():
    want = {(False, False): ("tg_surrogate_loss", ""), (True, False): ("tg_surrogate_loss_ref", "r"),
            (False, True): ("tg_surrogate_loss_std", "0s"), (True, True): ("tg_surrogate_loss_std", "rs")}
    for (ref, std), (want_name, code) in want.items():
        name, tail = K.head_entry("tg_surrogate_loss", REF if ref else None, STD if std else None)
        assert name == want_name
        _check_tail(tail, code, None)
        _fits(name, 1 + len(tail) + 1)


def test_no_grad_forward_entries():
    want = {("f32", RELU): ("tg_mlp_f32_forward", ()), ("f32", TANH): ("tg_mlp_f32_forward_act", (TANH,)),
            ("f32w", RELU): ("tg_mlp_f32w_forward", ()), ("f32r", RELU): ("tg_mlp_f32r_forward", ())}
    prefix = {"f32": 7, "f32w": 7, "f32r": 10}      # input, in_pad, stream | H, layers / table, layers / w0, table, H, layers, outputs | rows, output
    for machine, act in itertools.product(("bf16", "f32", "f32w", "f32r"), (RELU, TANH)):
        if (machine, act) not in want:
            with pytest.raises(AssertionError):
                M.forward_entry(machine, act)
            continue
        name, tail = M.forward_entry(machine, act)
        assert (name, tail) == want[machine, act]
        _fits(name, prefix[machine] + len(tail) + 1)


def test_fused_rollout_entries():
    PT, ON = 0x1000, (0x2000, 5.0)
    # (f32?, act, parameter table?, obs_norm?) -> (entry, arguments after the env parameters, tail)
    want = {
        (False, False, False): lambda act: ("tg_fused_rollout", (), ()),
        (False, True, False): lambda act: ("tg_fused_rollout_dr", (PT,), ()),
        (False, False, True): lambda act: ("tg_fused_rollout_on", (None,), ON),
        (False, True, True): lambda act: ("tg_fused_rollout_on", (PT,), ON),
        (True, False, False): lambda act: ("tg_fused_rollout_f32", (), ()) if act == RELU else ("tg_fused_rollout_f32_act", (), (act,)),
        (True, True, False): lambda act: ("tg_fused_rollout_f32_act_dr", (PT,), (act,)),
        (True, False, True): lambda act: ("tg_fused_rollout_f32_on", (None,), (act,) + ON),
        (True, True, True): lambda act: ("tg_fused_rollout_f32_on", (PT,), (act,) + ON),
    }
    for f32, act, pt, on in itertools.product((False, True), (RELU, TANH), (False, True), (False, True)):
        name, table, tail = R.fused_entry(f32, act, PT if pt else None, ON if on else None)
        assert (name, table, tail) == want[f32, pt, on](act), (f32, act, pt, on)
        # env parameters | trajectory, weight stream, biases / table, H, layers, [envs per workgroup,] sigma, rng, env offset, first step, end
        _fits(name, 1 + len(table) + (11 if f32 else 10) + len(tail) + 1)


def test_per_step_rollout_entries():
    PT = 0x1000
    want = {(False, False): ("tg_rollout_step", ()), (False, True): ("tg_rollout_step_dr", (PT,)),
            (True, False): ("tg_rollout_forced", ()), (True, True): ("tg_rollout_forced_dr", (PT,))}
    for (forced, pt), w in want.items():
        name, table = R.step_entry(forced, PT if pt else None)
        assert (name, table) == w
        # env parameters | trajectory, then (first step, end) or (step, mean, its row stride, sigma, rng, env offset)
        _fits(name, 1 + len(table) + (3 if forced else 7) + 1)


def test_one_feature_entries():
    """The pairs hip_ops picks with suffixed(): (base, suffix, the feature's arguments, the call's other arguments stream included)."""
    assert K.suffixed("tg_x", "_y", None) == ("tg_x", ()) and K.suffixed("tg_x", "_y", [1, 2.0]) == ("tg_x_y", (1, 2.0))
    for base, suffix, extra, others in (("tg_learn_compact", "_on", 2, 2), ("tg_ppo_returns", "_boot", 2, 13),
                                        ("tg_rollout_final_state", "_dr", 1, 5)):
        _fits(base, others)
        _fits(base + suffix, others + extra)
