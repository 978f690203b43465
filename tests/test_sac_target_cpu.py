"""DeviceActor's Q nets without a GPU: the shape predicate, the refusals of a wrong combination (the LDS verdict is the library's:
tg_policy_q_fits reads widths alone), the declarations."""
import re

import pytest

import policy_step_ref as R
import trajopt_grpo_amd as tg
from conftest import REPO

# (S, A, H, actor hidden layers, critic hidden layers, activation) of tests/test_sac_target_gpu.py
CASES = [(3, 1, 64, 1, 2, "ReLU"), (10, 2, 128, 3, 1, "Tanh"), (20, 4, 256, 2, 2, "ReLU"), (28, 4, 64, 2, 2, "Tanh")]


def build(S, A, H, nh_a, nh_q, act, q_in=None, q_H=None, q_act=None, head="squashed"):
    actor = R.make_net(S, H, nh_a, 2 * A if head == "squashed" else A, act, seed=0)
    q = [R.make_net(q_in or S + A, q_H or H, nh_q, 1, q_act or act, seed=1 + k) for k in range(2)]
    return lambda: tg.DeviceActor(actor, q_nets=q, num_envs=4, head=head, log_std=None, device="cpu")


@pytest.mark.parametrize("S,A,H,nh_a,nh_q,act", CASES)
def test_supports_and_the_constructor_accept_the_shape_set(S, A, H, nh_a, nh_q, act):
    assert tg.DeviceActor.supports(R.make_net(S + A, H, nh_q, 1, act, seed=0), "q") is None
    with pytest.raises(tg._native.NativeLibraryError, match="no CPU fallback"):     # (past every check of the nets)
        build(S, A, H, nh_a, nh_q, act)()


@pytest.mark.parametrize("net,word", [(lambda: R.make_net(6, 64, 2, 2, "Tanh", 0), "2 outputs of a Q critic"),
                                      (lambda: R.make_net(33, 64, 2, 1, "Tanh", 0), "input width 33"),
                                      (lambda: R.make_net(6, 96, 2, 1, "Tanh", 0), "width 96")])
def test_supports_names_the_reason(net, word):
    assert word in tg.DeviceActor.supports(net(), "q")


@pytest.mark.parametrize("make,word", [(build(5, 1, 64, 2, 2, "ReLU", q_H=128), "128 wide"),
                                       (build(5, 1, 64, 2, 2, "ReLU", q_act="Tanh"), "with Tanh"),
                                       (build(5, 1, 64, 2, 2, "ReLU", q_in=8), "reads 8 inputs"),
                                       (build(30, 4, 64, 2, 2, "ReLU"), "input width 34"),
                                       (build(5, 1, 64, 2, 2, "ReLU", head="gaussian"), "squashed head"),
                                       (build(28, 4, 256, 5, 5, "ReLU"), "of LDS")])
def test_a_wrong_combination_raises_value_error_with_the_reason(make, word):
    with pytest.raises(ValueError, match="DeviceActor: the Q nets are not supported: .*" + word):
        make()


def test_new_symbols_are_declared_bound_and_exported_and_the_abi_is_still_13():
    N, lib = tg._native, tg._native.load()
    header = open(f"{REPO}/include/trajopt_grpo_hip.h").read()
    for name in ("tg_policy_q_fits", "tg_policy_q_values", "tg_policy_sac_target"):
        declared = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\);", header).group(1).split(",")
        assert len(declared) == len(N.SIGNATURES[name][1]) and hasattr(lib, name), name
    body = re.search(r"typedef struct tg_policy_q_args \{(.*?)\} tg_policy_q_args;", header, re.S).group(1)
    assert re.findall(r"\s([a-z_0-9]+);", body) == [name for name, _ in N.PolicyQArgs._fields_]
    assert lib.tg_abi_version() == N.ABI_VERSION == 13
