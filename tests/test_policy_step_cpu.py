"""DeviceActor without a GPU: the float64 restatement against torch and philox_fp64, the shape predicate, the declarations."""
import re

import numpy as np
import pytest
import torch

import philox_fp64 as P
import policy_step_ref as R
import trajopt_grpo_amd as tg
from conftest import REPO


@pytest.mark.parametrize("S,H,nh,O,act", [(5, 64, 2, 1, "Tanh"), (3, 64, 1, 1, "ReLU"), (20, 256, 5, 8, "ReLU")])
def test_restated_mlp_is_the_module_in_float64(S, H, nh, O, act):
    net = R.make_net(S, H, nh, O, act, seed=1)
    x = torch.randn(33, S, dtype=torch.float64)
    want = net.double()(x).detach().numpy()
    assert np.abs(R.mlp(net.float(), x.numpy()) - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


def test_restated_eps_is_sample_eps_with_the_call_count_as_t():
    seed, off, n, A, T = 0xDEADBEEF12345, 70, 9, 3, 4
    want = P.sample_eps(seed, R.STREAM, off + np.arange(n), T, A)[0]            # [A][T][n]
    for t in range(T):
        assert np.array_equal(R.eps(seed, off, np.full(n, t), A)[0], want[:, t, :].T)


@pytest.mark.parametrize("S,H,nh,O,act,head", [(3, 64, 1, 1, "ReLU", "gaussian"), (20, 256, 5, 4, "Tanh", "gaussian"),
                                                 (32, 128, 3, 8, "ReLU", "squashed"), (5, 64, 2, 1, "Tanh", "value")])
def test_supports_accepts_the_shape_set(S, H, nh, O, act, head):
    assert tg.DeviceActor.supports(R.make_net(S, H, nh, O, act, seed=0), head) is None


@pytest.mark.parametrize("label,net,head,word", R.refused_nets())
def test_supports_names_the_reason(label, net, head, word):
    why = tg.DeviceActor.supports(net(), head)
    assert isinstance(why, str) and word in why, why


def test_symbols_are_declared_bound_and_exported_and_the_abi_is_still_13():
    N, lib = tg._native, tg._native.load()
    header = open(f"{REPO}/include/trajopt_grpo_hip.h").read()
    for name in ("tg_policy_step_limits", "tg_policy_step", "tg_policy_values"):
        declared = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\);", header).group(1).split(",")
        assert len(declared) == len(N.SIGNATURES[name][1]) and hasattr(lib, name), name
    for struct, cls in (("tg_policy_net", N.PolicyNet), ("tg_policy_step_args", N.PolicyStepArgs)):
        body = re.search(r"typedef struct " + struct + r" \{(.*?)\} " + struct + ";", header, re.S).group(1)
        assert re.findall(r"\s([a-z_]+)(?:\[\w+\])?;", body) == [name for name, _ in cls._fields_]
    lim = [N.C.c_int32() for _ in range(3)]
    assert lib.tg_policy_step_limits(*(N.C.byref(v) for v in lim)) == 0
    assert [v.value for v in lim] == [tg.policy_step.MAX_OBS_DIM, tg.policy_step.MAX_HIDDEN_LAYERS, tg.policy_step.MAX_ACT_DIM]
    assert int(re.search(r"#define\s+TG_POLICY_STEP_STREAM\s+(0x[0-9a-f]+)u", header).group(1), 16) == N.TG_POLICY_STEP_STREAM == R.STREAM
    assert lib.tg_abi_version() == N.ABI_VERSION == 13 and "DeviceActor" in tg.__all__
