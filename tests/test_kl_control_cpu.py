"""kl_stats / desired_kl without a GPU: constructor validation, the new entry points against _native.SIGNATURES and the header, the
float64 restatement's own invariants (tests/kl_control_fp64.py) and the inputs the GPU tests use."""
import math
import os
import re

import numpy as np
import pytest
import torch

import kl_control_fp64 as F
import trajopt_grpo_amd as tg
from trajopt_grpo_amd import _native as N

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _grpo(lr=3e-4, opt=None, **kw):
    pol = tg.GaussianActor_NeuralNetwork(5, 1, (16,), cov=0.5, device="cpu")
    opt = opt(pol) if opt is not None else torch.optim.Adam(pol.parameters(), lr=lr)
    return tg.GRPO(epsilon=0.2, beta=0.0, gamma=0.9, policy=pol, optimizer=opt, updates_per_iter=1, **kw)


def _ppo(lr=3e-4, **kw):
    pol = tg.GaussianActorCritic_NeuralNetwork(5, 1, (16,), cov=0.5, device="cpu")
    return tg.PPO(epsilon=0.2, policy=pol, optimizer=torch.optim.Adam(pol.parameters(), lr=lr), ref_model=None, updates_per_iter=1, **kw)


@pytest.mark.parametrize("make", [_grpo, _ppo])
def test_defaults_and_metadata(make):
    a = make()
    assert a.kl_stats is False and a.desired_kl is None and a.lr_bounds == (1e-5, 1e-2) and a.lr_factor == 1.5
    assert not {"kl_stats", "desired_kl", "lr_bounds", "lr_factor"} & set(a.metadata())
    b = make(kl_stats=True)
    assert b.kl_stats is True and b.desired_kl is None and b.metadata()["kl_stats"] is True and "desired_kl" not in b.metadata()
    c = make(desired_kl=0.01, lr_bounds=(1e-4, 1e-3), lr_factor=2)
    assert c.kl_stats is True and c.desired_kl == 0.01
    md = c.metadata()
    assert md["desired_kl"] == 0.01 and md["lr_bounds"] == [1e-4, 1e-3] and md["lr_factor"] == 2.0


@pytest.mark.parametrize("make", [_grpo, _ppo])
@pytest.mark.parametrize("kw", [
    {"desired_kl": 0.0}, {"desired_kl": -0.01}, {"desired_kl": float("nan")}, {"desired_kl": float("inf")}, {"desired_kl": True},
    {"desired_kl": "0.01"},
    {"lr_bounds": (1e-2, 1e-5)}, {"lr_bounds": (0.0, 1e-2)}, {"lr_bounds": (1e-5, float("inf"))}, {"lr_bounds": (1e-5,)}, {"lr_bounds": 1e-3},
    {"lr_factor": 1.0}, {"lr_factor": 0.5}, {"lr_factor": float("nan")},
    {"kl_stats": 1},
])
def test_constructor_refuses(make, kw):
    with pytest.raises(ValueError):
        make(**kw)


def test_param_groups_must_share_one_lr():
    def two_groups(pol):
        ps = list(pol.parameters())
        return torch.optim.Adam([{"params": ps[:1], "lr": 1e-3}, {"params": ps[1:], "lr": 3e-4}])
    with pytest.raises(ValueError, match="param groups"):
        _grpo(opt=two_groups, desired_kl=0.01)
    _grpo(opt=two_groups, kl_stats=True)                # (measuring alone scales nothing)
    _grpo(opt=two_groups)


def test_lr_outside_the_bounds_is_refused_at_the_first_learn():
    for lr in (1e-6, 0.1):
        a = _grpo(lr=lr, desired_kl=0.01)
        with pytest.raises(ValueError, match="lr_bounds"):
            a._kl_entry_check()
    a = _grpo(lr=1e-3, desired_kl=0.01)
    a._kl_entry_check()
    assert a._kl_bounds_checked
    _grpo(lr=0.1, kl_stats=True)._kl_entry_check()      # (measuring alone: any lr)


def test_new_entry_points_are_declared_bound_and_exported():
    lib = N.load()
    header = open(os.path.join(REPO, "include", "trajopt_grpo_hip.h")).read()
    declared = set(re.findall(r"\b(tg_[a-z0-9_]+)\s*\(", header))
    want = {"tg_policy_shift_blocks": 1, "tg_policy_shift": 15, "tg_policy_shift_finish": 4, "tg_lr_adapt": 8}
    for name, n_args in want.items():
        assert name in declared and name in N.SIGNATURES and hasattr(lib, name), name
        assert len(N.SIGNATURES[name][1]) == n_args, name
    assert lib.tg_abi_version() == N.ABI_VERSION == int(re.search(r"#define\s+TG_ABI_VERSION\s+(\d+)", header).group(1))
    sig = N.SIGNATURES["tg_lr_adapt"][1]
    assert all(t is N.C.c_double for t in sig[1:6])     # desired_kl, factor, lr_min, lr_max and lr BY VALUE, in double
    assert N.SIGNATURES["tg_policy_shift"][1][9] is N.C.c_double and N.SIGNATURES["tg_policy_shift"][1][10] is N.C.c_double


def test_block_count_is_host_arithmetic_of_rows_alone():
    lib = N.load()
    for rows in F.EXACT_ROWS + [-1, 2 * 4096, 1023 * 4096 + 1, 1024 * 4096, 10 ** 9]:
        assert lib.tg_policy_shift_blocks(rows) == F.blocks(rows), rows


def test_native_argument_checks_need_no_device():
    lib = N.load()
    var = (N.C.c_float * 1)(1.0)
    # both / neither of var and d_log_std; a clip range that does not contain 0; a device log_std beyond four columns
    assert lib.tg_policy_shift(0, 1, 0, 1, 1, 0, var, 0x1000, 1, -0.2, 0.2, 0, 0, 0, None) == N.TG_ERR_ARG
    assert lib.tg_policy_shift(0, 1, 0, 1, 1, 0, None, None, 1, -0.2, 0.2, 0, 0, 0, None) == N.TG_ERR_ARG
    assert lib.tg_policy_shift(0, 1, 0, 1, 1, 0, var, None, 1, 0.1, 0.2, 0, 0, 0, None) == N.TG_ERR_ARG
    assert lib.tg_policy_shift(0, 5, 0, 5, 1, 0, None, 0x1000, 5, -0.2, 0.2, 0, 0, 0, None) == N.TG_ERR_ARG
    assert lib.tg_policy_shift(0, 1, 0, 1, 1, 0, var, None, 1, -0.2, 0.2, -1, 0, 0, None) == N.TG_ERR_ARG
    assert lib.tg_policy_shift(0, 1, 0, 1, 1, 0, var, None, 1, -0.2, 0.2, 0, 0, 0, None) == N.TG_OK        # rows == 0: nothing is launched
    assert lib.tg_policy_shift(0, 1, 0, 1, 1, 0, var, None, 1, -0.2, 0.2, 5, 0, 0, None) == N.TG_ERR_ARG   # null pointers with rows
    assert lib.tg_lr_adapt(None, 0.01, 1.5, 1e-5, 1e-2, 1e-3, None, None) == N.TG_ERR_ARG
    assert lib.tg_lr_adapt(0x1000, 0.01, 1.0, 1e-5, 1e-2, 1e-3, 0x1000, None) == N.TG_ERR_ARG
    assert lib.tg_lr_adapt(0x1000, 0.01, 1.5, 1e-2, 1e-5, 1e-3, 0x1000, None) == N.TG_ERR_ARG
    assert lib.tg_policy_shift_finish(None, 3, 0x1000, None) == N.TG_ERR_ARG


# ---- the restatement's own invariants ----
def test_k3_is_nonnegative_and_zero_at_zero():
    d = np.concatenate([np.linspace(-5, 5, 20001), [0.0, 1e-300, -1e-300, 1e-9, -1e-9, 2.0 ** -30]])
    k3 = F.k3_of(d)
    assert np.all(k3 >= 0.0) and F.k3_of(0.0) == 0.0
    small = np.abs(d) < 1e-4
    assert np.all(np.abs(k3[small] - 0.5 * d[small] ** 2) <= 1e-3 * d[small] ** 2 + 1e-24)


def test_lr_rule_branches_and_clamps():
    out = {k: F.lr_rule(*v) for k, v in F.LR_CASES.items()}
    assert out["above"][3] == 1e-3 / 1.5 and out["below"][3] == 1e-3 * 1.5 and out["between"][3] == 1e-3
    assert out["at_upper_threshold"][3] == 1e-3 and out["at_lower_threshold"][3] == 1e-3          # strict comparisons
    assert out["clamp_min"][3] == 1e-5 and out["clamp_max"][3] == 1e-2
    assert out["no_rows"][3] == 1e-3 and math.isnan(out["no_rows"][0]) and math.isnan(out["no_rows"][1])
    assert out["nan_sum"][3] == 1e-3 and math.isnan(out["nan_sum"][0]) and out["nan_sum"][1] == 0.01
    assert out["measure_only"][3] == 1e-3 and out["measure_only"][0] == 0.03
    assert out["factor_2"][3] == 0.15
    for k, v in out.items():
        assert v[2] == F.LR_CASES[k][5], k


def test_dyadic_inputs_are_exact_and_clip_on_both_sides():
    lo, hi = F.log_bounds(0.2)
    for A in (1, 4):
        mean, act, old, var = F.dyadic_inputs(A, 4097)
        assert np.all(mean * 64 == np.round(mean * 64)) and np.abs(mean).max() < 4 and np.abs(act).max() < 4 and np.all(var == 1)
        ref = F.dyadic_reference(mean, act, old, 0.2)
        d = ref["d"]
        assert (d < lo).sum() > 100 and (d > hi).sum() > 100 and ((d >= lo) & (d <= hi)).sum() > 100
        assert ref["n_edge"] == 0 and ref["sums"][0] == 4097 and ref["sums"][1] > 0
        # d is the exact difference of two float32 numbers
        lp = F.dyadic_logp(mean, act)
        assert np.all((lp.astype(np.float64) - d).astype(np.float32) == old)


@pytest.mark.parametrize("name", sorted(F.GENERAL_CASES))
def test_general_inputs_have_no_edge_rows(name):
    inp = F.general_inputs(name)
    A = inp["A"]
    ref = F.general_reference(inp["mean_buf"][:, :A], inp["act"], inp["logp_old"], F.GENERAL_EPSILON, inp.get("var"), inp.get("log_std"))
    lo, hi = F.log_bounds(F.GENERAL_EPSILON)
    d = ref["d"]
    assert ref["n_edge"] == 0
    assert (d < lo).sum() > 50 and (d > hi).sum() > 50 and ((d >= lo) & (d <= hi)).sum() > 50
    assert ref["bound_k3"] < 1e-3 * ref["sums"][1] and ref["bound_d"] < 1e-2 * np.abs(d).sum()      # the bounds say something
