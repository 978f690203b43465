"""target_kl / kl_every without a GPU: the restatement of tg_kl_control (tests/kl_stop_fp64.py) on hand-computed cases, constructor
validation, metadata(), the five new entry points against the header and _native.SIGNATURES, and their argument checks."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import kl_stop_fp64 as S
import trajopt_grpo_amd as tg
from trajopt_grpo_amd import _native as N

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"tg_kl_control": 10, "tg_adam_step_ctl": 13, "tg_adam_step_push_ctl": 17, "tg_adam_step_ctl_clip": 14, "tg_adam_step_push_ctl_clip": 18}


def _grpo(**kw):
    pol = tg.GaussianActor_NeuralNetwork(5, 1, (16,), cov=0.5, device="cpu")
    return tg.GRPO(epsilon=0.2, beta=0.0, gamma=0.9, policy=pol, optimizer=torch.optim.Adam(pol.parameters(), lr=3e-4), updates_per_iter=4, **kw)


def _ppo(**kw):
    pol = tg.GaussianActorCritic_NeuralNetwork(5, 1, (16,), cov=0.5, device="cpu")
    return tg.PPO(epsilon=0.2, policy=pol, optimizer=torch.optim.Adam(pol.parameters(), lr=3e-4), ref_model=None, updates_per_iter=4, **kw)


# ---- the restatement, by hand ----
def test_the_threshold_is_strict():
    at = S.kl_control(*S.CASES["at_threshold_does_not_stop"])
    assert at[S.LAST_KL] == 0.375 == 1.5 * 0.25 and at[S.STOPPED] == 0.0 and at[S.STOP_UPDATE] == 0.0 and at[S.CHECKS] == 1.0
    above = S.kl_control(*S.CASES["next_double_above_stops"])
    assert above[S.LAST_KL] == np.nextafter(0.375, 1.0) and above[S.STOPPED] == 1.0 and above[S.STOP_UPDATE] == 3.0
    assert above[S.KL_AT_STOP] == above[S.LAST_KL] and above[S.LR] == 1e-3 and above[S.LAST_CLIP] == 3.0 / 128.0


def test_nan_and_no_rows_neither_adapt_nor_stop():
    for name in ("nan_sum", "nan_rows", "no_rows"):
        out = S.kl_control(*S.CASES[name])
        assert out[S.STOPPED] == 0.0 and out[S.LR] == 1e-3 and math.isnan(out[S.LAST_KL]) and out[S.CHECKS] == 1.0, name
    assert S.kl_control(*S.CASES["nan_sum"])[S.LAST_CLIP] == 3.0 / 128.0


def test_a_latched_block_comes_back_unchanged():
    before = S.CASES["latched_stays"][0]
    after = S.kl_control(*S.CASES["latched_stays"])
    assert after is not before and np.array_equal(S.bits(after), S.bits(before))


def test_the_lr_rule_at_both_bounds_and_with_a_stop():
    lo = S.kl_control(*S.CASES["lr_clamp_min"])
    hi = S.kl_control(*S.CASES["lr_clamp_max"])
    assert lo[S.LR] == 1e-5 and hi[S.LR] == 1e-2 and lo[S.STOPPED] == hi[S.STOPPED] == 0.0       # (1.2e-5 / 1.5 < 1e-5, 9e-3 * 1.5 > 1e-2)
    both = S.kl_control(*S.CASES["stop_and_adapt"])                          # the check that latches adapts too
    assert both[S.STOPPED] == 1.0 and both[S.LR] == 1e-3 / 1.5 and both[S.STOP_UPDATE] == 7.0 and both[S.KL_AT_STOP] == 3.0
    off = S.kl_control(*S.CASES["target_off"])
    assert off[S.STOPPED] == 0.0 and off[S.LR] == 1e-3 and off[S.LAST_KL] == 3.0


def test_five_checks_through_one_block():
    seq = S.run_sequence()
    assert [b[S.STOPPED] for b in seq] == [0.0, 0.0, 1.0, 1.0, 1.0] and [b[S.CHECKS] for b in seq] == [1.0, 2.0, 3.0, 3.0, 3.0]
    a = 1e-3 / 1.5
    assert [b[S.LR] for b in seq] == [a, a * 1.5, a * 1.5 / 1.5, a * 1.5 / 1.5, a * 1.5 / 1.5]
    assert seq[2][S.STOP_UPDATE] == 3.0 and seq[2][S.KL_AT_STOP] == 0.5
    for later in seq[3:]:
        assert np.array_equal(S.bits(later), S.bits(seq[2]))


# ---- keywords ----
@pytest.mark.parametrize("make", [_grpo, _ppo])
def test_defaults_and_metadata(make):
    a = make()
    assert a.target_kl is None and a.kl_stop_factor == 1.5 and a.kl_every is None and a.kl_stats is False and not a._kl_ctl
    assert not {"target_kl", "kl_stop_factor", "kl_every"} & set(a.metadata())
    b = make(target_kl=0.02)
    assert b.kl_stats is True and b._kl_ctl and not b._kl_adapt_checks
    assert b.metadata()["target_kl"] == 0.02 and b.metadata()["kl_stop_factor"] == 1.5 and "kl_every" not in b.metadata()
    assert "desired_kl" not in b.metadata() and "kl_stats" not in b.metadata()
    c = make(target_kl=1, kl_stop_factor=2, kl_every=3, desired_kl=0.01)
    md = c.metadata()
    assert md["target_kl"] == 1.0 and md["kl_stop_factor"] == 2.0 and md["kl_every"] == 3 and md["desired_kl"] == 0.01 and c._kl_adapt_checks
    d = make(desired_kl=0.01, kl_every=1)
    assert d._kl_ctl and d._kl_adapt_checks and d.metadata()["kl_every"] == 1 and "target_kl" not in d.metadata()
    e = make(desired_kl=0.01)                                               # (today's behaviour: no control block)
    assert not e._kl_ctl and not e._kl_adapt_checks and set(e.metadata()) >= {"desired_kl"} and "kl_every" not in e.metadata()
    f = make(desired_kl=0.01, target_kl=0.02)                               # (checks stop; the rate still moves once per learn())
    assert f._kl_ctl and not f._kl_adapt_checks


@pytest.mark.parametrize("make", [_grpo, _ppo])
@pytest.mark.parametrize("kw", [
    {"target_kl": 0.0}, {"target_kl": -0.01}, {"target_kl": float("nan")}, {"target_kl": float("inf")}, {"target_kl": True},
    {"target_kl": "0.01"},
    {"target_kl": 0.01, "kl_stop_factor": 0.0}, {"target_kl": 0.01, "kl_stop_factor": -1.5}, {"target_kl": 0.01, "kl_stop_factor": float("nan")},
    {"target_kl": 0.01, "kl_stop_factor": float("inf")}, {"target_kl": 0.01, "kl_stop_factor": None}, {"kl_stop_factor": "1.5"},
    {"target_kl": 0.01, "kl_every": 0}, {"target_kl": 0.01, "kl_every": -1}, {"target_kl": 0.01, "kl_every": 1.0},
    {"target_kl": 0.01, "kl_every": True}, {"target_kl": 0.01, "kl_every": "2"}, {"desired_kl": 0.01, "kl_every": 0},
    {"kl_every": 1}, {"kl_every": 2, "kl_stats": True},
])
def test_constructor_refuses(make, kw):
    with pytest.raises(ValueError):
        make(**kw)


def test_train_ppo_has_the_flags():
    src = open(os.path.join(REPO, "tools", "train_ppo.py")).read()
    assert "--target-kl" in src and "--kl-every" in src


# ---- the library ----
def test_new_entry_points_are_declared_bound_and_exported():
    lib = N.load()
    header = open(os.path.join(REPO, "include", "trajopt_grpo_hip.h")).read()
    declared = set(re.findall(r"\b(tg_[a-z0-9_]+)\s*\(", header))
    for name, n_args in NEW.items():
        assert name in declared and name in N.SIGNATURES and hasattr(lib, name), name
        assert len(N.SIGNATURES[name][1]) == n_args, name
    assert lib.tg_abi_version() == N.ABI_VERSION == 13 == int(re.search(r"#define\s+TG_ABI_VERSION\s+(\d+)", header).group(1))
    for name in NEW:
        if name != "tg_kl_control":                     # ... the plain entry point's arguments, then d_ctl, lr_from_ctl, bc1, stream
            plain = N.SIGNATURES[name.replace("_ctl", "")][1]
            assert N.SIGNATURES[name][1] == plain[:-1] + [N.C.c_void_p, N.C.c_int32, N.C.c_double, N.C.c_void_p], name


def test_struct_sizes_are_unchanged():
    sizes = {"EnvParams": 120, "Traj": 64, "AdamTensor": 40, "AdamRider": 96, "RefPenalty": 16, "LearnedStd": 16, "ChainLoss": 144, "LossArgs": 192,
             "DwJob": 64, "CompactArgs": 160}
    for name, size in sizes.items():
        assert ctypes.sizeof(getattr(N, name)) == size, name
    header = open(os.path.join(REPO, "include", "trajopt_grpo_hip.h")).read()
    assert "typedef struct tg_adam_tensor { float* p; float* g; float* m; float* v; int64_t first; } tg_adam_tensor;" in header


FAKE, ADAM = 0x1000, (1e-3, 0.9, 0.999, 1e-8, 1)


def _adam_args(name, table=FAKE, n=2, total=100, adam=ADAM, seg=FAKE, n_seg=1, inv=FAKE, coef=FAKE, ctl=FAKE, from_ctl=1, bc1=0.1):
    args = [table, n, total, *adam, 0]
    if "_push" in name:
        args += [seg, n_seg, inv, inv]
    if name.endswith("_clip"):
        args += [coef]
    return args + [ctl, from_ctl, bc1, None]


@pytest.mark.parametrize("name", [n for n in NEW if n != "tg_kl_control"])
def test_ctl_adam_entry_points_check_their_arguments_and_launch_nothing(name):
    """Every refusal comes back as TG_ERR_ARG before any launch (this machine has no device: a launch would be TG_ERR_HIP)."""
    lib = N.load()
    fn = getattr(lib, name)

    def refused(text, **kw):
        assert fn(*_adam_args(name, **kw)) == N.TG_ERR_ARG and text in lib.tg_last_error(), (kw, lib.tg_last_error())
    refused(b"null", table=None)
    refused(b"d_ctl is null", ctl=None)
    refused(b"8-B aligned", ctl=0x1004)
    refused(b"lr_from_ctl = 2", from_ctl=2)
    refused(b"lr_from_ctl = -1", from_ctl=-1)
    for bad in (0.0, -0.1, 1.5, float("nan")):
        refused(b"bc1", bc1=bad)
    refused(b"0 tensors outside 1..64", n=0)
    refused(b"65 tensors outside 1..64", n=65)
    refused(b"bad sizes", total=-1)
    refused(b"bad sizes", adam=(1e-3, 0.9, 0.999, 1e-8, 0))
    refused(b"beta1 = 0.4", adam=(1e-3, 0.4, 0.999, 1e-8, 1))
    if "_push" in name:
        refused(b"null pointer", seg=None)
        refused(b"null pointer", inv=None)
        refused(b"33 segments outside 1..32", n_seg=33)
    if name.endswith("_clip"):
        refused(b"null d_coef", coef=None)
    assert fn(*_adam_args(name, total=0)) == N.TG_OK                        # an empty table: nothing to launch
    assert fn(*_adam_args(name, total=0, bc1=1.0, from_ctl=0)) == N.TG_OK


def test_kl_control_checks_its_arguments_and_launches_nothing():
    lib = N.load()
    ok = dict(sums=FAKE, target=0.01, stop=1.5, desired=0.01, factor=1.5, lo=1e-5, hi=1e-2, update=1, ctl=FAKE)

    def refused(**kw):
        a = {**ok, **kw}
        rc = lib.tg_kl_control(a["sums"], a["target"], a["stop"], a["desired"], a["factor"], a["lo"], a["hi"], a["update"], a["ctl"], None)
        assert rc == N.TG_ERR_ARG and b"tg_kl_control" in lib.tg_last_error(), (kw, rc, lib.tg_last_error())
    refused(sums=None)
    refused(ctl=None)
    refused(ctl=0x1004)
    refused(sums=0x1004)
    refused(target=float("inf"))
    refused(target=float("nan"))
    refused(desired=float("nan"))
    refused(stop=0.0)
    refused(stop=float("nan"))
    refused(factor=1.0)
    refused(lo=1e-2, hi=1e-5)
    refused(update=0)
    refused(update=-3)
