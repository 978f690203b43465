"""Global gradient-norm clipping, host side (no GPU): the entry points of the C ABI and their refusals (checked before anything is
launched: the pointers below are never dereferenced), and the `max_grad_norm` keyword of the two learners."""
import math

import pytest
import torch

import trajopt_grpo_amd as tg

N = tg._native
CLIP_ENTRIES = ["tg_grad_clip_coef", "tg_adam_step_clip", "tg_adam_step_push_clip"]
FAKE = 256
ADAM = (1e-3, 0.9, 0.999, 1e-8, 1)          # lr, beta1, beta2, eps, step


def test_clip_entry_points_are_exported_and_the_abi_is_13():
    lib = N.load()
    for name in CLIP_ENTRIES + ["tg_grad_clip_workspace"]:
        assert name in N.SIGNATURES and hasattr(lib, name), name
    assert lib.tg_abi_version() == N.ABI_VERSION == 13
    # one float64 partial per block of 4,096 elements, at most 1,024 blocks; nothing for an empty buffer
    assert lib.tg_grad_clip_workspace(0) == 0 and lib.tg_grad_clip_workspace(-5) == 0
    assert lib.tg_grad_clip_workspace(1) == 8 and lib.tg_grad_clip_workspace(4096) == 8 and lib.tg_grad_clip_workspace(4097) == 16
    assert lib.tg_grad_clip_workspace(1 << 40) == 8 * 1024


def test_grad_clip_coef_refusals():
    lib = N.load()
    assert lib.tg_grad_clip_coef(None, 10, 1.0, FAKE, FAKE, None) < 0 and b"null pointer" in lib.tg_last_error()
    assert lib.tg_grad_clip_coef(FAKE, 10, 1.0, None, FAKE, None) < 0 and b"null pointer" in lib.tg_last_error()
    assert lib.tg_grad_clip_coef(FAKE, 10, 1.0, FAKE, None, None) < 0 and b"null pointer" in lib.tg_last_error()
    assert lib.tg_grad_clip_coef(FAKE, 0, 1.0, None, FAKE, None) < 0 and b"null pointer" in lib.tg_last_error()
    assert lib.tg_grad_clip_coef(FAKE, -1, 1.0, FAKE, FAKE, None) < 0 and b"negative size -1" in lib.tg_last_error()
    for bad in (0.0, -2.0, math.inf, -math.inf, math.nan):
        assert lib.tg_grad_clip_coef(FAKE, 10, bad, FAKE, FAKE, None) < 0, bad
        assert b"must be finite and > 0" in lib.tg_last_error(), bad


def test_adam_step_clip_refusals():
    lib = N.load()
    assert lib.tg_adam_step_clip(FAKE, 2, 100, *ADAM, 0, None, None) < 0 and b"tg_adam_step_clip: null d_coef" in lib.tg_last_error()
    assert lib.tg_adam_step_clip(None, 2, 100, *ADAM, 0, FAKE, None) < 0 and b"tg_adam_step_clip: null table" in lib.tg_last_error()
    assert lib.tg_adam_step_clip(FAKE, 0, 100, *ADAM, 0, FAKE, None) < 0 and b"0 tensors outside 1..64" in lib.tg_last_error()
    assert lib.tg_adam_step_clip(FAKE, 65, 100, *ADAM, 0, FAKE, None) < 0 and b"65 tensors outside 1..64" in lib.tg_last_error()
    assert lib.tg_adam_step_clip(FAKE, 2, -1, *ADAM, 0, FAKE, None) < 0 and b"bad sizes" in lib.tg_last_error()
    assert lib.tg_adam_step_clip(FAKE, 2, 100, 1e-3, 0.9, 0.999, 1e-8, 0, 0, FAKE, None) < 0 and b"bad sizes" in lib.tg_last_error()
    assert lib.tg_adam_step_clip(FAKE, 2, 100, 1e-3, 0.4, 0.999, 1e-8, 1, 0, FAKE, None) < 0 and b"beta1 = 0.4" in lib.tg_last_error()
    # total == 0: accepted, nothing launched
    assert lib.tg_adam_step_clip(FAKE, 2, 0, *ADAM, 0, FAKE, None) == 0


def test_adam_step_push_clip_refusals():
    lib = N.load()
    push = (FAKE, 3, FAKE, FAKE)            # segments, n_segments, inv_start, inv_dst
    assert lib.tg_adam_step_push_clip(FAKE, 2, 100, *ADAM, 0, *push, None, None) < 0
    assert b"tg_adam_step_push_clip: null d_coef" in lib.tg_last_error()
    for hole in (0, 9, 11, 12):             # table, segments, inv_start, inv_dst
        args = [FAKE, 2, 100, *ADAM, 0, *push, FAKE, None]
        args[hole] = None
        assert lib.tg_adam_step_push_clip(*args) < 0 and b"tg_adam_step_push_clip: null pointer" in lib.tg_last_error(), hole
    assert lib.tg_adam_step_push_clip(FAKE, 2, 100, *ADAM, 0, FAKE, 0, FAKE, FAKE, FAKE, None) < 0
    assert b"0 segments outside 1..32" in lib.tg_last_error()
    assert lib.tg_adam_step_push_clip(FAKE, 2, 100, *ADAM, 0, FAKE, 33, FAKE, FAKE, FAKE, None) < 0
    assert b"33 segments outside 1..32" in lib.tg_last_error()
    assert lib.tg_adam_step_push_clip(FAKE, 65, 100, *ADAM, 0, *push, FAKE, None) < 0 and b"65 tensors outside 1..64" in lib.tg_last_error()
    assert lib.tg_adam_step_push_clip(FAKE, 2, 0, *ADAM, 0, *push, FAKE, None) == 0


def _grpo(**kw):
    pol = tg.GaussianActor_NeuralNetwork(5, 1, (128, 128), cov=0.5, device="cpu")
    return tg.GRPO(0.15, 0.5, 0.9, pol, torch.optim.Adam(pol.parameters(), lr=3e-4), updates_per_iter=3, **kw)


def _ppo(**kw):
    pol = tg.GaussianActorCritic_NeuralNetwork(20, 4, (64, 64), cov=0.3, device="cpu")
    return tg.PPO(0.2, pol, torch.optim.Adam(pol.parameters(), lr=3e-4), None, 2, batch_size=None, **kw)


@pytest.mark.parametrize("make", [_grpo, _ppo], ids=["GRPO", "PPO"])
def test_max_grad_norm_is_validated_at_construction(make):
    for bad in (0, 0.0, -1.0, math.inf, -math.inf, math.nan, "1.0", True):
        with pytest.raises(ValueError, match="max_grad_norm"):
            make(max_grad_norm=bad)
    assert make().max_grad_norm is None and make(max_grad_norm=None).max_grad_norm is None
    assert make(max_grad_norm=2).max_grad_norm == 2.0 and isinstance(make(max_grad_norm=2).max_grad_norm, float)


def test_metadata_gains_the_key_only_when_the_keyword_is_given():
    assert _grpo().metadata() == {"algorithm": "GRPO", "epsilon": 0.15, "beta": 0.5, "updates_per_iter": 3}
    assert _grpo(max_grad_norm=0.5).metadata() == {"algorithm": "GRPO", "epsilon": 0.15, "beta": 0.5, "updates_per_iter": 3,
                                                   "max_grad_norm": 0.5}
    plain = {"algorithm": "PPO", "epsilon": 0.2, "c1": 0.5, "kl_coeff": 0.5, "gamma": 0.99, "lam": 0.95, "entropy": 0.01,
             "batch_size": None, "updates_per_iter": 2}
    assert _ppo().metadata() == plain
    assert _ppo(max_grad_norm=10.0).metadata() == {**plain, "max_grad_norm": 10.0}


def test_no_rider_is_offered_with_a_clip():
    """Decided before anything touches the device: the rider applies the step while gradient elements are still being completed."""
    algo = _grpo(max_grad_norm=1.0)
    algo._mlps[id(algo.policy.actor)] = type("M", (), {"_f32": object()})()      # (stands for a net on the fp32 chain learner)
    assert algo._adam_rider(algo.policy.actor, last=False, whole_update=True) is None
