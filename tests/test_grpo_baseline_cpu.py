"""GRPO(baseline=..., adv_scale=...) without a GPU: keyword validation and the metadata round trip, tg_grpo_step_advantage in the
header / the library's exports / the binding and every argument refusal of it (no launch), and the NumPy restatement of the
kernel's order (tests/grpo_baseline_fp64.py) inside the order-free float64 version's bounds on every shape, mask and value recipe
the GPU tests use."""
import json
import os
import re

import numpy as np
import pytest
import torch

import grpo_baseline_fp64 as F
import trajopt_grpo_amd as tg
from trajopt_grpo_amd import _native as N

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "tg_grpo_step_advantage"


def _grpo(**kw):
    pol = tg.GaussianActor_NeuralNetwork(5, 1, (16,), cov=0.5, device="cpu")
    return tg.GRPO(epsilon=0.15, beta=0.5, gamma=0.9, policy=pol, optimizer=torch.optim.Adam(pol.parameters(), lr=3e-4), updates_per_iter=3, **kw)


def test_defaults_are_the_group_baseline():
    a = _grpo()
    assert a.baseline == "group" and a.adv_scale == "std"
    assert a.metadata() == _grpo(baseline="group").metadata() == _grpo(baseline="group", adv_scale="std").metadata()
    assert not {"baseline", "adv_scale"} & set(a.metadata())            # (the default leaves the metadata as it was)


@pytest.mark.parametrize("kw", [{"baseline": "step"}, {"baseline": "step", "adv_scale": "std"}, {"baseline": "step", "adv_scale": "none"}])
def test_step_keywords_are_kept(kw):
    a = _grpo(**kw)
    assert a.baseline == "step" and a.adv_scale == kw.get("adv_scale", "std")
    assert a.metadata()["baseline"] == "step" and a.metadata()["adv_scale"] == a.adv_scale


@pytest.mark.parametrize("kw, names", [
    ({"baseline": "time"}, ("group", "step")), ({"baseline": None}, ("group", "step")), ({"baseline": "Step"}, ("group", "step")),
    ({"baseline": 1}, ("group", "step")),
    ({"baseline": "step", "adv_scale": "mean"}, ("std", "none")), ({"baseline": "step", "adv_scale": None}, ("std", "none")),
    ({"adv_scale": "var"}, ("std", "none")),
    ({"baseline": "group", "adv_scale": "none"}, ("std",)), ({"adv_scale": "none"}, ("std",)),
])
def test_bad_keywords_name_the_allowed_values(kw, names):
    with pytest.raises(ValueError) as e:
        _grpo(**kw)
    for name in names:
        assert repr(name) in str(e.value), str(e.value)


def test_metadata_round_trip(tmp_path):
    a = _grpo(baseline="step", adv_scale="none", max_grad_norm=0.5)
    md = json.loads(json.dumps(a.metadata()))
    b = _grpo(**{k: md[k] for k in ("baseline", "adv_scale", "max_grad_norm")})
    assert b.metadata() == a.metadata() and (b.baseline, b.adv_scale) == ("step", "none")

    class Stub:
        def metadata(self):
            return {}
    pipe = tg.pipelines.Pipeline.__new__(tg.pipelines.Pipeline)         # the checkpoint's metadata.json carries the algorithm's
    pipe.test_name = pipe.checkpoint_name = pipe.today = "x"
    pipe.env_name = "CartPole"
    pipe.policy = pipe.buffer = Stub()
    pipe.algorithm = a
    pipe.visualizer = pipe.publisher = pipe.logger = None
    pipe.env = tg.CartPole()
    path = tmp_path / "metadata.json"
    path.write_text(json.dumps(pipe.get_metadata()))
    back = pipe.load_metadata(str(path))["algorithm"]
    assert back["baseline"] == "step" and back["adv_scale"] == "none" and back == a.metadata()


def test_the_factory_forwards_the_keywords():
    pol = tg.GaussianActor_NeuralNetwork(5, 1, (16,), cov=0.5, device="cpu")

    class Manager:                                                       # (the factory only hands it on)
        pass
    made = {}
    orig = tg.pipelines._assemble
    tg.pipelines._assemble = lambda *a, **k: made.setdefault("algorithm", a[4])
    try:
        tg.pipelines.create_cartpole_pipeline_grpo("t", "c", policy=pol, rollout_manager=Manager(), buffer=object(), baseline="step",
                                                   adv_scale="none")
        assert (made["algorithm"].baseline, made["algorithm"].adv_scale) == ("step", "none")
        made.clear()
        tg.pipelines.create_cartpole_pipeline_grpo("t", "c", policy=pol, rollout_manager=Manager(), buffer=object())
        assert (made["algorithm"].baseline, made["algorithm"].adv_scale) == ("group", "std")
        with pytest.raises(ValueError):
            tg.pipelines.create_cartpole_pipeline_grpo("t", "c", policy=pol, rollout_manager=Manager(), buffer=object(), baseline="t")
    finally:
        tg.pipelines._assemble = orig


def test_entry_point_is_declared_bound_and_exported():
    lib = N.load()
    header = open(os.path.join(REPO, "include", "trajopt_grpo_hip.h")).read()
    m = re.search(r"\bint\s+" + ENTRY + r"\s*\(([^)]*)\)\s*;", header)
    assert m is not None, "not declared"
    params = [p.strip() for p in m.group(1).split(",")]
    res, args = N.SIGNATURES[ENTRY]
    assert hasattr(lib, ENTRY) and res is N.C.c_int and len(args) == len(params) == 10
    want = [N.C.c_void_p if "*" in p else {"int64_t": N.C.c_int64, "int32_t": N.C.c_int32, "int": N.C.c_int}[p.split()[0]] for p in params]
    assert list(args) == want, (params, args)
    assert lib.tg_abi_version() == N.ABI_VERSION == 13 == int(re.search(r"#define\s+TG_ABI_VERSION\s+(\d+)", header).group(1))
    makefile = open(os.path.join(REPO, "trajopt-grpo_amd", "csrc", "Makefile")).read()
    assert "grpo_baseline.hip" in re.search(r"^SRCS\s*=(.*)$", makefile, re.M).group(1).split()


P = 0x1000      # a fake device address: every call below is refused, or returns, before anything is launched


@pytest.mark.parametrize("args, text", [
    ((0, P, 8, 4, 2, 1, P, P, P), "null pointer"), ((P, 0, 8, 4, 2, 1, P, P, P), "null pointer"),
    ((P, P, 8, 4, 2, 1, 0, P, P), "null pointer"), ((P, P, 8, 4, 2, 1, P, 0, P), "null pointer"),
    ((P, P, 8, 4, 2, 1, P, P, 0), "null pointer"),
    ((P, P, 8, 4, 0, 1, P, P, P), "group_size 0"), ((P, P, 8, 4, -2, 1, P, P, P), "group_size -2"),
    ((P, P, 9, 4, 2, 1, P, P, P), "n=9 must be a multiple of group_size=2"), ((P, P, -8, 4, 2, 1, P, P, P), "n=-8"),
    ((P, P, 8, 0, 2, 1, P, P, P), "horizon 0"), ((P, P, 8, -1, 2, 1, P, P, P), "horizon -1"),
    ((P, P, 8, 4, 2, 2, P, P, P), "mode 2"), ((P, P, 8, 4, 2, -1, P, P, P), "mode -1"),
])
def test_argument_refusals(args, text):
    lib = N.load()
    rc = getattr(lib, ENTRY)(*args, None)
    assert rc == N.TG_ERR_ARG and rc < 0
    msg = lib.tg_last_error().decode()
    assert msg.startswith(ENTRY + ":") and text in msg, msg


def test_no_envs_is_ok_without_a_launch():
    lib = N.load()
    for mode in (0, 1):
        assert getattr(lib, ENTRY)(P, P, 0, 4, 2, mode, P, P, P, None) == N.TG_OK == 0


def test_lane_counts():
    assert [F.lanes(E) for E in (1, 4, 5, 8, 9, 63, 64, 65, 128, 129, 253, 256, 257, 4100)] == [1, 1, 2, 2, 4, 16, 16, 32, 32, 64, 64, 64, 64, 64]


@pytest.mark.parametrize("shape", F.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_restatement_is_inside_the_fp64_bounds(shape):
    worst = 0.0
    for mk in F.MASKS:
        for vk in F.VALUES:
            R, mask, E = F.case(shape, mk, vk)
            for scale in (True, False):
                A, group, tab = F.kernel_order(R, mask, E, scale)
                tag = f"{shape} {mk} {vk} scale={scale}"
                assert A.dtype == np.float32 and np.isfinite(A).all() and np.isfinite(group).all() and np.isfinite(tab).all(), tag
                worst = max(worst, F.check_against_order_free(tag, A, group, R, mask, E, scale))
                if vk in ("constant", "zeros") or E == 1:               # every residual is exactly +0
                    assert not A.view(np.uint32).any() and group[:, 0].max() == 0.0, tag
                T, G = shape[0], shape[1]
                valid = (mask != 0).reshape(T, G, E)
                assert np.array_equal(tab[0], valid.sum(axis=2).T) and np.array_equal(group[:, 1], valid.sum(axis=(0, 2)))
                assert np.array_equal(group[:, 2], valid.any(axis=2).sum(axis=0))
    print(f"{shape}: worst |restatement - fp64| / bound = {worst:.3f}")


def test_masks_hold_the_cases_they_name():
    rng = np.random.default_rng(0)
    T, G, E = 9, 2, 5
    pre = F.make_mask("prefix", T, G, E, rng)
    assert pre[:, 0].sum() == 0 and (np.diff(pre.astype(int), axis=0) <= 0).all()
    holes = F.make_mask("holes", T, G, E, rng)
    assert (holes == 0).any() and (holes > 1).any()
    one = F.make_mask("one_live", T, G, E, rng).reshape(T, G, E)
    assert (one[T // 2].sum(axis=1) == 1).all()
    assert F.make_mask("none_live", T, G, E, rng)[T // 2].sum() == 0
    R, mask, _ = F.case((9, 2, 5), "holes", "normal")
    assert (R[mask == 0] == F.GARBAGE).all() and np.isfinite(R).all()
