"""The privileged critic without a GPU: the constructor keyword and its refusals, off being the old policy byte for byte, the two nets'
widths, policy.value() / forward() against the NumPy restatement (tests/privileged_fp64.py) exactly, checkpoints and both load refusals,
the spec the learner hands tg_privileged_rows, the C entry point's refusals (host code, no launch), and that a plain PPO never reaches
the new path."""
import copy
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import privileged_fp64 as Y

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANGES = {"tether_length": (0.5, 2.0), "mass": (0.7, 1.4), "Izz": (0.9, 0.9)}        # mapping order != p[] order; one hi == lo


@pytest.fixture(scope="module")
def tg():
    import trajopt_grpo_amd as tg
    return tg


def _policy(tg, S=5, **kw):
    return tg.GaussianActorCritic_NeuralNetwork(S, 2, (16, 16), cov=[0.1, 0.4], device="cpu", **kw)


def test_keyword_is_validated_and_belongs_to_the_actor_critic_only(tg):
    for off in (None, {}):
        assert _policy(tg, privileged_critic=off).privileged_critic is None
    for bad in (3, "mass", [("mass", (0.5, 2.0))], True):
        with pytest.raises(ValueError, match="privileged_critic"):
            _policy(tg, privileged_critic=bad)
    for rng in ((0.0, 1.0), (-1.0, 1.0), (2.0, 1.0), (1.0, float("inf")), (float("nan"), 1.0), (1.0,), (1.0, 2.0, 3.0), "ab", None, 1.0):
        with pytest.raises(ValueError, match="privileged_critic.*mass"):
            _policy(tg, privileged_critic={"mass": rng})
    with pytest.raises(ValueError, match="privileged_critic.*13"):
        _policy(tg, privileged_critic={f"p{i}": (0.5, 2.0) for i in range(13)})
    assert len(_policy(tg, privileged_critic={f"p{i}": (0.5, 2.0) for i in range(12)}).privileged_center) == 12
    with pytest.raises(TypeError):
        tg.GaussianActorCritic_NeuralNetwork(5, 2, (8,), "ReLU", 0.1, "cpu", False, False, 10.0, 1e-8, False, 1e-8, RANGES)   # keyword-only
    with pytest.raises(TypeError, match="privileged_critic"):
        tg.GaussianActor_NeuralNetwork(5, 2, (8,), device="cpu", privileged_critic=RANGES)
    pol = _policy(tg, privileged_critic=RANGES)
    assert list(pol.privileged_critic) == list(RANGES) and pol.privileged_critic == {k: (float(a), float(b)) for k, (a, b) in RANGES.items()}
    c, s = Y.center_scale(RANGES)
    assert pol.privileged_center == c == [1.25, 0.5 * (0.7 + 1.4), 0.9] and pol.privileged_scale == s == [2.0 / 1.5, 2.0 / (1.4 - 0.7), 0.0]
    assert all(type(v) is float for v in pol.privileged_center + pol.privileged_scale)


def test_off_is_the_old_policy_byte_for_byte(tg):
    torch.manual_seed(3)
    plain = _policy(tg)
    torch.manual_seed(3)
    off = _policy(tg, privileged_critic={})
    sd_a, sd_b = plain.state_dict(), off.state_dict()
    assert set(sd_a) == set(sd_b) == {"actor", "critic"}
    for net in ("actor", "critic"):
        assert list(sd_a[net]) == list(sd_b[net])
        for k in sd_a[net]:
            assert sd_a[net][k].shape == sd_b[net][k].shape and sd_a[net][k].numpy().tobytes() == sd_b[net][k].numpy().tobytes()
    assert plain.metadata() == off.metadata() and "privileged_critic" not in off.metadata()
    x = torch.randn(7, 5)
    assert torch.equal(plain.value(x), off.value(x))
    with pytest.raises(ValueError, match="privileged_critic"):
        off.value(x, factors=torch.ones(7, 1))


def test_widths_and_metadata(tg):
    pol = _policy(tg, privileged_critic=RANGES)
    assert pol.actor.network[0].in_features == 5 and pol.critic.network[0].in_features == 5 + 3
    assert pol.actor.input_dim == 5 and pol.critic.input_dim == 8 and pol.input_dim == 5
    md, plain = pol.metadata(), _policy(tg).metadata()
    assert md["privileged_critic"] == {"tether_length": [0.5, 2.0], "mass": [0.7, 1.4], "Izz": [0.9, 0.9]}
    assert list(md["privileged_critic"]) == list(RANGES)
    assert md["num_parameters"] == plain["num_parameters"] + 3 * 16 and md["input_dim"] == 5
    assert {k: v for k, v in md.items() if k not in ("privileged_critic", "num_parameters")} == \
           {k: v for k, v in plain.items() if k != "num_parameters"}
    twin = copy.deepcopy(pol)                                                             # (the learners' old_policy)
    assert twin.privileged_critic == pol.privileged_critic and twin.critic.network[0].in_features == 8
    assert all(torch.equal(p, q) for p, q in zip(twin.parameters(), pol.parameters()))


@pytest.mark.parametrize("normalize_obs", [False, True])
@pytest.mark.parametrize("normalize_value", [False, True])
def test_value_is_the_critic_of_the_concatenated_row_exactly(tg, normalize_obs, normalize_value):
    rng = np.random.default_rng(7)
    torch.manual_seed(11)
    pol = _policy(tg, privileged_critic=RANGES, normalize_obs=normalize_obs, normalize_value=normalize_value)
    if normalize_obs:
        pol.obs_norm.set(rng.normal(size=5), rng.uniform(0.3, 3.0, size=5), 1000)
    if normalize_value:
        pol.value_norm.set(97.3, 911.7, 1000)
    obs = torch.from_numpy(rng.normal(size=(257, 5)).astype(np.float32) * 4.0)
    lo, hi = np.array([r[0] for r in RANGES.values()]), np.array([r[1] for r in RANGES.values()])
    factors = lo + (hi - lo) * rng.uniform(size=(257, 3))
    factors[0], factors[1] = lo, hi                                                       # the ends of the range
    x = Y.features_of_factors(factors, *Y.center_scale(RANGES))
    assert x.dtype == np.float32 and np.array_equal(x[0], [-1.0, -1.0, 0.0]) and np.array_equal(x[1], [1.0, 1.0, 0.0])
    assert np.all(np.abs(x) <= 1.0) and not np.any(x[:, 2])                               # hi == lo: the column is zero
    assert np.array_equal(pol.privileged_features(torch.from_numpy(factors)).numpy(), x)
    with torch.no_grad():
        seen = pol.obs_norm.normalize(obs) if normalize_obs else obs                      # (the privileged columns are not normalised)
        want = pol.critic(torch.cat([seen, torch.from_numpy(x)], dim=1)).squeeze()
        if normalize_value:
            want = pol.value_norm.denormalize(want)
        got = pol.value(obs, torch.from_numpy(factors))
        assert got.dtype == torch.float32 and torch.equal(got, want)
        assert torch.equal(pol.value(obs.numpy(), factors), want)                         # NumPy inputs, as the reference's API takes them
        # factors=None is the nominal vehicle: every factor 1
        nominal = pol.value(obs)
        assert torch.equal(nominal, pol.value(obs, torch.ones(257, 3, dtype=torch.float64))) and not torch.equal(nominal, got)
        assert torch.equal(pol.value(obs[3]), nominal[3]) or torch.allclose(pol.value(obs[3]), nominal[3], rtol=0, atol=1e-5)
        torch.manual_seed(5)
        a1, lp1, v1 = pol.forward(obs, torch.from_numpy(factors))
        torch.manual_seed(5)
        a2, lp2, v2 = pol(obs)
        raw = pol.critic(torch.cat([seen, torch.from_numpy(x)], dim=1))
        assert np.array_equal(a1, a2) and torch.equal(lp1, lp2)                           # the actor does not see the factors
        assert torch.equal(v1, raw) and v2.shape == v1.shape and not torch.equal(v1, v2)  # forward() returns the critic's raw output
    with pytest.raises(ValueError, match="3 columns"):
        pol.value(obs, torch.ones(257, 2))
    assert pol.value(obs, torch.from_numpy(factors)).requires_grad


def test_checkpoint_round_trip_and_both_refusals(tg, tmp_path):
    torch.manual_seed(1)
    pol, plain = _policy(tg, privileged_critic=RANGES), _policy(tg)
    pol.save(str(tmp_path))
    sd = torch.load(tmp_path / "policy.pt", weights_only=True)
    assert set(sd) == {"actor", "critic"} and sd["critic"]["network.0.weight"].shape == (16, 8) and sd["actor"]["network.0.weight"].shape == (16, 5)
    again = _policy(tg, privileged_critic=RANGES)
    again.load(str(tmp_path))
    assert all(torch.equal(p, q) for p, q in zip(again.parameters(), pol.parameters()))
    x, f = torch.randn(9, 5), torch.rand(9, 3) + 0.6
    assert torch.equal(again.value(x, f), pol.value(x, f))
    # a privileged checkpoint into a plain policy, and a checkpoint of another width into a privileged one: ValueError, by name
    before = [p.detach().clone() for p in plain.parameters()]
    with pytest.raises(ValueError, match="privileged_critic"):
        plain.load(str(tmp_path))
    with pytest.raises(ValueError, match="privileged_critic"):
        plain.load_state_dict(pol.state_dict())
    assert all(torch.equal(p, q) for p, q in zip(plain.parameters(), before))              # refused before anything was copied
    with pytest.raises(ValueError, match="privileged_critic"):
        pol.load_state_dict(plain.state_dict())
    with pytest.raises(ValueError, match="privileged_critic"):
        _policy(tg, privileged_critic={"mass": (0.7, 1.4)}).load_state_dict(pol.state_dict())
    pol.load_state_dict(again.state_dict())                                                # equal widths load as ever
    plain.load_state_dict(_policy(tg).state_dict())


def test_spec_maps_names_to_parameter_slots_in_mapping_order(tg):
    A, N = tg.algorithms, tg._native
    assert C.sizeof(N.PrivilegedSpec) == 4 + 12 * 4 + 4 + 3 * 12 * 8 and N.PrivilegedSpec.nominal.offset == 56     # 4 bytes of padding
    quad = tg.QuadPole(max_steps=16)
    pol = tg.GaussianActorCritic_NeuralNetwork(20, 4, (16,), device="cpu", privileged_critic=RANGES)
    spec = A.privileged_spec(pol, quad)
    assert spec.count == 3 and list(spec.index)[:3] == [3, 0, 6] == [quad.RANDOMIZABLE[k] for k in RANGES]
    p = quad.native_params().p
    assert list(spec.nominal)[:3] == [p[3], p[0], p[6]] == [0.5, 1.5, p[6]]
    assert list(spec.center)[:3] == pol.privileged_center and list(spec.scale)[:3] == pol.privileged_scale
    quad.mass = 2.0                                                                        # attributes are live parameters
    assert A.privileged_spec(pol, quad).nominal[1] == 2.0
    cart = tg.CartPole(max_steps=16)
    pol_c = tg.GaussianActorCritic_NeuralNetwork(5, 1, (16,), device="cpu", privileged_critic={"length": (0.5, 1.5), "masscart": (0.8, 1.2)})
    spec = A.privileged_spec(pol_c, cart)
    assert spec.count == 2 and list(spec.index)[:2] == [2, 0] and list(spec.nominal)[:2] == [cart.native_params().p[2], cart.native_params().p[0]]
    with pytest.raises(ValueError, match="tether_length"):
        A.privileged_spec(pol, cart)


def test_entry_point_is_declared_bound_and_refuses_bad_arguments_on_the_host(tg):
    N = tg._native
    header = open(os.path.join(REPO, "include", "trajopt_grpo_hip.h")).read()
    assert "tg_privileged_rows" in set(re.findall(r"\b(tg_[a-z0-9_]+)\s*\(", header)) and "tg_privileged_spec" in header
    assert len(N.SIGNATURES["tg_privileged_rows"][1]) == 13
    lib = N.load()
    spec = N.PrivilegedSpec()
    spec.count = 2
    for k, (i, nom) in enumerate(((3, 0.5), (0, 1.5))):
        spec.index[k], spec.nominal[k], spec.center[k], spec.scale[k] = i, nom, 1.25, 4.0 / 3.0
    buf = (C.c_char * 256)()
    ptr = (C.addressof(buf) + 15) // 16 * 16                                               # a 16-byte aligned host address: never read
    ok = dict(src=ptr, src_pad=8, S=5, idx=ptr, rows=4, n=4, ptab=ptr, spec=spec, dst=ptr, dst_pad=8, bf16=0, ones=-1)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.tg_privileged_rows(a["src"], a["src_pad"], a["S"], a["idx"], a["rows"], a["n"], a["ptab"],
                                      None if a["spec"] is None else C.byref(a["spec"]), a["dst"], a["dst_pad"], a["bf16"], a["ones"], None)

    def changed(**kw):
        s = N.PrivilegedSpec.from_buffer_copy(spec)
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(s, k)[v[0]] = v[1]
            else:
                setattr(s, k, v)
        return s

    assert call(rows=0) == 0 and call(rows=0, idx=None) == 0                               # nothing to do: TG_OK, no launch
    refused = [dict(src=None), dict(ptab=None), dict(spec=None), dict(dst=None), dict(spec=changed(count=0)), dict(spec=changed(count=13)),
               dict(spec=changed(index=(1, 12))), dict(spec=changed(index=(0, -1))), dict(spec=changed(index=(1, 3))),
               dict(S=0), dict(S=9), dict(S=7), dict(dst_pad=4, S=3, src_pad=4, spec=changed(count=2)), dict(ones=0), dict(ones=6), dict(ones=8),
               dict(ones=-2), dict(src_pad=6), dict(dst_pad=12, bf16=1), dict(src_pad=12, bf16=1), dict(dst_pad=68), dict(src_pad=68),
               dict(spec=changed(nominal=(0, 0.0))), dict(spec=changed(nominal=(1, float("inf")))), dict(spec=changed(nominal=(1, float("nan")))),
               dict(spec=changed(center=(0, float("nan")))), dict(spec=changed(scale=(1, float("inf")))), dict(n=0), dict(n=-4),
               dict(rows=-1), dict(idx=None, rows=5)]
    for kw in refused:
        assert call(**kw) == N.TG_ERR_ARG, kw
        assert b"tg_privileged_rows" in lib.tg_last_error(), kw
    assert call(ones=7, rows=0) == 0 and call(S=6, rows=0) == 0 and call(bf16=1, src_pad=8, dst_pad=16, rows=0) == 0
    if not torch.cuda.is_available():
        with pytest.raises(N.NativeLibraryError, match="no CPU fallback"):
            tg.hip_ops.privileged_rows(torch.zeros(4, 8), 5, None, 4, torch.ones(12, 4, dtype=torch.float64), spec, torch.zeros(4, 8))


def test_a_plain_policy_never_reaches_the_privileged_path(tg, monkeypatch):
    """privileged_critic off: the learner's one gate returns None before it looks at the buffer, the engine or the library."""
    K, A = tg.hip_ops, tg.algorithms

    def boom(*a, **k):
        raise AssertionError("the privileged path was entered by a plain policy")

    monkeypatch.setattr(K, "privileged_rows", boom)
    monkeypatch.setattr(A, "privileged_spec", boom)
    monkeypatch.setattr(K.N, "PrivilegedSpec", boom)
    monkeypatch.setattr(A.PPO, "_critic_rows", boom)
    monkeypatch.setattr(A.PPO, "_privileged_rows", boom)
    pol = _policy(tg)
    ppo = tg.PPO(0.2, pol, torch.optim.Adam(pol.parameters(), lr=1e-3), None, 2, batch_size=None)
    assert ppo._privileged_setup(object(), object()) is None
    assert "privileged_critic" not in ppo.metadata()
    # ... and a privileged policy without an engine behind the buffer is refused there, by name
    priv = _policy(tg, privileged_critic=RANGES)
    ppo = tg.PPO(0.2, priv, torch.optim.Adam(priv.parameters(), lr=1e-3), None, 2, batch_size=None)
    assert ppo.old_policy.privileged_critic == priv.privileged_critic and "privileged_critic" not in ppo.metadata()
    with pytest.raises(ValueError, match="privileged_critic.*no rollout engine"):
        ppo._privileged_setup(object(), object())


def test_train_ppo_tool_has_the_switch():
    src = open(os.path.join(REPO, "tools", "train_ppo.py")).read()
    assert "--privileged-critic" in src and "privileged_critic" in src
