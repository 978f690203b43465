"""PopArt without a GPU: the new entry point in the header, the library and the binding (ABI still 13), its refusals before any launch,
the constructor keyword, the host path of ValueNorm._merge(head=...) against the NumPy restatement (tests/popart_fp64.py) bit for
bit, the restatement's own preservation bound, and that the bound is a demand: the un-rescaled head misses it by orders of
magnitude on the same inputs."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import popart_fp64 as P
import value_norm_fp64 as Y

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 1e-8
# statistics moves (before: 5000 returns of mean 100, sigma 30): the batch's (size, mean, sigma).  The mean moves by at least one sigma
# and sigma by a factor of 2 and of 1 / 2 (the acceptance conditions below check what the merged statistics make of them)
MOVES = {"sigma_doubles": (20000, 180.0, 56.0), "sigma_halves": (200000, 60.0, 13.0), "mean_moves": (5000, 190.0, 30.0)}


@pytest.fixture(scope="module")
def tg():
    import trajopt_grpo_amd as tg
    return tg


def _policy(tg, **kw):
    return tg.GaussianActorCritic_NeuralNetwork(5, 2, (16, 16), cov=[0.1, 0.4], device="cpu", **kw)


def _move(name):
    """(stats_before, moments of the batch, stats_after) of one of MOVES, from fixed seeds."""
    rng = np.random.default_rng(sorted(MOVES).index(name))
    before = Y.merge(0.0, 0.0, 0.0, Y.moments(100.0 + 30.0 * rng.normal(size=5000)))
    n, mean, std = MOVES[name]
    mom = Y.moments(mean + std * rng.normal(size=n))
    return before, mom, Y.merge(*before, mom)


def test_the_symbol_is_declared_exported_and_bound_and_the_abi_is_still_13(tg):
    N = tg._native
    header = open(os.path.join(REPO, "include", "trajopt_grpo_hip.h")).read()
    declared = set(re.findall(r"\b(tg_[a-z0-9_]+)\s*\(", header))
    lib = N.load()
    name = "tg_value_norm_merge_popart"
    assert name in declared and name in N.SIGNATURES and hasattr(lib, name)
    assert int(re.search(r"#define\s+TG_ABI_VERSION\s+(\d+)", header).group(1)) == N.ABI_VERSION == lib.tg_abi_version() == 13
    res, args = N.SIGNATURES[name]
    assert res is C.c_int and len(args) == 11 and args[1] is C.c_double and args[8] is C.c_int32
    assert len(N.SIGNATURES["tg_value_norm_merge"][1]) == 8                              # the plain entry point: as it was
    assert callable(tg.hip_ops.value_norm_merge_popart)


def test_every_argument_refusal_comes_before_a_launch(tg):
    """Host memory stands in for the device pointers: a call that passed the checks would launch on them, so each call below breaks
    exactly one rule and must come back TG_ERR_ARG with the rule's message."""
    lib = tg._native.load()
    d = (C.c_double * 4)()
    f = (C.c_float * 8)()
    pd, pf = C.cast(d, C.c_void_p), C.cast(f, C.c_void_p)
    good = dict(mom=None, eps=1e-8, count=pd, mean=pd, m2=pd, table=pf, norm8=None, w=pf, hidden=4, b=pf)

    def call(**kw):
        a = dict(good, **kw)
        return lib.tg_value_norm_merge_popart(a["mom"], a["eps"], a["count"], a["mean"], a["m2"], a["table"], a["norm8"], a["w"],
                                              a["hidden"], a["b"], None)
    for key in ("count", "mean", "m2", "table"):
        assert call(**{key: None}) == -1 and b"null pointer" in lib.tg_last_error(), key
    for key in ("w", "b"):
        assert call(**{key: None}) == -1 and b"null critic head" in lib.tg_last_error(), key
    for eps in (-1e-8, float("nan")):
        assert call(eps=eps) == -1 and b"eps" in lib.tg_last_error()
    for hidden in (0, -3):
        assert call(hidden=hidden) == -1 and b"hidden" in lib.tg_last_error()
    if not torch.cuda.is_available():
        z = [torch.zeros(1, dtype=torch.float64) for _ in range(3)]
        with pytest.raises(tg._native.NativeLibraryError, match="no CPU fallback"):
            tg.hip_ops.value_norm_merge_popart(None, 1e-8, *z, torch.zeros(4), None, torch.zeros(1, 4), torch.zeros(1))


def test_the_keyword_is_validated_off_by_default_and_shows_in_metadata(tg):
    pol = _policy(tg, normalize_value=True)
    assert pol.value_norm.popart is False and "popart" not in pol.metadata()
    on = _policy(tg, normalize_value=True, popart=True)
    assert on.value_norm.popart is True and on.metadata()["popart"] is True and on.metadata()["normalize_value"] is True
    with pytest.raises(ValueError, match="normalize_value=True"):
        _policy(tg, popart=True)
    for bad in (1, "yes", None, 0.0):
        with pytest.raises(ValueError, match="popart"):
            _policy(tg, normalize_value=True, popart=bad)
    with pytest.raises(TypeError):
        tg.GaussianActor_NeuralNetwork(5, 2, (8,), device="cpu", popart=True)            # no critic, no keyword
    # the checkpoint has no new keys, and loads either way round
    assert set(on.state_dict()) == set(pol.state_dict())
    pol.load_state_dict(on.state_dict())
    on.load_state_dict(pol.state_dict())
    # PPO shares the object with its copy; GRPO ignores the flag
    ppo = tg.PPO(0.2, on, torch.optim.Adam(on.parameters(), lr=1e-3), None, 1, batch_size=None)
    assert ppo.old_policy.value_norm is on.value_norm
    assert "popart" not in tg.GRPO(0.2, 0.0, 0.99, on, torch.optim.Adam(on.parameters(), lr=1e-3)).metadata()


@pytest.mark.parametrize("name", sorted(MOVES))
def test_the_host_path_is_the_restatement_bit_for_bit(tg, name):
    before, mom, after = _move(name)
    pol = _policy(tg, normalize_value=True, popart=True)
    vn, head = pol.value_norm, pol.critic.network[-1]
    assert tuple(head.weight.shape) == (1, 16) and tuple(head.bias.shape) == (1,)
    w0, b0 = head.weight.detach().numpy().copy(), head.bias.detach().numpy().copy()
    norm8 = torch.arange(8, dtype=torch.float32) + 0.25
    # the first merge fills empty statistics: the head keeps its bits
    first = Y.moments(100.0 + 30.0 * np.random.default_rng(sorted(MOVES).index(name)).normal(size=5000))
    vn._merge(torch.from_numpy(first), norm8, head=head)
    assert (float(vn.count), float(vn.mean), float(vn.m2)) == before
    assert np.array_equal(head.weight.detach().numpy().view(np.int32), w0.view(np.int32))
    assert np.array_equal(head.bias.detach().numpy().view(np.int32), b0.view(np.int32))
    # the second moves them: statistics and table as the plain merge leaves them, the head as the restatement's
    vn._merge(torch.from_numpy(mom), norm8, head=head)
    assert (float(vn.count), float(vn.mean), float(vn.m2)) == after
    assert np.array_equal(vn.table.numpy().view(np.int32), Y.table(*after, EPS).view(np.int32))
    assert norm8[2] == vn.table[0] and norm8[3] == vn.table[2]
    w1, b1 = P.rescale(w0, b0, before, after, EPS)
    assert not np.array_equal(w1, w0) and not np.array_equal(b1, b0)
    assert np.array_equal(head.weight.detach().numpy().view(np.int32), w1.view(np.int32))
    assert np.array_equal(head.bias.detach().numpy().view(np.int32), b1.view(np.int32))
    # a plain policy fed the same moments holds the same statistics (and its head never moves)
    plain = _policy(tg, normalize_value=True)
    for m in (first, mom):
        plain.value_norm._merge(torch.from_numpy(m))
    assert (float(plain.value_norm.count), float(plain.value_norm.mean), float(plain.value_norm.m2)) == after
    assert torch.equal(plain.value_norm.table, vn.table)
    # nothing to merge, an empty batch, frozen-style None, set() and load_state(): not a bit of the head moves
    kept = (head.weight.detach().clone(), head.bias.detach().clone())
    vn._merge(None, None, head=head)
    vn._merge(torch.tensor([0.0, 5.0, 25.0], dtype=torch.float64), None, head=head)
    vn.set(3.0, 4.0, 100.0)
    vn.load_state(*(torch.tensor([x], dtype=torch.float64) for x in after))
    assert torch.equal(head.weight, kept[0]) and torch.equal(head.bias, kept[1])
    # a head of another shape or dtype is refused
    with pytest.raises(ValueError, match="PopArt rescales"):
        vn._merge(torch.from_numpy(mom), None, head=torch.nn.Linear(16, 2))
    with pytest.raises(ValueError, match="PopArt rescales"):
        vn._merge(torch.from_numpy(mom), None, head=torch.nn.Linear(16, 1).double())


def test_a_zero_sigma_skips_the_rescale(tg):
    """eps = 0 and a history without variance: sigma_a = 0, nothing to preserve -- restatement and host path alike."""
    before = Y.merge(0.0, 0.0, 0.0, Y.moments(np.full(7, 3.25)))
    assert before[2] == 0.0
    mom = Y.moments(np.array([1.0, 2.0, 4.0]))
    after = Y.merge(*before, mom)
    w, b = np.array([0.5, -0.25, 3.0], dtype=np.float32), np.array([0.125], dtype=np.float32)
    assert not P.rescaled(before, after, 0.0) and P.rescaled(before, after, 1e-8)
    w1, b1 = P.rescale(w, b, before, after, 0.0)
    assert np.array_equal(w1, w) and np.array_equal(b1, b)
    pol = tg.GaussianActorCritic_NeuralNetwork(5, 2, (16, 16), device="cpu", normalize_value=True, value_eps=0.0, popart=True)
    head = pol.critic.network[-1]
    kept = (head.weight.detach().clone(), head.bias.detach().clone())
    pol.value_norm.load_state(*(torch.tensor([x], dtype=torch.float64) for x in before))
    pol.value_norm._merge(torch.from_numpy(mom), None, head=head)
    assert (float(pol.value_norm.count), float(pol.value_norm.mean), float(pol.value_norm.m2)) == after
    assert torch.equal(head.weight, kept[0]) and torch.equal(head.bias, kept[1])
    # empty statistics before the merge, and no merge at all
    assert not P.rescaled((0.0, 0.0, 0.0), after, 1e-8) and not P.rescaled(after, after, 1e-8)


@pytest.mark.parametrize("hidden", [8, 264])
@pytest.mark.parametrize("name", sorted(MOVES))
def test_the_restatement_preserves_the_outputs_within_its_bound_and_the_bound_demands_it(name, hidden):
    before, mom, after = _move(name)
    sa, sn = float(P.sigma(before, EPS)), float(P.sigma(after, EPS))
    # conditions on the inputs: the mean moved by at least one (old) sigma, sigma by the factor the case is named after
    assert abs(after[1] - before[1]) >= sa
    lo, hi = {"sigma_doubles": (1.9, 2.1), "sigma_halves": (0.45, 0.55), "mean_moves": (1.6, 2.0)}[name]
    assert lo < sn / sa < hi
    rng = np.random.default_rng(100 + hidden)
    w = (rng.normal(size=hidden) / np.sqrt(hidden)).astype(np.float32)
    b = np.array([0.3], dtype=np.float32)
    h = np.maximum(rng.normal(size=(64, hidden)), 0.0).astype(np.float32)                # hidden rows behind a ReLU
    w1, b1 = P.rescale(w, b, before, after, EPS)
    y, y1 = P.predict(w, b, before, EPS, h), P.predict(w1, b1, after, EPS, h)
    bound = P.preservation_bound(w1, b1, b, before, after, EPS, h)
    err = np.abs(y1 - y).astype(np.float64)
    print(name, hidden, "max |y' - y| / bound", float((err / bound).max()), "bound / sigma_n", float(bound.max() / sn))
    assert np.all(err <= bound)
    # not vacuous: the same head read with the new statistics, un-rescaled, misses the bound by a factor of at least 100
    y0 = P.predict(w, b, after, EPS, h)
    miss = np.abs(y0 - y).astype(np.float64)
    assert np.all(miss >= 100.0 * bound), float((miss / bound).min())
