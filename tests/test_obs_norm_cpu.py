"""Running observation normalisation without a GPU: keyword validation, the ObsNorm surface, checkpoints and their two refusals,
metadata, the host path's normalised observation against the NumPy restatement (tests/obs_norm_fp64.py) bit for bit, that
restatement's successive merges against NumPy on the concatenated data, and the exported / bound symbols (ABI still 13)."""
import copy
import os
import re

import numpy as np
import pytest
import torch

import obs_norm_fp64 as Y

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("tg_obs_moments_workspace", "tg_obs_moments", "tg_obs_norm_merge", "tg_obs_normalize_rows", "tg_learn_compact_on",
               "tg_fused_rollout_on", "tg_fused_rollout_f32_on")


@pytest.fixture(scope="module")
def tg():
    import trajopt_grpo_amd as tg
    return tg


def _policies(tg, **kw):
    return (tg.GaussianActor_NeuralNetwork(5, 2, (16, 16), cov=[0.1, 0.4], device="cpu", **kw),
            tg.GaussianActorCritic_NeuralNetwork(5, 2, (16, 16), cov=[0.1, 0.4], device="cpu", **kw))


def _stats(seed=0, S=5):
    rng = np.random.default_rng(seed)
    return rng.normal(size=S) * np.logspace(-2, 2, S), np.logspace(-3, 3, S) * rng.uniform(0.5, 2.0, size=S), 1234.0


def test_keywords_are_validated_and_default_off(tg):
    for pol in _policies(tg):
        assert pol.obs_norm is None and "normalize_obs" not in pol.metadata() and "obs_clip" not in pol.metadata()
        assert not any(k.startswith("obs_norm") for k in pol.state_dict())
    for cls in (tg.GaussianActor_NeuralNetwork, tg.GaussianActorCritic_NeuralNetwork):
        for bad in (1, "yes", None, 0.0):
            with pytest.raises(ValueError, match="normalize_obs"):
                cls(5, 2, (8,), device="cpu", normalize_obs=bad)
        for bad in (0, -1.0, float("inf"), float("nan"), "10", True):
            with pytest.raises(ValueError, match="obs_clip"):
                cls(5, 2, (8,), device="cpu", normalize_obs=True, obs_clip=bad)
        for bad in (-1e-8, float("nan"), float("inf"), "1e-8", None, True):
            with pytest.raises(ValueError, match="obs_eps"):
                cls(5, 2, (8,), device="cpu", normalize_obs=True, obs_eps=bad)
        with pytest.raises(TypeError):
            cls(5, 2, (8,), "ReLU", 0.1, "cpu", False, True)                # keyword-only


def test_obs_norm_object_and_its_table(tg):
    for pol in _policies(tg, normalize_obs=True, obs_clip=None):
        on = pol.obs_norm
        assert on.count.dtype == on.mean.dtype == on.m2.dtype == torch.float64
        assert on.count.shape == (1,) and on.mean.shape == (5,) and on.m2.shape == (5,)
        assert on.table.dtype == torch.float32 and on.table.shape == (2, 5) and on.table.is_contiguous()
        assert torch.equal(on.table, torch.stack([torch.zeros(5), torch.ones(5)]))        # count == 0: mean 0, rstd 1
        assert on.frozen is False and on.freeze() is on and on.frozen is True and on.unfreeze().frozen is False
        assert on.clip is None and on.clip_value == float("inf")
        ptr = on.table.data_ptr()
        mean, var, count = _stats()
        on.set(mean, var, count)
        assert on.table.data_ptr() == ptr                                              # rewritten in place
        assert float(on.count) == count and np.array_equal(on.mean.numpy(), mean) and np.array_equal(on.m2.numpy(), var * count)
        assert np.array_equal(on.table.numpy(), Y.table(count, mean, var * count, 1e-8))
        assert np.allclose(on.var.numpy(), var, rtol=1e-15)
        on.set(mean, var, 0)
        assert torch.equal(on.table, torch.stack([torch.zeros(5), torch.ones(5)]))
        for bad in ((mean[:4], var, 1.0), (mean, -var, 1.0), (mean, var, -1.0), (mean, var, float("nan"))):
            with pytest.raises(ValueError):
                on.set(*bad)
        # a copy of the policy owns a copy of the statistics (the learners share the object with their old_policy themselves)
        twin = copy.deepcopy(pol)
        assert twin.obs_norm is not on and torch.equal(twin.obs_norm.table, on.table) and twin.actor is not pol.actor
        with pytest.raises(AttributeError):
            on.clip = 3.0                                                                 # fixed at construction


def test_metadata_only_when_on(tg):
    for pol in _policies(tg, normalize_obs=True, obs_clip=5):
        md = pol.metadata()
        assert md["normalize_obs"] is True and md["obs_clip"] == 5.0
    for pol in _policies(tg, normalize_obs=True, obs_clip=None):
        assert pol.metadata()["obs_clip"] is None


def test_checkpoint_round_trip_and_the_two_refusals(tg, tmp_path):
    mean, var, count = _stats(1)
    for i, (pol, fresh, plain) in enumerate(zip(_policies(tg, normalize_obs=True), _policies(tg, normalize_obs=True), _policies(tg))):
        pol.obs_norm.set(mean, var, count)
        sd = pol.state_dict()
        for k, t in (("obs_norm.count", pol.obs_norm.count), ("obs_norm.mean", pol.obs_norm.mean), ("obs_norm.m2", pol.obs_norm.m2)):
            assert torch.equal(sd[k], t) and sd[k].dtype == torch.float64
        fresh.load_state_dict(sd)
        assert torch.equal(fresh.obs_norm.mean, pol.obs_norm.mean) and torch.equal(fresh.obs_norm.table, pol.obs_norm.table)
        d = tmp_path / f"p{i}"
        d.mkdir()
        pol.save(str(d))
        again = _policies(tg, normalize_obs=True)[i]
        tab_ptr = again.obs_norm.table.data_ptr()
        again.load(str(d))
        assert again.obs_norm.table.data_ptr() == tab_ptr
        for a, b in ((again.obs_norm.count, pol.obs_norm.count), (again.obs_norm.mean, pol.obs_norm.mean), (again.obs_norm.m2, pol.obs_norm.m2),
                     (again.obs_norm.table, pol.obs_norm.table)):
            assert torch.equal(a, b)
        for p, q in zip(again.parameters(), pol.parameters()):
            assert torch.equal(p, q)
        # statistics into a policy that reads raw observations: refused; and the reverse
        with pytest.raises(ValueError, match="normalize_obs=True"):
            plain.load(str(d))
        with pytest.raises(ValueError, match="normalize_obs=True"):
            plain.load_state_dict(sd)
        with pytest.raises(ValueError, match="obs_norm"):
            fresh.load_state_dict(plain.state_dict())


def test_host_path_reads_the_normalised_observation_bit_for_bit(tg):
    mean, var, count = _stats(2)
    rng = np.random.default_rng(3)
    x64 = mean + rng.normal(size=(257, 5)) * np.sqrt(var) * 4.0                 # far enough out for a clamp at 2.5 to bind on some
    for clip in (2.5, None):
        for pol, plain in zip(_policies(tg, normalize_obs=True, obs_clip=clip), _policies(tg)):
            pol.obs_norm.set(mean, var, count)
            plain.load_state_dict({k: v for k, v in pol.state_dict().items() if not k.startswith("obs_norm")})
            want = Y.normalize(x64, pol.obs_norm.table.numpy(), clip)
            for x in (torch.from_numpy(x64), torch.from_numpy(x64.astype(np.float32)), x64.astype(np.float32)):
                got = pol._prep_obs(x)
                assert got.dtype == torch.float32 and np.array_equal(got.numpy(), want)
            if clip is not None:
                frac = float((np.abs(want) == np.float32(clip)).mean())
                assert 0.0 < frac < 1.0
            xn = torch.from_numpy(want)
            act = torch.from_numpy(rng.normal(size=(257, 2)).astype(np.float32))
            lp, _ = pol.log_prob(torch.from_numpy(x64), act)
            lp_plain, _ = plain.log_prob(xn, act)
            assert torch.equal(lp, lp_plain)
            if pol.critic is not None:
                assert torch.equal(pol.value(torch.from_numpy(x64)), plain.value(xn))
            torch.manual_seed(7)
            a1, l1, _ = pol.forward(torch.from_numpy(x64))
            torch.manual_seed(7)
            a2, l2, _ = plain.forward(xn)
            assert np.array_equal(a1, a2) and torch.equal(l1, l2)


def test_three_successive_merges_against_numpy_on_the_concatenated_data(tg):
    rng = np.random.default_rng(4)
    S = 7
    scale, shift = np.logspace(-3, 3, S), rng.normal(size=S) * np.logspace(3, -3, S)
    batches = [shift + rng.normal(size=(n, S)) * scale * (1.0 + 0.3 * i) + 0.1 * i * scale for i, n in enumerate((311, 17, 1024))]
    count, mean, m2, tab = Y.statistics(batches, 1e-8)
    allx = np.concatenate(batches).astype(np.longdouble)
    mean_ref = allx.mean(0)
    m2_ref = ((allx - mean_ref) ** 2).sum(0)
    means_before, c, mu, q = [], 0.0, np.zeros(S), np.zeros(S)
    for x in batches:
        means_before.append(mu.copy())
        c, mu, q = Y.merge(c, mu, q, Y.moments(x, mu))
    e_mean, e_m2 = Y.merge_bounds(batches, means_before)
    assert count == float(allx.shape[0])
    assert np.all(np.abs(mean - mean_ref.astype(np.float64)) <= e_mean + Y.U * np.abs(mean))
    assert np.all(np.abs(m2 - m2_ref.astype(np.float64)) <= e_m2 + Y.U * np.abs(m2))
    # (the bounds are bounds, not slack: relative to the sums they bound -- the first batch's deviations are taken from 0, so a
    # feature whose mean dwarfs its spread has sum d^2 ~ count * mean^2 there)
    assert np.all(e_mean <= 1e-12 * (np.abs(mean) + scale)) and np.all(e_m2 <= 1e-12 * (m2 + count * mean ** 2))
    # the table: one f32 rounding (2^-24) on top of the statistics' own bounds (d rstd / rstd = -1/2 d var / (var + eps))
    var_ref = (m2_ref / allx.shape[0]).astype(np.float64)
    rstd_ref = 1.0 / np.sqrt(var_ref + 1e-8)
    assert np.all(np.abs(tab[1] - rstd_ref) <= rstd_ref * (2.0 ** -24 + 0.5 * e_m2 / (m2_ref.astype(np.float64) + count * 1e-8) + 8 * Y.U))
    assert np.all(np.abs(tab[0] - mean_ref.astype(np.float64)) <= np.abs(mean) * 2.0 ** -24 + e_mean)
    # the CPU policy object's own merge is the same arithmetic
    pol = tg.GaussianActor_NeuralNetwork(S, 2, (8,), device="cpu", normalize_obs=True)
    for x in batches:
        pol.obs_norm._merge(torch.from_numpy(Y.moments(x, pol.obs_norm.mean.numpy())))
    assert float(pol.obs_norm.count) == count and np.array_equal(pol.obs_norm.mean.numpy(), mean) and np.array_equal(pol.obs_norm.m2.numpy(), m2)
    assert np.array_equal(pol.obs_norm.table.numpy(), tab)


def test_ref_model_must_agree_on_normalize_obs(tg):
    pol, ref = _policies(tg, normalize_obs=True)[0], _policies(tg)[0]
    opt = torch.optim.Adam(pol.parameters(), lr=1e-3)
    with pytest.raises(ValueError, match="normalize_obs"):
        tg.GRPO(0.2, 0.1, 0.99, pol, opt, ref_model=ref)
    with pytest.raises(ValueError, match="normalize_obs"):
        tg.GRPO(0.2, 0.1, 0.99, ref, torch.optim.Adam(ref.parameters(), lr=1e-3), ref_model=pol)
    algo = tg.GRPO(0.2, 0.1, 0.99, pol, opt, ref_model=copy.deepcopy(pol))               # the project's idiom for a reference policy
    assert algo.old_policy.obs_norm is pol.obs_norm and algo.ref_model.obs_norm is not pol.obs_norm
    assert algo.old_policy.actor is not pol.actor
    shared = copy.deepcopy(pol)
    shared.obs_norm = pol.obs_norm
    with pytest.raises(ValueError, match="shares"):
        tg.GRPO(0.2, 0.1, 0.99, pol, opt, ref_model=shared)
    ppo_pol = _policies(tg, normalize_obs=True)[1]
    ppo = tg.PPO(0.2, ppo_pol, torch.optim.Adam(ppo_pol.parameters(), lr=1e-3), None, 1)
    assert ppo.old_policy.obs_norm is ppo_pol.obs_norm
    # old_policy <- policy copies weights only: the shared statistics are not loaded onto themselves
    with torch.no_grad():
        next(iter(pol.actor.parameters())).add_(1.0)
    algo.sync_old_policy()
    assert all(torch.equal(p, q) for p, q in zip(pol.parameters(), algo.old_policy.parameters()))
    with pytest.raises(ValueError, match="64"):
        tg.GaussianActor_NeuralNetwork(65, 2, (8,), device="cpu", normalize_obs=True)


def test_new_symbols_are_declared_exported_and_bound_and_the_abi_stays(tg):
    N = tg._native
    header = open(os.path.join(REPO, "include", "trajopt_grpo_hip.h")).read()
    declared = set(re.findall(r"\b(tg_[a-z0-9_]+)\s*\(", header))
    lib = N.load()
    for name in NEW_SYMBOLS:
        assert name in declared and name in N.SIGNATURES and hasattr(lib, name), name
    assert int(re.search(r"#define\s+TG_ABI_VERSION\s+(\d+)", header).group(1)) == 13 == N.ABI_VERSION == lib.tg_abi_version()
    import ctypes as C
    assert C.sizeof(N.CompactArgs) == 160                                       # tg_compact_args is what it was
    # refused on the host, before any launch
    assert lib.tg_obs_norm_merge(None, 5, 1e-8, None, None, None, None, None) == -1 and b"null pointer" in lib.tg_last_error()
    assert lib.tg_obs_normalize_rows(None, 0, 1, 1, 4, 5, None, 10.0, None, 8, 0, -1, None) == -1
    assert lib.tg_learn_compact_on(None, None, 10.0, None) == -1 and b"table" in lib.tg_last_error()
    assert lib.tg_fused_rollout_on(None, None, None, None, None, 128, 2, None, None, 0, 0, 1, None, 10.0, None) == -1
    assert lib.tg_fused_rollout_f32_on(None, None, None, None, None, 64, 2, 32, None, None, 0, 0, 1, 0, None, 10.0, None) == -1
    assert lib.tg_obs_moments_workspace(40 * 144, 20) == 6 * 20 * 3 * 8          # ceil(5760 / 1024) workgroups per feature


def test_train_ppo_tool_has_the_switch():
    src = open(os.path.join(REPO, "tools", "train_ppo.py")).read()
    assert "--normalize-obs" in src and "normalize_obs" in src
