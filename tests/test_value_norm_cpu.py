"""Running value normalisation without a GPU: keyword validation, the ValueNorm surface, checkpoints and their two refusals, metadata,
policy.value() against the NumPy restatement (tests/value_norm_fp64.py) bit for bit, that restatement's successive merges against
two-pass extended-precision statistics of the concatenated data within the bound derived there, the host merge path against the
restatement bit for bit, last_stats' derived numbers against their definitions, and the exported / bound symbols."""
import copy
import math
import os
import re

import numpy as np
import pytest
import torch

import value_norm_fp64 as Y

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("tg_scatter_rows_affine", "tg_boot_values_affine", "tg_value_norm_merge")
IDENTITY = torch.tensor([0.0, 1.0, 1.0, 0.0])


@pytest.fixture(scope="module")
def tg():
    import trajopt_grpo_amd as tg
    return tg


def _policy(tg, **kw):
    return tg.GaussianActorCritic_NeuralNetwork(5, 2, (16, 16), cov=[0.1, 0.4], device="cpu", **kw)


def test_keywords_are_validated_default_off_and_refused_by_the_actor_only_policy(tg):
    pol = _policy(tg)
    assert pol.value_norm is None and "normalize_value" not in pol.metadata() and "value_eps" not in pol.metadata()
    assert set(pol.state_dict()) == {"actor", "critic"}
    for bad in (1, "yes", None, 0.0):
        with pytest.raises(ValueError, match="normalize_value"):
            _policy(tg, normalize_value=bad)
    for bad in (-1e-8, float("nan"), float("inf"), "1e-8", None, True):
        with pytest.raises(ValueError, match="value_eps"):
            _policy(tg, normalize_value=True, value_eps=bad)
    with pytest.raises(TypeError):
        tg.GaussianActorCritic_NeuralNetwork(5, 2, (8,), "ReLU", 0.1, "cpu", False, False, 10.0, 1e-8, True)    # keyword-only
    # a policy without a critic has no value to normalise: the keyword does not exist there, on or off
    for kw in ({"normalize_value": True}, {"normalize_value": False}, {"value_eps": 1e-8}):
        with pytest.raises(TypeError, match="normalize_value|value_eps"):
            tg.GaussianActor_NeuralNetwork(5, 2, (8,), device="cpu", **kw)
    actor_only = tg.GaussianActor_NeuralNetwork(5, 2, (8,), device="cpu")
    assert actor_only.value_norm is None and "normalize_value" not in actor_only.metadata()


def test_value_norm_object_and_its_table(tg):
    pol = _policy(tg, normalize_value=True)
    vn = pol.value_norm
    assert isinstance(vn, tg.policies.ValueNorm)
    for t in (vn.count, vn.mean, vn.m2):
        assert t.dtype == torch.float64 and t.shape == (1,)
    assert vn.table.dtype == torch.float32 and vn.table.shape == (4,) and vn.table.is_contiguous()
    assert torch.equal(vn.table, IDENTITY)                                               # count == 0: the identity
    assert vn.frozen is False and vn.freeze() is vn and vn.frozen is True and vn.unfreeze().frozen is False
    assert vn.eps == 1e-8 and _policy(tg, normalize_value=True, value_eps=0.5).value_norm.eps == 0.5
    with pytest.raises(AttributeError):
        vn.eps = 1.0                                                                     # fixed at construction
    ptr = vn.table.data_ptr()
    vn.set(123.25, 817.5, 4321)
    assert vn.table.data_ptr() == ptr                                                    # rewritten in place
    assert float(vn.count) == 4321.0 and float(vn.mean) == 123.25 and float(vn.m2) == 817.5 * 4321 and float(vn.var) == 817.5
    assert np.array_equal(vn.table.numpy(), Y.table(4321.0, 123.25, 817.5 * 4321, 1e-8))
    assert vn.table[1] == np.float32(math.sqrt(817.5 + 1e-8)) and vn.table[3] == 0
    vn.set(5.0, 2.0, 0)
    assert torch.equal(vn.table, IDENTITY)
    for bad in ((1.0, -1.0, 1.0), (1.0, 1.0, -1.0), (float("nan"), 1.0, 1.0), (1.0, 1.0, float("inf"))):
        with pytest.raises(ValueError):
            vn.set(*bad)
    # state() / load_state() round trip, the table rebuilt from the statistics
    vn.set(-3.5, 0.04, 77)
    other = _policy(tg, normalize_value=True).value_norm
    tab_ptr = other.table.data_ptr()
    other.load_state(*(vn.state()[k] for k in tg.policies.VALUE_NORM_KEYS))
    assert other.table.data_ptr() == tab_ptr
    for a, b in ((other.count, vn.count), (other.mean, vn.mean), (other.m2, vn.m2), (other.table, vn.table)):
        assert torch.equal(a, b)
    with pytest.raises(ValueError):
        other.load_state(torch.zeros(2, dtype=torch.float64), vn.mean, vn.m2)
    # a copy of the policy owns a copy of the statistics; the learners share the object with their old_policy themselves
    twin = copy.deepcopy(pol)
    assert twin.value_norm is not vn and torch.equal(twin.value_norm.table, vn.table) and twin.critic is not pol.critic
    twin.value_norm.set(0.0, 1.0, 1)
    assert float(vn.mean) == -3.5
    assert vn.to("cpu") is vn and pol.to("cpu") is pol and pol.value_norm is vn


def test_metadata_only_when_on(tg):
    md = _policy(tg, normalize_value=True, value_eps=1e-5).metadata()
    assert md["normalize_value"] is True and md["value_eps"] == 1e-5
    assert {k: v for k, v in md.items() if k not in ("normalize_value", "value_eps")} == _policy(tg).metadata() | {"cov": md["cov"]}


def test_checkpoint_round_trip_and_the_two_refusals(tg, tmp_path):
    pol, fresh, plain = _policy(tg, normalize_value=True), _policy(tg, normalize_value=True), _policy(tg)
    pol.value_norm.set(97.0, 900.0, 12345)
    sd = pol.state_dict()
    assert set(sd) == {"actor", "critic", "value_norm.count", "value_norm.mean", "value_norm.m2"}
    for k, t in (("value_norm.count", pol.value_norm.count), ("value_norm.mean", pol.value_norm.mean), ("value_norm.m2", pol.value_norm.m2)):
        assert torch.equal(sd[k], t) and sd[k].dtype == torch.float64
    fresh.load_state_dict(sd)
    assert torch.equal(fresh.value_norm.m2, pol.value_norm.m2) and torch.equal(fresh.value_norm.table, pol.value_norm.table)
    pol.save(str(tmp_path))
    again = _policy(tg, normalize_value=True)
    tab_ptr = again.value_norm.table.data_ptr()
    again.load(str(tmp_path))
    assert again.value_norm.table.data_ptr() == tab_ptr
    for a, b in ((again.value_norm.count, pol.value_norm.count), (again.value_norm.mean, pol.value_norm.mean),
                 (again.value_norm.m2, pol.value_norm.m2), (again.value_norm.table, pol.value_norm.table)):
        assert torch.equal(a, b)
    for p, q in zip(again.parameters(), pol.parameters()):
        assert torch.equal(p, q)
    # statistics into a policy whose critic is not normalised: refused; and the reverse
    with pytest.raises(ValueError, match="normalize_value=True"):
        plain.load(str(tmp_path))
    with pytest.raises(ValueError, match="normalize_value=True"):
        plain.load_state_dict(sd)
    with pytest.raises(ValueError, match="value_norm"):
        fresh.load_state_dict(plain.state_dict())
    # together with the observation statistics: both sets of keys travel
    both = _policy(tg, normalize_value=True, normalize_obs=True)
    both.value_norm.set(1.5, 2.5, 10)
    both2 = _policy(tg, normalize_value=True, normalize_obs=True)
    both2.load_state_dict(both.state_dict())
    assert torch.equal(both2.value_norm.table, both.value_norm.table)


def test_policy_value_is_the_denormalised_critic_bit_for_bit(tg):
    rng = np.random.default_rng(3)
    pol, plain = _policy(tg, normalize_value=True), _policy(tg)
    plain.load_state_dict({k: v for k, v in pol.state_dict().items() if not k.startswith("value_norm")})
    x = torch.from_numpy(rng.normal(size=(257, 5)).astype(np.float32))
    assert torch.equal(pol.value(x), plain.value(x))                                     # identity statistics: v * 1 + 0 is exact
    pol.value_norm.set(97.3, 911.7, 1000)                                                # a table of no powers of two
    tab = pol.value_norm.table.numpy()
    with torch.no_grad():
        raw = plain.value(x)
        got = pol.value(x)
    assert got.dtype == torch.float32 and got.shape == raw.shape
    assert np.array_equal(got.numpy(), Y.denormalize(raw.numpy(), tab))
    assert torch.equal(got, pol.value_norm.denormalize(raw))
    fma = (raw.double() * float(tab[1]) + float(tab[0])).float()                         # one rounding: what a contracted FMA would give
    assert not torch.equal(got, fma)                                                     # (the two-rounding form is distinguishable here)
    r = torch.from_numpy((97.3 + 30.0 * rng.normal(size=513)).astype(np.float32))
    assert np.array_equal(pol.value_norm.normalize(r).numpy(), Y.normalize(r.numpy(), tab))
    _, _, v = pol.forward(x)                                                             # forward() returns the critic's raw output, as before
    assert torch.equal(v.detach().squeeze(), raw)
    assert pol.value(x).requires_grad                                                    # still differentiable in the critic


def test_three_merged_batches_against_two_pass_statistics_of_the_concatenation(tg):
    rng = np.random.default_rng(4)
    # returns of mean ~100 and std ~30: S2 ~ 12 x the squared deviations, the uncentred form's cancellation is exercised
    batches = [100.0 + 3.0 * i + (30.0 + 2.0 * i) * rng.normal(size=n) for i, n in enumerate((4177, 160, 20011))]
    count, mean, m2, tab = Y.statistics(batches, 1e-8)
    c_ref, mean_ref, m2_ref = Y.exact(batches)
    e_mean, e_m2 = Y.merge_bounds(batches)
    print("value_norm merge: err mean / bound", abs(mean - mean_ref) / e_mean, "err m2 / bound", abs(m2 - m2_ref) / e_m2)
    assert count == c_ref == float(sum(b.size for b in batches))
    assert abs(mean - mean_ref) <= e_mean + Y.U * abs(mean)
    assert abs(m2 - m2_ref) <= e_m2 + Y.U * abs(m2)
    # the bounds are bounds, not slack: a small multiple of the reordering bound N u of the sums they start from (S1 ~ count * mean,
    # S2 = m2 + count * mean^2; e2 + 2 |mb| e1 is 3 N u S2 at most)
    assert e_mean <= 2.0 * Y.gamma(int(count)) * abs(mean) and e_m2 <= 4.0 * Y.gamma(int(count)) * (m2 + count * mean ** 2)
    s1, s2 = Y.moments(batches[0])[1:]
    assert s2 > 10.0 * (s2 - s1 * s1 / batches[0].size)                                  # (the cancellation is there)
    # the table: one f32 rounding on top of the statistics' own bounds (d sigma / sigma = 1/2 d var / (var + eps))
    sigma_ref = math.sqrt(m2_ref / c_ref + 1e-8)
    rel = 2.0 ** -24 + 0.5 * e_m2 / (m2_ref + c_ref * 1e-8) + 8 * Y.U
    assert abs(float(tab[0]) - mean_ref) <= abs(mean_ref) * 2.0 ** -24 + e_mean
    assert abs(float(tab[1]) - sigma_ref) <= sigma_ref * rel and abs(float(tab[2]) - 1.0 / sigma_ref) <= rel / sigma_ref
    assert tab[3] == 0.0
    # the CPU policy object's own merge is the same arithmetic, and it hands the critic's target constants to norm8
    vn = _policy(tg, normalize_value=True).value_norm
    norm8 = torch.arange(8, dtype=torch.float32) + 0.5
    for r in batches:
        vn._merge(torch.from_numpy(Y.moments(r)), norm8)
    assert float(vn.count) == count and float(vn.mean) == mean and float(vn.m2) == m2
    assert np.array_equal(vn.table.numpy(), tab)
    assert norm8.tolist() == [0.5, 1.5, float(tab[0]), float(tab[2]), 4.5, 5.5, 6.5, 7.5]
    # nothing to merge: the statistics keep their bits, the table is rewritten from them
    kept = [t.clone() for t in (vn.count, vn.mean, vn.m2, vn.table)]
    vn._merge(None)
    vn._merge(torch.tensor([0.0, 5.0, 25.0], dtype=torch.float64))
    for a, b in zip(kept, (vn.count, vn.mean, vn.m2, vn.table)):
        assert torch.equal(a, b)
    # a single merge into empty statistics is the batch's own mean and squared deviations
    c1, mu1, q1 = Y.merge(0.0, 0.0, 0.0, Y.moments(batches[1]))
    _, mu_ref, q_ref = Y.exact(batches[1:2])
    b_mean, b_m2 = Y.merge_bounds(batches[1:2])
    assert c1 == 160.0 and abs(mu1 - mu_ref) <= b_mean and abs(q1 - q_ref) <= b_m2


def test_last_stats_numbers_follow_their_definitions(tg):
    f = tg.algorithms._value_norm_stats
    rng = np.random.default_rng(5)
    ret = 100.0 + 30.0 * rng.normal(size=1000)
    adv = 12.0 * rng.normal(size=1000) + 1.0
    mom = torch.tensor([[adv.size, adv.sum(), (adv * adv).sum()], [ret.size, ret.sum(), (ret * ret).sum()]], dtype=torch.float64)
    out = f(torch.tensor([2000.0, 99.0, 2000.0 * 850.0], dtype=torch.float64), mom, 1e-8)
    assert out["value_count"] == 2000.0 and out["value_mean"] == 99.0 and out["value_std"] == math.sqrt(850.0 + 1e-8)
    assert out["explained_variance"] == pytest.approx(1.0 - adv.var() / ret.var(), rel=1e-10)          # population variances
    out = f(torch.zeros(3, dtype=torch.float64), torch.tensor([[4.0, 2.0, 3.0], [4.0, 8.0, 16.0]], dtype=torch.float64), 1e-8)
    assert (out["value_mean"], out["value_std"], out["value_count"]) == (0.0, 1.0, 0.0)
    assert math.isnan(out["explained_variance"])                                         # var(ret) == 0


def test_learners_share_the_statistics_with_old_policy_and_ppo_metadata_is_unchanged(tg):
    pol, plain = _policy(tg, normalize_value=True), _policy(tg)
    kw = dict(gamma=0.98, lam=0.9, batch_size=None, max_grad_norm=0.5)
    ppo = tg.PPO(0.2, pol, torch.optim.Adam(pol.parameters(), lr=1e-3), None, 3, **kw)
    ppo_plain = tg.PPO(0.2, plain, torch.optim.Adam(plain.parameters(), lr=1e-3), None, 3, **kw)
    want = {"algorithm": "PPO", "epsilon": 0.2, "c1": 0.5, "kl_coeff": 0.5, "gamma": 0.98, "lam": 0.9, "entropy": 0.01,
            "batch_size": None, "updates_per_iter": 3, "max_grad_norm": 0.5}
    assert ppo_plain.metadata() == want == ppo.metadata()                                # the flag is the policy's: PPO's metadata stands
    assert ppo.old_policy.value_norm is pol.value_norm and ppo.old_policy.critic is not pol.critic
    assert ppo_plain.old_policy.value_norm is None
    # old_policy <- policy copies weights only: the shared statistics are not loaded onto themselves
    pol.value_norm.set(50.0, 4.0, 9)
    with torch.no_grad():
        next(iter(pol.critic.parameters())).add_(1.0)
    ppo.sync_old_policy()
    assert all(torch.equal(p, q) for p, q in zip(pol.parameters(), ppo.old_policy.parameters()))
    ppo._copy_policy_to_old()
    assert float(pol.value_norm.mean) == 50.0 and not any(k.startswith("value_norm") for k in ppo._weights_state(pol))
    # GRPO ignores the statistics (and still shares them with its copy, so that a checkpoint of either agrees)
    grpo = tg.GRPO(0.2, 0.0, 0.99, pol, torch.optim.Adam(pol.parameters(), lr=1e-3))
    assert grpo.old_policy.value_norm is pol.value_norm and "normalize_value" not in grpo.metadata()


def test_new_symbols_are_declared_exported_and_bound(tg):
    import ctypes as C
    N, K = tg._native, tg.hip_ops
    header = open(os.path.join(REPO, "include", "trajopt_grpo_hip.h")).read()
    declared = set(re.findall(r"\b(tg_[a-z0-9_]+)\s*\(", header))
    lib = N.load()
    for name in NEW_SYMBOLS:
        assert name in declared and name in N.SIGNATURES and hasattr(lib, name), name
    assert int(re.search(r"#define\s+TG_ABI_VERSION\s+(\d+)", header).group(1)) == N.ABI_VERSION == lib.tg_abi_version()
    # the argument counts the wrappers pass (stream included), and the pair hip_ops picks with suffixed()
    assert len(N.SIGNATURES["tg_scatter_rows"][1]) == 6 and len(N.SIGNATURES["tg_scatter_rows_affine"][1]) == 7
    assert K.suffixed("tg_scatter_rows", "_affine", None) == ("tg_scatter_rows", ())
    assert K.suffixed("tg_scatter_rows", "_affine", (0x1000,)) == ("tg_scatter_rows_affine", (0x1000,))
    assert len(N.SIGNATURES["tg_boot_values_affine"][1]) == 7 and len(N.SIGNATURES["tg_value_norm_merge"][1]) == 8
    assert N.SIGNATURES["tg_value_norm_merge"][1][1] is C.c_double
    # refused on the host, before any launch
    assert lib.tg_scatter_rows_affine(None, 1, None, 4, None, None, None) == -1 and b"table" in lib.tg_last_error()
    assert lib.tg_boot_values_affine(None, 1, None, 4, None, None, None) == -1 and b"table" in lib.tg_last_error()
    assert lib.tg_value_norm_merge(None, 1e-8, None, None, None, None, None, None) == -1 and b"null pointer" in lib.tg_last_error()
    if not torch.cuda.is_available():
        with pytest.raises(N.NativeLibraryError, match="no CPU fallback"):
            K.value_norm_merge(None, 1e-8, *(torch.zeros(1, dtype=torch.float64) for _ in range(3)), torch.zeros(4))


def test_train_ppo_tool_has_the_switch():
    src = open(os.path.join(REPO, "tools", "train_ppo.py")).read()
    assert "--normalize-value" in src and "normalize_value" in src
