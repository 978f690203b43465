"""The restatement of the project's random draws (tests/philox_fp64.py) against published Philox vectors and against the
distributions it must produce.  No GPU: the kernels are held to this restatement by test_rng_fp64_gpu.py.

The p-value thresholds are deterministic: every input below comes from fixed seeds."""
import math

import numpy as np
import pytest

import philox_fp64 as P

MASK = P.MASK

# Random123's known-answer vectors for Philox4x32-10 (kat_vectors of the Random123 distribution)
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((MASK,) * 4, (MASK, MASK), (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


@pytest.mark.parametrize("ctr,key,want", KAT, ids=["zeros", "ones", "pi"])
def test_philox_matches_the_published_known_answers(ctr, key, want):
    assert P.philox4x32_10(ctr, key) == list(want)
    got = P.philox4x32_10_np(*(np.array([c]) for c in ctr), np.array([key[0]]), np.array([key[1]]))
    assert [int(w[0]) for w in got] == list(want)


def test_draw_lays_out_counter_and_key_as_the_kernels_do():
    """Philox::draw: counter (idx lo, idx hi, sub, stream), key (seed lo, seed hi)."""
    seed, idx, sub, stream = 0x0123456789ABCDEF, 0xFEDCBA9876543210, 17, 5
    want = P.philox4x32_10((0x76543210, 0xFEDCBA98, 17, 5), (0x89ABCDEF, 0x01234567))
    assert P.draw(seed, idx, sub, stream) == want
    # every field of the counter and key reaches the output
    for other in [(seed ^ 1, idx, sub, stream), (seed ^ (1 << 40), idx, sub, stream), (seed, idx ^ 1, sub, stream),
                  (seed, idx ^ (1 << 33), sub, stream), (seed, idx, sub + 1, stream), (seed, idx, sub, stream + 1)]:
        assert P.draw(*other) != want


def test_scalar_and_vectorised_forms_agree():
    rng = np.random.default_rng(1)
    n = 2000
    seeds = [int(x) for x in rng.integers(0, 2 ** 63, n, dtype=np.uint64)]
    seeds[:4] = [0, 5, 2 ** 40 + 3, 2 ** 64 - 1]
    idx = [int(x) for x in rng.integers(0, 2 ** 63, n, dtype=np.uint64)]
    idx[:4] = [0, 2 ** 32 + 7, 2 ** 32 - 1, 2 ** 64 - 1]
    sub = [int(x) for x in rng.integers(0, 2 ** 32, n, dtype=np.uint64)]
    sub[:2] = [0, P.SUB_RESET]
    stream = [int(x) for x in rng.integers(0, 2 ** 32, n, dtype=np.uint64)]
    got = P.draw_np(np.array(seeds, dtype=np.uint64), np.array(idx, dtype=np.uint64), np.array(sub, dtype=np.uint64),
                    np.array(stream, dtype=np.uint64))
    for j in range(n):
        assert [int(w[j]) for w in got] == P.draw(seeds[j], idx[j], sub[j], stream[j]), j


def test_uniforms_are_the_kernels_conversions():
    w = np.array([0, 0xFF, 0x100, 0xFFFFFFFF], dtype=np.uint64)
    assert P.u01(w).tolist() == [2.0 ** -24, 2.0 ** -24, 2.0 ** -23, 1.0]                # (0, 1]: log() stays finite
    assert P.u01d(np.uint64(0), np.uint64(0x7FF)) == 0.0
    assert P.u01d(np.uint64(0), np.uint64(0x800)) == 2.0 ** -53
    assert P.u01d(np.uint64(MASK), np.uint64(MASK)) == 1.0 - 2.0 ** -53                  # [0, 1)


def test_box_muller_pairs_cos_with_the_even_component():
    """eps[2h] = r cos(2 pi v), eps[2h+1] = r sin(2 pi v), with r from word 2h and v from word 2h+1."""
    words = [np.uint64(0x80000000), np.uint64(0x20000000), np.uint64(0xFFFFFFFF), np.uint64(0x3FFFFFFF)]
    eps, _ = P.box_muller(words, 4)
    r = math.sqrt(-2.0 * math.log(float(P.u01(words[0]))))
    v = float(P.u01(words[1]))                                                              # 1/8 + 2^-24 of a turn
    assert eps[0] == pytest.approx(r * math.cos(2 * math.pi * v), abs=1e-15)
    assert eps[1] == pytest.approx(r * math.sin(2 * math.pi * v), abs=1e-15)
    assert eps[2] == 0.0 and eps[3] == 0.0                                                  # u01 = 1: radius 0


def _eps(seed, stream, n_env, T, A=4):
    eps, *_ = P.sample_eps(seed, stream, np.arange(n_env), T, A)
    return eps                                                                               # [A][T][n]


def test_box_muller_output_is_standard_normal():
    """KS of 2^20 outputs (all four components of 2^18 draws) against N(0, 1), and their moments."""
    eps = _eps(seed=11, stream=0, n_env=1 << 16, T=4)
    x = eps.reshape(-1)
    assert x.size == 1 << 20
    D, p = P.ks_pvalue(x, P.normal_cdf)
    assert p > 1e-3, (D, p)
    assert abs(x.mean()) < 5e-3 and abs(x.std() - 1.0) < 5e-3
    # the 24-bit u01 truncates the tails at sqrt(-2 ln 2^-24) ~ 5.77 (intrinsic, not a defect)
    assert np.abs(x).max() <= math.sqrt(48.0 * math.log(2.0))


def test_components_and_successive_steps_are_uncorrelated():
    """The four components of one draw, (env, t) against (env, t + 1), and stream k against stream k + 1."""
    n = 1 << 17
    eps = _eps(seed=3, stream=2, n_env=n, T=2)
    lim = 6.0 / math.sqrt(n)
    c = np.corrcoef(eps[:, 0, :])
    assert np.abs(c - np.eye(4)).max() < lim, c
    for k in range(4):
        assert abs(np.corrcoef(eps[k, 0], eps[k, 1])[0, 1]) < lim
    # a radius shared by a pair shows in the squares, not in the components
    assert abs(np.corrcoef(eps[0, 0] ** 2, eps[1, 0] ** 2)[0, 1]) < lim
    assert abs(np.corrcoef(eps[2, 0] ** 2, eps[3, 0] ** 2)[0, 1]) < lim
    nxt = _eps(seed=3, stream=3, n_env=n, T=1)
    for k in range(4):
        assert abs(np.corrcoef(eps[k, 0], nxt[k, 0])[0, 1]) < lim


RANGES = {"CartPole": {"theta": (-math.pi, math.pi)}, "QuadPole2D": {"theta": (-math.pi, math.pi)},
          "PendulumSwingup": {"theta": (-math.pi, math.pi)}, "Pendulum": {"theta": (math.pi - 0.05, math.pi + 0.05)},
          "QuadPole": {"alpha": (-1.0, 1.0), "beta": (-1.0, 1.0)}}


@pytest.mark.parametrize("name", list(RANGES))
def test_reset_angles_follow_the_reference_ranges(name):
    """KS of every sampled reset angle against the reference's uniform range (cartpole_env.py:103, quadrotor_env.py:543-544
    and :951, pendulum_env.py:89-91); QuadPole's alpha and beta come from different words."""
    n = 1 << 18
    _, ang = P.reset_states(name, 9, 4, n)
    for k, (lo, hi) in RANGES[name].items():
        a = ang[k]
        assert a.min() >= lo and a.max() < hi
        D, p = P.ks_pvalue(a, P.uniform_cdf(lo, hi))
        assert p > 1e-3, (k, D, p)
    if name == "QuadPole":
        assert abs(np.corrcoef(ang["alpha"], ang["beta"])[0, 1]) < 6.0 / math.sqrt(n)


@pytest.mark.parametrize("name", list(RANGES))
def test_reset_states_are_the_reference_maps_of_the_angles(name):
    o, ang = P.reset_states(name, 2 ** 40 + 3, 1, 4096, key_offset=2 ** 32 + 5, key_div=3)
    if name == "QuadPole":
        a, b = ang["alpha"], ang["beta"]
        q = o[13:17]
        assert np.allclose((q * q).sum(0), 1.0, atol=1e-15, rtol=0)
        assert np.allclose(2 * np.arctan2(q[1], q[0]), a, atol=1e-14) and np.allclose(2 * np.arctan2(q[2], q[0]), b, atol=1e-14)
        assert np.array_equal(o[6], np.ones(4096)) and not np.delete(o, [6, 13, 14, 15, 16], axis=0).any()
    else:
        th = ang["theta"]
        s, c = {"CartPole": (2, 3), "QuadPole2D": (7, 8)}.get(name, (0, 1))
        assert np.array_equal(o[s], np.sin(th)) and np.array_equal(o[c], np.cos(th))
    # key_div = 3: three consecutive keys share one draw
    assert np.array_equal(o[:, 0::3][:, :1365], o[:, 1::3][:, :1365]) and np.array_equal(o[:, 1::3][:, :1365], o[:, 2::3][:, :1365])
    assert not np.array_equal(o[:, 0], o[:, 3])
