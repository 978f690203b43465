"""DeviceReplayBuffer on the MI355X (run with `-m gpu`): one tg_replay_push launch per add(), one tg_replay_sample launch per batch.

The yardstick is tests/replay_ref.py, the NumPy restatement of the rule (itself held to the brute-force per-row definition by
tests/test_replay_cpu.py): every array and counter of the device object equals the restatement's BIT FOR BIT after every push, the
sampled indices equal the restatement's Philox draws exactly, and every sampled row equals the storage row its index names."""
import numpy as np
import pytest
import torch

import replay_ref as RR

pytestmark = pytest.mark.gpu

SHAPES = [(5, 1), (3, 1), (10, 2), (20, 4)]                                  # (S, A) of CartPole, Pendulum, QuadPole2D, QuadPole
RINGS = [(1, 1), (2, 2), (3, 3), (7, 3), (6, 5)]                             # (K, n_step)
SLOTS = [1, 64, 70, 130]


@pytest.fixture(scope="module")
def tg():
    import trajopt_grpo_amd as tg
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return tg


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


# ------------------------------------------------------------------------------------------------------------------------------
# helpers
# ------------------------------------------------------------------------------------------------------------------------------
def bits(x):
    x = x.detach().cpu().contiguous().numpy() if isinstance(x, torch.Tensor) else np.ascontiguousarray(x)
    return x.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[x.dtype.itemsize])


def device_arrays(buf):
    return {"obs": buf.obs, "act": buf.act, "next_obs": buf.next_obs, "rew": buf.rew, "disc": buf.disc, "nstep": buf.nstep,
            "last_obs": buf._last_obs, "cursor": buf.cursor, "filled": buf.filled, "open": buf.open}


def assert_same(buf, ref, where=""):
    want = ref.arrays() if isinstance(ref, RR.ReplayRef) else device_arrays(ref)
    for name, got in device_arrays(buf).items():
        assert np.array_equal(bits(got), bits(want[name])), f"{name} differs {where}"


def scripted_dones(n, pushes, n_step, seed):
    """(terminated, truncated) bool [pushes][n].  Slots i % 3 == 0: terminated on pushes 0 and 1 (the very first push, and two in a
    row), then truncated once every n_step + 2 pushes (n_step + 1 pushes without a done between).  Slots i % 3 == 1: truncated on
    push 0 -- the push on which slot 0 terminates --, terminated on push 1, never again.  The others: random, p = 0.3."""
    rng = np.random.default_rng(seed)
    term, trunc = np.zeros((pushes, n), bool), np.zeros((pushes, n), bool)
    for i in range(n):
        if i % 3 == 0:
            term[:2, i] = True
            trunc[2 + n_step + 1::n_step + 2, i] = True
        elif i % 3 == 1:
            trunc[0, i] = True
            term[1:2, i] = True
        else:
            done = rng.random(pushes) < 0.3
            term[:, i] = done & (rng.random(pushes) < 0.5)
            trunc[:, i] = done & ~term[:, i]
    return term, trunc


def random_inputs(rng, n, S, A):
    return (rng.standard_normal((n, A)).astype(np.float32), rng.standard_normal((n, S)).astype(np.float32),
            rng.standard_normal(n).astype(np.float32), rng.standard_normal((n, S)).astype(np.float32))


def to_dev(dev, *arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays)


def fill(buf, ref, dev, pushes, seed=0, p_done=0.25):
    """`pushes` random pushes into both (after a start), with random dones."""
    rng = np.random.default_rng(seed)
    first = rng.standard_normal((ref.n, ref.S)).astype(np.float32)
    buf.start(*to_dev(dev, first))
    ref.start(first)
    push_random(buf, ref, dev, pushes, rng, p_done)
    return rng


def push_random(buf, ref, dev, pushes, rng, p_done=0.25):
    for _ in range(pushes):
        act, obs, rew, fin = random_inputs(rng, ref.n, ref.S, ref.A)
        done = rng.random(ref.n) < p_done
        term = done & (rng.random(ref.n) < 0.5)
        trunc = done & ~term
        a, o, r, f, te, tr = to_dev(dev, act, obs, rew, fin, term, trunc)
        buf.add(a, o, r, te, tr, {"final_obs": f})
        ref.push(act, obs, rew, term, trunc, fin)


# ------------------------------------------------------------------------------------------------------------------------------
# 1. push, bit for bit
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K, n_step", RINGS)
@pytest.mark.parametrize("S, A", SHAPES)
def test_push_equals_the_restatement_after_every_push(tg, dev, S, A, K, n_step):
    pushes = 3 * K + 2                                                       # the ring wraps more than twice
    for n in SLOTS:
        rng = np.random.default_rng(1000 * S + 100 * K + n)
        term, trunc = scripted_dones(n, pushes, n_step, seed=n + K)
        if n >= 3:
            assert term[0, 0] and term[1, 0] and trunc[0, 1] and term[1, 1]  # first push; consecutive; both kinds in one push
            assert not (term | trunc)[2:2 + n_step + 1, 0].any()             # no done for longer than n_step
        buf = tg.DeviceReplayBuffer(S, A, n, K, n_step=n_step, gamma=0.97, device=dev)
        ref = RR.ReplayRef(S, A, n, K, n_step=n_step, gamma=0.97)
        assert np.array_equal(buf.discount, ref.g) and len(buf) == 0 and buf.capacity == K * n
        first = rng.standard_normal((n, S)).astype(np.float32)
        buf.start(*to_dev(dev, first))
        ref.start(first)
        assert_same(buf, ref, "after start")
        for t in range(pushes):
            act, obs, rew, fin = random_inputs(rng, n, S, A)
            a, o, r, f, te, tr = to_dev(dev, act, obs, rew, fin, term[t], trunc[t])
            buf.add(a, o, r, te, tr, {"final_obs": f})
            ref.push(act, obs, rew, term[t], trunc[t], fin)
            assert_same(buf, ref, f"after push {t} (S={S} A={A} n={n} K={K} n_step={n_step})")
            assert len(buf) == ref.rows == min(t + 1, K) * n
        assert (buf.n_step, buf.gamma, buf.capacity_steps) == (n_step, 0.97, K)


@pytest.mark.parametrize("S, A", SHAPES)
def test_push_takes_non_contiguous_and_offset_views(tg, dev, S, A):
    n, K, n_step = 70, 4, 3
    rng = np.random.default_rng(S)
    buf = tg.DeviceReplayBuffer(S, A, n, K, n_step=n_step, gamma=0.9, device=dev)
    ref = RR.ReplayRef(S, A, n, K, n_step=n_step, gamma=0.9)
    first = rng.standard_normal((n + 1, S)).astype(np.float32)
    buf.start(to_dev(dev, first)[0][1:])                                     # an offset view: starts S floats into its parent
    ref.start(first[1:])
    for t in range(2 * K + 1):
        act = rng.standard_normal((n, 2 * A)).astype(np.float32)
        obs = rng.standard_normal((n + 1, S)).astype(np.float32)
        fin = rng.standard_normal((S, n)).astype(np.float32)
        rew = rng.standard_normal((n, 2)).astype(np.float32)
        flags = rng.random((n, 2)) < 0.2
        flags[:, 1] &= ~flags[:, 0]
        a, o, f, r, fl = to_dev(dev, act, obs, fin, rew, flags)
        views = (a[:, ::2], o[1:], r[:, 1], fl[:, 0], fl[:, 1], f.t())
        assert not views[0].is_contiguous() and views[1].data_ptr() != o.data_ptr() and not views[5].is_contiguous()
        buf.add(*views[:5], {"final_obs": views[5]})
        ref.push(act[:, ::2], obs[1:], rew[:, 1], flags[:, 0], flags[:, 1], fin.T)
        assert_same(buf, ref, f"after push {t}")


def test_the_class_refuses_bad_arguments_before_any_launch(tg, dev):
    n, S, A = 6, 5, 1
    buf = tg.DeviceReplayBuffer(S, A, n, 4, n_step=2, device=dev)
    good = dict(actions=torch.zeros(n, A, device=dev), obs=torch.zeros(n, S, device=dev), reward=torch.zeros(n, device=dev),
                terminated=torch.zeros(n, dtype=torch.bool, device=dev), truncated=torch.zeros(n, dtype=torch.bool, device=dev),
                info={"final_obs": torch.zeros(n, S, device=dev)})
    with pytest.raises(RuntimeError, match="before start"):
        buf.add(**good)
    with pytest.raises(RuntimeError, match="empty buffer"):
        buf.sample(4)
    buf.start(good["obs"])
    for key, bad in (("actions", torch.zeros(n, A + 1, device=dev)), ("actions", torch.zeros(n, A, dtype=torch.float64, device=dev)),
                     ("obs", torch.zeros(n + 1, S, device=dev)), ("obs", torch.zeros(n, S)), ("reward", torch.zeros(n, 1, device=dev)),
                     ("terminated", torch.zeros(n, dtype=torch.int32, device=dev)), ("truncated", torch.zeros(n, device=dev)),
                     ("info", {}), ("info", {"final_obs": torch.zeros(n, S - 1, device=dev)}), ("info", {"final_obs": torch.zeros(n, S)}),
                     ("actions", np.zeros((n, A), np.float32))):
        with pytest.raises(ValueError, match="DeviceReplayBuffer"):
            buf.add(**{**good, key: bad})
    with pytest.raises(ValueError, match="obs must be"):
        buf.start(torch.zeros(n, S + 1, device=dev))
    assert len(buf) == 0 and int(buf.filled.sum()) == 0                      # nothing was launched
    buf.add(**good)
    for kw in (dict(batch=0), dict(batch=None), dict(indices=torch.zeros(3, dtype=torch.int32, device=dev)),
               dict(indices=torch.zeros(3, dtype=torch.int64)), dict(batch=2, indices=torch.zeros(3, dtype=torch.int64, device=dev)),
               dict(indices=torch.zeros(0, dtype=torch.int64, device=dev))):
        with pytest.raises(ValueError, match="DeviceReplayBuffer"):
            buf.sample(**kw)
    buf.clear()
    assert len(buf) == 0 and int(buf._slots.abs().sum()) == 0
    with pytest.raises(RuntimeError, match="empty buffer"):
        buf.sample(4)


# ------------------------------------------------------------------------------------------------------------------------------
# 2. sample
# ------------------------------------------------------------------------------------------------------------------------------
def check_batch(out, ref_out, buf):
    obs, act, rew, nxt, disc, idx = out
    assert idx.dtype == torch.int64 and np.array_equal(idx.cpu().numpy(), ref_out[5]), "indices differ from the restatement's draws"
    for got, want in zip(out[:5], ref_out[:5]):
        assert np.array_equal(bits(got), bits(want))
    rows = idx.clamp(0, buf.capacity - 1)
    ok = ((idx >= 0) & (idx < len(buf))).cpu().numpy()
    for got, store in ((obs, buf.obs), (act, buf.act), (rew, buf.rew), (nxt, buf.next_obs), (disc, buf.disc)):
        assert np.array_equal(bits(got)[ok], bits(store[rows])[ok]), "a sampled row is not the storage row its index names"


@pytest.mark.parametrize("S, A", SHAPES)
def test_sample_draws_the_restatements_rows(tg, dev, S, A):
    n, K, n_step, seed = 7, 5, 2, 0xDEADBEEF12345
    buf = tg.DeviceReplayBuffer(S, A, n, K, n_step=n_step, seed=seed, device=dev)
    ref = RR.ReplayRef(S, A, n, K, n_step=n_step, seed=seed)
    rng = fill(buf, ref, dev, 3)                                             # partly filled: filled = 3 < K, R = 21
    assert len(buf) == ref.rows == 21
    for stage in ("partly filled", "full"):
        for B in (1, 63, 64, 257):
            out = buf.sample(B)
            assert [tuple(t.shape) for t in out] == [(B, S), (B, A), (B,), (B, S), (B,), (B,)]
            check_batch(out, ref.sample(B), buf)
        first = [t.clone() for t in buf.sample(64)]
        second = buf.sample(64)
        ref.sample(64), ref.sample(64)
        assert not torch.equal(first[5], second[5]), "two successive calls drew the same rows"
        assert int(second[5].min()) >= 0 and int(second[5].max()) < len(buf)
        push_random(buf, ref, dev, 4, rng)                                   # -> 7 pushes: the ring is full and has wrapped
    assert len(buf) == K * n
    # a rebuilt object with the same seed repeats the draws
    twin = tg.DeviceReplayBuffer(S, A, n, K, n_step=n_step, seed=seed, device=dev)
    twin.load_state_dict({**buf.state_dict(), "ordinal": 0})
    again = RR.ReplayRef(S, A, n, K, n_step=n_step, seed=seed)
    again.filled[:] = K
    assert np.array_equal(twin.sample(63)[5].cpu().numpy(), again.sample_indices(63))
    other = tg.DeviceReplayBuffer(S, A, n, K, n_step=n_step, seed=seed + 1, device=dev)
    other.load_state_dict({**buf.state_dict(), "ordinal": 0, "seed": seed + 1})
    assert not np.array_equal(other.sample(63)[5].cpu().numpy(), again.sample_indices(63))


@pytest.mark.parametrize("S, A", SHAPES)
def test_sample_with_indices_gathers_them_and_out_of_range_rows_are_nan(tg, dev, S, A):
    n, K = 7, 5
    buf = tg.DeviceReplayBuffer(S, A, n, K, n_step=2, device=dev)
    ref = RR.ReplayRef(S, A, n, K, n_step=2)
    fill(buf, ref, dev, 3)
    R = len(buf)
    assert R == 21 < buf.capacity
    for idx in ([0, R - 1, -1, R, 3], [R], [5], list(range(R)) + [-1, R, buf.capacity, 2 ** 40, -2 ** 40] + list(range(R - 1, -1, -1))):
        want = ref.sample(indices=idx)
        out = buf.sample(indices=torch.tensor(idx, dtype=torch.int64, device=dev))
        check_batch(out, want, buf)
        bad = np.array([not 0 <= v < R for v in idx])
        for t in out[:5]:
            t = t.cpu().numpy().reshape(len(idx), -1)
            assert np.isnan(t[bad]).all() and not np.isnan(t[~bad]).any()    # NaN rows, and their neighbours intact


# ------------------------------------------------------------------------------------------------------------------------------
# 3. with the real env
# ------------------------------------------------------------------------------------------------------------------------------
def env_cases(tg):
    tight = tg.QuadPole2D(max_steps=12)                                      # a box the full-thrust slots leave within the episode:
    tight.spatial_bounds = ((-0.05, 0.05), (-0.05, 0.05))                    # terminations, which the two cases above may never see
    return {"CartPole": (tg.CartPole(max_steps=8), 70, False), "QuadPole2D": (tg.QuadPole2D(max_steps=6), 64, False),
            "QuadPole2D-tight": (tight, 64, True)}


@pytest.mark.parametrize("case", ["CartPole", "QuadPole2D", "QuadPole2D-tight"])
def test_with_the_vector_env(tg, dev, case):
    env, n, must_terminate = env_cases(tg)[case]
    n_step, K, steps = 3, 8, 30
    venv = tg.DeviceVecEnv(env, n, seed=11, device=dev)
    buf = tg.DeviceReplayBuffer.for_env(venv, K, n_step=n_step, gamma=0.95)
    S, A = venv.S, venv.A
    ref = RR.ReplayRef(S, A, n, K, n_step=n_step, gamma=0.95)
    g = ref.g
    obs0, _ = venv.reset()
    buf.start(obs0)
    ref.start(obs0.cpu().numpy())
    gen = torch.Generator().manual_seed(5)
    closed = {}                                                              # row -> ("term" | "trunc", final_obs row, reset obs row)
    n_term = n_trunc = 0
    for t in range(steps):
        actions = (torch.rand(n, A, generator=gen) * 2 - 1) * (0.1 if must_terminate else 1.0)
        actions[0::2] = 1.0 - 0.05 * torch.rand(n // 2 + n % 2, A, generator=gen)          # even slots: (nearly) full thrust / push
        actions = actions.to(dev)
        obs, rew, term, trunc, info = venv.step(actions)
        buf.add(actions, obs, rew, term, trunc, info)                        # the env's own buffers, no clone
        h = [x.cpu().numpy().copy() for x in (actions, obs, rew, term, trunc, info["final_obs"])]
        c, opened = int(ref.cursor[0]), ref.open.copy()
        ref.push(*h)
        assert_same(buf, ref, f"after step {t}")
        for i in range(n):
            touched = [((c - j) % K) * n + i for j in range(opened[i] + 1)]
            closed.pop(touched[0], None)                                     # the new row took this place in the ring
            if h[3][i] or h[4][i]:
                for row in touched:
                    closed[row] = ("term" if h[3][i] else "trunc", h[5][i].copy(), h[1][i].copy())
        n_term, n_trunc = n_term + int(h[3].sum()), n_trunc + int(h[4].sum())
        assert not (h[3] & h[4]).any()
        # the properties, read from the device object
        disc, nstep, nxt = buf.disc.cpu().numpy(), buf.nstep.cpu().numpy(), buf.next_obs.cpu().numpy()
        assert (nstep[:len(buf)] >= 1).all() and (nstep[:len(buf)] <= n_step).all()
        for row, (kind, final, fresh) in closed.items():
            if kind == "term":
                assert disc[row] == 0.0
            else:
                assert disc[row] == g[nstep[row]] and disc[row] > 0
            assert np.array_equal(nxt[row], final) and not np.array_equal(nxt[row], fresh), "next_obs is not that step's final_obs"
    assert n_trunc > 0 and len(closed) > 0
    if must_terminate:
        assert n_term > 0, "the tight box produced no termination"


# ------------------------------------------------------------------------------------------------------------------------------
# 4. graph capture
# ------------------------------------------------------------------------------------------------------------------------------
def test_step_and_add_replay_from_a_captured_graph(tg, dev):
    n, K, n_step, replays = 70, 4, 3, 10
    made = []
    for _ in range(2):
        venv = tg.DeviceVecEnv(tg.CartPole(max_steps=8), n, seed=3, device=dev)
        buf = tg.DeviceReplayBuffer.for_env(venv, K, n_step=n_step, gamma=0.9)
        obs0, _ = venv.reset()
        buf.start(obs0)
        made.append((venv, buf))
    (venv_g, buf_g), (venv_e, buf_e) = made
    gen = torch.Generator().manual_seed(9)
    feed = (torch.rand(replays + 1, n, venv_g.A, generator=gen) * 2 - 1).to(dev)
    actions = feed[0].clone()
    for venv, buf in made:                                                   # one eager step each: nothing is first-called under capture
        buf.add(actions, *venv.step(actions))
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):                             # one stream, a linear chain: step, then push
        buf_g.add(actions, *venv_g.step(actions))
    for k in range(replays):
        actions.copy_(feed[k + 1])                                           # refilled in place
        graph.replay()
        buf_e.add(feed[k + 1], *venv_e.step(feed[k + 1]))
    torch.cuda.synchronize()
    assert_same(buf_g, buf_e, "graph against eager")
    assert int(buf_g.filled[0]) == K and int(buf_g.cursor[0]) == (replays + 1) % K


# ------------------------------------------------------------------------------------------------------------------------------
# 5. checkpoint round trip
# ------------------------------------------------------------------------------------------------------------------------------
def test_checkpoint_round_trip_continues_bit_for_bit(tg, dev):
    S, A, n, K, n_step = 10, 2, 70, 4, 3
    buf = tg.DeviceReplayBuffer(S, A, n, K, n_step=n_step, gamma=0.93, seed=77, device=dev)
    ref = RR.ReplayRef(S, A, n, K, n_step=n_step, gamma=0.93, seed=77)
    rng = fill(buf, ref, dev, 6)
    for _ in range(2):
        check_batch(buf.sample(33), ref.sample(33), buf)
    sd = buf.state_dict()
    assert sd["ordinal"] == 2 and sd["pushes"] == 6 and sd["seed"] == 77 and sd["obs"].data_ptr() != buf.obs.data_ptr()
    twin = tg.DeviceReplayBuffer(S, A, n, K, n_step=n_step, gamma=0.93, seed=1, device=dev)
    twin.load_state_dict(sd)
    assert_same(twin, buf, "after load")
    assert len(twin) == len(buf) == K * n and twin.seed == 77
    for _ in range(5):                                                       # the same further pushes into each
        act, obs, rew, fin = random_inputs(rng, n, S, A)
        done = rng.random(n) < 0.25
        term = done & (rng.random(n) < 0.5)
        a, o, r, f, te, tr = to_dev(dev, act, obs, rew, fin, term, done & ~term)
        for b in (buf, twin):
            b.add(a, o, r, te, tr, {"final_obs": f})
        ref.push(act, obs, rew, term, done & ~term, fin)
    assert_same(twin, buf, "after the further pushes")
    assert_same(buf, ref, "against the restatement")
    for B in (64, 5):
        first, second = [t.clone() for t in buf.sample(B)], twin.sample(B)
        for x, y in zip(first, second):
            assert np.array_equal(bits(x), bits(y))
        check_batch(second, ref.sample(B), twin)
    with pytest.raises(ValueError, match="n_step"):
        tg.DeviceReplayBuffer(S, A, n, K, n_step=2, gamma=0.93, device=dev).load_state_dict(sd)
    with pytest.raises(ValueError, match="outside the ring"):
        twin.load_state_dict({**sd, "slots": torch.full_like(sd["slots"], K + 1)})


# ------------------------------------------------------------------------------------------------------------------------------
# 6. 64-bit offsets
# ------------------------------------------------------------------------------------------------------------------------------
# integer-valued inputs in closed form of (push p, env i, feature k): the same expressions serve torch (device) and NumPy (expected)
def f_obs(p, i, k): return (p * 7 + i * 3 + k) % 1021
def f_fin(p, i, k): return 2000 + (p * 11 + i * 5 + k * 3) % 997
def f_act(p, i, k): return (p * 5 + i + k * 2) % 509
def f_rew(p, i): return (p * 3 + i) % 13
def f_term(p, i): return (i + p) % 11 == 0
def f_trunc(p, i): return ((i + p) % 7 == 3) & ~f_term(p, i)


def test_offsets_past_two_to_the_31_bytes(tg, dev):
    S, A, n, K, n_step, pushes = 20, 4, 2 ** 20, 28, 2, 30
    assert K * n * S * 4 > 2 ** 31
    buf = tg.DeviceReplayBuffer(S, A, n, K, n_step=n_step, gamma=0.5, device=dev)
    g = buf.discount
    i_d = torch.arange(n, device=dev)
    kS, kA = torch.arange(S, device=dev)[None, :], torch.arange(A, device=dev)[None, :]
    buf.start(f_obs(-1, i_d[:, None], kS).float())
    for p in range(pushes):
        buf.add(f_act(p, i_d[:, None], kA).float(), f_obs(p, i_d[:, None], kS).float(), f_rew(p, i_d).float(), f_term(p, i_d),
                f_trunc(p, i_d), {"final_obs": f_fin(p, i_d[:, None], kS).float()})
    edge = 2 ** 31 // (S * 4)                                                # the row that holds byte 2^31 of obs and of next_obs
    rows = np.concatenate([np.arange(512), np.arange(edge - 512, edge + 512), np.arange(K * n - 512, K * n)])
    slot, i = rows // n, rows % n
    p = np.where(slot + K < pushes, slot + K, slot)                          # the push whose row the time slot holds now
    kS_h, kA_h = np.arange(S)[None, :], np.arange(A)[None, :]
    two = ~(f_term(p, i) | f_trunc(p, i)) & (p + 1 < pushes)                 # the row was extended by the next push
    q = np.where(two, p + 1, p)                                              # the push that closed (or last extended) the row
    done_q = f_term(q, i) | f_trunc(q, i)
    pc, qc, ic = p[:, None], q[:, None], i[:, None]                         # (columns, to broadcast against the feature index)
    want = {"obs": f_obs(pc - 1, ic, kS_h).astype(np.float32), "act": f_act(pc, ic, kA_h).astype(np.float32),
            "next_obs": np.where(done_q[:, None], f_fin(qc, ic, kS_h), f_obs(qc, ic, kS_h)).astype(np.float32),
            "rew": np.where(two, (f_rew(p, i).astype(np.float32) + g[1] * f_rew(p + 1, i).astype(np.float32)).astype(np.float32),
                            f_rew(p, i).astype(np.float32)),
            "disc": np.where(f_term(q, i), np.float32(0), np.where(two, g[2], g[1])).astype(np.float32),
            "nstep": np.where(two, 2, 1).astype(np.uint8)}
    rows_d = torch.from_numpy(rows).to(dev)
    for name, expected in want.items():
        assert np.array_equal(getattr(buf, name)[rows_d].cpu().numpy(), expected), name
    out = buf.sample(indices=rows_d)
    for got, name in zip(out[:5], ("obs", "act", "rew", "next_obs", "disc")):
        assert np.array_equal(got.cpu().numpy(), want[name]), f"sampled {name}"
    assert np.array_equal(out[5].cpu().numpy(), rows)
    assert int(buf.cursor[0]) == pushes % K and int(buf.cursor[-1]) == pushes % K and int(buf.filled[n // 2]) == K
    assert np.array_equal(buf._last_obs[-3:].cpu().numpy(), f_obs(pushes - 1, np.arange(n - 3, n)[:, None], kS_h).astype(np.float32))
