"""DeviceRolloutStorage on the MI355X (run with `-m gpu`): one launch per add(), compute_returns(), shuffle() and minibatch().

The yardsticks are tests/segment_ref.py -- the NumPy restatement, BIT FOR BIT, and the fp64 per-row definition of GAE within the
bound derived there -- and, with the real vector env, the torch composition of tools/vec_env_ppo.py on the same tensors, bit for bit."""
import numpy as np
import pytest
import torch

import segment_ref as SR
from test_segment_cpu import ROWS, restated, segment_case

pytestmark = pytest.mark.gpu

P, GAMMA, LAM, DEV = 8, 0.97, 0.9, torch.device("cuda", 0)                   # P: TG_SEGMENT_GAE_PREFETCH
SLOTS = [1, 64, 70, 130]                                                     # workgroups of 64 slots: short of one, one, past one, past two


@pytest.fixture(scope="module")
def tg():
    import trajopt_grpo_amd as tg
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return tg


def same(a, b):
    """Equal bit for bit (tensors or arrays)."""
    a, b = (x.detach().cpu().contiguous().numpy() if isinstance(x, torch.Tensor) else np.ascontiguousarray(x) for x in (a, b))
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def to_dev(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays)


def new_storage(tg, rng, S, A, n, L, **kw):
    st = tg.DeviceRolloutStorage(S, A, n, L, gamma=GAMMA, lam=LAM, device=DEV, **kw)
    st.start(*to_dev(rng.standard_normal((n, S)).astype(np.float32)))
    return st


def feed(st, case, rng):
    """One segment of `case` into `st`, then its returns; -> what the storage must hold, by attribute name."""
    reward, term, trunc, fv, val, last = case
    (L, n), S, A = reward.shape, st.obs_dim, st.act_dim
    obs = np.concatenate([st.obs[0].cpu().numpy()[None], rng.standard_normal((L, n, S)).astype(np.float32)])
    act, logp = rng.standard_normal((L, n, A)).astype(np.float32), rng.standard_normal((L, n)).astype(np.float32)
    for t in range(L):
        st.add(*to_dev(act[t], logp[t], val[t], obs[t + 1], reward[t], term[t], trunc[t], fv[t]))
    st.compute_returns(*to_dev(last))
    rew, flags, (adv, ret) = restated(*case, GAMMA, LAM)
    obs[0], first_obs = obs[L], obs[0].copy()                                # (the last push put the next segment's row 0 in place)
    return dict(obs=obs, first_obs=first_obs, act=act, logp=logp, val=val, rew=rew, flags=flags, adv=adv, ret=ret)


def assert_segment(st, case, want, where):
    for name, array in want.items():
        assert same(getattr(st, name), array), f"{name} differs from the restatement {where}"
    want_adv, want_ret, mag, ops = SR.gae_fp64(*case, GAMMA, LAM)
    bound_adv, bound_ret = SR.gae_bound(mag, ops, case[4])
    assert (np.abs(st.adv.cpu().numpy() - want_adv) <= bound_adv).all() and (np.abs(st.ret.cpu().numpy() - want_ret) <= bound_ret).all()


@pytest.mark.parametrize("L", [1, 2, P, P + 1, 2 * P + 1])
@pytest.mark.parametrize("S, A", [(5, 1), (20, 4)])
def test_push_and_gae_equal_the_restatement_and_segments_follow_on(tg, S, A, L):
    for n in SLOTS:
        rng = np.random.default_rng(1000 * S + 10 * L + n)
        st = new_storage(tg, rng, S, A, n, L)
        first, second = segment_case(L, n, seed=n + L), segment_case(L, n, seed=n + L + 1)
        assert_segment(st, first, feed(st, first, rng), f"(S={S} A={A} n={n} L={L})")
        row0 = st.obs[0].clone()                                             # no start(): row 0 of the second segment is row L of the first
        assert_segment(st, second, feed(st, second, rng), f"in the second segment (S={S} A={A} n={n} L={L})")
        fresh = tg.DeviceRolloutStorage(S, A, n, L, gamma=GAMMA, lam=LAM, device=DEV)      # ... and equals a fresh object fed the same data
        fresh.start(row0)
        for t in range(L):
            fresh.add(st.act[t], st.logp[t], st.val[t], st.obs[t + 1], *to_dev(*(second[j][t] for j in range(4))))
        fresh.compute_returns(*to_dev(second[5]))
        assert all(same(getattr(fresh, name), getattr(st, name)) for name in ("first_obs", "obs", "rew", "flags", "adv", "ret"))


def critic(x):                                                               # any fixed function of the observation will do
    return torch.tanh(x).sum(-1) * 0.5


def one_step(venv, st, obs_t, actions, logp):
    obs, rew, term, trunc, info = venv.step(actions)
    st.add(actions, logp, critic(obs_t), obs, rew, term, trunc, critic(info["final_obs"]))


def torch_composition(venv, L, feed_a, feed_l, gamma, lam):
    """tools/vec_env_ppo.py lines 41-60 with `critic` above and the fed actions; -> the buffers, adv and ret of one segment."""
    n = venv.num_envs
    buf = {k: torch.empty(L, n, *w, device=DEV) for k, w in (("obs", (venv.S,)), ("act", (venv.A,)), ("logp", ()), ("val", ()), ("rew", ()), ("done", ()))}
    obs = venv._obs
    for t in range(L):
        buf["obs"][t].copy_(obs)
        buf["act"][t], buf["logp"][t], buf["val"][t] = feed_a[t], feed_l[t], critic(buf["obs"][t])
        obs, rew, terminated, truncated, info = venv.step(feed_a[t])
        boot = torch.where(truncated, critic(info["final_obs"]), 0.0)
        buf["rew"][t] = rew + gamma * boot
        buf["done"][t] = terminated | truncated
    buf["adv"] = torch.empty(L, n, device=DEV)
    last, nxt = torch.zeros(n, device=DEV), critic(obs)
    for t in reversed(range(L)):
        live = 1.0 - buf["done"][t]
        delta = buf["rew"][t] + gamma * nxt * live - buf["val"][t]
        last = delta + gamma * lam * live * last
        buf["adv"][t], nxt = last, buf["val"][t]
    return {**buf, "ret": buf["adv"] + buf["val"]}


@pytest.mark.parametrize("captured", [False, True])
def test_with_the_vector_env_equals_the_torch_composition(tg, captured):
    """The tool bootstraps wherever `truncated` is set, the kernel where truncated and not terminated: the two agree bit for bit on
    steps that never carry both flags, which is every step of DeviceVecEnv (here the clock ends every CartPole episode)."""
    n, L, gamma, lam = 70, 17, 0.99, 0.95
    venv, twin = (tg.DeviceVecEnv(tg.CartPole(max_steps=8), n, seed=3, device=DEV) for _ in range(2))
    st = tg.DeviceRolloutStorage.for_env(venv, L, gamma=gamma, lam=lam)
    st.start(venv.reset()[0])
    twin.reset()
    gen = torch.Generator().manual_seed(9)
    feed_a = (torch.rand(2 * L, n, venv.A, generator=gen) * 2 - 1).to(DEV)
    feed_l = torch.randn(2 * L, n, generator=gen).to(DEV)
    actions, logp, obs_t = feed_a[0].clone(), feed_l[0].clone(), st.obs[0].clone()
    one_step(venv, st, obs_t, actions, logp)                                 # step 0 eagerly: nothing is first-called under capture
    graph = torch.cuda.CUDAGraph() if captured else None
    if captured:
        stream = torch.cuda.Stream(device=DEV)
        stream.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.graph(graph, stream=stream):                         # one stream, a linear chain: critic, step, critic, push
            one_step(venv, st, obs_t, actions, logp)
    for seg in range(2):
        for t in range(1 if seg == 0 else 0, L):
            actions.copy_(feed_a[seg * L + t])                               # refilled in place
            logp.copy_(feed_l[seg * L + t])
            obs_t.copy_(st.obs[t])
            graph.replay() if captured else one_step(venv, st, obs_t, actions, logp)      # L replays per segment (L - 1 in the first)
        st.compute_returns(critic(st.obs[L]))
        want = torch_composition(twin, L, feed_a[seg * L:], feed_l[seg * L:], gamma, lam)
        got = {**{k: getattr(st, k) for k in ("act", "logp", "val", "rew", "adv", "ret")}, "done": st.done.float(),
               "obs": torch.cat([st.first_obs[None], st.obs[1:L]])}
        for name in want:
            assert same(got[name], want[name]), f"{name} differs from the torch composition in segment {seg}"
        assert same(st.obs[L], twin._obs) and same(st.obs[0], twin._obs)
        assert int((st.flags == 2).sum()) >= n and not bool((st.flags == 3).any())       # truncations in mid-column, never both flags


@pytest.mark.parametrize("rows", ROWS)
def test_shuffle_and_minibatches(tg, rows):
    L, n = {1190: (17, 70), 4097: (17, 241)}.get(rows, (1, rows))
    S, A, seed = (20, 4, 2 ** 40 + 7) if rows % 2 else (5, 1, 11)
    rng = np.random.default_rng(rows)
    st = new_storage(tg, rng, S, A, n, L, seed=seed)
    want = feed(st, segment_case(L, n, seed=rows), rng)
    first = st.shuffle().clone()
    assert first.dtype == torch.int64 and same(first, SR.permutation(rows, seed, 0)[0])
    assert same(st.shuffle(), SR.permutation(rows, seed, 1)[0]) and (rows <= 3 or not same(first, st.idx))
    idx = st.idx.cpu().numpy()
    assert np.array_equal(np.sort(idx), np.arange(rows))
    seen = np.concatenate([want["first_obs"][None], want["obs"][1:L]])      # (row 0 already holds the next segment's first observation)
    stored = [a.reshape(rows, *a.shape[2:])[idx] for a in [seen] + [want[k] for k in ("act", "logp", "adv", "ret", "val")]]
    for m in sorted({1, min(3, rows), rows}):
        B = -(-rows // m)
        parts = [[t.clone() for t in st.minibatch(k, m)] for k in range(-(-rows // B))]
        assert all(len(p[0]) == B for p in parts[:-1]) and sum(len(p[0]) for p in parts) == rows
        assert all(same(torch.cat([p[j] for p in parts]), stored[j]) for j in range(6)), f"minibatches of {m} are not the stored rows in idx order"


def test_checkpoint_round_trip_mid_segment_continues_bit_for_bit(tg):
    S, A, n, L = 10, 2, 70, 9
    rng = np.random.default_rng(5)
    st = new_storage(tg, rng, S, A, n, L, seed=77)
    case = segment_case(L, n, seed=1)
    steps = [to_dev(rng.standard_normal((n, A)).astype(np.float32), rng.standard_normal(n).astype(np.float32), case[4][t],
                    rng.standard_normal((n, S)).astype(np.float32), case[0][t], case[1][t], case[2][t], case[3][t]) for t in range(L)]
    for t in range(4):
        st.add(*steps[t])
    st.shuffle()
    twin = tg.DeviceRolloutStorage(S, A, n, L, gamma=GAMMA, lam=LAM, seed=1, device=DEV)
    twin.load_state_dict(st.state_dict())
    assert twin.seed == 77 and int(twin._step[0]) == 4
    for both in (st, twin):
        for t in range(4, L):
            both.add(*steps[t])
        both.compute_returns(*to_dev(case[5]))
        both.shuffle()
    assert all(same(getattr(twin, name), getattr(st, name)) for name in tg.DeviceRolloutStorage._TENSORS)
    assert same(st.idx, SR.permutation(L * n, 77, 1)[0])
    assert all(same(a, b) for a, b in zip([t.clone() for t in st.minibatch(1, 4)], twin.minibatch(1, 4)))
