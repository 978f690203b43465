"""DeviceVecEnv on the MI355X (run with `-m gpu`): n auto-resetting env slots behind one tg_vec_env_step launch per step.

The yardstick is the code that already exists, never the new kernel: episode k of slot i, as the vector env produced it, must equal
BIT FOR BIT the existing path run in isolation on that episode --
  initial state   tg_env_reset(seed, stream_id = k, key_offset = env_offset + i, key_div = 1);
  trajectory      the teacher-forced replay of the actions the slot was fed through tg_rollout_forced (`_dr` / `_sub` / `_lag` for the
                  variants, with the vector env's own parameter table): observations and rewards rounded to f32, the length;
  the end         final_obs and the truncated flag against tg_rollout_final_state*; episode_return against the f64 left-to-right
                  sum of the replay's rewards.
Even slots get a saturated action plus N(0, 0.05^2) noise (they fail), odd slots the noise alone (they run to the clock): every run
asserts, from the yardstick's flags, that both kinds of ending occurred and that every slot completed at least two episodes."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = {"f32": torch.float32, "f64": torch.float64}
SATURATED = {"CartPole": [1.0], "QuadPole2D": [1.0, -1.0], "QuadPole": [1.0, 1.0, -1.0, -1.0], "Pendulum": [0.0]}
T, STEPS = 48, 150              # the issue's shapes: 150 steps at max_steps = 48


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


def make_env(tg, name, horizon=T, substeps=1, tau=0.0, randomize=None):
    env = tg.environments.ENV_CLASSES[name](max_steps=horizon)
    env.substeps = substeps
    env.motor_time_constant = tau
    if randomize:
        env.randomize(randomize, seed=5)
    return env


def make_actions(name, n, steps, seed=1234, first_slot=0):
    """[steps][n][A] float32: even GLOBAL slots saturated + noise, odd slots the noise alone (seeded; a shard takes its columns)."""
    A = len(SATURATED[name])
    g = torch.Generator().manual_seed(seed)
    total = first_slot + n
    noise = torch.randn(steps, total, A, generator=g) * 0.05
    base = torch.zeros(total, A)
    base[0::2] = torch.tensor(SATURATED[name])
    return (noise + base)[:, first_slot:, :].contiguous()


def run(vec, actions, dev, seed):
    """reset(seed) and one step per row of `actions`; everything the env returned, on the host.  One synchronisation at the end."""
    steps, n, _ = actions.shape
    S = vec.S
    act_d = actions.to(dev)
    rec = {"obs": torch.empty(steps, n, S, device=dev), "rew": torch.empty(steps, n, device=dev),
           "term": torch.empty(steps, n, dtype=torch.bool, device=dev), "trunc": torch.empty(steps, n, dtype=torch.bool, device=dev),
           "fobs": torch.empty(steps, n, S, device=dev), "fret": torch.empty(steps, n, device=dev),
           "flen": torch.empty(steps, n, dtype=torch.int32, device=dev)}
    obs0, _ = vec.reset(seed=seed) if seed is not None else vec.reset()
    rec["obs0"] = obs0.clone()
    rec["ord0"] = vec.episode_ordinals
    ptrs = None
    for t in range(steps):
        obs, rew, term, trunc, info = vec.step(act_d[t])
        here = (obs.data_ptr(), rew.data_ptr(), term.data_ptr(), trunc.data_ptr(), info["final_obs"].data_ptr(),
                info["episode_return"].data_ptr(), info["episode_length"].data_ptr())
        assert ptrs is None or here == ptrs, "step() must return the same storage every call"
        ptrs = here
        assert term.dtype == torch.bool and trunc.dtype == torch.bool and obs.dtype == torch.float32 and rew.dtype == torch.float32
        rec["obs"][t].copy_(obs); rec["rew"][t].copy_(rew); rec["term"][t].copy_(term); rec["trunc"][t].copy_(trunc)
        rec["fobs"][t].copy_(info["final_obs"]); rec["fret"][t].copy_(info["episode_return"]); rec["flen"][t].copy_(info["episode_length"])
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in rec.items()}


def reset_states(tg, vec, ordinal, dev):
    """The yardstick's initial states of episode ordinal `ordinal` for every slot: [S][n] in the arithmetic dtype."""
    Nn = tg._native
    s0 = torch.empty(vec.S, vec.num_envs, dtype=vec.dtype, device=dev)
    with torch.cuda.device(dev):
        Nn.check(Nn.load().tg_env_reset(C.byref(vec.params), Nn.dtype_code(vec.dtype), s0.data_ptr(), vec.num_envs, vec.num_envs,
                                        vec.seed, int(ordinal), vec.env_offset, 1, Nn.stream_ptr(dev)), "tg_env_reset")
    return s0


def replay(tg, vec, s0, acts, dev):
    """The existing path on one episode per slot: tg_rollout_forced* from s0 [S][n] under acts [n][T][A] (zeros behind what the
    slot was fed) with the vector env's parameters, variant and table, then tg_rollout_final_state*."""
    Nn, Ro, K = tg._native, tg.rollout, tg.hip_ops
    n, horizon = vec.num_envs, vec.horizon
    tr = Ro.DeviceTrajectory(vec.S, vec.A, horizon, n, 1, n, vec.dtype, dev)
    motor_kw = {}
    with torch.cuda.device(dev):
        st = Nn.stream_ptr(dev)
        Nn.check(Nn.load().tg_rollout_begin(C.byref(tr.native()), vec.S, vec.A, st), "tg_rollout_begin")
        tr.obs[:, 0, :].copy_(s0)
        tr.act.copy_(torch.as_tensor(acts).permute(2, 1, 0).to(dev))
        if vec.lag:
            tr.motor = torch.zeros(vec.A, horizon + 1, n, dtype=torch.float32, device=dev)
            motor_kw = {"motor": tr.motor.data_ptr()}
        ptab = None if vec.env_params is None else vec.env_params.data_ptr()
        name, table = Ro.step_entry(True, ptab, vec.substeps, **motor_kw)
        Nn.check(getattr(Nn.load(), name)(C.byref(vec.params), *table, C.byref(tr.native()), 0, horizon,
                                          *Ro.sub_tail(vec.substeps, **motor_kw), st), name)
        s_final, timeout = K.rollout_final_state(vec.params, tr, env_params=vec.env_params, substeps=vec.substeps, motor=tr.motor)
    torch.cuda.synchronize()
    return {"obs": tr.obs.cpu().numpy(), "rew": tr.rew.cpu().numpy(), "len": tr.len.cpu().numpy(), "s_final": s_final.cpu().numpy(),
            "timeout": timeout.cpu().numpy()}


def check_against_the_existing_path(tg, vec, got, actions, dev, what):
    """Every episode of every slot against its isolated replay; -> (failure ends, clock ends, completed episodes per slot)."""
    steps, n, A = actions.shape
    horizon = vec.horizon
    acts = actions.numpy()
    done = got["term"] | got["trunc"]
    assert not (got["term"] & got["trunc"]).any(), f"{what}: a slot both terminated and truncated"
    starts = [[0] + [int(t) + 1 for t in np.nonzero(done[:, i])[0]] for i in range(n)]
    completed = np.array([len(s) - 1 for s in starts])
    failures = clock = 0
    for k in range(int(completed.max()) + 1):
        fed = np.zeros((n, horizon, A), dtype=np.float32)
        span = {}
        for i in range(n):
            if k < len(starts[i]) and starts[i][k] < steps:
                b = starts[i][k]
                e = starts[i][k + 1] if k + 1 < len(starts[i]) else steps          # one past the episode's last observed step
                assert e - b <= horizon, f"{what}: slot {i} episode {k} ran {e - b} steps past the horizon {horizon}"
                fed[i, :e - b] = acts[b:e, i]
                span[i] = (b, e - b, k + 1 < len(starts[i]))
        assert (got["ord0"] == 0).all()
        s0 = reset_states(tg, vec, k, dev)
        ref = replay(tg, vec, s0, fed, dev)
        s0_32 = s0.cpu().numpy().astype(np.float32)
        ref_obs32, ref_rew32 = ref["obs"].astype(np.float32), ref["rew"].astype(np.float32)
        for i, (b, m, complete) in span.items():
            tag = f"{what}: slot {i} episode {k} (steps {b}..{b + m - 1})"
            first = got["obs0"][i] if b == 0 else got["obs"][b - 1, i]
            assert np.array_equal(bits(first), bits(s0_32[:, i])), f"{tag}: initial state"
            assert np.array_equal(bits(got["rew"][b:b + m, i]), bits(ref_rew32[:m, i])), f"{tag}: rewards"
            inner = m - 1 if complete else m                                         # (the last step of a complete episode returns the reset)
            assert np.array_equal(bits(got["obs"][b:b + inner, i]), bits(ref_obs32[:, 1:inner + 1, i].T)), f"{tag}: observations"
            if not complete:
                assert ref["len"][i] > m or ref["len"][i] <= 0, f"{tag}: the replay ended at {ref['len'][i]}, the vector env went on"
                continue
            last = b + m - 1
            assert ref["len"][i] == m == got["flen"][last, i], f"{tag}: length {m} / {got['flen'][last, i]} against {ref['len'][i]}"
            assert np.array_equal(bits(got["fobs"][last, i]), bits(ref["s_final"][i])), f"{tag}: final_obs"
            assert bool(got["trunc"][last, i]) == bool(ref["timeout"][i]) and bool(got["term"][last, i]) != bool(ref["timeout"][i]), \
                f"{tag}: truncated / terminated against the yardstick's clock flag {ref['timeout'][i]}"
            total = np.cumsum(ref["rew"][:m, i].astype(np.float64))[-1]              # (cumsum: strictly left to right)
            assert np.array_equal(bits(got["fret"][last, i]), bits(np.float32(total))), f"{tag}: episode_return"
            failures += int(not ref["timeout"][i])
            clock += int(ref["timeout"][i])
    return failures, clock, completed


def run_and_check(tg, dev, env, name, n, dtype, steps, seed=7, env_offset=0, what=""):
    vec = tg.DeviceVecEnv(env, n, seed=seed, dtype=dtype, device=dev, env_offset=env_offset)
    actions = make_actions(name, n, steps, first_slot=env_offset)
    got = run(vec, actions, dev, seed)
    failures, clock, completed = check_against_the_existing_path(tg, vec, got, actions, dev, what)
    print(f"{what}: {failures} failure ends, {clock} clock ends, episodes per slot {completed.min()}..{completed.max()}")
    assert completed.min() >= 2, f"{what}: a slot completed {completed.min()} episodes: the reset path is not exercised"
    return vec, got, failures, clock


# ------------------------------------------------------------------------------------------------------------------------------
# 1. every env, dtype and launch shape against the existing path
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 64, 70, 130])
@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("name", ["CartPole", "QuadPole2D", "QuadPole"])
def test_every_episode_is_the_existing_path_run_in_isolation(tg, dev, name, dt, n):
    what = f"{name} {dt} n={n}"
    vec, got, failures, clock = run_and_check(tg, dev, make_env(tg, name), name, n, DTYPES[dt], STEPS, what=what)
    assert vec.variant == "plain"
    assert failures >= 1, f"{what}: no episode ended in a failure"
    if n > 1:                                                                    # (slot 0 alone is a saturated slot)
        assert clock >= 1, f"{what}: no episode ran to the clock"


@pytest.mark.parametrize("n", [1, 64, 70, 130])
def test_pendulum_runs_to_the_clock(tg, dev, n):
    what = f"Pendulum f32 n={n}"
    vec, got, failures, clock = run_and_check(tg, dev, make_env(tg, "Pendulum"), "Pendulum", n, torch.float32, STEPS, what=what)
    assert failures == 0 and clock >= 2 * n and not got["term"].any()


def test_pendulum_terminates_after_exactly_term_steps_balanced_steps(tg, dev):
    n = 70
    env = make_env(tg, "Pendulum", horizon=200)
    term_steps = int(env.native_params().p[4])
    assert term_steps == 101                                                     # 0.05 s steps: the fp64 sum first exceeds 5 s there
    vec = tg.DeviceVecEnv(env, n, seed=3, device=dev)
    vec.reset()
    upright = torch.tensor([0.0, -1.0, 0.0]).repeat(n, 1)
    obs = vec.set_state(upright)
    assert torch.equal(obs.cpu(), upright) and torch.equal(vec.state.cpu(), upright) and not bool(vec.episode_steps.any())
    zero = torch.zeros(n, 1, device=dev)
    term, trunc, length = [], [], None
    for t in range(term_steps + 5):
        _, _, te, tr, info = vec.step(zero)
        term.append(te.clone()); trunc.append(tr.clone())
        if t == term_steps - 1:
            length = info["episode_length"].clone()
    term, trunc = torch.stack(term).cpu(), torch.stack(trunc).cpu()
    assert not trunc.any()
    assert term[term_steps - 1].all() and int(term.sum()) == n, "terminated must fire at step term_steps and at no other"
    assert bool((length.cpu() == term_steps).all())
    # the yardstick agrees: the replay from the same states under the same actions ends there, and not by the clock
    ref = replay(tg, vec, upright.t().contiguous().to(dev), np.zeros((n, 200, 1), dtype=np.float32), dev)
    assert (ref["len"] == term_steps).all() and not ref["timeout"].any()


def test_one_plain_step_is_tg_env_step(tg, dev):
    Nn = tg._native
    for name in ("CartPole", "QuadPole2D", "QuadPole", "Pendulum"):
        for dt in (torch.float32, torch.float64):
            n = 70
            vec = tg.DeviceVecEnv(make_env(tg, name), n, seed=11, dtype=dt, device=dev)
            vec.reset()
            assert vec.variant == "plain"
            state = vec.state.t().contiguous()                                   # [S][n]
            actions = make_actions(name, n, 1)[0].to(dev)
            nxt = torch.empty_like(state)
            steps = torch.zeros(n, dtype=torch.int32, device=dev)
            rew, trunc = torch.empty(n, dtype=dt, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
            with torch.cuda.device(dev):
                Nn.check(Nn.load().tg_env_step(C.byref(vec.params), Nn.dtype_code(dt), state.data_ptr(), n, actions.t().contiguous().data_ptr(),
                                               n, nxt.data_ptr(), n, steps.data_ptr(), None, rew.data_ptr(), trunc.data_ptr(), n,
                                               Nn.stream_ptr(dev)), "tg_env_step")
            obs, reward, term, tr, _ = vec.step(actions)
            assert not bool(term.any()) and not bool(tr.any()) and not bool(trunc.any())
            assert np.array_equal(bits(obs), bits(nxt.t().float())), f"{name} {dt}: observation"
            assert np.array_equal(bits(reward), bits(rew.float())), f"{name} {dt}: reward"
            assert np.array_equal(bits(vec.state), bits(nxt.t())), f"{name} {dt}: the state in the arithmetic dtype"


# ------------------------------------------------------------------------------------------------------------------------------
# 2. the variants
# ------------------------------------------------------------------------------------------------------------------------------
# name -> (env settings, DeviceVecEnv.variant, horizon, steps).  The horizons keep the physics of the plain shape: on the CPU oracle
# (oracle/envs.py, 70 envs, the rotor lag restated in float32) the saturated slots leave the bounds between physics steps 35 and 48
# with and without the lag and the idle slots stay inside for 80, so 48 (plain), 3 x 16 and 2 x 32 physics steps see both endings and
# 64 lagged steps leave the failures room; every run is three episodes long.
VARIANTS = {"sub3": (dict(substeps=3), "sub", 16, 60), "lag": (dict(tau=0.05), "lag", 64, 200),
            "lag_sub2": (dict(substeps=2, tau=0.05), "lag", 32, 100), "dr": (dict(randomize={"mass": (0.8, 1.25)}), "dr", T, STEPS),
            "lag_dr": (dict(tau=0.05, randomize={"mass": (0.8, 1.25)}), "lag+dr", 64, 200)}


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", ["QuadPole2D", "QuadPole"])
def test_variants_against_their_existing_entries(tg, dev, name, variant, dt):
    kw, label, horizon, steps = VARIANTS[variant]
    if name == "QuadPole2D" and "randomize" in kw:
        kw = dict(kw, randomize={"mq": (0.8, 1.25)})
    what = f"{name} {variant} {dt}"
    vec, got, failures, clock = run_and_check(tg, dev, make_env(tg, name, horizon, **kw), name, 70, DTYPES[dt], steps, what=what)
    assert vec.variant == label
    assert failures >= 1 and clock >= 1, f"{what}: {failures} failure ends, {clock} clock ends"


@pytest.mark.parametrize("name, key", [("QuadPole2D", "mq"), ("QuadPole", "mass")])
def test_parameter_table_is_per_reset(tg, dev, name, key):
    Nn = tg._native
    n, seed, off = 70, 21, 64
    env = make_env(tg, name, randomize={key: (0.8, 1.25)})
    vec = tg.DeviceVecEnv(env, n, seed=seed, device=dev, env_offset=off)

    def drawn(stream_id):
        tab = torch.empty(12, n, dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            Nn.check(Nn.load().tg_env_randomize(C.byref(env.native_params()), C.byref(env.randomize_spec()), tab.data_ptr(), n, seed,
                                                stream_id, off, 1, Nn.stream_ptr(dev)), "tg_env_randomize")
        return tab

    _, info = vec.reset(seed=seed)
    assert info["env_params"] is vec.env_params and vec.variant == "dr"
    first = vec.env_params.clone()
    assert np.array_equal(bits(first), bits(drawn(0)))
    slot = env.parameter_slots()[key]
    assert float(first[slot].min()) < float(first[slot].max())                   # vehicles differ
    actions = make_actions(name, n, STEPS, first_slot=off).to(dev)
    ended = torch.zeros(n, dtype=torch.bool, device=dev)
    for t in range(STEPS):
        _, _, te, tr, info = vec.step(actions[t])
        ended |= te | tr
        assert info["env_params"] is vec.env_params
    assert bool(ended.all()) and np.array_equal(bits(vec.env_params), bits(first)), "the table must survive the auto-resets"
    vec.reset()
    assert np.array_equal(bits(vec.env_params), bits(drawn(1))) and not torch.equal(vec.env_params, first)
    env.randomize(None)
    _, info = vec.reset()
    assert "env_params" not in info and vec.env_params is None and vec.variant == "plain"


def test_cartpole_ends_at_max_steps_before_its_own_clock(tg, dev):
    n = 70
    env = make_env(tg, "CartPole", horizon=8)
    assert env.native_params().time_trunc_step == 9                               # the env's own clock would fire a step later
    vec = tg.DeviceVecEnv(env, n, seed=2, device=dev)
    vec.reset()
    actions = (make_actions("CartPole", n, 8) * 0).to(dev)
    for t in range(8):
        _, _, term, trunc, info = vec.step(actions[t])
        if t < 7:
            assert not bool(term.any()) and not bool(trunc.any())
    assert bool(trunc.all()) and not bool(term.any()) and bool((info["episode_length"] == 8).all())
    assert not bool(vec.episode_steps.any()) and bool((vec.episode_ordinals == 1).all())


# ------------------------------------------------------------------------------------------------------------------------------
# 3. sharding, determinism, buffers
# ------------------------------------------------------------------------------------------------------------------------------
KEYS = ("obs0", "obs", "rew", "term", "trunc", "fret", "flen")


@pytest.mark.parametrize("variant", ["plain", "lag_dr"])
def test_shards_are_the_slots_of_one_object(tg, dev, variant):
    name, seed = "QuadPole", 9
    kw, _, horizon, steps = ({}, "plain", T, STEPS) if variant == "plain" else VARIANTS[variant]
    actions = make_actions(name, 130, steps)
    whole = run(tg.DeviceVecEnv(make_env(tg, name, horizon, **kw), 130, seed=seed, device=dev), actions, dev, seed)
    parts = [run(tg.DeviceVecEnv(make_env(tg, name, horizon, **kw), m, seed=seed, device=dev, env_offset=off),
                 actions[:, off:off + m].contiguous(), dev, seed) for off, m in ((0, 64), (64, 66))]          # the same action rows
    assert (whole["term"] | whole["trunc"]).any(axis=0).all()
    for key in KEYS:
        joined = np.concatenate([p[key] for p in parts], axis=0 if key == "obs0" else 1)
        if key in ("fret", "flen"):                                              # (defined where the slot ended)
            ended = whole["term"] | whole["trunc"]
            assert np.array_equal(bits(joined)[ended], bits(whole[key])[ended]), key
        else:
            assert np.array_equal(bits(joined), bits(whole[key])), key
    ended = whole["term"] | whole["trunc"]
    joined = np.concatenate([p["fobs"] for p in parts], axis=1)
    assert np.array_equal(bits(joined)[ended], bits(whole["fobs"])[ended]), "final_obs"


@pytest.mark.parametrize("name", ["CartPole", "QuadPole"])
def test_four_wave_workgroups_are_the_slots_of_small_objects(tg, dev, name):
    """Above 2^18 slots the launch takes 256-thread workgroups (four waves, each with its own staging region; here the last
    workgroup has a full wave, a wave of 6 rows and two waves wholly beyond n).  Its first and last rows must be, bit for bit, the
    one-wave objects at the same global indices, which the tests above hold to the existing path."""
    n, seed, steps = (1 << 18) + 70, 17, 100
    windows = ((0, 130), ((1 << 18) - 256, 326))                                 # (env_offset, slots) of the small objects
    A = len(SATURATED[name])
    g = torch.Generator(device=dev).manual_seed(5)
    base = torch.zeros(n, A, device=dev)
    base[0::2] = torch.tensor(SATURATED[name], device=dev)
    big = tg.DeviceVecEnv(make_env(tg, name), n, seed=seed, device=dev)
    small = [tg.DeviceVecEnv(make_env(tg, name), m, seed=seed, device=dev, env_offset=off) for off, m in windows]
    first = [big.reset(seed=seed)[0]] + [v.reset(seed=seed)[0] for v in small]
    for (off, m), obs in zip(windows, first[1:]):
        assert np.array_equal(bits(first[0][off:off + m]), bits(obs))
    ended_any = [torch.zeros(m, dtype=torch.bool, device=dev) for _, m in windows]
    kinds = torch.zeros(2, dtype=torch.int64, device=dev)
    for t in range(steps):
        actions = base + 0.05 * torch.randn(n, A, device=dev, generator=g)
        whole = big.step(actions)
        for w, ((off, m), v) in enumerate(zip(windows, small)):
            part = v.step(actions[off:off + m])
            ended = part[2] | part[3]
            ended_any[w] |= ended
            kinds += torch.stack([part[2].sum(), part[3].sum()])
            for a, b in zip(whole[:4], part[:4]):
                assert torch.equal(a[off:off + m].view(torch.uint8), b.view(torch.uint8)), f"{name} step {t} rows {off}.."
            for key in ("final_obs", "episode_return", "episode_length"):
                assert torch.equal(whole[4][key][off:off + m][ended], part[4][key][ended]), f"{name} step {t} {key} rows {off}.."
    assert all(bool(e.all()) for e in ended_any) and bool((kinds > 0).all())     # every compared slot was reset; both kinds of ending
    assert torch.equal(big.episode_ordinals[-326:], small[1].episode_ordinals)


def test_a_seeded_reset_repeats_and_an_unseeded_one_moves_on(tg, dev):
    name, n, seed = "QuadPole2D", 70, 13
    vec = tg.DeviceVecEnv(make_env(tg, name), n, seed=0, device=dev)
    actions = make_actions(name, n, STEPS)
    a = run(vec, actions, dev, seed)
    b = run(vec, actions, dev, seed)
    ended = a["term"] | a["trunc"]
    for key in KEYS:
        assert np.array_equal(bits(a[key])[ended] if key in ("fret", "flen") else bits(a[key]),
                              bits(b[key])[ended] if key in ("fret", "flen") else bits(b[key])), key
    assert np.array_equal(bits(a["fobs"])[ended], bits(b["fobs"])[ended])
    before = vec.episode_ordinals.cpu()
    obs, _ = vec.reset()
    assert torch.equal(vec.episode_ordinals.cpu(), before + 1) and bool((before >= 2).all())
    assert not bool(vec.episode_steps.any())
    fresh = obs.cpu().numpy()
    assert not np.array_equal(fresh, a["obs0"]) and (fresh != a["obs0"]).any(axis=1).all(), "fresh ordinals give fresh initial states"
    # ... and they are the yardstick's draws for those ordinals
    for k in np.unique(before.numpy() + 1):
        s0 = reset_states(tg, vec, int(k), dev).cpu().numpy().astype(np.float32)
        rows = np.nonzero(before.numpy() + 1 == k)[0]
        assert np.array_equal(bits(fresh[rows]), bits(s0[:, rows].T))


def test_interface_contract(tg, dev):
    vec = tg.DeviceVecEnv(make_env(tg, "QuadPole"), 5, device=dev)
    assert vec.num_envs == 5 and vec.observation_space.shape == (5, 20) and vec.action_space.shape == (5, 4)
    with pytest.raises(RuntimeError, match="before reset"):
        vec.step(torch.zeros(5, 4, device=dev))
    obs, info = vec.reset(seed=4)
    assert obs.shape == (5, 20) and obs.dtype == torch.float32 and info == {}
    with pytest.raises(ValueError, match="float32"):
        vec.step(torch.zeros(5, 4, device=dev, dtype=torch.float64))
    with pytest.raises(ValueError, match="float32"):
        vec.step(torch.zeros(4, 4, device=dev))
    with pytest.raises(tg._native.NativeLibraryError):
        vec.step(torch.zeros(5, 4))
    wide = torch.zeros(5, 8, device=dev)
    out = vec.step(wide[:, ::2])                                                  # not contiguous: made so
    assert set(out[4]) == {"final_obs", "episode_return", "episode_length"}
    assert bool((vec.episode_steps == 1).all())
    vec.close()
    with pytest.raises(RuntimeError, match="closed"):
        vec.step(torch.zeros(5, 4, device=dev))
