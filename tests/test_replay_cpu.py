"""CPU: the replay buffer's ABI (tg_replay, tg_replay_start / _push / _sample) and DeviceReplayBuffer's host side -- symbols, struct
layout, every refusal (code and message, nothing launched: the pointers handed over are not device memory) -- and the rule itself:
the in-place NumPy restatement (tests/replay_ref.py) against the brute-force per-row definition of an n-step transition, bit for bit."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import trajopt_grpo_amd as tg
import replay_ref as RR

N = tg._native
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(REPO, "include", "trajopt_grpo_hip.h")).read()
FAKE = 0x10000          # a non-null, 16-byte aligned address no refused call may touch
POINTERS = ("d_obs", "d_act", "d_next_obs", "d_rew", "d_disc", "d_nstep", "d_last_obs", "d_cursor", "d_filled", "d_open")
ENTRIES = ("tg_replay_start", "tg_replay_push", "tg_replay_sample")


def test_symbols_are_declared_bound_and_exported_and_the_abi_is_still_13():
    lib = N.load()
    for name in ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", HEADER), f"{name} is not declared"
        assert name in N.SIGNATURES and hasattr(lib, name)
    assert "typedef struct tg_replay {" in HEADER
    assert lib.tg_abi_version() == N.ABI_VERSION == 13
    assert int(re.search(r"#define\s+TG_ABI_VERSION\s+(\d+)", HEADER).group(1)) == 13
    assert tg.DeviceReplayBuffer is tg.replay.DeviceReplayBuffer and "DeviceReplayBuffer" in tg.__all__


def test_replay_struct_layout_matches_the_header():
    body = re.search(r"typedef struct tg_replay \{(.*?)\} tg_replay;", HEADER, re.S).group(1)
    fields = re.findall(r"^\s*([A-Za-z0-9_]+\s*\*?)\s+([a-z_]+)(?:\[(\d+)\])?;", body, re.M)
    size = {"float*": 8, "uint8_t*": 8, "int32_t*": 8, "int64_t": 8, "int32_t": 4, "float": 4}
    assert [name for _, name, _ in fields] == [name for name, _ in N.Replay._fields_]
    off = 0
    for ctype, name, count in fields:
        width = size[ctype.replace(" ", "")]
        off = (off + width - 1) // width * width
        total = width * int(count or 1)
        assert getattr(N.Replay, name).offset == off and getattr(N.Replay, name).size == total, name
        off += total
    assert off == 172 and C.sizeof(N.Replay) == 176                       # (8-byte alignment pads the tail)
    assert N.Replay.n.offset == 80 and N.Replay.capacity_steps.offset == 88 and N.Replay.n_step.offset == 100
    assert N.Replay.discount.offset == 104 and N.Replay.discount.size == 17 * 4


def make_replay(n=8, K=4, S=5, A=1, n_step=2, **over):
    r = N.Replay()
    for name in POINTERS:
        setattr(r, name, over.get(name, FAKE))
    r.n, r.capacity_steps, r.obs_dim, r.act_dim, r.n_step = n, K, S, A, n_step
    for j, g in enumerate(RR.discount_table(0.99, min(max(n_step, 0), 16))):
        r.discount[j] = float(g)
    return r


def call(entry, r, **over):
    lib = N.load()
    rp = None if r is None else C.byref(r)
    if entry == "tg_replay_start":
        rc = lib.tg_replay_start(rp, over.get("obs", FAKE), None)
    elif entry == "tg_replay_push":
        rc = lib.tg_replay_push(rp, *(over.get(k, FAKE) for k in ("actions", "obs", "reward", "terminated", "truncated", "final_obs")),
                                None)
    else:
        rc = lib.tg_replay_sample(rp, over.get("batch", 16), over.get("indices", None), 1, 0,
                                  *(over.get(k, FAKE) for k in ("o_obs", "o_act", "o_rew", "o_next_obs", "o_disc", "o_idx")), None)
    return rc, lib.tg_last_error().decode()


@pytest.mark.parametrize("entry", ENTRIES)
def test_entries_refuse_null_pointers(entry):
    cases = [call(entry, None)] + [call(entry, make_replay(**{name: None})) for name in POINTERS]
    own = {"tg_replay_start": ("obs",), "tg_replay_push": ("actions", "obs", "reward", "terminated", "truncated", "final_obs"),
           "tg_replay_sample": ("o_obs", "o_act", "o_rew", "o_next_obs", "o_disc", "o_idx")}[entry]
    cases += [call(entry, make_replay(), **{k: None}) for k in own]
    for rc, msg in cases:
        assert rc == N.TG_ERR_ARG and f"{entry}: null pointer" in msg, (rc, msg)


@pytest.mark.parametrize("entry", ENTRIES)
def test_entries_refuse_bad_sizes_and_alignment(entry):
    for r in (make_replay(n=0), make_replay(n=-2), make_replay(K=0)):
        rc, msg = call(entry, r)
        assert rc == N.TG_ERR_ARG and f"{entry}: bad sizes" in msg, (rc, msg)
    for k in (0, -1, 17):
        rc, msg = call(entry, make_replay(K=32, n_step=k))
        assert rc == N.TG_ERR_ARG and f"n_step={k} outside [1, 16]" in msg, (rc, msg)
    rc, msg = call(entry, make_replay(K=2, n_step=3))
    assert rc == N.TG_ERR_ARG and "capacity_steps=2 < n_step=3" in msg, (rc, msg)
    rc, msg = call(entry, make_replay(K=2 ** 11, n=2 ** 20))
    assert rc == N.TG_ERR_ARG and "rows >= 2^31" in msg, (rc, msg)
    assert call(entry, make_replay(K=2 ** 11 - 1, n=2 ** 20, d_obs=FAKE + 4))[0] == N.TG_ERR_ARG    # (2^31 - 2^20 rows pass that check)
    for S, A in ((0, 1), (33, 1), (5, 0), (5, 9)):
        rc, msg = call(entry, make_replay(S=S, A=A))
        assert rc == N.TG_ERR_UNSUPPORTED and f"obs_dim={S} outside [1, 32] or act_dim={A} outside [1, 8]" in msg, (rc, msg)
    for name in ("d_obs", "d_act", "d_next_obs", "d_last_obs"):
        rc, msg = call(entry, make_replay(**{name: FAKE + 4}))
        assert rc == N.TG_ERR_ARG and "must be 16-byte aligned" in msg, (rc, msg)


def test_sample_refuses_bad_batches_and_unaligned_outputs():
    for b in (0, -5, 2 ** 31):
        rc, msg = call("tg_replay_sample", make_replay(), batch=b)
        assert rc == N.TG_ERR_ARG and f"batch={b} outside [1, 2^31)" in msg, (rc, msg)
    for k in ("o_obs", "o_act", "o_rew", "o_next_obs", "o_disc", "o_idx"):
        rc, msg = call("tg_replay_sample", make_replay(), **{k: FAKE + 8})
        assert rc == N.TG_ERR_ARG and "the outputs must be 16-byte aligned" in msg, (rc, msg)


def test_the_class_refuses_on_the_host_before_any_launch():
    B = tg.DeviceReplayBuffer
    for kw, match in (({"n_step": 0}, "n_step=0 outside"), ({"n_step": 17, "capacity_steps": 32}, "n_step=17 outside"),
                      ({"n_step": 3, "capacity_steps": 2}, "capacity_steps=2 < n_step=3"),
                      ({"num_envs": 2 ** 20, "capacity_steps": 2 ** 11}, "rows >= 2\\^31"), ({"gamma": 0.0}, "gamma=0.0 not in"),
                      ({"gamma": 1.5}, "gamma=1.5 not in"), ({"gamma": float("nan")}, "not in"), ({"num_envs": 0}, "num_envs=0"),
                      ({"obs_dim": 33}, "obs_dim=33"), ({"act_dim": 9}, "act_dim=9"), ({"seed": -1}, "seed -1"),
                      ({"seed": 2 ** 64}, "seed")):
        args = {"obs_dim": 5, "act_dim": 1, "num_envs": 4, "capacity_steps": 8, "device": "cpu", **kw}
        with pytest.raises(ValueError, match=match):
            B(args.pop("obs_dim"), args.pop("act_dim"), args.pop("num_envs"), args.pop("capacity_steps"), **args)
    with pytest.raises(N.NativeLibraryError, match="no CPU fallback"):
        B(5, 1, 4, 8, device="cpu")
    with pytest.raises(N.NativeLibraryError, match="no CPU fallback"):      # (gamma = 1 is inside the range)
        B(5, 1, 4, 8, gamma=1.0, n_step=8, device="cpu")
    assert np.array_equal(tg.replay.discount_table(1.0, 3), np.ones(4, np.float32))


def test_discount_table_is_the_float64_power_rounded_once():
    g = tg.replay.discount_table(0.99, 16)
    assert g.dtype == np.float32 and g.shape == (17,) and g[0] == 1.0
    assert np.array_equal(g, RR.discount_table(0.99, 16))
    for j in range(17):
        assert g[j] == np.float32(np.float64(0.99) ** j)
    running = np.float32(1.0)                                              # (a float32 running product is NOT the table)
    diff = 0
    for j in range(1, 17):
        running = np.float32(running * np.float32(0.99))
        diff += int(running != g[j])
    assert diff > 0


@pytest.mark.parametrize("n, K, n_step", [(1, 1, 1), (3, 2, 2), (5, 3, 3), (4, 5, 5), (7, 7, 3), (2, 16, 16), (6, 4, 4)])
def test_restatement_equals_the_brute_force_per_row_definition(n, K, n_step):
    S, A = 3, 2
    rng = np.random.default_rng(100 * n + 10 * K + n_step)
    for p_done, with_cuts in ((0.0, False), (0.15, False), (0.5, True), (0.9, False)):
        ref = RR.ReplayRef(S, A, n, K, n_step=n_step, gamma=0.97)
        history = [[] for _ in range(n)]
        prev = rng.standard_normal((n, S)).astype(np.float32)
        ref.start(prev)
        for t in range(4 * K + 3):                                          # the ring wraps several times
            act = rng.standard_normal((n, A)).astype(np.float32)
            obs = rng.standard_normal((n, S)).astype(np.float32)
            fin = rng.standard_normal((n, S)).astype(np.float32)
            rew = rng.standard_normal(n).astype(np.float32)
            done = rng.random(n) < p_done
            term = done & (rng.random(n) < 0.5)
            trunc = done & ~term
            ref.push(act, obs, rew, term, trunc, fin)
            for i in range(n):
                history[i].append(dict(obs=prev[i].copy(), act=act[i], rew=rew[i], term=bool(term[i]), trunc=bool(trunc[i]),
                                       nx=(fin[i] if done[i] else obs[i]), cut=False))
            prev = obs.copy()
            if with_cuts and t % 5 == 3:                                    # a venv.reset() + start() in mid-stream
                prev = rng.standard_normal((n, S)).astype(np.float32)
                ref.start(prev)
                for i in range(n):
                    history[i][-1]["cut"] = True
            rows = RR.brute_force_rows(history, n, K, n_step, ref.g)
            assert len(rows) == ref.rows == min(t + 1, K) * n
            for row, (o, a, r, nx, d, k) in rows.items():
                assert np.array_equal(ref.obs[row], o) and np.array_equal(ref.act[row], a), (t, row)
                assert ref.rew[row].view(np.uint32) == np.float32(r).view(np.uint32), (t, row)
                assert np.array_equal(ref.next_obs[row], nx) and ref.disc[row] == d and ref.nstep[row] == k <= n_step, (t, row)
            assert np.all(ref.cursor == (t + 1) % K) and np.all(ref.filled == min(t + 1, K)) and np.all(ref.open <= n_step - 1)


def test_index_map_stays_inside_the_stored_rows():
    for R in (1, 7, 2 ** 31 - 1):
        for w in (0, 1, 2 ** 31, 2 ** 32 - 1):
            row = int(RR.index_map(w, R))
            assert 0 <= row < R and row == (w * R) >> 32
    assert int(RR.index_map(2 ** 32 - 1, 2 ** 31 - 1)) == 2 ** 31 - 2
    w = np.arange(0, 2 ** 32, 2 ** 32 // 7 // 3, dtype=np.uint64)
    assert set(RR.index_map(w, 7).tolist()) == set(range(7))
