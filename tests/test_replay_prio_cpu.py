"""CPU: the prioritised replay ABI (tg_replay_prio and its five entries: symbols, struct size, the level layout, every refusal with
nothing launched) and the restatement (tests/replay_prio_ref.py) held to the definition of proportional sampling in float64."""
import ctypes as C
import re

import numpy as np
import pytest

import trajopt_grpo_amd as tg
import replay_prio_ref as PR
from test_replay_cpu import FAKE, HEADER, make_replay

N = tg._native
ENTRIES = ("tg_replay_prio_push", "tg_replay_prio_update", "tg_replay_prio_sample", "tg_replay_prio_rebuild")
OUTS = ("o_obs", "o_act", "o_rew", "o_next_obs", "o_disc", "o_idx", "o_raw", "o_weight")


def make_prio(rows=32, **over):
    p = N.ReplayPrio()
    assert N.load().tg_replay_prio_levels(rows, C.byref(p)) > 0
    p.d_tree, p.d_max = over.pop("d_tree", FAKE), over.pop("d_max", FAKE)
    for name, value in over.items():
        setattr(p, name, value)
    return p


def call(entry, r, p, **over):
    lib = N.load()
    rp, pp = (None if x is None else C.byref(x) for x in (r, p))
    args = {"tg_replay_prio_push": (rp, pp), "tg_replay_prio_rebuild": (pp,),
            "tg_replay_prio_update": (rp, pp, over.get("batch", 16), over.get("idx", FAKE), over.get("td", FAKE), over.get("alpha", 0.6),
                                      over.get("eps", 1e-6)),
            "tg_replay_prio_sample": (rp, pp, over.get("batch", 16), None, 1, 0, over.get("beta", 0.4), *(over.get(k, FAKE) for k in OUTS))}
    return getattr(lib, entry)(*args[entry], None), lib.tg_last_error().decode()


def test_symbols_struct_sizes_and_the_level_layout():
    lib = N.load()
    for name in ENTRIES + ("tg_replay_prio_levels",):
        assert re.search(r"\b(int|int64_t)\s+" + name + r"\s*\(", HEADER) and name in N.SIGNATURES and hasattr(lib, name), name
    assert "typedef struct tg_replay_prio {" in HEADER and "152 bytes" in HEADER
    assert C.sizeof(N.ReplayPrio) == 152 and C.sizeof(N.Replay) == 176 and lib.tg_abi_version() == N.ABI_VERSION == 13
    for R in (1, 64, 65, 4096, 4097, 262145, 2 ** 31 - 1):
        p = N.ReplayPrio()
        want, floats = PR.levels(R)
        assert lib.tg_replay_prio_levels(R, C.byref(p)) == floats and p.levels == len(want) <= 7
        assert [(p.offset[l], p.size[l]) for l in range(p.levels)] == want and want[-1][1] == 1 and want[0] == (0, R)
        assert all(off % 64 == 0 for off, _ in want) and all(p.size[l] == 0 for l in range(p.levels, 8))
    for R in (0, -1, 2 ** 31):
        assert lib.tg_replay_prio_levels(R, C.byref(N.ReplayPrio())) == N.TG_ERR_ARG and f"rows={R} outside" in lib.tg_last_error().decode()


@pytest.mark.parametrize("entry", ENTRIES)
def test_entries_refuse_before_any_launch(entry):
    r, rebuild = make_replay(), entry == "tg_replay_prio_rebuild"           # 8 slots x 4 time slots = 32 rows
    moved = make_prio()
    moved.offset[1] = 128
    cases = [(r, None, "null pointer"), (r, make_prio(d_tree=None), "null pointer"), (r, make_prio(d_max=None), "null pointer"),
             (r, make_prio(d_tree=FAKE + 4), "16-byte aligned"), (r, make_prio(levels=1), "do not fit"), (r, make_prio(levels=8), "do not fit"),
             (r, make_prio(levels=3), "are not tg_replay_prio_levels'"), (r, moved, "are not tg_replay_prio_levels'")]
    if not rebuild:
        cases += [(None, make_prio(), "null pointer"), (make_replay(d_rew=None), make_prio(), "null pointer"),
                  (r, make_prio(rows=33), "do not fit 32 rows"), (make_replay(K=2, n_step=3), make_prio(rows=16), "capacity_steps=2 < n_step=3")]
    for rr, pp, text in cases:
        rc, msg = call(entry, rr, pp)
        assert rc == N.TG_ERR_ARG and f"{entry}: " in msg and text in msg, (rc, msg)
    if not rebuild:
        rc, msg = call(entry, make_replay(S=33), make_prio())
        assert rc == N.TG_ERR_UNSUPPORTED and "obs_dim=33" in msg, (rc, msg)
    own = {"tg_replay_prio_update": [{"alpha": -0.5}, {"eps": float("nan")}, {"alpha": float("inf")}, {"idx": None}, {"td": None}],
           "tg_replay_prio_sample": [{"beta": -1.0}, {"beta": float("nan")}] + [{k: FAKE + 8} for k in OUTS] + [{k: None} for k in OUTS]}
    for kw in own.get(entry, []) + ([{"batch": b} for b in (0, -5, 2 ** 31)] if entry in own else []):
        rc, msg = call(entry, r, make_prio(), **kw)
        assert rc == N.TG_ERR_ARG and entry in msg and ("batch" not in kw or f"batch={kw['batch']} outside [1, 2^31)" in msg), (kw, rc, msg)
    for kw in ({"alpha": -0.1}, {"beta": float("nan")}, {"priority_eps": float("inf")}):      # and the class, on the host
        with pytest.raises(ValueError, match=next(iter(kw))):
            tg.DeviceReplayBuffer(5, 1, 4, 8, prioritized=True, device="cpu", **kw)


def test_restatement_samples_in_proportion_to_the_priorities():
    """300 rows over three levels: priorities 10^u, u uniform in [-3, 3], every fifth row and one whole node zero.  B = 65,536 stratified
    draws put within 2 of B p_i / sum p on every row in exact arithmetic; the third is for the float32 sums and prefixes."""
    rng = np.random.default_rng(7)
    rows, B = 300, 65536
    p = (10.0 ** rng.uniform(-3, 3, rows)).astype(np.float32)
    p[::5] = 0
    p[128:192] = 0
    assert p[p > 0].max() / p[p > 0].min() > 1e5
    tree = PR.build(p)
    assert len(tree) == 3 and tree[1][2] == 0 and tree[2][0] == PR.node_sum(tree[1])
    assert abs(float(tree[-1][0]) / p.astype(np.float64).sum() - 1) < 64 * 2.0 ** -24
    x = rng.standard_normal((5, 64)).astype(np.float32)                    # the two orders, each against its definition, lane by lane
    want, s = x.copy(), x.copy()
    for d in (1, 2, 4, 8, 16, 32):
        prev = want.copy()
        for i in range(d, 64):
            want[:, i] = prev[:, i] + prev[:, i - d]
    for d in (32, 16, 8, 4, 2, 1):
        for i in range(d):
            s[:, i] = s[:, i] + s[:, i + d]
    assert np.array_equal(PR.scan(x), want) and np.array_equal(PR.node_sum(x), s[:, 0])
    idx = PR.descend(tree, seed=0x1234ABCD5678, ordinal=(3 << 32) | 9, B=B)
    assert idx.min() >= 0 and idx.max() < rows and (p[idx] > 0).all(), "a zero-priority row was drawn"
    expect = B * p.astype(np.float64) / p.astype(np.float64).sum()
    assert np.abs(np.bincount(idx, minlength=rows) - expect).max() <= 3
    assert not np.array_equal(idx, PR.descend(tree, seed=0x1234ABCD5678, ordinal=(3 << 32) | 10, B=B))
