"""CPU: deterministic evaluation and parameter sweeps -- the new entry points in header / exports / binding, tg_param_grid's layout,
every refusal of the entry points (no launch) and of Evaluator, the self-consistency of the NumPy restatements, and
Pipeline.train(eval_every=...) with a stub evaluator."""
import csv
import ctypes as C
import inspect
import math
import os
import re

import numpy as np
import pytest

import trajopt_grpo_amd as tg

import evaluation_fp64 as EV

N = tg._native
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["tg_env_param_grid", "tg_eval_tile_states", "tg_eval_cells"]


def test_header_exports_and_binding_agree_on_the_new_symbols():
    lib = N.load()
    header = open(os.path.join(REPO, "include", "trajopt_grpo_hip.h")).read()
    declared = set(re.findall(r"\b(tg_[a-z0-9_]+)\s*\(", header))
    for name in NEW_SYMBOLS:
        assert name in declared and name in N.SIGNATURES and hasattr(lib, name), name
    assert lib.tg_abi_version() == 13 == N.ABI_VERSION
    assert len(N.SIGNATURES["tg_env_param_grid"][1]) == 6 and len(N.SIGNATURES["tg_eval_tile_states"][1]) == 4
    assert len(N.SIGNATURES["tg_eval_cells"][1]) == 6
    assert C.sizeof(N.EnvParams) == 4 * 4 + 8 + 12 * 8 and C.sizeof(N.Traj) == 6 * 8 + 8 + 4 + 4      # layouts kept
    # tg_param_grid: count, index[12], levels[12], 4 B of padding, the device pointer, episodes_per_cell
    assert C.sizeof(N.ParamGrid) == 4 + 12 * 4 + 12 * 4 + 4 + 8 + 8 == 120
    assert (N.ParamGrid.count.offset, N.ParamGrid.index.offset, N.ParamGrid.levels.offset) == (0, 4, 52)
    assert (N.ParamGrid.d_values.offset, N.ParamGrid.episodes_per_cell.offset) == (104, 112)
    assert "eval_kernels.hip" in open(os.path.join(REPO, "trajopt-grpo_amd", "csrc", "Makefile")).read()


def test_run_takes_deterministic_and_defaults_to_sampling():
    sig = inspect.signature(tg.DeviceRollout.run)
    assert sig.parameters["deterministic"].default is False
    sig = inspect.signature(tg.Evaluator.__init__)
    assert [sig.parameters[k].default for k in ("episodes", "sweep", "seed", "deterministic", "compute_dtype")] == [256, None, 0, True, None]
    assert inspect.signature(tg.Pipeline.train).parameters["eval_every"].default is None


def _grid(count=1, index=0, levels=2, E=4, values=4096):
    g = N.ParamGrid()
    g.count, g.d_values, g.episodes_per_cell = count, values, E
    for k in range(min(count, 12)):
        g.index[k], g.levels[k] = (index + k) % 12, levels
    return g


def test_param_grid_refuses_bad_arguments_without_a_launch():
    lib = N.load()
    p = N.default_params(N.TG_ENV_QUADPOLE, 16)
    fake = C.c_void_p(4096)                                           # never dereferenced: every call below is refused on the host

    def call(g, tab=fake, n=8, off=0, params=p):
        return lib.tg_env_param_grid(None if params is None else C.byref(params), None if g is None else C.byref(g), tab, n, off, None)

    assert call(_grid(), tab=None) == N.TG_ERR_ARG and b"null parameter table" in lib.tg_last_error()
    assert call(None) == N.TG_ERR_ARG and call(_grid(), params=None) == N.TG_ERR_ARG
    assert call(_grid(values=None)) == N.TG_ERR_ARG and b"null factor list" in lib.tg_last_error()
    for count in (13, -1):
        assert call(_grid(count=count)) == N.TG_ERR_ARG and b"count" in lib.tg_last_error()
    for index in (12, -1):
        g = _grid()
        g.index[0] = index
        assert call(g) == N.TG_ERR_ARG and b"outside p[0..11]" in lib.tg_last_error()
    g = _grid(count=2)
    g.index[1] = g.index[0]
    assert call(g) == N.TG_ERR_ARG and b"twice" in lib.tg_last_error()
    for levels in (0, -3):
        assert call(_grid(levels=levels)) == N.TG_ERR_ARG and b"levels" in lib.tg_last_error()
    assert call(_grid(E=3), n=8) == N.TG_ERR_ARG and b"not a multiple" in lib.tg_last_error()
    assert call(_grid(E=0)) == N.TG_ERR_ARG
    assert call(_grid(), off=-4) == N.TG_ERR_ARG
    assert call(_grid(levels=2, E=4), n=12) == N.TG_ERR_ARG and b"beyond the grid" in lib.tg_last_error()     # 2 cells hold 8 envs
    assert call(_grid(levels=2, E=4), n=8, off=4) == N.TG_ERR_ARG


def test_tile_states_and_cells_refuse_bad_arguments_without_a_launch():
    lib = N.load()
    fake = 4096
    tr = N.Traj()
    assert lib.tg_eval_tile_states(None, 5, 4, None) == N.TG_ERR_ARG
    assert lib.tg_eval_tile_states(C.byref(tr), 5, 4, None) == N.TG_ERR_ARG and b"null pointer" in lib.tg_last_error()
    tr.d_obs = tr.d_rew = tr.d_len = fake
    tr.n, tr.horizon, tr.dtype = 12, 8, N.TG_F32
    assert lib.tg_eval_tile_states(C.byref(tr), 5, 5, None) == N.TG_ERR_ARG and b"not a multiple" in lib.tg_last_error()
    assert lib.tg_eval_tile_states(C.byref(tr), 5, 0, None) == N.TG_ERR_ARG
    assert lib.tg_eval_tile_states(C.byref(tr), 0, 4, None) == N.TG_ERR_ARG
    assert lib.tg_eval_tile_states(C.byref(tr), 5, 12, None) == N.TG_OK                  # one cell: nothing to copy, nothing launched
    tr.dtype = 7
    assert lib.tg_eval_tile_states(C.byref(tr), 5, 4, None) == N.TG_ERR_ARG and b"dtype" in lib.tg_last_error()
    assert lib.tg_eval_cells(C.byref(tr), fake, 4, fake, fake, None) == N.TG_ERR_ARG and b"dtype" in lib.tg_last_error()
    tr.dtype = N.TG_F64
    for args in ((None, 4, fake, fake), (fake, 4, None, fake), (fake, 4, fake, None)):
        assert lib.tg_eval_cells(C.byref(tr), *args, None) == N.TG_ERR_ARG and b"null pointer" in lib.tg_last_error()
    assert lib.tg_eval_cells(None, fake, 4, fake, fake, None) == N.TG_ERR_ARG
    assert lib.tg_eval_cells(C.byref(tr), fake, 5, fake, fake, None) == N.TG_ERR_ARG and b"not a multiple" in lib.tg_last_error()
    assert lib.tg_eval_cells(C.byref(tr), fake, 0, fake, fake, None) == N.TG_ERR_ARG
    tr.d_len = None
    assert lib.tg_eval_cells(C.byref(tr), fake, 4, fake, fake, None) == N.TG_ERR_ARG


# ---- Evaluator: validation at construction, no device ----
def test_evaluator_validates_the_sweep_and_names_the_key():
    env = tg.QuadPole(max_steps=32)
    ev = tg.Evaluator(env, None, episodes=5, sweep={"tether_length": [0.5, 2.0], "mass": [0.8, 1.0, 1.25]})
    assert ev.sweep_names == ("mass", "tether_length") and ev.cells == 6            # p[] order, whatever the dictionary's
    assert ev.engine is None                                                       # nothing is allocated before the first evaluate()
    assert tg.Evaluator(env, None).cells == 1 and tg.Evaluator(env, None, sweep={}).cells == 1
    for key in ("spatial_bounds", "bound", "timestep", "max_steps", "no_such_parameter", "tether"):
        with pytest.raises(ValueError, match=re.escape(repr(key))):
            tg.Evaluator(env, None, sweep={"mass": [1.0], key: [1.0]})
    for bad in ([0.0], [-1.0], [1.0, math.inf], [math.nan], [], "ab", 3.0, [1.0, "x"], None):
        with pytest.raises(ValueError, match=re.escape(repr("mass"))):
            tg.Evaluator(env, None, sweep={"mass": bad})
    with pytest.raises(ValueError, match="sweep must map"):
        tg.Evaluator(env, None, sweep=[("mass", [1.0])])
    with pytest.raises(ValueError, match="do not fit"):
        tg.Evaluator(env, None, episodes=2 ** 20, sweep={"mass": [1.0] * 64, "gravity": [1.0] * 64})
    assert tg.Evaluator(tg.Pendulum(), None).early_name == "balanced" and tg.Evaluator(tg.CartPole(), None).early_name == "failure"


def test_evaluator_refuses_everything_else():
    env = tg.CartPole(max_steps=16)
    for episodes in (0, -1, 2.5, "8", True, None):
        with pytest.raises(ValueError, match="episodes"):
            tg.Evaluator(env, None, episodes=episodes)
    for seed in (-1, 2 ** 63, 1.5, "0", True):
        with pytest.raises(ValueError, match="seed"):
            tg.Evaluator(env, None, seed=seed)
    for det in (0, 1, None, "yes"):
        with pytest.raises(ValueError, match="deterministic"):
            tg.Evaluator(env, None, deterministic=det)
    with pytest.raises(ValueError, match="swarm"):
        tg.Evaluator(tg.QuadPoleSwarm(n_agents=4, max_steps=16), None)
    # the caller's env is not edited: a sweep switches randomisation off on the evaluator's own copy
    env = tg.QuadPole(max_steps=16).randomize({"mass": (0.8, 1.25)}, seed=3)
    ev = tg.Evaluator(env, None, sweep={"gravity": [0.9, 1.1]})
    assert ev._eval_env().randomization is None and env.randomization == {"mass": (0.8, 1.25)}
    assert tg.Evaluator(env, None)._eval_env().randomization == {"mass": (0.8, 1.25)}      # no sweep: the drawn vehicles


def test_result_table_and_summary_from_cell_rows():
    cells = np.array([[4, 10.0, 30.0, 1.0, 4.0, 40, 3, 1], [0, 0.0, 0.0, np.inf, -np.inf, 0, 0, 0], [2, -2.0, 4.0, -2.0, 0.0, 6, 0, 2]])

    class Dev:                                                                     # stands in for a device tensor
        def __init__(self, a):
            self.a = a

        def cpu(self):
            return self

        def numpy(self):
            return self.a
    sweep = [("mass", 0, [0.8, 1.0, 1.25])]
    res = tg.EvalResult(Dev(cells), Dev(np.arange(12.0)), sweep, 4, "failure")
    assert res.returns.shape == (3, 4) and res.sweep_names == ("mass",)
    t = res.table
    assert [r["factors"] for r in t] == [(0.8,), (1.0,), (1.25,)] and [r["episodes"] for r in t] == [4, 0, 2]
    assert t[0]["return_mean"] == 2.5 and t[0]["return_std"] == math.sqrt(30.0 / 4 - 2.5 ** 2) and t[0]["length_mean"] == 10.0
    assert t[0]["timeout_frac"] == 0.75 and t[0]["early_frac"] == 0.25 and (t[0]["return_min"], t[0]["return_max"]) == (1.0, 4.0)
    assert all(math.isnan(t[1][k]) for k in ("return_mean", "return_std", "return_min", "return_max", "length_mean", "timeout_frac"))
    s = res.summary
    assert s["episodes"] == 6 and s["return_mean"] == 8.0 / 6 and (s["return_min"], s["return_max"]) == (-2.0, 4.0) and s["cells"] == 3
    # two swept parameters: the last one runs fastest
    res = tg.EvalResult(Dev(np.zeros((6, 8))), Dev(np.zeros(6)), [("mass", 0, [0.8, 1.0, 1.25]), ("tether_length", 3, [0.5, 2.0])], 1, "failure")
    assert [res.factors(c) for c in range(6)] == [(0.8, 0.5), (0.8, 2.0), (1.0, 0.5), (1.0, 2.0), (1.25, 0.5), (1.25, 2.0)]


# ---- the restatements ----
NOMINAL = [1.5, 0.5, 9.80665, 0.5, 0.4, 0.4, 0.25, 0.1, 0.5, 1.5, 0.0, 0.0]


def test_restated_grid_decodes_row_major_in_p_order():
    sweep = [(3, [0.5, 2.0]), (0, [0.8, 1.0, 1.25])]                               # listed out of p[] order on purpose
    E = 5
    tab = EV.grid_table(NOMINAL, sweep, E, 30)
    assert EV.decode_cell(4, [3, 2]) == [2, 0]
    for c in range(6):
        col = tab[:, c * E:(c + 1) * E]
        assert np.all(col == col[:, :1])                                           # the E episodes of a cell share one vehicle
        assert col[0, 0] == 1.5 * [0.8, 1.0, 1.25][c // 2] and col[3, 0] == 0.5 * [0.5, 2.0][c % 2]
        for r in range(12):
            if r not in (0, 3):
                assert np.all(col[r] == NOMINAL[r])
    assert np.array_equal(tab[:, 5:10][0], np.full(5, 1.5 * 0.8)) and tab[0, 10] == 1.5               # a factor of 1.0: the nominal bits
    assert np.array_equal(EV.grid_table(NOMINAL, sweep, E, 20, env_offset=10), tab[:, 10:])           # a shard is a slice
    assert np.array_equal(EV.grid_table(NOMINAL, list(reversed(sweep)), E, 30), tab)                  # the listing order does not matter
    assert np.array_equal(EV.grid_table(NOMINAL, [], 3, 6), np.repeat(np.array(NOMINAL)[:, None], 6, axis=1))


@pytest.mark.parametrize("E", [1, 70, 256, 700])
def test_restated_cell_sums_agree_with_fsum(E):
    """Any summation order of E doubles is within (E - 1) u sum |x| of the exact sum, u = 2^-53 (Higham, 4.2); math.fsum is the
    exact sum rounded once (one more u |sum|): E 2^-53 sum |x| bounds the difference."""
    rng = np.random.default_rng(E)
    T, Cc = 37, 3
    n = Cc * E
    rew = (rng.standard_normal((T, n)) * 50).astype(np.float32)
    length = rng.integers(-2, T + 1, n).astype(np.int32)
    length[0], length[n - 1] = 1, T
    timeout = rng.integers(0, 2, n).astype(np.uint8)
    ret = EV.episode_returns(rew, length)
    cells = EV.cell_stats(ret, length, timeout, E, T)
    for i in (0, n - 1, n // 2):
        L = int(length[i])
        want = math.fsum(float(v) for v in rew[:L, i]) if 1 <= L <= T else 0.0
        assert abs(ret[i] - want) <= T * 2.0 ** -53 * float(np.abs(rew[:max(L, 0), i].astype(np.float64)).sum())
    for c in range(Cc):
        sl = slice(c * E, (c + 1) * E)
        ok = (length[sl] >= 1) & (length[sl] <= T)
        r = ret[sl][ok]
        assert cells[c, 0] == ok.sum() and cells[c, 5] == length[sl][ok].sum()
        assert cells[c, 6] + cells[c, 7] == cells[c, 0] and cells[c, 6] == (timeout[sl][ok] != 0).sum()
        assert abs(cells[c, 1] - math.fsum(r)) <= E * 2.0 ** -53 * float(np.abs(r).sum())
        assert abs(cells[c, 2] - math.fsum(float(v) * float(v) for v in r)) <= (E + 1) * 2.0 ** -53 * float((r * r).sum())
        if ok.any():
            assert cells[c, 3] == r.min() and cells[c, 4] == r.max()


def test_restated_empty_cell_reports_no_episode_and_the_reduction_identities():
    T, E = 9, 6
    ret = np.zeros(2 * E)
    length = np.array([0, -3, T + 1, 0, 0, -1] + [T] * E, dtype=np.int32)
    cells = EV.cell_stats(ret, length, np.ones(2 * E, dtype=np.uint8), E, T)
    assert list(cells[0]) == [0, 0, 0, np.inf, -np.inf, 0, 0, 0]
    assert list(cells[1]) == [E, 0, 0, 0, 0, E * T, E, 0]


# ---- Pipeline.evaluate / train(eval_every) with a stub evaluator ----
class _Stub:
    def __init__(self):
        self.calls = []

    def metadata(self):
        return {}

    def sample(self):
        self.calls.append("sample")

    def learn(self, buf):
        self.calls.append("learn")

    def save(self, path):
        with open(os.path.join(path, f"{id(self)}.saved"), "a") as f:
            f.write("x")


class _StubResult:
    sweep_names = ("mass",)

    def __init__(self, score):
        self.table = [{"cell": c, "factors": (f,), "episodes": 4, "return_mean": score + c, "return_std": 1.0, "return_min": 0.0,
                       "return_max": 9.0, "length_mean": 7.5, "timeout_frac": 0.5, "early_frac": 0.5} for c, f in enumerate((0.8, 1.25))]
        self.summary = {"return_mean": score}


class _StubEvaluator:
    def __init__(self, scores):
        self.scores, self.at = list(scores), []

    def evaluate(self):
        self.at.append(self.pipe.epochs_done)
        return _StubResult(self.scores[len(self.at) - 1])


def _pipeline(tmp_path, monkeypatch, scores):
    monkeypatch.chdir(tmp_path)
    stubs = [_Stub() for _ in range(3)]
    ev = _StubEvaluator(scores)
    pipe = tg.Pipeline("t", "c", lambda: tg.CartPole(max_steps=8), stubs[0], stubs[1], None, stubs[2], None, None, save_freq=1000)
    pipe.evaluator = ev
    ev.pipe = pipe
    return pipe, ev


def test_train_evaluates_on_the_right_epochs_and_keeps_the_best(tmp_path, monkeypatch):
    pipe, ev = _pipeline(tmp_path, monkeypatch, [5.0, 3.0, 7.0, float("nan")])
    best = os.path.join(pipe.archive_path, "best")
    seen = []
    write = pipe._write_checkpoint
    pipe._write_checkpoint = lambda path: (seen.append((pipe.epochs_done, path)), write(path))
    pipe.train(9, eval_every=2)
    assert ev.at == [2, 4, 6, 8]                                                   # after every second epoch
    assert pipe.best_return == 7.0
    assert [(e, p) for e, p in seen if p == best] == [(2, best), (6, best)]        # only on improvement; NaN is none
    assert os.path.exists(os.path.join(best, "metadata.json"))
    rows = list(csv.reader(open(os.path.join(pipe.archive_path, "evaluation.csv"))))
    assert rows[0] == ["epoch", "cell", "mass"] + list(tg.Pipeline.EVAL_COLUMNS)
    assert len(rows) == 1 + 4 * 2                                                  # one row per epoch x cell
    assert [r[0] for r in rows[1:]] == ["2", "2", "4", "4", "6", "6", "8", "8"] and [r[1] for r in rows[1:3]] == ["0", "1"]
    assert [float(r[2]) for r in rows[1:3]] == [0.8, 1.25] and float(rows[1][4]) == 5.0 and float(rows[2][4]) == 6.0
    # a later train() goes on counting epochs, and an equal score is no improvement
    ev.scores += [7.0]
    pipe.train(1, eval_every=1)
    assert ev.at[-1] == 10 and [e for e, p in seen if p == best] == [2, 6]


def test_train_without_eval_every_never_evaluates(tmp_path, monkeypatch):
    pipe, ev = _pipeline(tmp_path, monkeypatch, [])
    pipe.train(3)
    pipe.train(2, eval_every=None)
    assert ev.at == [] and pipe.epochs_done == 5 and pipe.best_return is None
    assert not os.path.exists(os.path.join(pipe.archive_path, "evaluation.csv"))
    assert not os.path.exists(os.path.join(pipe.archive_path, "best"))
    for bad in (0, -2, 1.5, True, "3"):
        with pytest.raises(ValueError, match="eval_every"):
            pipe.train(1, eval_every=bad)
    res = pipe.evaluator
    ev.scores = [1.0]
    out = pipe.evaluate()                                                          # on its own: returns the result, writes the table
    assert out.summary["return_mean"] == 1.0 and os.path.exists(os.path.join(pipe.archive_path, "evaluation.csv"))
