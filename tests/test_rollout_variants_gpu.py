"""The wiring of the env variants on the MI355X (run with `-m gpu`): every rollout kernel family launches one of eight instantiations
-- the plain env, PerEnv<> with a parameter table, Substepped<> through a `_sub` entry, ObsNormed<> with an observation-normalisation
table (the fused families only), and their nestings -- chosen on the host from what the entry point was handed.

For each variant V and each wrapper w in V, with the other wrappers' inputs non-trivial (a table that differs from env to env,
statistics that are not the identity, k = 2):
  * V with w's input non-trivial must DIFFER from V with w's input trivial (a uniform table, identity statistics, k = 1): w's input
    does reach the kernel;
  * V with w's input trivial must equal V-without-w BIT FOR BIT: whole buffers (obs, act, rew, mask, len), filled with NaN / 0xFF
    before each run.
Chained over the wrappers this holds every variant to the plain kernel, which the sibling suites pin to the reference.

Per-step families (step: teacher-forced and sampling with sigma = 0; forced; final_state): the three envs with substeps, f32 and
f64, n = 65 (one full wave and one lane; the speculative arm), T = 6, and one f32 case at n = 2^18 + 64, T = 2 (the other arm, 256
threads per block).  Fused bf16: QuadPole, H = 128, one hidden layer, n = 65 (4 waves) and n = 32768 (8 waves).  Fused fp32:
QuadPole, H = 64, one hidden layer, n = 65, 16 and 32 envs per workgroup."""
import ctypes as C
import itertools

import pytest
import torch

import substeps_ref as SR
from test_fused_rollout_fp64 import f32_policy

pytestmark = pytest.mark.gpu

DTYPES = {"f32": torch.float32, "f64": torch.float64}
NONTRIVIAL = {"table": "varied", "k": 2, "on": "real"}
TRIVIAL = {"table": "uniform", "k": 1, "on": "identity"}
KEYS = ("obs", "act", "rew", "mask", "len")


@pytest.fixture(scope="module")
def tg():
    import trajopt_grpo_amd as tg
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return tg


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


# ------------------------------------------------------------------------------------------------------------------------------
# inputs, made once per shape and left unchanged
# ------------------------------------------------------------------------------------------------------------------------------
_INPUTS = {}


def params(tg, name, T, k):
    """k None: the plain entries' params (max_steps = T); else the physics clock's of a `_sub` entry (max_steps = T k)."""
    env = tg.environments.ENV_CLASSES[name](max_steps=T)
    if k is None:
        return env.native_params()
    env.substeps = k
    return env.physics_params()


def inputs(tg, dev, name, n, T):
    """s0 f64 [S][n]: the env's own resets, pushed along x at speeds spread over +-vmax (some episodes leave the bounds within T
    steps); actions f32 [A][T][n] in [-1.2, 1.2]; factors f64 [12][n] in [0.8, 1.25] (row by row, env by env)."""
    key = (name, n, T)
    if key not in _INPUTS:
        Nn, (S, A) = tg._native, SR.DIMS[name]
        p = params(tg, name, T, None)
        s0 = torch.empty(S, n, dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            Nn.check(Nn.load().tg_env_reset(C.byref(p), Nn.dtype_code(torch.float64), s0.data_ptr(), n, n, 12, 0, 0, 1, Nn.stream_ptr(dev)), "tg_env_reset")
        col, _, vmax = SR.PUSH[name]
        gen = torch.Generator().manual_seed(1234 + n + T)
        s0[col] = (torch.linspace(-vmax, vmax, n, dtype=torch.float64)[torch.randperm(n, generator=gen)]).to(dev)
        act = ((torch.rand(A, T, n, generator=gen) * 2.4 - 1.2).float()).to(dev)
        fac = (0.8 + 0.45 * torch.rand(12, n, generator=gen, dtype=torch.float64)).to(dev)
        torch.cuda.synchronize()
        _INPUTS[key] = (s0, act, fac)
    return _INPUTS[key]


def table_of(tg, dev, name, n, T, p, which):
    """None, or the f64 [12][n] parameter table: p's own values in every column (uniform), or scaled env by env (varied)."""
    if which is None:
        return None
    nominal = torch.tensor([float(v) for v in p.p], dtype=torch.float64, device=dev).reshape(12, 1)
    tab = nominal.repeat(1, n)
    if which == "varied":
        tab = tab * inputs(tg, dev, name, n, T)[2]
    return tab.contiguous()


def blank_traj(tg, dev, name, n, T, dtype, s0, act=None):
    """Slot 0 = s0, len = 0 (the kernels' own state), the given actions; everything a kernel is to write holds NaN / 0xFF."""
    S, A = SR.DIMS[name]
    tr = tg.rollout.DeviceTrajectory(S, A, T, n, 1, n, dtype, dev)
    tr.obs.fill_(float("nan"))
    tr.obs[:, 0, :].copy_(s0.to(dtype))
    tr.rew.fill_(float("nan"))
    tr.mask.fill_(0xFF)
    if act is None:
        tr.act.fill_(float("nan"))
    else:
        tr.act.copy_(act)
    return tr


def snap(tr):
    torch.cuda.synchronize()
    return {key: getattr(tr, key).clone() for key in KEYS}


def bits(x):
    return x.view({4: torch.int32, 8: torch.int64}[x.element_size()]) if x.is_floating_point() else x


def same(a, b):
    return all(a[key].dtype == b[key].dtype and torch.equal(bits(a[key]), bits(b[key])) for key in a)


def first_difference(a, b):
    return next((key for key in a if not torch.equal(bits(a[key]), bits(b[key]))), None)


def check_variants(run, wrappers):
    """The two properties of the module docstring, for every non-empty subset of `wrappers`; run(**inputs) -> {name: tensor},
    memoised: the run of V-without-w is the all-non-trivial run of the smaller variant."""
    memo = {}

    def cached(**kw):
        key = tuple(sorted(kw.items()))
        if key not in memo:
            memo[key] = run(**{w: kw.get(w) for w in wrappers})
        return memo[key]

    for size in range(1, len(wrappers) + 1):
        for V in itertools.combinations(wrappers, size):
            full = {w: NONTRIVIAL[w] for w in V}
            for w in V:
                trivial = cached(**{**full, w: TRIVIAL[w]})
                without = cached(**{x: v for x, v in full.items() if x != w})
                assert not same(cached(**full), trivial), f"variant {V}: the input of `{w}` does not reach the kernel"
                assert same(trivial, without), f"variant {V} with a trivial `{w}` against the variant without it: " \
                                               f"{first_difference(trivial, without)} differs"
    launched = {tuple(w for w, _ in key) for key in memo}               # every nesting, the plain kernel included, did run
    assert launched == {V for size in range(len(wrappers) + 1) for V in itertools.combinations(sorted(wrappers), size)}


# ------------------------------------------------------------------------------------------------------------------------------
# the per-step families
# ------------------------------------------------------------------------------------------------------------------------------
def entry_args(base, table, k):
    """(entry name, arguments between the params and the trajectory, arguments in front of the stream)."""
    if k is not None:
        return base + "_sub", (None if table is None else table.data_ptr(),), (k,)
    if table is not None:
        return base + "_dr", (table.data_ptr(),), ()
    return base, (), ()


def run_per_step(tg, dev, family, name, n, T, dtype, table, k):
    Nn, lib = tg._native, tg._native.load()
    S, A = SR.DIMS[name]
    s0, act, _ = inputs(tg, dev, name, n, T)
    p = params(tg, name, T, k)
    tab = table_of(tg, dev, name, n, T, p, table)
    st = Nn.stream_ptr(dev)
    with torch.cuda.device(dev):
        if family == "final_state":
            base = final_base(tg, dev, name, n, T, dtype)
            name_, head, tail = entry_args("tg_rollout_final_state", tab, k)
            s_final = torch.full((n, S), float("nan"), dtype=torch.float32, device=dev)
            timeout = torch.full((n,), 0xFF, dtype=torch.uint8, device=dev)
            Nn.check(getattr(lib, name_)(C.byref(p), *head, C.byref(base.native()), s_final.data_ptr(), timeout.data_ptr(), *tail, st), name_)
            torch.cuda.synchronize()
            return {"s_final": s_final, "timeout": timeout}
        sampled = family == "step_means"
        tr = blank_traj(tg, dev, name, n, T, dtype, s0, None if sampled else act)
        nat = tr.native()
        if family == "forced":
            name_, head, tail = entry_args("tg_rollout_forced", tab, k)
            Nn.check(getattr(lib, name_)(C.byref(p), *head, C.byref(nat), 0, T, *tail, st), name_)
        else:
            name_, head, tail = entry_args("tg_rollout_step", tab, k)
            zero = (C.c_float * A)(*([0.0] * A))
            rng = torch.tensor([7, 0], dtype=torch.int64, device=dev)
            for t in range(T):
                if sampled:                                              # sampling around the same actions with sigma = 0
                    mean = act[:, t, :].t().contiguous()
                    Nn.check(getattr(lib, name_)(C.byref(p), *head, C.byref(nat), t, mean.data_ptr(), A, zero, rng.data_ptr(), 0, *tail, st), name_)
                else:
                    Nn.check(getattr(lib, name_)(C.byref(p), *head, C.byref(nat), t, None, 0, None, None, 0, *tail, st), name_)
    return snap(tr)


_FINAL_BASE = {}


def final_base(tg, dev, name, n, T, dtype):
    """The recorded trajectory that every tg_rollout_final_state variant re-steps the last transition of: one plain forced run."""
    key = (name, n, T, dtype)
    if key not in _FINAL_BASE:
        Nn = tg._native
        s0, act, _ = inputs(tg, dev, name, n, T)
        tr = blank_traj(tg, dev, name, n, T, dtype, s0, act)
        Nn.check(Nn.load().tg_rollout_forced(C.byref(params(tg, name, T, None)), C.byref(tr.native()), 0, T, Nn.stream_ptr(dev)), "tg_rollout_forced")
        torch.cuda.synchronize()
        assert int(tr.len.min()) >= 1 and int(tr.len.max()) == T            # every episode has a last transition; some ran to the horizon
        assert T < 6 or bool((tr.len < T).any())                            # ... and some left the bounds before it
        _FINAL_BASE[key] = tr
    return _FINAL_BASE[key]


@pytest.mark.parametrize("family", ["step_forced", "step_means", "forced", "final_state"])
@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("name", SR.ENVS)
def test_per_step_variants(tg, dev, name, dt, family):
    n, T = 65, 6
    check_variants(lambda table, k: run_per_step(tg, dev, family, name, n, T, DTYPES[dt], table, k), ("table", "k"))


@pytest.mark.parametrize("family", ["step_forced", "step_means", "final_state"])
def test_per_step_variants_past_the_speculative_limit(tg, dev, family):
    """n > 2^18: the kernels' non-speculative arm and 256 threads per block (tg_rollout_forced always runs 64)."""
    n, T = (1 << 18) + 64, 2
    check_variants(lambda table, k: run_per_step(tg, dev, family, "QuadPole", n, T, torch.float32, table, k), ("table", "k"))


# ------------------------------------------------------------------------------------------------------------------------------
# the fused families
# ------------------------------------------------------------------------------------------------------------------------------
_POLICY = {}


def fused_setup(tg, dev, kind, block):
    """(policy, weight stream) of the smallest net a fused kernel takes: one hidden layer of 128 (bf16) or 64 (fp32)."""
    key = (kind, block)
    if key not in _POLICY:
        H = 128 if kind == "bf16" else 64
        pol = f32_policy(tg, 20, 4, (H,), dev, seed=13)
        M = tg.mlp
        frag = M.FragmentStream(pol.actor, H) if kind == "bf16" else M.RegisterStreamF32(pol.actor, H, block)
        frag.refresh()
        _POLICY[key] = (pol, frag, H)
    return _POLICY[key]


def obs_norm_table(dev, which, S=20):
    """None, or (f32 [2][S] = {mean, rstd}, clip): the identity (mean 0, rstd 1, no clamp), or statistics that move every feature."""
    if which is None:
        return None
    if which == "identity":
        return torch.cat([torch.zeros(S), torch.ones(S)]).float().to(dev), float("inf")
    gen = torch.Generator().manual_seed(99)
    return torch.cat([0.3 * torch.randn(S, generator=gen), 0.5 + 1.5 * torch.rand(S, generator=gen)]).float().to(dev), 1.5


def run_fused(tg, dev, kind, block, n, T, table, k, on):
    Nn, lib = tg._native, tg._native.load()
    name = "QuadPole"
    pol, frag, H = fused_setup(tg, dev, kind, block)
    s0, _, _ = inputs(tg, dev, name, n, T)
    p = params(tg, name, T, k)
    tab = table_of(tg, dev, name, n, T, p, table)
    stats = obs_norm_table(dev, on)
    f32 = kind != "bf16"
    base = "tg_fused_rollout_f32" if f32 else "tg_fused_rollout"
    ptr = None if tab is None else tab.data_ptr()
    on_args = (None, 0.0) if stats is None else (stats[0].data_ptr(), stats[1])
    act_arg = (Nn.TG_ACT_RELU,) if f32 else ()
    if k is not None:
        entry, head, tail = base + "_sub", (ptr,), act_arg + on_args + (k,)
    elif stats is not None:
        entry, head, tail = base + "_on", (ptr,), act_arg + on_args
    elif tab is not None:
        entry, head, tail = base + "_dr", (ptr,), ()
    else:
        entry, head, tail = base, (), ()
    weights = (frag.table.data_ptr(), H, 1, block) if f32 else (frag.bias.data_ptr(), H, 1)
    sigma = (C.c_float * 4)(*[float(v) for v in torch.sqrt(pol.var)])
    rng = torch.tensor([21, 0], dtype=torch.int64, device=dev)
    tr = blank_traj(tg, dev, name, n, T, torch.float32, s0)
    with torch.cuda.device(dev):
        Nn.check(getattr(lib, entry)(C.byref(p), *head, C.byref(tr.native()), frag.stream.data_ptr(), *weights, sigma, rng.data_ptr(), 0, 0, T,
                                     *tail, Nn.stream_ptr(dev)), entry)
    return snap(tr)


@pytest.mark.parametrize("n,T", [(65, 6), (32768, 3)], ids=["4waves", "8waves"])
def test_fused_bf16_variants(tg, dev, n, T):
    check_variants(lambda table, k, on: run_fused(tg, dev, "bf16", None, n, T, table, k, on), ("table", "k", "on"))


@pytest.mark.parametrize("block", [16, 32])
def test_fused_f32_variants(tg, dev, block):
    check_variants(lambda table, k, on: run_fused(tg, dev, "f32", block, 65, 6, table, k, on), ("table", "k", "on"))
