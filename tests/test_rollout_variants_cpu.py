"""The refusals of the rollout entry points, host side (no GPU): for every entry of the per-step, fused bf16 and fused fp32 families --
plain, `_dr`, `_on`, `_act`, `_sub` -- a table of calls with ONE fault each, held to the exact return code and the exact
tg_last_error text.  Every refusal comes before any launch: the pointers below are never dereferenced.  A message raised in a family's
shared checks carries the plain entry's name also through `_dr`, `_on` and `_act`; the `_sub` entries carry their own."""
import ctypes as C

import pytest

import trajopt_grpo_amd as tg

N = tg._native
FAKE = 256
T, K, NENV = 8, 2, 4
OK, ARG, UNS = N.TG_OK, N.TG_ERR_ARG, N.TG_ERR_UNSUPPORTED

STEP = ["tg_rollout_step", "tg_rollout_step_dr", "tg_rollout_step_sub"]
FORCED = ["tg_rollout_forced", "tg_rollout_forced_dr", "tg_rollout_forced_sub"]
FINAL = ["tg_rollout_final_state", "tg_rollout_final_state_dr", "tg_rollout_final_state_sub"]
BF16 = ["tg_fused_rollout", "tg_fused_rollout_dr", "tg_fused_rollout_on", "tg_fused_rollout_sub"]
F32 = ["tg_fused_rollout_f32", "tg_fused_rollout_f32_act", "tg_fused_rollout_f32_dr", "tg_fused_rollout_f32_act_dr", "tg_fused_rollout_f32_on",
       "tg_fused_rollout_f32_sub"]
ENTRIES = STEP + FORCED + FINAL + BF16 + F32


def has(name, what):
    """Which optional arguments an entry takes: 'table' (d_ptab), 'on' (d_obs_norm, clip), 'act' (activation), 'sub' (substeps)."""
    tail = name.rsplit("_", 1)[-1]
    return {"table": tail in ("dr", "on", "sub"), "on": tail in ("on", "sub") and name not in STEP + FORCED + FINAL,
            "act": name in F32 and ("_act" in name or tail in ("on", "sub")), "sub": tail == "sub"}[what]


def good(name):
    """The arguments of a call with no fault, by name.  A `_sub` entry gets the physics clock's params (max_steps = T K) and substeps K."""
    sub = has(name, "sub")
    a = {"p": tg.QuadPole(max_steps=T * K if sub else T).native_params(), "tr": N.Traj(), "table": FAKE, "t": 0, "d_mean": None, "stride": 0,
         "sigma": (C.c_float * 4)(0.1, 0.1, 0.1, 0.1), "rng": FAKE, "t_begin": 0, "t_end": T, "d_s_final": FAKE, "d_timeout": FAKE,
         "weights": FAKE, "bias": FAKE, "hidden": 128, "layers": 2, "block": 32, "act": N.TG_ACT_RELU, "on": FAKE, "clip": 5.0, "substeps": K}
    tr = a["tr"]
    tr.d_obs = tr.d_act = tr.d_rew = tr.d_mask = tr.d_len = tr.d_counters = FAKE
    tr.n, tr.horizon, tr.dtype = NENV, T, N.TG_F32
    return a


def call(name, a):
    lib = N.load()
    p = None if a["p"] is None else C.byref(a["p"])
    head = (p,) + ((a["table"],) if has(name, "table") else ()) + (C.byref(a["tr"]),)
    tail = ((a["substeps"],) if has(name, "sub") else ()) + (None,)
    if name in STEP:
        args = head + (a["t"], a["d_mean"], a["stride"], a["sigma"], a["rng"], 0) + tail
    elif name in FORCED:
        args = head + (a["t_begin"], a["t_end"]) + tail
    elif name in FINAL:
        args = head + (a["d_s_final"], a["d_timeout"]) + tail
    else:
        on = (a["on"], a["clip"]) if has(name, "on") else ()
        act = (a["act"],) if has(name, "act") else ()
        block = (a["block"],) if name in F32 else ()
        args = head + (a["weights"], a["bias"], a["hidden"], a["layers"]) + block + (a["sigma"], a["rng"], 0, a["t_begin"], a["t_end"]) + act + on + tail
    rc = getattr(lib, name)(*args)
    return rc, (None if rc == OK else lib.tg_last_error().decode())


def _set(**kw):
    return lambda a: a.update(kw)


def _traj(**kw):
    def f(a):
        for key, val in kw.items():
            setattr(a["tr"], key, val)
    return f


def _params(**kw):
    def f(a):
        for key, val in kw.items():
            setattr(a["p"], key, val)
    return f


def _pendulum(a):
    a["p"] = tg.Pendulum(max_steps=a["p"].max_steps).native_params()


def _agents_32_in_blocks_of_16(a):
    a["p"].agents, a["block"], a["tr"].n = 32, 16, 32


def _sampling(**kw):
    def f(a):
        a.update(d_mean=FAKE, stride=4)
        a.update(kw)
    return f


# fault -> (the entries it applies to, what it does to the arguments of good())
EVERY, SUBS = ENTRIES, [e for e in ENTRIES if has(e, "sub")]
FUSED = BF16 + F32
FAULTS = {
    "null params": (EVERY, _set(p=None)),
    "null trajectory buffer": (EVERY, _traj(d_act=None)),
    "null table": ([e for e in ENTRIES if e.endswith("_dr")], _set(table=None)),
    "null output": (FINAL, _set(d_timeout=None)),
    "null weights": (FUSED, _set(weights=None)),
    "null obs-norm table": ([e for e in FUSED if e.endswith("_on")], _set(on=None)),
    "no envs": (EVERY, _traj(n=0)),
    "f64 trajectory": (FUSED, _traj(dtype=N.TG_F64)),
    "unknown dtype": (STEP + FORCED + FINAL, _traj(dtype=7)),
    "t negative": (STEP, _set(t=-1)),
    "t at the horizon": (STEP, _set(t=T)),
    "range starts below 0": (FORCED + FUSED, _set(t_begin=-1)),
    "range runs backwards": (FORCED + FUSED, _set(t_begin=5, t_end=4)),
    "range ends past the horizon": (FORCED + FUSED, _set(t_end=T + 1)),
    "horizon mismatch": (EVERY, _traj(horizon=T + 1)),
    "sampling without sigma": (STEP, _sampling(sigma=None)),
    "sampling without rng": (STEP, _sampling(rng=None)),
    "mean rows too short": (STEP, _sampling(stride=3)),
    "clip zero": ([e for e in FUSED if has(e, "on")], _set(clip=0.0)),
    "clip negative": ([e for e in FUSED if has(e, "on")], _set(clip=-2.5)),
    "substeps zero": (SUBS, _set(substeps=0)),
    "substeps 65": (SUBS, _set(substeps=65)),
    "substeps of another clock": (SUBS, _set(substeps=K + 1)),
    "swarm": ([e for e in ENTRIES if e in FINAL + SUBS], _params(agents=4)),   # (a valid swarm elsewhere: NENV bodies of one env)
    "agents not a power of two": (EVERY, _params(agents=3)),
    "agents above the limit": (STEP + FORCED + FUSED, _params(agents=128)),
    "agents above block_envs": (F32, _agents_32_in_blocks_of_16),
    "pendulum through sub": (SUBS, _pendulum),
    "unknown env": (EVERY, _params(env_id=99)),
    "width not instantiated": (FUSED, _set(hidden=96)),
    "bf16 width on fp32": (F32, _set(hidden=256)),
    "no hidden layers": (FUSED, _set(layers=0)),
    "too many hidden layers": (FUSED, _set(layers=17)),
    "five hidden layers": (F32, _set(layers=5)),
    "unknown activation": ([e for e in F32 if has(e, "act")], _set(act=7)),
    "block_envs 8": (F32, _set(block=8)),
    "block_envs 64": (F32, _set(block=64)),
    # not faults: an empty step range launches nothing and succeeds
    "empty range at 0": (FORCED + FUSED, _set(t_begin=0, t_end=0)),
    "empty range at 3": (FORCED + FUSED, _set(t_begin=3, t_end=3)),
    "empty range at the horizon": (FORCED + FUSED, _set(t_begin=T, t_end=T)),
    "clip ignored without a table": (["tg_fused_rollout_sub", "tg_fused_rollout_f32_sub"], _set(on=None, clip=0.0, t_begin=2, t_end=2)),
}
CASES = [(entry, fault) for fault, (entries, _) in FAULTS.items() for entry in entries]

# Recorded from the library as it stood before the launches were unified: (return code, tg_last_error) of every case.
EXPECTED = {
    ('tg_rollout_step', 'null params'): (ARG, 'tg_rollout_step: null pointer'),
    ('tg_rollout_step_dr', 'null params'): (ARG, 'tg_rollout_step: null pointer'),
    ('tg_rollout_step_sub', 'null params'): (ARG, 'tg_rollout_step_sub: null pointer'),
    ('tg_rollout_forced', 'null params'): (ARG, 'tg_rollout_forced: null pointer'),
    ('tg_rollout_forced_dr', 'null params'): (ARG, 'tg_rollout_forced: null pointer'),
    ('tg_rollout_forced_sub', 'null params'): (ARG, 'tg_rollout_forced_sub: null pointer'),
    ('tg_rollout_final_state', 'null params'): (ARG, 'tg_rollout_final_state: null pointer'),
    ('tg_rollout_final_state_dr', 'null params'): (ARG, 'tg_rollout_final_state: null pointer'),
    ('tg_rollout_final_state_sub', 'null params'): (ARG, 'tg_rollout_final_state_sub: null pointer'),
    ('tg_fused_rollout', 'null params'): (ARG, 'tg_fused_rollout: null pointer'),
    ('tg_fused_rollout_dr', 'null params'): (ARG, 'tg_fused_rollout: null pointer'),
    ('tg_fused_rollout_on', 'null params'): (ARG, 'tg_fused_rollout: null pointer'),
    ('tg_fused_rollout_sub', 'null params'): (ARG, 'tg_fused_rollout_sub: null pointer'),
    ('tg_fused_rollout_f32', 'null params'): (ARG, 'tg_fused_rollout_f32: null pointer'),
    ('tg_fused_rollout_f32_act', 'null params'): (ARG, 'tg_fused_rollout_f32: null pointer'),
    ('tg_fused_rollout_f32_dr', 'null params'): (ARG, 'tg_fused_rollout_f32: null pointer'),
    ('tg_fused_rollout_f32_act_dr', 'null params'): (ARG, 'tg_fused_rollout_f32: null pointer'),
    ('tg_fused_rollout_f32_on', 'null params'): (ARG, 'tg_fused_rollout_f32: null pointer'),
    ('tg_fused_rollout_f32_sub', 'null params'): (ARG, 'tg_fused_rollout_f32_sub: null pointer'),
    ('tg_rollout_step', 'null trajectory buffer'): (ARG, 'tg_rollout_step: null pointer'),
    ('tg_rollout_step_dr', 'null trajectory buffer'): (ARG, 'tg_rollout_step: null pointer'),
    ('tg_rollout_step_sub', 'null trajectory buffer'): (ARG, 'tg_rollout_step_sub: null pointer'),
    ('tg_rollout_forced', 'null trajectory buffer'): (ARG, 'tg_rollout_forced: null pointer'),
    ('tg_rollout_forced_dr', 'null trajectory buffer'): (ARG, 'tg_rollout_forced: null pointer'),
    ('tg_rollout_forced_sub', 'null trajectory buffer'): (ARG, 'tg_rollout_forced_sub: null pointer'),
    ('tg_rollout_final_state', 'null trajectory buffer'): (ARG, 'tg_rollout_final_state: null pointer'),
    ('tg_rollout_final_state_dr', 'null trajectory buffer'): (ARG, 'tg_rollout_final_state: null pointer'),
    ('tg_rollout_final_state_sub', 'null trajectory buffer'): (ARG, 'tg_rollout_final_state_sub: null pointer'),
    ('tg_fused_rollout', 'null trajectory buffer'): (ARG, 'tg_fused_rollout: null trajectory pointer'),
    ('tg_fused_rollout_dr', 'null trajectory buffer'): (ARG, 'tg_fused_rollout: null trajectory pointer'),
    ('tg_fused_rollout_on', 'null trajectory buffer'): (ARG, 'tg_fused_rollout: null trajectory pointer'),
    ('tg_fused_rollout_sub', 'null trajectory buffer'): (ARG, 'tg_fused_rollout_sub: null trajectory pointer'),
    ('tg_fused_rollout_f32', 'null trajectory buffer'): (ARG, 'tg_fused_rollout_f32: null trajectory pointer'),
    ('tg_fused_rollout_f32_act', 'null trajectory buffer'): (ARG, 'tg_fused_rollout_f32: null trajectory pointer'),
    ('tg_fused_rollout_f32_dr', 'null trajectory buffer'): (ARG, 'tg_fused_rollout_f32: null trajectory pointer'),
    ('tg_fused_rollout_f32_act_dr', 'null trajectory buffer'): (ARG, 'tg_fused_rollout_f32: null trajectory pointer'),
    ('tg_fused_rollout_f32_on', 'null trajectory buffer'): (ARG, 'tg_fused_rollout_f32: null trajectory pointer'),
    ('tg_fused_rollout_f32_sub', 'null trajectory buffer'): (ARG, 'tg_fused_rollout_f32_sub: null trajectory pointer'),
    ('tg_rollout_step_dr', 'null table'): (ARG, 'tg_rollout_step_dr: null parameter table'),
    ('tg_rollout_forced_dr', 'null table'): (ARG, 'tg_rollout_forced_dr: null parameter table'),
    ('tg_rollout_final_state_dr', 'null table'): (ARG, 'tg_rollout_final_state_dr: null parameter table'),
    ('tg_fused_rollout_dr', 'null table'): (ARG, 'tg_fused_rollout_dr: null parameter table'),
    ('tg_fused_rollout_f32_dr', 'null table'): (ARG, 'tg_fused_rollout_f32_dr: null parameter table'),
    ('tg_fused_rollout_f32_act_dr', 'null table'): (ARG, 'tg_fused_rollout_f32_act_dr: null parameter table'),
    ('tg_rollout_final_state', 'null output'): (ARG, 'tg_rollout_final_state: null pointer'),
    ('tg_rollout_final_state_dr', 'null output'): (ARG, 'tg_rollout_final_state: null pointer'),
    ('tg_rollout_final_state_sub', 'null output'): (ARG, 'tg_rollout_final_state_sub: null pointer'),
    ('tg_fused_rollout', 'null weights'): (ARG, 'tg_fused_rollout: null pointer'),
    ('tg_fused_rollout_dr', 'null weights'): (ARG, 'tg_fused_rollout: null pointer'),
    ('tg_fused_rollout_on', 'null weights'): (ARG, 'tg_fused_rollout: null pointer'),
    ('tg_fused_rollout_sub', 'null weights'): (ARG, 'tg_fused_rollout_sub: null pointer'),
    ('tg_fused_rollout_f32', 'null weights'): (ARG, 'tg_fused_rollout_f32: null pointer'),
    ('tg_fused_rollout_f32_act', 'null weights'): (ARG, 'tg_fused_rollout_f32: null pointer'),
    ('tg_fused_rollout_f32_dr', 'null weights'): (ARG, 'tg_fused_rollout_f32: null pointer'),
    ('tg_fused_rollout_f32_act_dr', 'null weights'): (ARG, 'tg_fused_rollout_f32: null pointer'),
    ('tg_fused_rollout_f32_on', 'null weights'): (ARG, 'tg_fused_rollout_f32: null pointer'),
    ('tg_fused_rollout_f32_sub', 'null weights'): (ARG, 'tg_fused_rollout_f32_sub: null pointer'),
    ('tg_fused_rollout_on', 'null obs-norm table'): (ARG, 'tg_fused_rollout_on: null observation-normalisation table'),
    ('tg_fused_rollout_f32_on', 'null obs-norm table'): (ARG, 'tg_fused_rollout_f32_on: null observation-normalisation table'),
    ('tg_rollout_step', 'no envs'): (ARG, 'tg_rollout_step: t=0 outside horizon 8'),
    ('tg_rollout_step_dr', 'no envs'): (ARG, 'tg_rollout_step: t=0 outside horizon 8'),
    ('tg_rollout_step_sub', 'no envs'): (ARG, 'tg_rollout_step_sub: t=0 outside horizon 8'),
    ('tg_rollout_forced', 'no envs'): (ARG, 'tg_rollout_forced: steps [0, 8) outside horizon 8'),
    ('tg_rollout_forced_dr', 'no envs'): (ARG, 'tg_rollout_forced: steps [0, 8) outside horizon 8'),
    ('tg_rollout_forced_sub', 'no envs'): (ARG, 'tg_rollout_forced_sub: steps [0, 8) outside horizon 8'),
    ('tg_rollout_final_state', 'no envs'): (ARG, 'tg_rollout_final_state: bad sizes n=0 T=8'),
    ('tg_rollout_final_state_dr', 'no envs'): (ARG, 'tg_rollout_final_state: bad sizes n=0 T=8'),
    ('tg_rollout_final_state_sub', 'no envs'): (ARG, 'tg_rollout_final_state_sub: bad sizes n=0 T=8'),
    ('tg_fused_rollout', 'no envs'): (ARG, 'tg_fused_rollout: horizon 8 != env.max_steps 8'),
    ('tg_fused_rollout_dr', 'no envs'): (ARG, 'tg_fused_rollout: horizon 8 != env.max_steps 8'),
    ('tg_fused_rollout_on', 'no envs'): (ARG, 'tg_fused_rollout: horizon 8 != env.max_steps 8'),
    ('tg_fused_rollout_sub', 'no envs'): (ARG, 'tg_fused_rollout_sub: bad step range [0, 8)'),
    ('tg_fused_rollout_f32', 'no envs'): (ARG, 'tg_fused_rollout_f32: horizon 8 != env.max_steps 8'),
    ('tg_fused_rollout_f32_act', 'no envs'): (ARG, 'tg_fused_rollout_f32: horizon 8 != env.max_steps 8'),
    ('tg_fused_rollout_f32_dr', 'no envs'): (ARG, 'tg_fused_rollout_f32: horizon 8 != env.max_steps 8'),
    ('tg_fused_rollout_f32_act_dr', 'no envs'): (ARG, 'tg_fused_rollout_f32: horizon 8 != env.max_steps 8'),
    ('tg_fused_rollout_f32_on', 'no envs'): (ARG, 'tg_fused_rollout_f32: horizon 8 != env.max_steps 8'),
    ('tg_fused_rollout_f32_sub', 'no envs'): (ARG, 'tg_fused_rollout_f32_sub: bad step range [0, 8)'),
    ('tg_fused_rollout', 'f64 trajectory'): (ARG, 'tg_fused_rollout: float32 trajectories only'),
    ('tg_fused_rollout_dr', 'f64 trajectory'): (ARG, 'tg_fused_rollout: float32 trajectories only'),
    ('tg_fused_rollout_on', 'f64 trajectory'): (ARG, 'tg_fused_rollout: float32 trajectories only'),
    ('tg_fused_rollout_sub', 'f64 trajectory'): (ARG, 'tg_fused_rollout_sub: float32 trajectories only'),
    ('tg_fused_rollout_f32', 'f64 trajectory'): (ARG, 'tg_fused_rollout_f32: float32 trajectories only'),
    ('tg_fused_rollout_f32_act', 'f64 trajectory'): (ARG, 'tg_fused_rollout_f32: float32 trajectories only'),
    ('tg_fused_rollout_f32_dr', 'f64 trajectory'): (ARG, 'tg_fused_rollout_f32: float32 trajectories only'),
    ('tg_fused_rollout_f32_act_dr', 'f64 trajectory'): (ARG, 'tg_fused_rollout_f32: float32 trajectories only'),
    ('tg_fused_rollout_f32_on', 'f64 trajectory'): (ARG, 'tg_fused_rollout_f32: float32 trajectories only'),
    ('tg_fused_rollout_f32_sub', 'f64 trajectory'): (ARG, 'tg_fused_rollout_f32_sub: float32 trajectories only'),
    ('tg_rollout_step', 'unknown dtype'): (UNS, 'unsupported env_id 2 / dtype 7'),
    ('tg_rollout_step_dr', 'unknown dtype'): (UNS, 'unsupported env_id 2 / dtype 7'),
    ('tg_rollout_step_sub', 'unknown dtype'): (UNS, 'unsupported env_id 2 / dtype 7'),
    ('tg_rollout_forced', 'unknown dtype'): (UNS, 'unsupported env_id 2 / dtype 7'),
    ('tg_rollout_forced_dr', 'unknown dtype'): (UNS, 'unsupported env_id 2 / dtype 7'),
    ('tg_rollout_forced_sub', 'unknown dtype'): (UNS, 'unsupported env_id 2 / dtype 7'),
    ('tg_rollout_final_state', 'unknown dtype'): (UNS, 'unsupported env_id 2 / dtype 7'),
    ('tg_rollout_final_state_dr', 'unknown dtype'): (UNS, 'unsupported env_id 2 / dtype 7'),
    ('tg_rollout_final_state_sub', 'unknown dtype'): (UNS, 'unsupported env_id 2 / dtype 7'),
    ('tg_rollout_step', 't negative'): (ARG, 'tg_rollout_step: t=-1 outside horizon 8'),
    ('tg_rollout_step_dr', 't negative'): (ARG, 'tg_rollout_step: t=-1 outside horizon 8'),
    ('tg_rollout_step_sub', 't negative'): (ARG, 'tg_rollout_step_sub: t=-1 outside horizon 8'),
    ('tg_rollout_step', 't at the horizon'): (ARG, 'tg_rollout_step: t=8 outside horizon 8'),
    ('tg_rollout_step_dr', 't at the horizon'): (ARG, 'tg_rollout_step: t=8 outside horizon 8'),
    ('tg_rollout_step_sub', 't at the horizon'): (ARG, 'tg_rollout_step_sub: t=8 outside horizon 8'),
    ('tg_rollout_forced', 'range starts below 0'): (ARG, 'tg_rollout_forced: steps [-1, 8) outside horizon 8'),
    ('tg_rollout_forced_dr', 'range starts below 0'): (ARG, 'tg_rollout_forced: steps [-1, 8) outside horizon 8'),
    ('tg_rollout_forced_sub', 'range starts below 0'): (ARG, 'tg_rollout_forced_sub: steps [-1, 8) outside horizon 8'),
    ('tg_fused_rollout', 'range starts below 0'): (ARG, 'tg_fused_rollout: bad step range [-1, 8)'),
    ('tg_fused_rollout_dr', 'range starts below 0'): (ARG, 'tg_fused_rollout: bad step range [-1, 8)'),
    ('tg_fused_rollout_on', 'range starts below 0'): (ARG, 'tg_fused_rollout: bad step range [-1, 8)'),
    ('tg_fused_rollout_sub', 'range starts below 0'): (ARG, 'tg_fused_rollout_sub: bad step range [-1, 8)'),
    ('tg_fused_rollout_f32', 'range starts below 0'): (ARG, 'tg_fused_rollout_f32: bad step range [-1, 8)'),
    ('tg_fused_rollout_f32_act', 'range starts below 0'): (ARG, 'tg_fused_rollout_f32: bad step range [-1, 8)'),
    ('tg_fused_rollout_f32_dr', 'range starts below 0'): (ARG, 'tg_fused_rollout_f32: bad step range [-1, 8)'),
    ('tg_fused_rollout_f32_act_dr', 'range starts below 0'): (ARG, 'tg_fused_rollout_f32: bad step range [-1, 8)'),
    ('tg_fused_rollout_f32_on', 'range starts below 0'): (ARG, 'tg_fused_rollout_f32: bad step range [-1, 8)'),
    ('tg_fused_rollout_f32_sub', 'range starts below 0'): (ARG, 'tg_fused_rollout_f32_sub: bad step range [-1, 8)'),
    ('tg_rollout_forced', 'range runs backwards'): (ARG, 'tg_rollout_forced: steps [5, 4) outside horizon 8'),
    ('tg_rollout_forced_dr', 'range runs backwards'): (ARG, 'tg_rollout_forced: steps [5, 4) outside horizon 8'),
    ('tg_rollout_forced_sub', 'range runs backwards'): (ARG, 'tg_rollout_forced_sub: steps [5, 4) outside horizon 8'),
    ('tg_fused_rollout', 'range runs backwards'): (ARG, 'tg_fused_rollout: bad step range [5, 4)'),
    ('tg_fused_rollout_dr', 'range runs backwards'): (ARG, 'tg_fused_rollout: bad step range [5, 4)'),
    ('tg_fused_rollout_on', 'range runs backwards'): (ARG, 'tg_fused_rollout: bad step range [5, 4)'),
    ('tg_fused_rollout_sub', 'range runs backwards'): (ARG, 'tg_fused_rollout_sub: bad step range [5, 4)'),
    ('tg_fused_rollout_f32', 'range runs backwards'): (ARG, 'tg_fused_rollout_f32: bad step range [5, 4)'),
    ('tg_fused_rollout_f32_act', 'range runs backwards'): (ARG, 'tg_fused_rollout_f32: bad step range [5, 4)'),
    ('tg_fused_rollout_f32_dr', 'range runs backwards'): (ARG, 'tg_fused_rollout_f32: bad step range [5, 4)'),
    ('tg_fused_rollout_f32_act_dr', 'range runs backwards'): (ARG, 'tg_fused_rollout_f32: bad step range [5, 4)'),
    ('tg_fused_rollout_f32_on', 'range runs backwards'): (ARG, 'tg_fused_rollout_f32: bad step range [5, 4)'),
    ('tg_fused_rollout_f32_sub', 'range runs backwards'): (ARG, 'tg_fused_rollout_f32_sub: bad step range [5, 4)'),
    ('tg_rollout_forced', 'range ends past the horizon'): (ARG, 'tg_rollout_forced: steps [0, 9) outside horizon 8'),
    ('tg_rollout_forced_dr', 'range ends past the horizon'): (ARG, 'tg_rollout_forced: steps [0, 9) outside horizon 8'),
    ('tg_rollout_forced_sub', 'range ends past the horizon'): (ARG, 'tg_rollout_forced_sub: steps [0, 9) outside horizon 8'),
    ('tg_fused_rollout', 'range ends past the horizon'): (ARG, 'tg_fused_rollout: bad step range [0, 9)'),
    ('tg_fused_rollout_dr', 'range ends past the horizon'): (ARG, 'tg_fused_rollout: bad step range [0, 9)'),
    ('tg_fused_rollout_on', 'range ends past the horizon'): (ARG, 'tg_fused_rollout: bad step range [0, 9)'),
    ('tg_fused_rollout_sub', 'range ends past the horizon'): (ARG, 'tg_fused_rollout_sub: bad step range [0, 9)'),
    ('tg_fused_rollout_f32', 'range ends past the horizon'): (ARG, 'tg_fused_rollout_f32: bad step range [0, 9)'),
    ('tg_fused_rollout_f32_act', 'range ends past the horizon'): (ARG, 'tg_fused_rollout_f32: bad step range [0, 9)'),
    ('tg_fused_rollout_f32_dr', 'range ends past the horizon'): (ARG, 'tg_fused_rollout_f32: bad step range [0, 9)'),
    ('tg_fused_rollout_f32_act_dr', 'range ends past the horizon'): (ARG, 'tg_fused_rollout_f32: bad step range [0, 9)'),
    ('tg_fused_rollout_f32_on', 'range ends past the horizon'): (ARG, 'tg_fused_rollout_f32: bad step range [0, 9)'),
    ('tg_fused_rollout_f32_sub', 'range ends past the horizon'): (ARG, 'tg_fused_rollout_f32_sub: bad step range [0, 9)'),
    ('tg_rollout_step', 'horizon mismatch'): (ARG, 'tg_rollout_step: trajectory horizon 9 != env.max_steps 8'),
    ('tg_rollout_step_dr', 'horizon mismatch'): (ARG, 'tg_rollout_step: trajectory horizon 9 != env.max_steps 8'),
    ('tg_rollout_step_sub', 'horizon mismatch'): (ARG, 'tg_rollout_step_sub: trajectory horizon 9 x substeps 2 != env.max_steps 16 (the params describe the physics clock)'),
    ('tg_rollout_forced', 'horizon mismatch'): (ARG, 'tg_rollout_forced: trajectory horizon 9 != env.max_steps 8'),
    ('tg_rollout_forced_dr', 'horizon mismatch'): (ARG, 'tg_rollout_forced: trajectory horizon 9 != env.max_steps 8'),
    ('tg_rollout_forced_sub', 'horizon mismatch'): (ARG, 'tg_rollout_forced_sub: trajectory horizon 9 x substeps 2 != env.max_steps 16 (the params describe the physics clock)'),
    ('tg_rollout_final_state', 'horizon mismatch'): (ARG, 'tg_rollout_final_state: trajectory horizon 9 != env.max_steps 8'),
    ('tg_rollout_final_state_dr', 'horizon mismatch'): (ARG, 'tg_rollout_final_state: trajectory horizon 9 != env.max_steps 8'),
    ('tg_rollout_final_state_sub', 'horizon mismatch'): (ARG, 'tg_rollout_final_state_sub: trajectory horizon 9 x substeps 2 != env.max_steps 16 (the params describe the physics clock)'),
    ('tg_fused_rollout', 'horizon mismatch'): (ARG, 'tg_fused_rollout: horizon 9 != env.max_steps 8'),
    ('tg_fused_rollout_dr', 'horizon mismatch'): (ARG, 'tg_fused_rollout: horizon 9 != env.max_steps 8'),
    ('tg_fused_rollout_on', 'horizon mismatch'): (ARG, 'tg_fused_rollout: horizon 9 != env.max_steps 8'),
    ('tg_fused_rollout_sub', 'horizon mismatch'): (ARG, 'tg_fused_rollout_sub: trajectory horizon 9 x substeps 2 != env.max_steps 16 (the params describe the physics clock)'),
    ('tg_fused_rollout_f32', 'horizon mismatch'): (ARG, 'tg_fused_rollout_f32: horizon 9 != env.max_steps 8'),
    ('tg_fused_rollout_f32_act', 'horizon mismatch'): (ARG, 'tg_fused_rollout_f32: horizon 9 != env.max_steps 8'),
    ('tg_fused_rollout_f32_dr', 'horizon mismatch'): (ARG, 'tg_fused_rollout_f32: horizon 9 != env.max_steps 8'),
    ('tg_fused_rollout_f32_act_dr', 'horizon mismatch'): (ARG, 'tg_fused_rollout_f32: horizon 9 != env.max_steps 8'),
    ('tg_fused_rollout_f32_on', 'horizon mismatch'): (ARG, 'tg_fused_rollout_f32: horizon 9 != env.max_steps 8'),
    ('tg_fused_rollout_f32_sub', 'horizon mismatch'): (ARG, 'tg_fused_rollout_f32_sub: trajectory horizon 9 x substeps 2 != env.max_steps 16 (the params describe the physics clock)'),
    ('tg_rollout_step', 'sampling without sigma'): (ARG, 'tg_rollout_step: sampling needs sigma and d_rng'),
    ('tg_rollout_step_dr', 'sampling without sigma'): (ARG, 'tg_rollout_step: sampling needs sigma and d_rng'),
    ('tg_rollout_step_sub', 'sampling without sigma'): (ARG, 'tg_rollout_step_sub: sampling needs sigma and d_rng'),
    ('tg_rollout_step', 'sampling without rng'): (ARG, 'tg_rollout_step: sampling needs sigma and d_rng'),
    ('tg_rollout_step_dr', 'sampling without rng'): (ARG, 'tg_rollout_step: sampling needs sigma and d_rng'),
    ('tg_rollout_step_sub', 'sampling without rng'): (ARG, 'tg_rollout_step_sub: sampling needs sigma and d_rng'),
    ('tg_rollout_step', 'mean rows too short'): (ARG, 'tg_rollout_step: mean_row_stride 3 < act_dim 4'),
    ('tg_rollout_step_dr', 'mean rows too short'): (ARG, 'tg_rollout_step: mean_row_stride 3 < act_dim 4'),
    ('tg_rollout_step_sub', 'mean rows too short'): (ARG, 'tg_rollout_step_sub: mean_row_stride 3 < act_dim 4'),
    ('tg_fused_rollout_on', 'clip zero'): (ARG, 'tg_fused_rollout_on: clip 0 (a number > 0; +inf: no clamp)'),
    ('tg_fused_rollout_sub', 'clip zero'): (ARG, 'tg_fused_rollout_sub: clip 0 (a number > 0; +inf: no clamp)'),
    ('tg_fused_rollout_f32_on', 'clip zero'): (ARG, 'tg_fused_rollout_f32_on: clip 0 (a number > 0; +inf: no clamp)'),
    ('tg_fused_rollout_f32_sub', 'clip zero'): (ARG, 'tg_fused_rollout_f32_sub: clip 0 (a number > 0; +inf: no clamp)'),
    ('tg_fused_rollout_on', 'clip negative'): (ARG, 'tg_fused_rollout_on: clip -2.5 (a number > 0; +inf: no clamp)'),
    ('tg_fused_rollout_sub', 'clip negative'): (ARG, 'tg_fused_rollout_sub: clip -2.5 (a number > 0; +inf: no clamp)'),
    ('tg_fused_rollout_f32_on', 'clip negative'): (ARG, 'tg_fused_rollout_f32_on: clip -2.5 (a number > 0; +inf: no clamp)'),
    ('tg_fused_rollout_f32_sub', 'clip negative'): (ARG, 'tg_fused_rollout_f32_sub: clip -2.5 (a number > 0; +inf: no clamp)'),
    ('tg_rollout_step_sub', 'substeps zero'): (ARG, 'tg_rollout_step_sub: substeps=0 outside [1, 64]'),
    ('tg_rollout_forced_sub', 'substeps zero'): (ARG, 'tg_rollout_forced_sub: substeps=0 outside [1, 64]'),
    ('tg_rollout_final_state_sub', 'substeps zero'): (ARG, 'tg_rollout_final_state_sub: substeps=0 outside [1, 64]'),
    ('tg_fused_rollout_sub', 'substeps zero'): (ARG, 'tg_fused_rollout_sub: substeps=0 outside [1, 64]'),
    ('tg_fused_rollout_f32_sub', 'substeps zero'): (ARG, 'tg_fused_rollout_f32_sub: substeps=0 outside [1, 64]'),
    ('tg_rollout_step_sub', 'substeps 65'): (ARG, 'tg_rollout_step_sub: substeps=65 outside [1, 64]'),
    ('tg_rollout_forced_sub', 'substeps 65'): (ARG, 'tg_rollout_forced_sub: substeps=65 outside [1, 64]'),
    ('tg_rollout_final_state_sub', 'substeps 65'): (ARG, 'tg_rollout_final_state_sub: substeps=65 outside [1, 64]'),
    ('tg_fused_rollout_sub', 'substeps 65'): (ARG, 'tg_fused_rollout_sub: substeps=65 outside [1, 64]'),
    ('tg_fused_rollout_f32_sub', 'substeps 65'): (ARG, 'tg_fused_rollout_f32_sub: substeps=65 outside [1, 64]'),
    ('tg_rollout_step_sub', 'substeps of another clock'): (ARG, 'tg_rollout_step_sub: trajectory horizon 8 x substeps 3 != env.max_steps 16 (the params describe the physics clock)'),
    ('tg_rollout_forced_sub', 'substeps of another clock'): (ARG, 'tg_rollout_forced_sub: trajectory horizon 8 x substeps 3 != env.max_steps 16 (the params describe the physics clock)'),
    ('tg_rollout_final_state_sub', 'substeps of another clock'): (ARG, 'tg_rollout_final_state_sub: trajectory horizon 8 x substeps 3 != env.max_steps 16 (the params describe the physics clock)'),
    ('tg_fused_rollout_sub', 'substeps of another clock'): (ARG, 'tg_fused_rollout_sub: trajectory horizon 8 x substeps 3 != env.max_steps 16 (the params describe the physics clock)'),
    ('tg_fused_rollout_f32_sub', 'substeps of another clock'): (ARG, 'tg_fused_rollout_f32_sub: trajectory horizon 8 x substeps 3 != env.max_steps 16 (the params describe the physics clock)'),
    ('tg_rollout_step_sub', 'swarm'): (UNS, 'tg_rollout_step_sub: swarm envs (agents=4) are not supported: the bodies of an env would have to stop at the same physics step'),
    ('tg_rollout_forced_sub', 'swarm'): (UNS, 'tg_rollout_forced_sub: swarm envs (agents=4) are not supported: the bodies of an env would have to stop at the same physics step'),
    ('tg_rollout_final_state', 'swarm'): (UNS, "tg_rollout_final_state: swarm envs (agents=4) are not supported: a swarm episode ends when any of its bodies does, which a body's own final state does not tell"),
    ('tg_rollout_final_state_dr', 'swarm'): (UNS, "tg_rollout_final_state: swarm envs (agents=4) are not supported: a swarm episode ends when any of its bodies does, which a body's own final state does not tell"),
    ('tg_rollout_final_state_sub', 'swarm'): (UNS, 'tg_rollout_final_state_sub: swarm envs (agents=4) are not supported: the bodies of an env would have to stop at the same physics step'),
    ('tg_fused_rollout_sub', 'swarm'): (UNS, 'tg_fused_rollout_sub: swarm envs (agents=4) are not supported: the bodies of an env would have to stop at the same physics step'),
    ('tg_fused_rollout_f32_sub', 'swarm'): (UNS, 'tg_fused_rollout_f32_sub: swarm envs (agents=4) are not supported: the bodies of an env would have to stop at the same physics step'),
    ('tg_rollout_step', 'agents not a power of two'): (ARG, 'tg_rollout_step: agents=3 must be a power of two <= 64 dividing n'),
    ('tg_rollout_step_dr', 'agents not a power of two'): (ARG, 'tg_rollout_step: agents=3 must be a power of two <= 64 dividing n'),
    ('tg_rollout_step_sub', 'agents not a power of two'): (UNS, 'tg_rollout_step_sub: swarm envs (agents=3) are not supported: the bodies of an env would have to stop at the same physics step'),
    ('tg_rollout_forced', 'agents not a power of two'): (ARG, 'tg_rollout_forced: agents=3 must be a power of two <= 64 dividing n'),
    ('tg_rollout_forced_dr', 'agents not a power of two'): (ARG, 'tg_rollout_forced: agents=3 must be a power of two <= 64 dividing n'),
    ('tg_rollout_forced_sub', 'agents not a power of two'): (UNS, 'tg_rollout_forced_sub: swarm envs (agents=3) are not supported: the bodies of an env would have to stop at the same physics step'),
    ('tg_rollout_final_state', 'agents not a power of two'): (UNS, "tg_rollout_final_state: swarm envs (agents=3) are not supported: a swarm episode ends when any of its bodies does, which a body's own final state does not tell"),
    ('tg_rollout_final_state_dr', 'agents not a power of two'): (UNS, "tg_rollout_final_state: swarm envs (agents=3) are not supported: a swarm episode ends when any of its bodies does, which a body's own final state does not tell"),
    ('tg_rollout_final_state_sub', 'agents not a power of two'): (UNS, 'tg_rollout_final_state_sub: swarm envs (agents=3) are not supported: the bodies of an env would have to stop at the same physics step'),
    ('tg_fused_rollout', 'agents not a power of two'): (ARG, 'tg_fused_rollout: agents=3 must be a power of two <= 32 dividing n'),
    ('tg_fused_rollout_dr', 'agents not a power of two'): (ARG, 'tg_fused_rollout: agents=3 must be a power of two <= 32 dividing n'),
    ('tg_fused_rollout_on', 'agents not a power of two'): (ARG, 'tg_fused_rollout: agents=3 must be a power of two <= 32 dividing n'),
    ('tg_fused_rollout_sub', 'agents not a power of two'): (UNS, 'tg_fused_rollout_sub: swarm envs (agents=3) are not supported: the bodies of an env would have to stop at the same physics step'),
    ('tg_fused_rollout_f32', 'agents not a power of two'): (ARG, 'tg_fused_rollout_f32: agents=3 must be a power of two <= 32 dividing n'),
    ('tg_fused_rollout_f32_act', 'agents not a power of two'): (ARG, 'tg_fused_rollout_f32: agents=3 must be a power of two <= 32 dividing n'),
    ('tg_fused_rollout_f32_dr', 'agents not a power of two'): (ARG, 'tg_fused_rollout_f32: agents=3 must be a power of two <= 32 dividing n'),
    ('tg_fused_rollout_f32_act_dr', 'agents not a power of two'): (ARG, 'tg_fused_rollout_f32: agents=3 must be a power of two <= 32 dividing n'),
    ('tg_fused_rollout_f32_on', 'agents not a power of two'): (ARG, 'tg_fused_rollout_f32: agents=3 must be a power of two <= 32 dividing n'),
    ('tg_fused_rollout_f32_sub', 'agents not a power of two'): (UNS, 'tg_fused_rollout_f32_sub: swarm envs (agents=3) are not supported: the bodies of an env would have to stop at the same physics step'),
    ('tg_rollout_step', 'agents above the limit'): (ARG, 'tg_rollout_step: agents=128 must be a power of two <= 64 dividing n'),
    ('tg_rollout_step_dr', 'agents above the limit'): (ARG, 'tg_rollout_step: agents=128 must be a power of two <= 64 dividing n'),
    ('tg_rollout_step_sub', 'agents above the limit'): (UNS, 'tg_rollout_step_sub: swarm envs (agents=128) are not supported: the bodies of an env would have to stop at the same physics step'),
    ('tg_rollout_forced', 'agents above the limit'): (ARG, 'tg_rollout_forced: agents=128 must be a power of two <= 64 dividing n'),
    ('tg_rollout_forced_dr', 'agents above the limit'): (ARG, 'tg_rollout_forced: agents=128 must be a power of two <= 64 dividing n'),
    ('tg_rollout_forced_sub', 'agents above the limit'): (UNS, 'tg_rollout_forced_sub: swarm envs (agents=128) are not supported: the bodies of an env would have to stop at the same physics step'),
    ('tg_fused_rollout', 'agents above the limit'): (ARG, 'tg_fused_rollout: agents=128 must be a power of two <= 32 dividing n'),
    ('tg_fused_rollout_dr', 'agents above the limit'): (ARG, 'tg_fused_rollout: agents=128 must be a power of two <= 32 dividing n'),
    ('tg_fused_rollout_on', 'agents above the limit'): (ARG, 'tg_fused_rollout: agents=128 must be a power of two <= 32 dividing n'),
    ('tg_fused_rollout_sub', 'agents above the limit'): (UNS, 'tg_fused_rollout_sub: swarm envs (agents=128) are not supported: the bodies of an env would have to stop at the same physics step'),
    ('tg_fused_rollout_f32', 'agents above the limit'): (ARG, 'tg_fused_rollout_f32: agents=128 must be a power of two <= 32 dividing n'),
    ('tg_fused_rollout_f32_act', 'agents above the limit'): (ARG, 'tg_fused_rollout_f32: agents=128 must be a power of two <= 32 dividing n'),
    ('tg_fused_rollout_f32_dr', 'agents above the limit'): (ARG, 'tg_fused_rollout_f32: agents=128 must be a power of two <= 32 dividing n'),
    ('tg_fused_rollout_f32_act_dr', 'agents above the limit'): (ARG, 'tg_fused_rollout_f32: agents=128 must be a power of two <= 32 dividing n'),
    ('tg_fused_rollout_f32_on', 'agents above the limit'): (ARG, 'tg_fused_rollout_f32: agents=128 must be a power of two <= 32 dividing n'),
    ('tg_fused_rollout_f32_sub', 'agents above the limit'): (UNS, 'tg_fused_rollout_f32_sub: swarm envs (agents=128) are not supported: the bodies of an env would have to stop at the same physics step'),
    ('tg_fused_rollout_f32', 'agents above block_envs'): (ARG, 'tg_fused_rollout_f32: agents=32 must be a power of two <= 16 dividing n'),
    ('tg_fused_rollout_f32_act', 'agents above block_envs'): (ARG, 'tg_fused_rollout_f32: agents=32 must be a power of two <= 16 dividing n'),
    ('tg_fused_rollout_f32_dr', 'agents above block_envs'): (ARG, 'tg_fused_rollout_f32: agents=32 must be a power of two <= 16 dividing n'),
    ('tg_fused_rollout_f32_act_dr', 'agents above block_envs'): (ARG, 'tg_fused_rollout_f32: agents=32 must be a power of two <= 16 dividing n'),
    ('tg_fused_rollout_f32_on', 'agents above block_envs'): (ARG, 'tg_fused_rollout_f32: agents=32 must be a power of two <= 16 dividing n'),
    ('tg_fused_rollout_f32_sub', 'agents above block_envs'): (UNS, 'tg_fused_rollout_f32_sub: swarm envs (agents=32) are not supported: the bodies of an env would have to stop at the same physics step'),
    ('tg_rollout_step_sub', 'pendulum through sub'): (UNS, 'tg_rollout_step_sub: Pendulum is not supported: its balance terminal and the running count kept in len count single steps'),
    ('tg_rollout_forced_sub', 'pendulum through sub'): (UNS, 'tg_rollout_forced_sub: Pendulum is not supported: its balance terminal and the running count kept in len count single steps'),
    ('tg_rollout_final_state_sub', 'pendulum through sub'): (UNS, 'tg_rollout_final_state_sub: Pendulum is not supported: its balance terminal and the running count kept in len count single steps'),
    ('tg_fused_rollout_sub', 'pendulum through sub'): (UNS, 'tg_fused_rollout_sub: Pendulum is not supported: its balance terminal and the running count kept in len count single steps'),
    ('tg_fused_rollout_f32_sub', 'pendulum through sub'): (UNS, 'tg_fused_rollout_f32_sub: Pendulum is not supported: its balance terminal and the running count kept in len count single steps'),
    ('tg_rollout_step', 'unknown env'): (UNS, 'unsupported env_id 99 / dtype 0'),
    ('tg_rollout_step_dr', 'unknown env'): (UNS, 'unsupported env_id 99 / dtype 0'),
    ('tg_rollout_step_sub', 'unknown env'): (UNS, 'unsupported env_id 99 / dtype 0'),
    ('tg_rollout_forced', 'unknown env'): (UNS, 'unsupported env_id 99 / dtype 0'),
    ('tg_rollout_forced_dr', 'unknown env'): (UNS, 'unsupported env_id 99 / dtype 0'),
    ('tg_rollout_forced_sub', 'unknown env'): (UNS, 'unsupported env_id 99 / dtype 0'),
    ('tg_rollout_final_state', 'unknown env'): (UNS, 'unsupported env_id 99 / dtype 0'),
    ('tg_rollout_final_state_dr', 'unknown env'): (UNS, 'unsupported env_id 99 / dtype 0'),
    ('tg_rollout_final_state_sub', 'unknown env'): (UNS, 'unsupported env_id 99 / dtype 0'),
    ('tg_fused_rollout', 'unknown env'): (UNS, 'tg_fused_rollout: env 99 with hidden width 128 is not instantiated (widths 128 and 256)'),
    ('tg_fused_rollout_dr', 'unknown env'): (UNS, 'tg_fused_rollout: env 99 with hidden width 128 is not instantiated (widths 128 and 256)'),
    ('tg_fused_rollout_on', 'unknown env'): (UNS, 'tg_fused_rollout: env 99 with hidden width 128 is not instantiated (widths 128 and 256)'),
    ('tg_fused_rollout_sub', 'unknown env'): (UNS, 'tg_fused_rollout_sub: env 99 with hidden width 128 is not instantiated (widths 128 and 256)'),
    ('tg_fused_rollout_f32', 'unknown env'): (UNS, 'tg_fused_rollout_f32: env 99 is not instantiated'),
    ('tg_fused_rollout_f32_act', 'unknown env'): (UNS, 'tg_fused_rollout_f32: env 99 is not instantiated'),
    ('tg_fused_rollout_f32_dr', 'unknown env'): (UNS, 'tg_fused_rollout_f32: env 99 is not instantiated'),
    ('tg_fused_rollout_f32_act_dr', 'unknown env'): (UNS, 'tg_fused_rollout_f32: env 99 is not instantiated'),
    ('tg_fused_rollout_f32_on', 'unknown env'): (UNS, 'tg_fused_rollout_f32: env 99 is not instantiated'),
    ('tg_fused_rollout_f32_sub', 'unknown env'): (UNS, 'tg_fused_rollout_f32_sub: env 99 is not instantiated'),
    ('tg_fused_rollout', 'width not instantiated'): (UNS, 'tg_fused_rollout: env 2 with hidden width 96 is not instantiated (widths 128 and 256)'),
    ('tg_fused_rollout_dr', 'width not instantiated'): (UNS, 'tg_fused_rollout: env 2 with hidden width 96 is not instantiated (widths 128 and 256)'),
    ('tg_fused_rollout_on', 'width not instantiated'): (UNS, 'tg_fused_rollout: env 2 with hidden width 96 is not instantiated (widths 128 and 256)'),
    ('tg_fused_rollout_sub', 'width not instantiated'): (UNS, 'tg_fused_rollout_sub: env 2 with hidden width 96 is not instantiated (widths 128 and 256)'),
    ('tg_fused_rollout_f32', 'width not instantiated'): (UNS, 'tg_fused_rollout_f32: hidden width 96 with 2 hidden layers is not instantiated (widths 64 / 128, 1..4 hidden layers)'),
    ('tg_fused_rollout_f32_act', 'width not instantiated'): (UNS, 'tg_fused_rollout_f32: hidden width 96 with 2 hidden layers is not instantiated (widths 64 / 128, 1..4 hidden layers)'),
    ('tg_fused_rollout_f32_dr', 'width not instantiated'): (UNS, 'tg_fused_rollout_f32: hidden width 96 with 2 hidden layers is not instantiated (widths 64 / 128, 1..4 hidden layers)'),
    ('tg_fused_rollout_f32_act_dr', 'width not instantiated'): (UNS, 'tg_fused_rollout_f32: hidden width 96 with 2 hidden layers is not instantiated (widths 64 / 128, 1..4 hidden layers)'),
    ('tg_fused_rollout_f32_on', 'width not instantiated'): (UNS, 'tg_fused_rollout_f32: hidden width 96 with 2 hidden layers is not instantiated (widths 64 / 128, 1..4 hidden layers)'),
    ('tg_fused_rollout_f32_sub', 'width not instantiated'): (UNS, 'tg_fused_rollout_f32_sub: hidden width 96 with 2 hidden layers is not instantiated (widths 64 / 128, 1..4 hidden layers)'),
    ('tg_fused_rollout_f32', 'bf16 width on fp32'): (UNS, 'tg_fused_rollout_f32: hidden width 256 with 2 hidden layers is not instantiated (widths 64 / 128, 1..4 hidden layers)'),
    ('tg_fused_rollout_f32_act', 'bf16 width on fp32'): (UNS, 'tg_fused_rollout_f32: hidden width 256 with 2 hidden layers is not instantiated (widths 64 / 128, 1..4 hidden layers)'),
    ('tg_fused_rollout_f32_dr', 'bf16 width on fp32'): (UNS, 'tg_fused_rollout_f32: hidden width 256 with 2 hidden layers is not instantiated (widths 64 / 128, 1..4 hidden layers)'),
    ('tg_fused_rollout_f32_act_dr', 'bf16 width on fp32'): (UNS, 'tg_fused_rollout_f32: hidden width 256 with 2 hidden layers is not instantiated (widths 64 / 128, 1..4 hidden layers)'),
    ('tg_fused_rollout_f32_on', 'bf16 width on fp32'): (UNS, 'tg_fused_rollout_f32: hidden width 256 with 2 hidden layers is not instantiated (widths 64 / 128, 1..4 hidden layers)'),
    ('tg_fused_rollout_f32_sub', 'bf16 width on fp32'): (UNS, 'tg_fused_rollout_f32_sub: hidden width 256 with 2 hidden layers is not instantiated (widths 64 / 128, 1..4 hidden layers)'),
    ('tg_fused_rollout', 'no hidden layers'): (ARG, 'tg_fused_rollout: 0 hidden layers unsupported'),
    ('tg_fused_rollout_dr', 'no hidden layers'): (ARG, 'tg_fused_rollout: 0 hidden layers unsupported'),
    ('tg_fused_rollout_on', 'no hidden layers'): (ARG, 'tg_fused_rollout: 0 hidden layers unsupported'),
    ('tg_fused_rollout_sub', 'no hidden layers'): (ARG, 'tg_fused_rollout_sub: 0 hidden layers unsupported'),
    ('tg_fused_rollout_f32', 'no hidden layers'): (UNS, 'tg_fused_rollout_f32: hidden width 128 with 0 hidden layers is not instantiated (widths 64 / 128, 1..4 hidden layers)'),
    ('tg_fused_rollout_f32_act', 'no hidden layers'): (UNS, 'tg_fused_rollout_f32: hidden width 128 with 0 hidden layers is not instantiated (widths 64 / 128, 1..4 hidden layers)'),
    ('tg_fused_rollout_f32_dr', 'no hidden layers'): (UNS, 'tg_fused_rollout_f32: hidden width 128 with 0 hidden layers is not instantiated (widths 64 / 128, 1..4 hidden layers)'),
    ('tg_fused_rollout_f32_act_dr', 'no hidden layers'): (UNS, 'tg_fused_rollout_f32: hidden width 128 with 0 hidden layers is not instantiated (widths 64 / 128, 1..4 hidden layers)'),
    ('tg_fused_rollout_f32_on', 'no hidden layers'): (UNS, 'tg_fused_rollout_f32: hidden width 128 with 0 hidden layers is not instantiated (widths 64 / 128, 1..4 hidden layers)'),
    ('tg_fused_rollout_f32_sub', 'no hidden layers'): (UNS, 'tg_fused_rollout_f32_sub: hidden width 128 with 0 hidden layers is not instantiated (widths 64 / 128, 1..4 hidden layers)'),
    ('tg_fused_rollout', 'too many hidden layers'): (ARG, 'tg_fused_rollout: 17 hidden layers unsupported'),
    ('tg_fused_rollout_dr', 'too many hidden layers'): (ARG, 'tg_fused_rollout: 17 hidden layers unsupported'),
    ('tg_fused_rollout_on', 'too many hidden layers'): (ARG, 'tg_fused_rollout: 17 hidden layers unsupported'),
    ('tg_fused_rollout_sub', 'too many hidden layers'): (ARG, 'tg_fused_rollout_sub: 17 hidden layers unsupported'),
    ('tg_fused_rollout_f32', 'too many hidden layers'): (UNS, 'tg_fused_rollout_f32: hidden width 128 with 17 hidden layers is not instantiated (widths 64 / 128, 1..4 hidden layers)'),
    ('tg_fused_rollout_f32_act', 'too many hidden layers'): (UNS, 'tg_fused_rollout_f32: hidden width 128 with 17 hidden layers is not instantiated (widths 64 / 128, 1..4 hidden layers)'),
    ('tg_fused_rollout_f32_dr', 'too many hidden layers'): (UNS, 'tg_fused_rollout_f32: hidden width 128 with 17 hidden layers is not instantiated (widths 64 / 128, 1..4 hidden layers)'),
    ('tg_fused_rollout_f32_act_dr', 'too many hidden layers'): (UNS, 'tg_fused_rollout_f32: hidden width 128 with 17 hidden layers is not instantiated (widths 64 / 128, 1..4 hidden layers)'),
    ('tg_fused_rollout_f32_on', 'too many hidden layers'): (UNS, 'tg_fused_rollout_f32: hidden width 128 with 17 hidden layers is not instantiated (widths 64 / 128, 1..4 hidden layers)'),
    ('tg_fused_rollout_f32_sub', 'too many hidden layers'): (UNS, 'tg_fused_rollout_f32_sub: hidden width 128 with 17 hidden layers is not instantiated (widths 64 / 128, 1..4 hidden layers)'),
    ('tg_fused_rollout_f32', 'five hidden layers'): (UNS, 'tg_fused_rollout_f32: hidden width 128 with 5 hidden layers is not instantiated (widths 64 / 128, 1..4 hidden layers)'),
    ('tg_fused_rollout_f32_act', 'five hidden layers'): (UNS, 'tg_fused_rollout_f32: hidden width 128 with 5 hidden layers is not instantiated (widths 64 / 128, 1..4 hidden layers)'),
    ('tg_fused_rollout_f32_dr', 'five hidden layers'): (UNS, 'tg_fused_rollout_f32: hidden width 128 with 5 hidden layers is not instantiated (widths 64 / 128, 1..4 hidden layers)'),
    ('tg_fused_rollout_f32_act_dr', 'five hidden layers'): (UNS, 'tg_fused_rollout_f32: hidden width 128 with 5 hidden layers is not instantiated (widths 64 / 128, 1..4 hidden layers)'),
    ('tg_fused_rollout_f32_on', 'five hidden layers'): (UNS, 'tg_fused_rollout_f32: hidden width 128 with 5 hidden layers is not instantiated (widths 64 / 128, 1..4 hidden layers)'),
    ('tg_fused_rollout_f32_sub', 'five hidden layers'): (UNS, 'tg_fused_rollout_f32_sub: hidden width 128 with 5 hidden layers is not instantiated (widths 64 / 128, 1..4 hidden layers)'),
    ('tg_fused_rollout_f32_act', 'unknown activation'): (ARG, 'tg_fused_rollout_f32_act: unknown activation 7'),
    ('tg_fused_rollout_f32_act_dr', 'unknown activation'): (ARG, 'tg_fused_rollout_f32_act: unknown activation 7'),
    ('tg_fused_rollout_f32_on', 'unknown activation'): (ARG, 'tg_fused_rollout_f32_act: unknown activation 7'),
    ('tg_fused_rollout_f32_sub', 'unknown activation'): (ARG, 'tg_fused_rollout_f32_sub: unknown activation 7'),
    ('tg_fused_rollout_f32', 'block_envs 8'): (ARG, 'tg_fused_rollout_f32: 8 envs per workgroup (16 or 32: the layout of d_wstream)'),
    ('tg_fused_rollout_f32_act', 'block_envs 8'): (ARG, 'tg_fused_rollout_f32: 8 envs per workgroup (16 or 32: the layout of d_wstream)'),
    ('tg_fused_rollout_f32_dr', 'block_envs 8'): (ARG, 'tg_fused_rollout_f32: 8 envs per workgroup (16 or 32: the layout of d_wstream)'),
    ('tg_fused_rollout_f32_act_dr', 'block_envs 8'): (ARG, 'tg_fused_rollout_f32: 8 envs per workgroup (16 or 32: the layout of d_wstream)'),
    ('tg_fused_rollout_f32_on', 'block_envs 8'): (ARG, 'tg_fused_rollout_f32: 8 envs per workgroup (16 or 32: the layout of d_wstream)'),
    ('tg_fused_rollout_f32_sub', 'block_envs 8'): (ARG, 'tg_fused_rollout_f32_sub: 8 envs per workgroup (16 or 32: the layout of d_wstream)'),
    ('tg_fused_rollout_f32', 'block_envs 64'): (ARG, 'tg_fused_rollout_f32: 64 envs per workgroup (16 or 32: the layout of d_wstream)'),
    ('tg_fused_rollout_f32_act', 'block_envs 64'): (ARG, 'tg_fused_rollout_f32: 64 envs per workgroup (16 or 32: the layout of d_wstream)'),
    ('tg_fused_rollout_f32_dr', 'block_envs 64'): (ARG, 'tg_fused_rollout_f32: 64 envs per workgroup (16 or 32: the layout of d_wstream)'),
    ('tg_fused_rollout_f32_act_dr', 'block_envs 64'): (ARG, 'tg_fused_rollout_f32: 64 envs per workgroup (16 or 32: the layout of d_wstream)'),
    ('tg_fused_rollout_f32_on', 'block_envs 64'): (ARG, 'tg_fused_rollout_f32: 64 envs per workgroup (16 or 32: the layout of d_wstream)'),
    ('tg_fused_rollout_f32_sub', 'block_envs 64'): (ARG, 'tg_fused_rollout_f32_sub: 64 envs per workgroup (16 or 32: the layout of d_wstream)'),
    ('tg_rollout_forced', 'empty range at 0'): (OK, None),
    ('tg_rollout_forced_dr', 'empty range at 0'): (OK, None),
    ('tg_rollout_forced_sub', 'empty range at 0'): (OK, None),
    ('tg_fused_rollout', 'empty range at 0'): (OK, None),
    ('tg_fused_rollout_dr', 'empty range at 0'): (OK, None),
    ('tg_fused_rollout_on', 'empty range at 0'): (OK, None),
    ('tg_fused_rollout_sub', 'empty range at 0'): (OK, None),
    ('tg_fused_rollout_f32', 'empty range at 0'): (OK, None),
    ('tg_fused_rollout_f32_act', 'empty range at 0'): (OK, None),
    ('tg_fused_rollout_f32_dr', 'empty range at 0'): (OK, None),
    ('tg_fused_rollout_f32_act_dr', 'empty range at 0'): (OK, None),
    ('tg_fused_rollout_f32_on', 'empty range at 0'): (OK, None),
    ('tg_fused_rollout_f32_sub', 'empty range at 0'): (OK, None),
    ('tg_rollout_forced', 'empty range at 3'): (OK, None),
    ('tg_rollout_forced_dr', 'empty range at 3'): (OK, None),
    ('tg_rollout_forced_sub', 'empty range at 3'): (OK, None),
    ('tg_fused_rollout', 'empty range at 3'): (OK, None),
    ('tg_fused_rollout_dr', 'empty range at 3'): (OK, None),
    ('tg_fused_rollout_on', 'empty range at 3'): (OK, None),
    ('tg_fused_rollout_sub', 'empty range at 3'): (OK, None),
    ('tg_fused_rollout_f32', 'empty range at 3'): (OK, None),
    ('tg_fused_rollout_f32_act', 'empty range at 3'): (OK, None),
    ('tg_fused_rollout_f32_dr', 'empty range at 3'): (OK, None),
    ('tg_fused_rollout_f32_act_dr', 'empty range at 3'): (OK, None),
    ('tg_fused_rollout_f32_on', 'empty range at 3'): (OK, None),
    ('tg_fused_rollout_f32_sub', 'empty range at 3'): (OK, None),
    ('tg_rollout_forced', 'empty range at the horizon'): (OK, None),
    ('tg_rollout_forced_dr', 'empty range at the horizon'): (OK, None),
    ('tg_rollout_forced_sub', 'empty range at the horizon'): (OK, None),
    ('tg_fused_rollout', 'empty range at the horizon'): (OK, None),
    ('tg_fused_rollout_dr', 'empty range at the horizon'): (OK, None),
    ('tg_fused_rollout_on', 'empty range at the horizon'): (OK, None),
    ('tg_fused_rollout_sub', 'empty range at the horizon'): (OK, None),
    ('tg_fused_rollout_f32', 'empty range at the horizon'): (OK, None),
    ('tg_fused_rollout_f32_act', 'empty range at the horizon'): (OK, None),
    ('tg_fused_rollout_f32_dr', 'empty range at the horizon'): (OK, None),
    ('tg_fused_rollout_f32_act_dr', 'empty range at the horizon'): (OK, None),
    ('tg_fused_rollout_f32_on', 'empty range at the horizon'): (OK, None),
    ('tg_fused_rollout_f32_sub', 'empty range at the horizon'): (OK, None),
    ('tg_fused_rollout_sub', 'clip ignored without a table'): (OK, None),
    ('tg_fused_rollout_f32_sub', 'clip ignored without a table'): (OK, None),
}


def test_the_table_covers_every_entry_point_and_every_case_has_a_record():
    lib = N.load()
    assert len(ENTRIES) == len(set(ENTRIES)) == 19 and all(hasattr(lib, e) and e in N.SIGNATURES for e in ENTRIES)
    assert set(EXPECTED) == set(CASES)
    for entry in ENTRIES:
        assert sum(1 for e, _ in CASES if e == entry) >= 8, entry
    for entry in FUSED:
        assert EXPECTED[entry, "empty range at 3"] == (OK, None)
    codes = {rc for rc, _ in EXPECTED.values()}
    assert codes == {OK, ARG, UNS}                                      # nothing here reaches a launch (TG_ERR_HIP without a GPU)


def test_a_call_without_a_fault_is_what_the_faults_are_measured_from():
    """good() itself passes every check: with an empty range (the fused and forced entries) it returns TG_OK."""
    for entry in FORCED + FUSED:
        a = good(entry)
        a.update(t_begin=1, t_end=1)
        assert call(entry, a) == (OK, None), entry


@pytest.mark.parametrize("entry,fault", CASES, ids=[f"{e}-{f.replace(' ', '_')}" for e, f in CASES])
def test_single_fault(entry, fault):
    a = good(entry)
    FAULTS[fault][1](a)
    assert call(entry, a) == EXPECTED[entry, fault]
