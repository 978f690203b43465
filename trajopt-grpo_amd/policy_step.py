"""DeviceActor: the policy step of an RL loop on DeviceVecEnv as ONE kernel launch.

`act(obs)` runs the actor net, draws the action, computes its log-density and -- with a critic -- the value of the same rows in one
launch (tg_policy_step, csrc/policy_step.hip); `values(x)` is the critic alone on any rows (tg_policy_values), for
`V(info["final_obs"])` and the last value of a segment.  One collection step is then `act`, `venv.step`, `add`: three launches, all
of them capturable into one hipGraph.

The nets stay plain `torch.nn` modules that the caller trains with `torch.optim`: the kernel reads `nn.Linear.weight` / `.bias` where
torch keeps them, and the pointer tables are filled from `param.data_ptr()` at every call.  An in-place optimizer step or a
`param.data.copy_()` is therefore seen by the next call, outside a captured graph and inside one.  A parameter REBOUND to new storage
(`param.data = other`, `load_state_dict(assign=True)`) is seen by the next eager call but not by a graph captured before it.

With `q_nets` (one Q critic on [obs, action] rows, or SAC's twin pair) two more launches exist (csrc/policy_q.hip): `q_values(obs, act)`
gives q1, q2 and min(q1, q2) of any rows, and `sac_target(next_obs, reward, discount, alpha)` is the whole off-policy target
y = reward + discount * (min(Q1', Q2')(s', a') - alpha * logp(a'|s')) with a' drawn by the actor, in ONE launch: a wave runs the
actor and then both critics on its 16 rows and hands a' over in registers.

`evaluate(obs, action)` is the learner's side under the gaussian head (csrc/policy_grad.hip): log-density, entropy and value of stored
rows as ONE autograd node over log_std and the nets' own parameters, forward and backward in HIP, so any torch loss of the three
fills `.grad` and any torch.optim steps the nets.

`rsample(obs)` and `q_evaluate(obs, act)` are SAC's two gradient steps (csrc/policy_sac_grad.hip): act()'s squashed-head draw as an
autograd node over the actor's parameters (the reparameterised path, eps held constant), and q_values() as a node over the Q nets'
parameters and the action.  The critic update is q_evaluate(b_obs, b_act); the actor update is a, logp = rsample(b_obs) followed by
q_evaluate(b_obs, a, detach_params=True); torch.min, the losses and torch.optim stay the caller's.

Not built: gradients to observations, through evaluate()'s action, sac_target() or the gaussian head's draw, graph capture of a
backward, bf16, more than 4 actions, LayerNorm or mixed activations, a trunk shared by actor and critic, Q nets whose width or
activation differs from the actor's, more than two critics, a target for TD3 / DDPG heads.  There is no silent torch fallback: a net
outside the kernel's set raises ValueError with supports()'s reason, and the caller's own torch code is the fallback.
"""
from __future__ import annotations

import ctypes as C
import types

import torch

from . import _native as N
from . import mlp as M

MAX_OBS_DIM, MAX_HIDDEN_LAYERS, MAX_ACT_DIM = 32, 5, 4          # tg_policy_step_limits
WIDTHS = (64, 128, 256)
HEADS = {"gaussian": N.TG_POLICY_HEAD_GAUSSIAN, "squashed": N.TG_POLICY_HEAD_SQUASHED}
_ACT = {"ReLU": N.TG_ACT_RELU, "Tanh": N.TG_ACT_TANH}


def _modules(net):
    if isinstance(net, torch.nn.Sequential):
        return list(net)
    inner = getattr(net, "network", None)
    return list(inner) if inner is not None else None


def _shape(net, head):
    """-> ((S, H, hidden layers, O, activation), None) of a net the kernel takes under `head` ("gaussian", "squashed" or "value"),
    or (None, the reason)."""
    mods = _modules(net)
    if mods is None:
        return None, f"{type(net).__name__} is neither an nn.Sequential nor a module with a `.network` Sequential"
    if len(mods) < 3 or len(mods) % 2 == 0 or any(not isinstance(m, torch.nn.Linear) for m in mods[0::2]):
        return None, "the net is not Linear [activation Linear]+"
    act = M.hidden_activation(types.SimpleNamespace(network=mods))
    if act is None:
        kinds = sorted({type(m).__name__ for m in mods[1::2]})
        return None, (f"mixed hidden activations {kinds}: one of ReLU / Tanh after every hidden layer" if len(kinds) > 1 else
                      f"hidden activation {kinds[0]}: only ReLU and Tanh are built")
    lin = mods[0::2]
    S, H, nh, O = lin[0].in_features, lin[0].out_features, len(lin) - 1, lin[-1].out_features
    if any(l.out_features != H for l in lin[:-1]) or any(l.in_features != H for l in lin[1:]):
        return None, "the hidden layers differ in width"
    if H not in WIDTHS:
        return None, f"hidden width {H}: only {WIDTHS} are built"
    if nh > MAX_HIDDEN_LAYERS:
        return None, f"{nh} hidden layers: at most {MAX_HIDDEN_LAYERS}"
    if not 1 <= S <= MAX_OBS_DIM:
        return None, f"input width {S} outside [1, {MAX_OBS_DIM}]"
    if any(l.bias is None for l in lin):
        return None, "a Linear layer without a bias"
    if head == "gaussian" and not 1 <= O <= MAX_ACT_DIM:
        return None, f"{O} outputs under the gaussian head: 1..{MAX_ACT_DIM} actions"
    if head == "squashed" and (O % 2 or not 2 <= O <= 2 * MAX_ACT_DIM):
        return None, f"{O} outputs under the squashed head: (mean, log-std) pairs of 1..{MAX_ACT_DIM} actions, so an even count <= {2 * MAX_ACT_DIM}"
    if head == "value" and O != 1:
        return None, f"{O} outputs of a critic: 1"
    if head == "q" and O != 1:
        return None, f"{O} outputs of a Q critic: 1"
    if head == "q" and S < 2:
        return None, f"input width {S} of a Q critic: at least one observation and one action"
    if head not in ("gaussian", "squashed", "value", "q"):
        return None, f"unknown head {head!r}"
    return (S, H, nh, O, act), None


def _widths(net):
    """tg_policy_net of `net` with the widths alone (no pointers)."""
    lin = _modules(net)[0::2]
    t = N.PolicyNet()
    t.n_layers = len(lin)
    t.activation = _ACT[M.hidden_activation(types.SimpleNamespace(network=_modules(net)))]
    for l, m in enumerate(lin):
        t.in_dim[l], t.out_dim[l] = m.in_features, m.out_features
    return t


def _q_refusal(actor_net, actor_shape, head, q_nets):
    """None if q_values() and (with a pair) sac_target() take `q_nets` beside the actor, else the reason.  What the nets must share is
    compared here; whether their tables and the weight ring fit in LDS is the library's verdict (tg_policy_q_fits)."""
    S, H, _, O, act = actor_shape
    A = O // 2
    if head != "squashed":
        return f"q_nets go with the squashed head (SAC's actor), not {head!r}"
    if not 1 <= len(q_nets) <= 2:
        return f"{len(q_nets)} Q nets: one, or a twin pair"
    for k, q in enumerate(q_nets, 1):
        shape, why = _shape(q, "q")
        if shape is None:
            return f"Q{k} is not supported: {why}"
        if shape[1] != H or shape[4] != act:
            return f"Q{k} is {shape[1]} wide with {shape[4]}, the actor {H} wide with {act}: one kernel body runs all three nets"
        if shape[0] != S + A:
            return f"Q{k} reads {shape[0]} inputs, the actor gives {S} observations + {A} actions"
    lib = N.load()
    tables = [_widths(q) for q in q_nets]
    forms = [(None, *tables, *([None] * (2 - len(tables))))]
    if len(tables) == 2:
        forms.append((_widths(actor_net), *tables))
    for actor, q1, q2 in forms:
        if lib.tg_policy_q_fits(C.byref(actor) if actor is not None else None, C.byref(q1), C.byref(q2) if q2 is not None else None, A):
            return lib.tg_last_error().decode("utf-8", "replace")
    return None


def _grad_views(flat, params):
    """The parameters' gradients as views of `flat` (one buffer per net: weight [out][in], bias [out], layer by layer)."""
    grads, at, net = [], 0, 0
    for p in params:
        if at == flat[net].numel():
            at, net = 0, net + 1
        grads.append(flat[net][at:at + p.numel()].view(p.shape))
        at += p.numel()
    return grads


class _Evaluate(torch.autograd.Function):
    """DeviceActor.evaluate as ONE autograd node over log_std and every weight / bias of both nets (csrc/policy_grad.hip): forward
    is tg_policy_eval_forward; backward is tg_policy_eval_backward, tg_policy_eval_weight_grad and tg_log_std_grad, and returns the
    gradients in torch's own shapes (views of one fresh buffer per net), so .grad accumulation, zero_grad, clip_grad_norm_ and any
    torch.optim work unchanged.  The parameters are saved tensors: torch itself refuses a backward() after an in-place step."""

    @staticmethod
    def forward(ctx, da, obs, action, log_std, *params):
        if log_std.dtype != torch.float32 or not log_std.is_contiguous() or log_std.device != da.device:
            raise ValueError(f"DeviceActor: log_std must be a contiguous float32 tensor on {da.device}")
        m = obs.shape[0]
        ws = da._eval_workspace(m)
        out = [torch.empty(m, dtype=torch.float32, device=da.device) for _ in range(3 if da.critic_net is not None else 2)]
        s = da._eval_args(ws, obs, action, log_std.detach(), out[0], out[1], out[2] if len(out) == 3 else None)
        actor, critic, _keep = da._eval_tables()
        with torch.cuda.device(da.device):
            N.check(da.lib.tg_policy_eval_forward(actor, critic, C.byref(s), N.stream_ptr(da.device)), "tg_policy_eval_forward")
        if any(ctx.needs_input_grad):
            ctx.da, ctx.ws = da, ws                                            # (tests/test_policy_grad_gpu.py reads ws.mu off the node)
            ctx.save_for_backward(obs, action, log_std, *params)
        else:
            da._eval_pool[m].append(ws)                                        # (no backward will come for it)
        return tuple(out)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *g):
        from . import hip_ops as K
        da, ws = ctx.da, ctx.ws
        if ws is None:
            raise RuntimeError("DeviceActor: this evaluate() was already backpropagated (its activations are gone)")
        obs, action, log_std, *params = ctx.saved_tensors
        m, dev = ws.m, da.device
        g = [torch.zeros(m, dtype=torch.float32, device=dev) if t is None else t.contiguous() for t in g]
        s = da._eval_args(ws, obs, action, log_std.detach(), None, None, None)
        s.d_g_logp, s.d_g_entropy, s.d_g_value = g[0].data_ptr(), g[1].data_ptr(), (g[2].data_ptr() if len(g) == 3 else 0)
        flat = [torch.empty(k, dtype=torch.float32, device=dev) if k else None for k in ws.grad_floats]
        s.d_grad_actor, s.d_grad_critic = (N.ptr(t) for t in flat)
        actor, critic, _keep = da._eval_tables()
        g_std = torch.zeros(da.A, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            N.check(da.lib.tg_policy_eval_backward(actor, critic, C.byref(s), N.stream_ptr(dev)), "tg_policy_eval_backward")
            N.check(da.lib.tg_policy_eval_weight_grad(actor, critic, C.byref(s), N.stream_ptr(dev)), "tg_policy_eval_weight_grad")
            K.log_std_grad(ws.std_rows, da.A, g_std)
        ctx.ws = None
        da._eval_pool[m].append(ws)
        return (None, None, None, g_std, *_grad_views(flat, params))


def _consumed(ctx, what):
    if ctx.ws is None:
        raise RuntimeError(f"DeviceActor: this {what}() was already backpropagated (its activations are gone)")
    return ctx.da, ctx.ws


class _RSample(torch.autograd.Function):
    """DeviceActor.rsample as ONE autograd node over the actor's weights and biases (csrc/policy_sac_grad.hip): forward is
    tg_policy_rsample_forward; backward is tg_policy_rsample_backward and the actor's tg_policy_sac_weight_grad."""

    @staticmethod
    def forward(ctx, da, grad_mode, obs, *params):
        n, dev = da.num_envs, da.device
        ws = da._sac_workspace("actor", n)
        action, logp = torch.empty(n, da.A, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.float32, device=dev)
        s = da._sac_args(ws, obs)
        s.d_action, s.d_logp, s.d_eps, s.d_calls = action.data_ptr(), logp.data_ptr(), da.eps.data_ptr(), da._calls.data_ptr()
        actor = da._table(da.actor_net, "the actor")
        with torch.cuda.device(dev):
            N.check(da.lib.tg_policy_rsample_forward(C.byref(actor), C.byref(s), N.stream_ptr(dev)), "tg_policy_rsample_forward")
        if grad_mode and any(ctx.needs_input_grad):                            # (needs_input_grad alone ignores torch.no_grad())
            ctx.da, ctx.ws = da, ws
            ctx.save_for_backward(obs, action, *params)
        else:
            da._sac_pool[("actor", n)].append(ws)                              # (no backward will come for it)
        return action, logp

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_action, g_logp):
        da, ws = _consumed(ctx, "rsample")
        obs, action, *params = ctx.saved_tensors
        n, dev = ws.m, da.device
        g_action = torch.zeros(n, da.A, dtype=torch.float32, device=dev) if g_action is None else g_action.contiguous()
        g_logp = torch.zeros(n, dtype=torch.float32, device=dev) if g_logp is None else g_logp.contiguous()
        flat = [torch.empty(ws.grad_floats[0], dtype=torch.float32, device=dev)]
        s = da._sac_args(ws, obs)
        s.d_action, s.d_g_action, s.d_g_logp, s.d_grad1 = action.data_ptr(), g_action.data_ptr(), g_logp.data_ptr(), flat[0].data_ptr()
        actor = da._table(da.actor_net, "the actor")
        with torch.cuda.device(dev):
            N.check(da.lib.tg_policy_rsample_backward(C.byref(actor), C.byref(s), N.stream_ptr(dev)), "tg_policy_rsample_backward")
            N.check(da.lib.tg_policy_sac_weight_grad(C.byref(actor), None, None, C.byref(s), N.stream_ptr(dev)), "tg_policy_sac_weight_grad")
        ctx.ws = None
        da._sac_pool[("actor", n)].append(ws)
        return (None, None, None, *_grad_views(flat, params))


class _QEvaluate(torch.autograd.Function):
    """DeviceActor.q_evaluate as ONE autograd node over the action and every weight / bias of the Q nets (csrc/policy_sac_grad.hip):
    forward is tg_policy_q_eval_forward; backward is tg_policy_q_eval_backward -- with the action gradient only if the action needs
    one -- and, only if a Q parameter needs one, the critics' tg_policy_sac_weight_grad."""

    @staticmethod
    def forward(ctx, da, grad_mode, obs, act, *params):
        m, dev, twin = obs.shape[0], da.device, len(da.q_nets) == 2
        ws = da._sac_workspace("q", m)
        out = [torch.empty(m, dtype=torch.float32, device=dev) for _ in da.q_nets]
        s = da._sac_args(ws, obs)
        s.d_act, s.d_q1, s.d_q2 = act.data_ptr(), out[0].data_ptr(), (out[1].data_ptr() if twin else 0)
        q = [da._table(net, f"Q{k + 1}") for k, net in enumerate(da.q_nets)]
        with torch.cuda.device(dev):
            N.check(da.lib.tg_policy_q_eval_forward(C.byref(q[0]), C.byref(q[1]) if twin else None, C.byref(s), N.stream_ptr(dev)),
                    "tg_policy_q_eval_forward")
        if grad_mode and any(ctx.needs_input_grad):                            # (needs_input_grad alone ignores torch.no_grad())
            ctx.da, ctx.ws = da, ws
            ctx.save_for_backward(obs, *params)
        else:
            da._sac_pool[("q", m)].append(ws)                                  # (no backward will come for it)
        return tuple(out)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *g):
        da, ws = _consumed(ctx, "q_evaluate")
        obs, *params = ctx.saved_tensors
        m, dev, twin = ws.m, da.device, len(da.q_nets) == 2
        need_act, need_params = ctx.needs_input_grad[3], any(ctx.needs_input_grad[4:])
        g = [torch.zeros(m, dtype=torch.float32, device=dev) if t is None else t.contiguous() for t in g]
        g_act = torch.empty(2, m, 4, dtype=torch.float32, device=dev) if need_act else None
        s = da._sac_args(ws, obs)
        s.d_g_q1, s.d_g_q2, s.d_g_act = g[0].data_ptr(), (g[1].data_ptr() if twin else 0), N.ptr(g_act)
        q = [da._table(net, f"Q{k + 1}") for k, net in enumerate(da.q_nets)]
        q1, q2 = C.byref(q[0]), (C.byref(q[1]) if twin else None)
        flat = None
        with torch.cuda.device(dev):
            N.check(da.lib.tg_policy_q_eval_backward(q1, q2, C.byref(s), N.stream_ptr(dev)), "tg_policy_q_eval_backward")
            if need_params:
                flat = [torch.empty(k, dtype=torch.float32, device=dev) for k in ws.grad_floats[1:1 + len(q)]]
                s.d_grad1, s.d_grad2 = flat[0].data_ptr(), (flat[1].data_ptr() if twin else 0)
                N.check(da.lib.tg_policy_sac_weight_grad(None, q1, q2, C.byref(s), N.stream_ptr(dev)), "tg_policy_sac_weight_grad")
        ctx.ws = None
        da._sac_pool[("q", m)].append(ws)
        if need_act:                                                           # the two critics' buffers added: one torch add
            g_act = (g_act[0] + g_act[1] if twin else g_act[0])[:, :da.A]
        return (None, None, None, g_act, *(_grad_views(flat, params) if need_params else [None] * len(params)))


class DeviceActor:
    """The policy step for `num_envs` slots on one GPU.

    actor_net, critic_net   Linear(S <= 32, H) act [Linear(H, H) act]{0..4} Linear(H, O), H in {64, 128, 256}, act ReLU or Tanh, float32:
                            an nn.Sequential or a module with such a `.network`.  The two may differ in width, depth and activation.
    head        "gaussian": O = A, a = mu + exp(log_std) eps with the state-independent `log_std` [A] (a device tensor or Parameter,
                read at every call); "squashed": O = 2 A, (mu, ls) = split(out), ls clamped to `log_std_bounds`, a = tanh(mu + exp(ls) eps)
                and the squash correction - sum log(1 - a^2 + 1e-6) in the log-density.
    q_nets      None, one Q net or a pair: Linear(S + A <= 32, H) act [Linear(H, H) act]{0..4} Linear(H, 1) with the ACTOR's H and
                activation (depths are free), under the squashed head: q_values() and, with a pair, sac_target().
    seed, env_offset        eps of slot i at its k-th sampled call is the Box-Muller of Philox(seed, env_offset + i, k, the policy step's
                stream constant): objects with consecutive offsets are, bit for bit, the slots of one larger object.

    `action` [n][A], `logp` [n], `value` [n] and `mean` [n][A] are this object's own buffers, the same at every call and overwritten by
    the next act() (DeviceVecEnv's rule): clone what you keep.  `mean` is the deterministic action of the last act(): mu, or tanh(mu)
    under the squashed head.  values() has a buffer of its own per row count."""

    def __init__(self, actor_net, critic_net=None, *, q_nets=None, num_envs: int, log_std=None, head: str = "gaussian",
                 log_std_bounds=(-5.0, 2.0), seed: int = 0, env_offset: int = 0, device=None):
        if head not in HEADS:
            raise ValueError(f"DeviceActor: head {head!r} is not one of {sorted(HEADS)}")
        shape, why = _shape(actor_net, head)
        if shape is None:
            raise ValueError(f"DeviceActor: the actor is not supported: {why}")
        self.S, self.H, self.hidden_layers, O, self.activation = shape
        self.A = O // 2 if head == "squashed" else O
        self.head, self.actor_net, self.critic_net = head, actor_net, critic_net
        if critic_net is not None:
            cshape, why = _shape(critic_net, "value")
            if cshape is None:
                raise ValueError(f"DeviceActor: the critic is not supported: {why}")
            if cshape[0] != self.S:
                raise ValueError(f"DeviceActor: the critic reads {cshape[0]} inputs, the actor {self.S}")
        self.q_nets = () if q_nets is None else ((q_nets,) if isinstance(q_nets, torch.nn.Module) else tuple(q_nets))
        if q_nets is not None:
            why = _q_refusal(actor_net, shape, head, self.q_nets)
            if why is not None:
                raise ValueError(f"DeviceActor: the Q nets are not supported: {why}")
        if int(num_envs) <= 0 or int(env_offset) < 0:
            raise ValueError(f"DeviceActor: num_envs={num_envs} must be positive and env_offset={env_offset} non-negative")
        self.num_envs, self.env_offset = int(num_envs), int(env_offset)
        self.seed = self._checked_seed(seed)
        self.device = torch.device(device) if device is not None else torch.device("cuda", 0)
        if self.device.type != "cuda":
            raise N.NativeLibraryError("DeviceActor needs an MI355X (cuda) device; there is no CPU fallback")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        lo, hi = (float(v) for v in log_std_bounds)
        if not lo <= hi:
            raise ValueError(f"DeviceActor: log_std_bounds {log_std_bounds} are empty")
        self.log_std_bounds = (lo, hi)
        if head == "gaussian":
            if not isinstance(log_std, torch.Tensor):
                raise ValueError("DeviceActor: the gaussian head needs `log_std`, a float32 device tensor [A]")
            if tuple(log_std.shape) != (self.A,):
                raise ValueError(f"DeviceActor: log_std must be [{self.A}], got {list(log_std.shape)}")
        elif log_std is not None:
            raise ValueError("DeviceActor: the squashed head takes its log-std from the net; `log_std` must be None")
        self.log_std = log_std
        self.lib = N.load()
        n, A, dev, f32 = self.num_envs, self.A, self.device, torch.float32
        self.action = torch.zeros(n, A, dtype=f32, device=dev)
        self.mean = torch.zeros(n, A, dtype=f32, device=dev)
        self.logp = torch.zeros(n, dtype=f32, device=dev)
        self.value = torch.zeros(n, dtype=f32, device=dev) if critic_net is not None else None
        self._calls = torch.zeros(n, dtype=torch.int32, device=dev)            # (the bits of a u32)
        self._values_out = {}
        self._q_out = {}
        self._eval_pool = {}                                                   # row count -> free evaluate() workspaces
        self._sac_pool = {}                                                    # ("actor" | "q", row count) -> free rsample() / q_evaluate() workspaces
        if head == "squashed":
            self.eps = torch.zeros(n, A, dtype=f32, device=dev)                # the draw of the last rsample()
        if len(self.q_nets) == 2:                                             # sac_target's by-products and its owned alpha
            self.q1, self.q2, self.qmin, self.y, self._alpha = (torch.zeros(k, dtype=f32, device=dev) for k in (n, n, n, n, 1))
        self._grid_limit = 0           # 0: two workgroups per CU; a test sets it to force further trips of a workgroup's row loop
        s = N.PolicyStepArgs()
        s.d_calls, s.d_action, s.d_logp, s.d_mean = (t.data_ptr() for t in (self._calls, self.action, self.logp, self.mean))
        s.d_value = N.ptr(self.value)
        s.n, s.env_offset, s.seed, s.head, s.act_dim = n, self.env_offset, self.seed, HEADS[head], A
        s.log_std_lo, s.log_std_hi = lo, hi
        self._native = s

    @classmethod
    def for_env(cls, venv, actor_net, critic_net=None, log_std=None, head: str = "gaussian", log_std_bounds=(-5.0, 2.0), seed=None):
        """The actor that fits a DeviceVecEnv: its slot count, widths, device and env_offset, and (unless given) its seed."""
        self = cls(actor_net, critic_net, num_envs=venv.num_envs, log_std=log_std, head=head, log_std_bounds=log_std_bounds,
                   seed=venv.seed if seed is None else seed, env_offset=venv.env_offset, device=venv.device)
        if self.S != venv.S or self.A != venv.A:
            raise ValueError(f"DeviceActor: the actor maps {self.S} inputs to {self.A} actions under the {head} head, the env has "
                             f"{venv.S} observations and {venv.A} actions")
        return self

    @staticmethod
    def supports(net, head: str = "gaussian"):
        """None if the kernel takes `net` under `head` ("gaussian", "squashed", "value" for a critic, "q" for a Q critic on [obs, action]
        rows), else the reason as a string.  What the Q nets must share with the actor is checked by the constructor."""
        return _shape(net, head)[1]

    @staticmethod
    def _checked_seed(seed) -> int:
        seed = int(seed)
        if not 0 <= seed < 2 ** 64:
            raise ValueError(f"DeviceActor: seed {seed} is not an unsigned 64-bit integer")
        return seed

    # ---- the tables: filled from the parameters' CURRENT storage at every call -----------------------------------------------------
    def _table(self, net, name):
        lin = _modules(net)[0::2]
        t = _widths(net)
        for l, m in enumerate(lin):
            for p, what in ((m.weight, "weight"), (m.bias, "bias")):
                if p.dtype != torch.float32 or not p.is_contiguous() or p.device != self.device:
                    raise ValueError(f"DeviceActor: {name} layer {l} {what} must be a contiguous float32 tensor on {self.device}, got "
                                     f"{p.dtype} on {p.device}{'' if p.is_contiguous() else ', not contiguous'}")
            if 0 < l < len(lin) - 1 and m.weight.data_ptr() % 16:
                raise ValueError(f"DeviceActor: {name} layer {l} weight is not 16-byte aligned")
            t.w[l], t.b[l] = m.weight.data_ptr(), m.bias.data_ptr()
        return t

    def _rows(self, x, name, rows, width=None):
        """`x` as a contiguous float32 [rows][width] (the observation width by default; 0: a vector [rows]) on this device."""
        width = self.S if width is None else width
        shape = ("m" if rows is None else rows,) + ((width,) if width else ())
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.dim() != len(shape) or (width and x.shape[1] != width) or \
                (rows is not None and x.shape[0] != rows) or x.shape[0] == 0:
            got = f"{x.dtype} {list(x.shape)}" if isinstance(x, torch.Tensor) else type(x).__name__
            raise ValueError(f"DeviceActor: {name} must be float32 {''.join(f'[{d}]' for d in shape)}, got {got}")
        if x.device != self.device:
            raise ValueError(f"DeviceActor: {name} is on {x.device}, the actor on {self.device} (there is no CPU fallback)")
        x = x.detach()
        return x if x.is_contiguous() else x.contiguous()

    # ---- the two launches ----------------------------------------------------------------------------------------------------------
    def act(self, obs, deterministic: bool = False):
        """-> (action [n][A], logp [n], value [n] or None) of `obs` [n][S] in one launch.  With `deterministic` the action is the
        mean (tanh(mu) under the squashed head), logp the log-density there, and the draw counters do not advance."""
        obs = self._rows(obs, "obs", self.num_envs)
        s = self._native
        s.d_obs, s.deterministic, s.grid_limit = obs.data_ptr(), int(bool(deterministic)), self._grid_limit
        if self.head == "gaussian":
            ls = self.log_std
            if ls.dtype != torch.float32 or not ls.is_contiguous() or ls.device != self.device:
                raise ValueError(f"DeviceActor: log_std must be a contiguous float32 tensor on {self.device}")
            s.d_log_std = ls.data_ptr()
        actor = self._table(self.actor_net, "the actor")
        critic = self._table(self.critic_net, "the critic") if self.critic_net is not None else None
        with torch.cuda.device(self.device):
            N.check(self.lib.tg_policy_step(C.byref(actor), C.byref(critic) if critic is not None else None, C.byref(s),
                                            N.stream_ptr(self.device)), "tg_policy_step")
        return self.action, self.logp, self.value

    def values(self, x):
        """-> value [m] of any rows `x` [m][S], the critic alone, in one launch.  The result is this object's buffer for m rows,
        overwritten by the next values() of the same row count."""
        if self.critic_net is None:
            raise ValueError("DeviceActor: values() needs a critic")
        x = self._rows(x, "x", None)
        m = x.shape[0]
        out = self._values_out.get(m)
        if out is None:
            out = self._values_out[m] = torch.zeros(m, dtype=torch.float32, device=self.device)
        critic = self._table(self.critic_net, "the critic")
        with torch.cuda.device(self.device):
            N.check(self.lib.tg_policy_values(C.byref(critic), x.data_ptr(), m, out.data_ptr(), self._grid_limit,
                                              N.stream_ptr(self.device)), "tg_policy_values")
        return out

    def q_values(self, obs, act):
        """-> (q1 [m], q2 [m] or None, min(q1, q2) [m] or None) of any rows `obs` [m][S], `act` [m][A]: the Q nets on the rows
        [obs, act] in one launch.  The results are this object's buffers for m rows, overwritten by the next q_values() of that
        row count."""
        if not self.q_nets:
            raise ValueError("DeviceActor: q_values() needs q_nets")
        obs = self._rows(obs, "obs", None)
        act = self._rows(act, "act", obs.shape[0], self.A)
        m, twin = obs.shape[0], len(self.q_nets) == 2
        out = self._q_out.get(m)
        if out is None:
            out = self._q_out[m] = tuple(torch.zeros(m, dtype=torch.float32, device=self.device) if k == 0 or twin else None
                                         for k in range(3))
        s = N.PolicyQArgs()
        s.d_obs, s.d_act, s.n, s.obs_dim, s.act_dim, s.grid_limit = obs.data_ptr(), act.data_ptr(), m, self.S, self.A, self._grid_limit
        s.d_q1, s.d_q2, s.d_qmin = (N.ptr(t) for t in out)
        q = [self._table(net, f"Q{k + 1}") for k, net in enumerate(self.q_nets)]
        with torch.cuda.device(self.device):
            N.check(self.lib.tg_policy_q_values(C.byref(q[0]), C.byref(q[1]) if twin else None, C.byref(s), N.stream_ptr(self.device)),
                    "tg_policy_q_values")
        return out

    def sac_target(self, next_obs, reward, discount, alpha):
        """-> y [n] = reward + discount * (min(Q1, Q2)(next_obs, a') - alpha * logp(a' | next_obs)) in one launch, every operation
        rounded to float32 on its own; a' is the actor's next draw on these slots (what act(next_obs) would have given: the same
        counters, which advance).  `q_nets` are the TARGET critics.  `alpha` is a 0-dim float32 device tensor, read by the kernel at
        every call (and at every replay of a captured one), or a float.  `self.action`, `self.logp`, `self.q1`, `self.q2` hold a',
        its log-density and the two critics' values; like y (`self.y`) they are overwritten by the next call."""
        if len(self.q_nets) != 2:
            raise ValueError("DeviceActor: sac_target() needs a pair of q_nets")
        n = self.num_envs
        obs = self._rows(next_obs, "next_obs", n)
        reward, discount = self._rows(reward, "reward", n, 0), self._rows(discount, "discount", n, 0)
        if isinstance(alpha, torch.Tensor):
            if alpha.dtype != torch.float32 or alpha.dim() != 0 or alpha.device != self.device:
                raise ValueError(f"DeviceActor: alpha must be a 0-dim float32 tensor on {self.device} or a float")
            alpha = alpha.detach()
        else:
            alpha = self._alpha.fill_(float(alpha))
        a = self._native
        s = N.PolicyQArgs()
        s.d_obs, s.d_reward, s.d_discount, s.d_alpha = obs.data_ptr(), reward.data_ptr(), discount.data_ptr(), alpha.data_ptr()
        s.d_calls, s.d_action, s.d_logp = a.d_calls, a.d_action, a.d_logp
        s.d_q1, s.d_q2, s.d_qmin, s.d_y = (t.data_ptr() for t in (self.q1, self.q2, self.qmin, self.y))
        s.n, s.env_offset, s.seed, s.obs_dim, s.act_dim, s.grid_limit = n, self.env_offset, self.seed, self.S, self.A, self._grid_limit
        s.log_std_lo, s.log_std_hi = self.log_std_bounds
        actor = self._table(self.actor_net, "the actor")
        q = [self._table(net, f"Q{k + 1}") for k, net in enumerate(self.q_nets)]
        with torch.cuda.device(self.device):
            N.check(self.lib.tg_policy_sac_target(C.byref(actor), C.byref(q[0]), C.byref(q[1]), C.byref(s), N.stream_ptr(self.device)),
                    "tg_policy_sac_target")
        return self.y

    # ---- the learner's re-evaluation: forward and backward in HIP, an ordinary autograd node ----------------------------------------
    def evaluate(self, obs, action):
        """-> (logp [m], entropy [m], value [m] or None) of stored rows `obs` [m][S], `action` [m][A] (any m >= 1), each with a grad_fn:
        any torch loss of the three fills `.grad` of actor_net's, critic_net's parameters and of `log_std` on backward().  logp is
        act()'s float32 expression with eps = (a - mu) / exp(log_std); entropy = sum_k(log_std_k + 0.5 + 0.5 log 2 pi) for every row
        (a gradient to log_std alone).  Gradients to obs / action are not built (ValueError if either requires one).  Fresh result
        tensors at every call.  The stored activations live in a workspace per row count m that this call's backward() consumes
        and hands back; a second evaluate() of the same m before that backward() owns a fresh workspace (both graphs stay valid)."""
        if self.head != "gaussian":
            raise ValueError(f"DeviceActor: the head is {self.head!r}; evaluate() is built for the gaussian head")
        for t, name in ((obs, "obs"), (action, "action")):
            if isinstance(t, torch.Tensor) and t.requires_grad:
                raise ValueError(f"DeviceActor: evaluate() builds no gradient to {name} (it requires one)")
        obs = self._rows(obs, "obs", None)
        action = self._rows(action, "action", obs.shape[0], self.A)
        nets = [self.actor_net] + ([self.critic_net] if self.critic_net is not None else [])
        params = [p for net in nets for m in _modules(net)[0::2] for p in (m.weight, m.bias)]
        out = _Evaluate.apply(self, obs, action, self.log_std, *params)
        return (out[0], out[1], out[2] if self.critic_net is not None else None)

    def _eval_workspace(self, m):
        """A free workspace for m rows (activations, dZ, head gradients, weight-gradient partials) and the gradient sizes."""
        pool = self._eval_pool.setdefault(m, [])
        if pool:
            return pool.pop()
        acts, grads, partial = (C.c_int64 * 2)(), (C.c_int64 * 2)(), C.c_int64()
        critic = _widths(self.critic_net) if self.critic_net is not None else None
        if self.lib.tg_policy_eval_workspace(C.byref(_widths(self.actor_net)), C.byref(critic) if critic is not None else None, m, acts,
                                             grads, C.byref(partial)):
            raise ValueError("DeviceActor: evaluate() does not take these nets: " + self.lib.tg_last_error().decode("utf-8", "replace"))
        new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=self.device)
        ws = types.SimpleNamespace(m=m, grad_floats=tuple(grads), mu=new(m, self.A), std_rows=new(m, 4), partials=new(partial.value),
                                   acts=[new(k) if k else None for k in acts], dz=[new(k) if k else None for k in acts],
                                   dout=[new(m, 4) if k else None for k in acts])
        return ws

    def _eval_args(self, ws, obs, action, log_std, logp, entropy, value):
        s = N.PolicyEvalArgs()
        s.d_obs, s.d_act, s.d_log_std, s.m, s.act_dim, s.grid_limit = obs.data_ptr(), action.data_ptr(), log_std.data_ptr(), ws.m, self.A, self._grid_limit
        s.d_mu, s.d_logp, s.d_entropy, s.d_value, s.d_std_rows, s.d_partials = (N.ptr(t) for t in (ws.mu, logp, entropy, value, ws.std_rows, ws.partials))
        s.d_acts_actor, s.d_acts_critic = (N.ptr(t) for t in ws.acts)
        s.d_dz_actor, s.d_dz_critic = (N.ptr(t) for t in ws.dz)
        s.d_dout_actor, s.d_dout_critic = (N.ptr(t) for t in ws.dout)
        return s

    def _eval_tables(self):
        actor = self._table(self.actor_net, "the actor")
        critic = self._table(self.critic_net, "the critic") if self.critic_net is not None else None
        return C.byref(actor), (C.byref(critic) if critic is not None else None), (actor, critic)

    # ---- SAC's gradient steps: the reparameterised draw and the Q critics as autograd nodes ------------------------------------------
    def rsample(self, obs):
        """-> (action [n][A], logp [n]) of `obs` [n][S], each with a grad_fn: the slot's next draw under the squashed head (with or
        without `q_nets`: the node reads the actor alone) -- what
        act(obs) would have given, bit for bit, from the same counters, which advance -- as ONE autograd node over the actor's
        parameters along a = tanh(mu + exp(ls) eps), eps held constant, through the log-std clamp (derivative 1 on the closed interval
        `log_std_bounds`, 0 outside) and the squash correction.  `self.eps` [n][A] holds the draw (overwritten by the next rsample()).
        Fresh result tensors at every call; the workspace rules are evaluate()'s.  No gradient to obs (ValueError if it requires one)."""
        if self.head != "squashed":
            raise ValueError(f"DeviceActor: the head is {self.head!r}; rsample() is built for the squashed head")
        if isinstance(obs, torch.Tensor) and obs.requires_grad:
            raise ValueError("DeviceActor: rsample() builds no gradient to obs (it requires one)")
        obs = self._rows(obs, "obs", self.num_envs)
        params = [p for m in _modules(self.actor_net)[0::2] for p in (m.weight, m.bias)]
        return _RSample.apply(self, torch.is_grad_enabled(), obs, *params)

    def q_evaluate(self, obs, act, detach_params: bool = False):
        """-> (q1 [m], q2 [m] or None) of any rows `obs` [m][S], `act` [m][A], each with a grad_fn: q_values()' bits as ONE autograd node
        over every weight and bias of the Q nets and -- if `act` requires a gradient (rsample()'s action) -- over `act`.  With
        `detach_params` the Q parameters stay out of the node (SAC's actor update: no weight gradient is launched for the critics);
        the same launch is skipped whenever no Q parameter needs a gradient, and the action gradient whenever `act` needs none.
        No gradient to obs (ValueError if it requires one)."""
        if not self.q_nets:
            raise ValueError("DeviceActor: q_evaluate() needs q_nets")
        if isinstance(obs, torch.Tensor) and obs.requires_grad:
            raise ValueError("DeviceActor: q_evaluate() builds no gradient to obs (it requires one)")
        obs = self._rows(obs, "obs", None)
        self._rows(act, "act", obs.shape[0], self.A)
        params = [] if detach_params else [p for net in self.q_nets for m in _modules(net)[0::2] for p in (m.weight, m.bias)]
        out = _QEvaluate.apply(self, torch.is_grad_enabled(), obs, act if act.is_contiguous() else act.contiguous(), *params)
        return (out[0], out[1] if len(self.q_nets) == 2 else None)

    def _sac_workspace(self, kind, m):
        """A free workspace of rsample() (`kind` "actor") or q_evaluate() ("q") for m rows: activations, dZ, head gradients, the
        weight-gradient partials, and the gradient sizes (actor, Q1, Q2)."""
        pool = self._sac_pool.setdefault((kind, m), [])
        if pool:
            return pool.pop()
        acts, grads, partial = (C.c_int64 * 3)(), (C.c_int64 * 3)(), (C.c_int64 * 2)()
        nets = [self.actor_net] if kind == "actor" else [None, *self.q_nets]
        tables = [_widths(net) if net is not None else None for net in nets] + [None] * (3 - len(nets))
        if self.lib.tg_policy_sac_grad_workspace(*(C.byref(t) if t is not None else None for t in tables), self.A, m, acts, grads, partial):
            raise ValueError("DeviceActor: rsample() / q_evaluate() do not take these nets: " + self.lib.tg_last_error().decode("utf-8", "replace"))
        new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=self.device)
        own = [0] if kind == "actor" else [1, 2][:len(self.q_nets)]
        ws = types.SimpleNamespace(m=m, kind=kind, grad_floats=tuple(grads), partials=new(partial[kind == "q"]),
                                   acts=[new(acts[k]) for k in own], dz=[new(acts[k]) for k in own],
                                   dout=[new(m, 8 if kind == "actor" else 4) for _ in own],
                                   head_rows=new(m, 8) if kind == "actor" else None, xcat=new(m, self.S + self.A) if kind == "q" else None)
        return ws

    def _sac_args(self, ws, obs):
        s = N.PolicySacGradArgs()
        s.d_obs, s.m, s.obs_dim, s.act_dim, s.grid_limit = obs.data_ptr(), ws.m, self.S, self.A, self._grid_limit
        s.env_offset, s.seed = self.env_offset, self.seed
        s.log_std_lo, s.log_std_hi = self.log_std_bounds
        two = lambda ts: (N.ptr(ts[0]), N.ptr(ts[1]) if len(ts) == 2 else None)
        (s.d_acts1, s.d_acts2), (s.d_dz1, s.d_dz2), (s.d_dout1, s.d_dout2) = two(ws.acts), two(ws.dz), two(ws.dout)
        s.d_xcat, s.d_head_rows, s.d_partials = N.ptr(ws.xcat), N.ptr(ws.head_rows), N.ptr(ws.partials)
        return s

    @property
    def calls(self) -> torch.Tensor:
        """A copy of every slot's count of sampled act() calls, int64 [n]."""
        return self._calls.long() & 0xFFFFFFFF

    # ---- checkpointing -------------------------------------------------------------------------------------------------------------
    def state_dict(self):
        """The draw counters and what keys the draws (the nets are the caller's)."""
        return {"calls": self._calls.clone(), "seed": self.seed, "env_offset": self.env_offset, "num_envs": self.num_envs}

    def load_state_dict(self, sd):
        """Take over a state_dict() of an object over the same slots: later draws agree bit for bit with the original's."""
        if int(sd["num_envs"]) != self.num_envs or int(sd["env_offset"]) != self.env_offset:
            raise ValueError(f"DeviceActor: state_dict is of {sd['num_envs']} slots at offset {sd['env_offset']}, this object of "
                             f"{self.num_envs} at {self.env_offset}")
        if tuple(sd["calls"].shape) != (self.num_envs,) or sd["calls"].dtype != torch.int32:
            raise ValueError("DeviceActor: state_dict's calls is not int32 [num_envs]")
        self._calls.copy_(sd["calls"])
        self.seed = self._native.seed = self._checked_seed(sd["seed"])
