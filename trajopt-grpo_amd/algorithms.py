"""GRPO and PPO with the reference's constructor / `learn(buffer)` surface, running on the GPU.

Mirrors algorithms/algorithm.py:3-35, algorithms/grpo.py:12-169 and algorithms/ppo.py:8-225.
`learn` reproduces the reference arithmetic as written, including:
  * reward-to-go with the next-step mask inside the recurrence (grpo.py:69-72);
  * GRPO group statistics over ALL valid steps of a group's E episodes, unbiased std, the
    epsilon inside std() (i.e. none) (grpo.py:115);
  * GRPO performs gradient DESCENT on J (grpo.py:137-145) -- `maximize=True`
    is the explicit, non-default divergence;
  * PPO `old_log_probs` come from the CURRENT policy (ppo.py:142-143); the critic regresses on
    batch-normalised returns while A = R_raw - V (ppo.py:111,139,169); the entropy of the
    fixed-covariance Gaussian is a constant (zero gradient).
  A policy built with learn_std=True (policies.py) has a learned per-dimension `log_std`: both learners then route every update through
  the `_std` entry points -- the heads read log_std on the device and emit its gradient, tg_log_std_grad adds it (and PPO's entropy
  bonus, -entropy per component and optimizer step) into log_std's window of the gradient bucket; no update reads it on the host.
  GRPO's one-rank Adam rider declines for such a policy (the optimizer owns more than the net's parameters).
What changes is where it runs: RTG / moments / normalisation / log-prob / the loss head are HIP
kernels over the device trajectory; the MLP forward/backward run through mlp.GemmMLP (forward chain
kernel, backward-data chain kernel, weight-gradient kernel); gradients of all ranks are summed
with ONE flat all-reduce per optimizer step.
"""
from __future__ import annotations

import copy
import math
import os
from abc import ABC, abstractmethod

import torch

from . import distributed as D
from . import hip_ops as K
from . import mlp as M
from . import optim as O
from . import policies as P
from .rollout import DeviceTrajectory


# 0: always a no-grad pass of the old policy for the old log-probabilities (for callers that write weights through `.data` between
# learn() calls and do not want the fold's bitwise check to stop them)
_FOLD_OLD_LOGP = os.environ.get("TG_FOLD_OLD_LOGP", "1") == "1"
_SMALL_N_RETURNS = 16384                                           # envs up to which tg_returns_moments replaces tg_rtg_scan + tg_masked_moments


class Algorithm(ABC):
    """algorithms/algorithm.py:3-35."""

    def __init__(self):
        pass

    @abstractmethod
    def learn(self, buffer):
        pass

    @abstractmethod
    def metadata(self):
        return {}

    @abstractmethod
    def save(self, path: str):
        pass

    @abstractmethod
    def load(self, path: str):
        pass


def device_trajectory(buffer, device) -> DeviceTrajectory:
    """The buffer's device trajectory; reference-layout CPU tensors (a legacy manager) are uploaded."""
    traj = getattr(buffer, "device_traj", None)
    if traj is not None:
        return traj
    obs, act = buffer.group_observations, buffer.group_actions
    rew, mask = buffer.group_rewards, buffer.group_masks
    G, E, T, S = obs.shape
    A = act.shape[-1]
    n = G * E
    tr = DeviceTrajectory(S, A, T, n, G, E, torch.float32, device)
    tr.obs[:, :T, :].copy_(obs.reshape(n, T, S).permute(2, 1, 0))
    tr.act.copy_(act.reshape(n, T, A).permute(2, 1, 0))
    tr.rew.copy_(rew.reshape(n, T).t())
    tr.mask.copy_(mask.reshape(n, T).t().to(torch.uint8))
    tr.len.copy_(mask.reshape(n, T).sum(1).to(torch.int32))
    return tr


class _StepLog:
    """One float32 row per optimizer step of a learn(), in device blocks of 64 rows: written on the device, read when last_stats asks."""
    def __init__(self, *width):
        self.width, self.blocks, self.steps = width, [], 0

    def next_row(self, device) -> torch.Tensor:                             # a [1, *width] view of its block
        row = self.steps % 64
        if row == 0:
            self.blocks.append(torch.empty(64, *self.width, dtype=torch.float32, device=device))
        self.steps += 1
        return self.blocks[-1][row:row + 1]

    def rows(self) -> torch.Tensor:
        return torch.cat(self.blocks)[:self.steps]


class _GpuLearner(Algorithm):
    # rows per forward/backward chunk (~8 KiB of activations, masks and dZ per row and net at 256x5 bf16).  One chunk for
    # everything was measured up to 3 % faster and, when the row count grows from one iteration to the next, up to 2x
    # slower (GB-sized blocks outgrow the caching allocator every time); a fixed first chunk keeps the big blocks reusable.
    chunk_rows = 1 << 22
    # (None until whatever first needs them sets them; class-level, so that every instance reads them plainly)
    _rollout_stream = _rollout_engine = _old_synced = _sum_rows = None
    _fold_pending = _differ_table = _count_pending = _count_pinned = None

    def _setup(self, policy, optimizer, chunk_rows, autocast_dtype, process_group, fused_mlp=True, max_grad_norm=None,
               kl_stats=False, desired_kl=None, lr_bounds=(1e-5, 1e-2), lr_factor=1.5, target_kl=None, kl_stop_factor=1.5, kl_every=None):
        self.policy, self.optimizer = policy, optimizer
        self._kl_setup(kl_stats, desired_kl, lr_bounds, lr_factor, target_kl, kl_stop_factor, kl_every)
        if max_grad_norm is not None:
            if isinstance(max_grad_norm, bool) or not isinstance(max_grad_norm, (int, float)) or not (math.isfinite(max_grad_norm) and max_grad_norm > 0):
                raise ValueError(f"max_grad_norm must be None or a finite number > 0, got {max_grad_norm!r}")
            max_grad_norm = float(max_grad_norm)
        self.max_grad_norm = max_grad_norm
        self._clip_log, self._std_log = _StepLog(2), _StepLog()      # (pre-clip norm | coefficient), sum(log_std): new per learn()
        if chunk_rows is not None:
            self.chunk_rows = int(chunk_rows)
        elif os.environ.get("TG_CHUNK_ROWS"):
            self.chunk_rows = int(os.environ["TG_CHUNK_ROWS"])
        self.autocast_dtype = autocast_dtype
        self.process_group = process_group
        self.fused_mlp = fused_mlp
        self._bucket = None
        self._fused_adam = None
        self._adam_covers_bucket = False
        self._refresher = None
        self._mlps = {}
        self._ws = M._Workspace()       # per-iteration tensors whose size follows the number of valid rows
        self._stats, self._stats_pending = {}, None
        self._small_bufs = {}           # ... and those whose size does not (_small)

    def learn(self, buffer) -> None:
        """One training iteration on `buffer` (algorithms/grpo.py:50-148, ppo.py:64-186).  The native kernels are
        launched through ctypes on the policy's device: make it the current one for the duration."""
        with torch.cuda.device(self.policy.device):
            # the fused fp32 rollout's weight stream of THIS policy's actor, if the buffer's manager has one: rebuilt by the launch
            # that follows every optimizer step, so the next rollout starts without a refresh of its own
            frag = getattr(getattr(getattr(buffer, "rollout_manager", None), "engine", None), "_frag", None)
            ok = (frag is not None and frag.rides_on_optimizer_step
                  and frag.lin == [m for m in self.policy.actor.network if isinstance(m, torch.nn.Linear)])
            self._rollout_stream = frag if ok else None
            # every per-row workspace (activations, dZ, mask bits, gathered rows) is allocated ONCE for the largest chunk an
            # iteration of this buffer can bring: 288 GB of HBM are there to be used, and growth by re-allocation stalls the queue
            traj = getattr(buffer, "device_traj", None)
            if traj is not None:
                cap = min(self.chunk_rows, traj.T * traj.n)
                self._ws.default_cap = max(self._ws.default_cap, cap)
                for m in self._mlps.values():
                    if m is not None:
                        m._ws.default_cap = max(m._ws.default_cap, cap)
            self._rollout_engine = getattr(getattr(buffer, "rollout_manager", None), "engine", None) if ok else None
            self._check_deferred()
            self._kl_entry_check()
            self._kl_run = None
            self._clip_log, self._std_log = _StepLog(2), _StepLog()
            obs_count = self._obs_norm_update(buffer)
            self._learn(buffer)
            if self.kl_stats:
                inner_kl = self._stats_pending or dict                      # (no update ran: the measurement is all there is)
                self._stats_pending = lambda: {**inner_kl(), **self._kl_stats_read()}
            if obs_count is not None and self._stats_pending is not None:
                inner0 = self._stats_pending
                self._stats_pending = lambda: {**inner0(), "obs_count": float(obs_count.item())}
            if self._clip_log.steps and self._stats_pending is not None:
                inner, clip_log = self._stats_pending, self._clip_log
                self._stats_pending = lambda: {**inner(), "grad_norm": clip_log.rows()[:, 0].tolist()}
            if self._kl_ctl and self._stats_pending is not None:
                inner_all, keys = self._stats_pending, self._KL_LIST_KEYS

                def cut():                  # the per-step lists end with the last step that was applied
                    st = inner_all()
                    n = st.get("n_updates")
                    return st if n is None else {k: v[:n] if (k in keys and isinstance(v, list)) else v for k, v in st.items()}
                self._stats_pending = cut

    def _obs_norm_update(self, buffer):
        """normalize_obs: the policy's running statistics take in this rollout's valid observations (one all-reduce across the ranks)
        and the table is rewritten -- BEFORE any row of this learn() is prepared, so that old log-probabilities, the old-policy pass,
        every update and the bootstrap rows read the one table.  A frozen normaliser keeps its bits.  Returns a device copy of the
        count (for last_stats), or None when the policy reads raw observations."""
        on = getattr(self.policy, "obs_norm", None)
        if on is None:
            return None
        if not on.frozen:
            on.update(device_trajectory(buffer, self.policy.device), self.process_group)
        return on.count.clone()

    def _entry_refresh(self, *nets):
        """The derived weight layouts of `nets` at the entry of learn(): rebuilt whatever the version keys say -- a weight written
        through `.data` since the last learn() leaves no trace in them -- by the one gather launch when there is one (the fused
        optimizer step's StreamRefresher), else by marking everything stale.  TG_TRUST_VERSION_KEYS=1: the keys decide, as they do
        between the updates of a learn()."""
        if M.N.TRUST_KEYS:
            return self._refresh(*nets)
        ref = self._refresher
        if ref is not None and ref[0][:len(nets)] == tuple(id(n) for n in nets) and ref[1].run():
            for net in nets:
                m = self._mlp(net)
                if m is not None:
                    m.refresh()
                    m._stale.update(("w", "dx"))           # (what the gather does not cover: rebuilt lazily, only if a path reads it)
            return
        for net in nets:
            m = self._mlp(net)
            if m is not None:
                m.refresh(force=True)

    def _masters_written(self, net):
        """A launch of the learner's own has just written fp32 masters of `net` by raw pointer (PopArt's rescale of the critic head):
        what optim.FusedAdam does after its raw writes -- the counter that stands in for torch's version keys moves, and every
        layout derived from the net is rebuilt from the masters.  The streams the optimizer step's own launch keeps current are
        rebuilt here (that launch marks them fresh whether or not a path has read them since); the per-layer copies and the packed
        backward-data fragments by the first path that reads them.  A net on torch autograd reads the masters themselves."""
        M.N.RAW_PARAM_WRITES[0] += 1
        m = self._mlp(net)
        if m is not None:
            m.refresh(force=True)
            for what, _ in m.streams():
                m._fresh(what)

    def _check_deferred(self):
        """Checks whose answers are copied to the host asynchronously: the mask's own row count against the rollout's statistic, the
        bitwise comparison behind the folded old-policy pass.  Read at the END of the learn() that enqueued them (both were written
        before its first update ran, so the host does not wait) and again at the next entry / statistics read for a learn() that
        raised in between.  The optimizer steps of that learn() have been applied by then: the error says the weights are suspect, it
        does not roll them back."""
        self._check_row_count()
        if self._fold_pending is not None:
            (host, ev), self._fold_pending = self._fold_pending, None
            ev.synchronize()
            if int(host[0]):
                raise RuntimeError("policy.actor and old_policy.actor held different weights although nothing had written either through "
                                   "torch since old_policy <- policy: they were modified through `.data` (or raw pointers).  The last "
                                   "learn() took its old log-probabilities from the current policy; set TG_FOLD_OLD_LOGP=0, or follow "
                                   "such a write with an in-place torch operation (p.add_(0)).")

    def _verify_old_is_current(self):
        """Enqueue the bitwise comparison of policy.actor with old_policy.actor (one launch; the flag is read at the next learn() entry
        or when the statistics are): the fold of the old-policy pass relies on version keys, which `.data` writes do not move."""
        a, b = list(self.policy.actor.parameters()), list(self.old_policy.actor.parameters())
        sig = tuple(p.data_ptr() for p in a + b)
        if self._differ_table is None or self._differ_table[0] != sig:
            rows, first = [], 0
            for p, q in zip(a, b):
                assert p.shape == q.shape and p.is_contiguous() and q.is_contiguous() and p.dtype == q.dtype == torch.float32
                rows.append([p.data_ptr(), q.data_ptr(), 0, 0, first])
                first += p.numel()
            dev = a[0].device
            self._differ_table = (sig, torch.tensor(rows, dtype=torch.int64).to(dev), len(rows), first,
                                  torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32).pin_memory())
        _, table, n, total, flag, host = self._differ_table
        flag.zero_()
        K.N.check(K.N.load().tg_params_differ(table.data_ptr(), n, total, flag.data_ptr(), K.N.stream_ptr(flag.device)), "tg_params_differ")
        host.copy_(flag, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(flag.device))
        self._fold_pending = (host, ev)

    @property
    def last_stats(self) -> dict:
        """Loss statistics of the last learn() as Python numbers.  They are read from the device when first asked for, not at the
        end of learn(): the host goes on to enqueue the next rollout while the last updates still run."""
        if self._stats_pending is not None:
            self._stats, self._stats_pending = self._stats_pending(), None
            self._check_deferred()
        return self._stats

    @last_stats.setter
    def last_stats(self, value) -> None:
        self._stats, self._stats_pending = value, None

    @torch.no_grad()
    def _copy_policy_to_old(self) -> None:
        """old_policy <- policy (grpo.py:148, ppo.py:186) as ONE multi-tensor copy when the two state dicts line up (they are
        deep copies of each other), else through load_state_dict."""
        def leaves(d):                                                      # (the actor-critic's state dict nests one per net)
            out = []
            for v in d.values():
                out += leaves(v) if isinstance(v, dict) else [v]
            return out

        src, dst = leaves(self._weights_state(self.policy)), leaves(self._weights_state(self.old_policy))
        if len(src) == len(dst) and all(torch.is_tensor(a) and torch.is_tensor(b) and a.shape == b.shape and a.dtype == b.dtype
                                        and a.device == b.device for a, b in zip(src, dst)):
            # ... and with them the weight streams already built from these weights (the launch after the last optimizer step):
            # the old policy's forward pass of the next learn() then needs no rebuild of its own
            marks = []
            for name in ("actor", "critic"):
                new, old = getattr(self.policy, name, None), getattr(self.old_policy, name, None)
                mn, mo = (self._mlps.get(id(new)), self._mlps.get(id(old))) if new is not None and old is not None else (None, None)
                if mn is None or mo is None:
                    continue
                k = mn._key()
                new_s, old_s = dict(mn.streams()), dict(mo.streams())
                for what in ("f32", "chain"):
                    sn, so = new_s.get(what), old_s.get(what)
                    if sn is None or so is None or what in mn._stale or mn._built.get(what) != k:
                        continue
                    ts = [(a, b) for (a, _), (b, _) in zip(sn.outputs, so.outputs)]
                    if all(a.shape == b.shape and a.dtype == b.dtype for a, b in ts):
                        src += [a for a, _ in ts]
                        dst += [b for _, b in ts]
                        marks.append((mo, what))
            torch._foreach_copy_(dst, src)
            for mo, what in marks:
                mo.mark_built(what)                                         # (keyed on the old net's weights AFTER the copy)
        else:
            self._load_old(self._weights_state(self.policy))
        self._old_synced = self._actor_keys()                               # old_policy.actor == policy.actor as long as both keys stand

    @staticmethod
    def _weights_state(pol) -> dict:
        """pol.state_dict() without the observation / return statistics: old_policy SHARES the policy's obs_norm and value_norm objects,
        there is nothing to copy."""
        return {k: v for k, v in pol.state_dict().items() if k not in P.OBS_NORM_KEYS and k not in P.VALUE_NORM_KEYS}

    def _load_old(self, weights) -> None:
        """old_policy.load_state_dict(weights) past its check that statistics come with a normalised policy (they are shared)."""
        old = self.old_policy
        on, vn = old.obs_norm, getattr(old, "value_norm", None)
        old.obs_norm = old.value_norm = None
        try:
            old.load_state_dict(weights)
        finally:
            old.obs_norm, old.value_norm = on, vn

    def _make_old_policy(self):
        """A deep copy of the policy (grpo.py:48, ppo.py:62) that reads states through the policy's own obs_norm object (and values
        through its value_norm object)."""
        old = copy.deepcopy(self.policy)
        old.obs_norm = getattr(self.policy, "obs_norm", None)
        old.value_norm = getattr(self.policy, "value_norm", None)
        return old

    def _actor_keys(self):
        """(key of policy.actor's parameters, key of old_policy.actor's): storage, torch version counters, raw-write count."""
        def key(pol):
            ps = list(pol.actor.parameters()) + ([pol.log_std] if getattr(pol, "log_std", None) is not None else [])
            return (tuple((p.data_ptr(), p._version) for p in ps), M.N.RAW_PARAM_WRITES[0])
        return key(self.policy), key(self.old_policy)

    def _old_actor_is_current(self) -> bool:
        """Nothing has written either actor since old_policy <- policy (grpo.py:148): their weights are the same bits, and so are
        their log-probabilities -- the first update's own forward pass can stand in for the old policy's."""
        return self._old_synced is not None and self._old_synced == self._actor_keys()

    def sync_old_policy(self) -> None:
        """old_policy <- policy.  The constructors deep-copy the policy BEFORE a checkpoint is loaded into it
        (pipelines/pipeline.py:93-100 loads after construction), so a resume must re-synchronise the copy -- GRPO's
        first learn() would otherwise form its ratios against the random-init weights."""
        self._load_old(self._weights_state(self.policy))
        self._old_synced = self._actor_keys()

    @property
    def bucket(self) -> D.GradBucket:
        if self._bucket is None:
            self._bucket = D.GradBucket(list(self.policy.parameters()))
        return self._bucket

    # ---- MLP execution: hand-scheduled GEMM path (mlp.py) when the net is a ReLU MLP (or a Tanh MLP of the fp32 chain learner's
    # shapes in float32), else autograd ----
    def _mlp(self, net):
        key = id(net)
        if key not in self._mlps:
            cd = self.autocast_dtype or torch.float32
            ok = ((self.fused_mlp and M.supports(net, cd)) or self._tanh_native(net)) and next(net.parameters()).is_cuda
            self._mlps[key] = M.GemmMLP(net, cd) if ok else None
            if not ok and self.fused_mlp:
                M.log_too_wide(net, cd)
            if self._mlps[key] is not None:
                self._mlps[key]._ws.default_cap = self._ws.default_cap
        return self._mlps[key]

    def _tanh_native(self, net) -> bool:
        """A Tanh net takes the fp32 chain learner (tg_mlp_f32_*_act) when it runs in float32 at that learner's shapes; any other Tanh
        net stays on torch autograd, as before, and says so once on the `trajopt_grpo_amd` logger."""
        if M.hidden_activation(net) != "Tanh":
            return False
        why = ("fused_mlp=False" if not self.fused_mlp else
               f"autocast_dtype={self.autocast_dtype}" if self.autocast_dtype not in (None, torch.float32) else
               None if M.f32_chain_supported(net) else
               "shape outside Linear(S<=32, H) Tanh [Linear(H, H) Tanh]{0..3} Linear(H, A<=4), H in {64, 128}")
        if why is not None:
            lin = [m for m in net.network if isinstance(m, torch.nn.Linear)]
            shape = f"{lin[0].in_features}-" + "-".join(str(l.out_features) for l in lin)
            if (shape, why) not in M._LOGGED_SHAPES:
                M._LOGGED_SHAPES.add((shape, why))
                M._LOG.info("%s Tanh: %s -- its update runs on torch autograd (the Tanh kernels are the fp32 chain learner's)", shape, why)
        return why is None

    def _refresh(self, *nets):
        for net in nets:
            m = self._mlp(net)
            if m is not None:
                m.refresh()

    def _clip_metadata(self) -> dict:
        return {} if self.max_grad_norm is None else {"max_grad_norm": self.max_grad_norm}

    def _zero_grads(self):
        """`optimizer.zero_grad()` (grpo.py:143, ppo.py:181) on the flat bucket -- skipped when the previous update's Adam launch
        already left every gradient zero (FusedAdam.step(zero_grads=True))."""
        fa = self._fused_adam
        if fa and fa.grads_zeroed:
            fa.grads_zeroed = False
            return
        self.bucket.zero_()

    def _optimizer_step(self, *nets, last=True):
        """`optimizer.step()` (grpo.py:145, ppo.py:183) and the refresh of every weight layout derived from `nets`.  A plain default
        torch.optim.Adam takes ONE launch on its own state tensors (optim.FusedAdam: bit-identical to torch's ~8) and one gather
        rebuilds all layouts; anything else -- hooks, a patched step, another optimizer -- runs as written, layouts refreshed lazily.
        last=False: another update of this learn() follows -- the Adam launch also zeroes the gradients it consumed (the final
        update's gradients stay in .grad, as after the reference's learn())."""
        refresher = self._optimizer_setup(*nets)
        # max_grad_norm: the fused step multiplies by the device-side coefficient itself; an optimizer it does not take (and a bucket
        # it does not cover) gets clip_grad_norm_'s own in-place scaling of the whole bucket -- by the device scalar, no host read
        coef = self._clip_coef() if self.max_grad_norm is not None else None
        in_step = coef is not None and bool(self._fused_adam) and self._adam_covers_bucket
        if coef is not None and not in_step:
            self.bucket.flat.mul_(coef)
        # target_kl / kl_every: the fused step reads the control block on the device (a latched block: the launch changes nothing)
        run = self._kl_run
        stepped = bool(self._fused_adam) and self._fused_adam.step(zero_grads=not last and self._adam_covers_bucket, refresher=refresher,
                                                                   clip_coef=coef if in_step else None,
                                                                   ctl=None if run is None else (run["ctl"], self._kl_adapt_checks))
        if not stepped:
            if in_step:                     # (refused before any launch: nothing has been scaled yet)
                self.bucket.flat.mul_(coef)
            if run is not None:
                # the waiting path: torch's own step cannot read the block, so the host reads the newest check first -- and does
                # not step behind a latch (the lr of that check is in the param groups by now)
                run["fused"] = False
                if run["checks"] and self._kl_read(len(run["checks"]) - 1):
                    return
            self.optimizer.step()
        if run is not None:
            run["enqueued"] += 1
        self._refresh(*nets)
        if stepped and not self._fused_adam.pushed:
            refresher.run()

    def _clip_coef(self):
        """tg_grad_clip_coef on the flat gradient bucket, after the all-reduce (every rank: the same bytes, the same bits): the
        device float32 [1] holding min(1, max_grad_norm / (norm + 1e-6)).  The norm itself stays in the row next to it until
        last_stats asks (rows of [64][2] blocks, one row per optimizer step of this learn(): nothing here visits the host)."""
        flat = self.bucket.flat
        if flat.dtype != torch.float32:
            raise RuntimeError(f"max_grad_norm needs float32 gradients, the bucket holds {flat.dtype}")
        out2 = self._clip_log.next_row(flat.device)[0]
        lib = K.N.load()
        work = self._small("clip_work", max(int(lib.tg_grad_clip_workspace(flat.numel())) // 8, 1), torch.float64, flat.device)
        with torch.cuda.device(flat.device):
            K.N.check(lib.tg_grad_clip_coef(flat.data_ptr(), flat.numel(), self.max_grad_norm, out2.data_ptr(), work.data_ptr(),
                                            K.N.stream_ptr(flat.device)), "tg_grad_clip_coef")
        return out2[1:2]

    def _optimizer_setup(self, *nets):
        """The fused optimizer step and the refresher of `nets`' derived layouts (None without a fused step), created on first use."""
        if self._fused_adam is None:
            self._fused_adam = O.FusedAdam(self.optimizer)
            if self._fused_adam:
                owned = {id(p) for g in self.optimizer.param_groups for p in g["params"]}
                self._adam_covers_bucket = all(id(p) in owned for p in self.bucket.params)
        if not self._fused_adam:
            return None
        extra = [] if self._rollout_stream is None else [self._rollout_stream]
        key = tuple(id(n) for n in nets) + tuple(id(x) for x in extra)
        if self._refresher is None or self._refresher[0] != key:
            self._refresher = (key, O.StreamRefresher(self._fused_adam, [self._mlp(n) for n in nets], extra))
            if extra and self._rollout_engine is not None:
                self._rollout_engine.entry_refresh = self._refresher[1].run          # the rollout's own entry rebuild: this one gather
        return self._refresher[1]

    def _adam_rider(self, net, last, whole_update):
        """`optimizer.step()` (grpo.py:145) as a rider of the backward pass's last launch, where nothing stands between the gradients
        and the step: the fp32 chain learner, one rank (no all-reduce), the update's rows in ONE chunk, and an optimizer that holds
        exactly this net's parameters.  None otherwise -- the caller then all-reduces and calls _optimizer_step() as before.
        It declines while a control block is active (target_kl / kl_every): there is no rider form of the `_ctl` step."""
        m = self._mlp(net)
        if not (whole_update and m is not None and m._f32 is not None) or D.rank_world(self.process_group)[1] != 1 or D._ALWAYS:
            return None                     # (TG_COLLECTIVES_AT_WORLD_1=1: the gradient all-reduce is wanted even at one rank)
        if self.max_grad_norm is not None:
            return None                     # (the norm needs every gradient element finished before any parameter moves)
        if self._kl_run is not None:
            return None                     # (the step must read the control block: tg_adam_step*_ctl)
        refresher = self._optimizer_setup(net)
        if refresher is None or not self._adam_covers_bucket:
            return None
        owned = {id(p) for g in self.optimizer.param_groups for p in g["params"]}
        if owned != {id(p) for p in net.parameters()}:
            return None
        return self._fused_adam.rider(zero_grads=not last, refresher=refresher)

    def _prep(self, net, X, cap_rows=0):
        m = self._mlp(net)
        on = getattr(self.policy, "obs_norm", None)
        if m is None:
            return X if on is None else on.normalize(X)
        return m.prepare_input(X, out=self._ws.get("xin", X.shape[0], m.in_pad, m.cd, X.device, cap_rows), obs_norm=on)

    def _forward(self, net, x, train=False, view=False):
        """fp32 output [rows][out].  train=True keeps what backward needs (activations or the autograd graph).
        view=True: may return a unit-column-stride view of the padded output (row stride > out) instead of a copy."""
        m = self._mlp(net)
        if m is not None:
            if view:
                return m.forward(x, keep=train, padded=True)[:, :m.out_dim]
            return m.forward(x, keep=train)
        with torch.set_grad_enabled(train):
            if self.autocast_dtype is not None:
                with torch.autocast("cuda", dtype=self.autocast_dtype):
                    y = net(x)
                return y.float()
            return net(x)

    def _backward(self, net, out, grad):
        m = self._mlp(net)
        if m is not None:
            m.backward(grad)
        else:
            out.backward(grad)

    def _gather_valid(self, traj):
        """Indices of valid (t, n) rows (time-major) and the gathered observations / actions."""
        flat = traj.mask.reshape(-1)
        if traj.host_valid_rows is not None and hasattr(torch, "nonzero_static"):
            # the count is on the host already (it rode on the rollout's statistics): no host-device round trip for the shape
            idx = torch.nonzero_static(flat, size=int(traj.host_valid_rows())).squeeze(1)
        else:
            idx = flat.nonzero().squeeze(1)
        rows_all, cap = traj.obs_rows(), traj.T * traj.n
        if rows_all.dtype == torch.float32:
            X = torch.index_select(rows_all, 0, idx, out=self._ws.get("X", idx.numel(), traj.S, torch.float32, idx.device, cap))
        else:
            X = rows_all.index_select(0, idx).float().contiguous()
        acts_all = traj.act_rows()
        act = torch.index_select(acts_all, 0, idx, out=self._ws.get("act", idx.numel(), traj.A, acts_all.dtype, idx.device, cap))
        return idx, X, act

    # ---- the prologue as four launches (csrc/learn_kernels.hip) ------------------------------------------------------
    def _check_row_count(self):
        """The flag of the previous learn()'s tg_learn_count, read long after it was written: the valid rows the mask held were not
        the number the rollout's statistic gave the host (a mask edited after sample(), a hand-built trajectory)."""
        if self._count_pending is None:
            return
        (host, ev, expected), self._count_pending = self._count_pending, None
        ev.synchronize()
        total = int(host[0])
        if total != expected:
            raise RuntimeError(f"the trajectory's mask held {total} valid rows, the rollout's statistic said {expected}: the last learn() "
                               "ran on truncated / padded rows (was the mask edited after sample()?)")

    def _prepare(self, traj, m, src0=None, moments=None, norm_mode=0, group_size=0, src1=None):
        """What `obs[mask]`, `act[mask]`, `adv[mask]` (algorithms/ppo.py:126-135, grpo.py:76-112) and GemmMLP.prepare_input() produce,
        straight from the device trajectory into the learner's workspaces: (idx int64 [rows], xin [rows][in_pad] compute dtype with the
        ones column, act [rows][A], src0's valid entries (normalised with `moments` when given), src1's valid entries).  None when
        this net has no GemmMLP or the trajectory's dtype is not f32 / f64 (the torch path then does it).
        = _prepare_finish(_prepare_enqueue(...)): the first half only enqueues, the second half is where the host waits for the row
        count -- whatever host work does not need the count belongs between the two."""
        return self._prepare_finish(self._prepare_enqueue(traj, m, src0, moments, norm_mode, group_size, src1))

    def _prepare_enqueue(self, traj, m, src0=None, moments=None, norm_mode=0, group_size=0, src1=None):
        if m is None or traj.obs.dtype not in (torch.float32, torch.float64) or m.in_pad > 64 or traj.S > m.in_pad:
            return None
        if m.in_pad % (8 if m.cd == torch.bfloat16 else 4) or m.cd not in (torch.bfloat16, torch.float32):
            return None
        dev, cap = traj.mask.device, traj.T * traj.n
        work = self._ws.get("cnt_work", (K.learn_count_workspace(cap) + 3) // 4, 1, torch.int32, dev)
        total = torch.empty(2, dtype=torch.int64, device=dev)
        # Everything is enqueued BEFORE the host asks for the row count: the kernels take the buffers' capacity, not the count, so
        # they queue up behind the rollout while the host is still waiting for the rollout's statistic -- and run while it prepares
        # the first forward launch (asked first, the count cost the GPU ~30 us of idle time per step at 4,096 envs).
        K.learn_count(traj.mask, -1, work, total)
        idx_c = self._ws.get("idx", cap, 1, torch.int64, dev, cap).view(-1)
        xin_c = self._ws.get("xin", cap, m.in_pad, m.cd, dev, cap)
        act_c = self._ws.get("act", cap, traj.A, torch.float32, dev, cap)
        d0_c = self._ws.get("row0", cap, 1, torch.float32, dev, cap).view(-1) if src0 is not None else None
        d1_c = self._ws.get("row1", cap, 1, torch.float32, dev, cap).view(-1) if src1 is not None else None
        ones = 31 if (m.in_pad == 32 and m.in_dim < 32 and m._f32 is None) else -1
        K.learn_compact(traj, work, cap, xin_c, ones, act_c, idx_c, src0, d0_c, src1, d1_c, moments, norm_mode, group_size,
                        obs_norm=getattr(self.policy, "obs_norm", None))
        return traj, total, idx_c, xin_c, act_c, d0_c, d1_c, ones

    def _prepare_finish(self, handle):
        if handle is None:
            return None
        traj, total, idx_c, xin_c, act_c, d0_c, d1_c, ones = handle
        dev = total.device
        if traj.host_valid_rows is not None:
            # the rollout's own statistic (on the host without a round trip); the count of the mask itself follows asynchronously and is
            # compared with it at the next learn() entry
            self._check_row_count()
            if self._count_pinned is None:
                self._count_pinned = torch.empty(2, dtype=torch.int64).pin_memory()
            self._count_pinned.copy_(total, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(dev))
            rows = int(traj.host_valid_rows())
            self._count_pending = (self._count_pinned, ev, rows)
        else:
            rows = int(total[0].item())
        idx, xin, act = idx_c[:rows], xin_c[:rows], act_c[:rows]
        d0 = d0_c[:rows] if d0_c is not None else None
        d1 = d1_c[:rows] if d1_c is not None else None
        M.set_ones_column(xin, ones >= 0)
        return idx, xin, act, d0, d1

    def _small(self, name, numel, dtype, device):
        """A cached device buffer whose size does not follow the row count (the row-sized workspace rounds up to a whole chunk)."""
        t = self._small_bufs.get(name)
        if t is None or t.numel() != numel or t.dtype != dtype or t.device != device:
            self._small_bufs[name] = t = torch.empty(numel, dtype=dtype, device=device)
        return t

    # ---- a learned log-std (policies: learn_std=True): the heads read it on the device and leave each row's d loss / d log_std in a
    # [rows][4] side output; tg_log_std_grad sums a chunk's rows into log_std's window of the gradient bucket ----
    def _learned_std(self):
        """policy.log_std (a device f32 Parameter whose .grad is its window of the flat bucket), or None: a fixed covariance, and
        none of the `_std` entry points is touched."""
        ls = getattr(self.policy, "log_std", None)
        if ls is None:
            return None
        if ls.dtype != torch.float32 or not ls.is_cuda or ls.numel() > 4:
            raise ValueError(f"a learned log_std must be a float32 device parameter of at most 4 action dimensions, got {ls.dtype} "
                             f"{tuple(ls.shape)} on {ls.device}")
        return ls

    def _std_rows(self, rows, dev, cap):
        return self._ws.get("std_rows", rows, 4, torch.float32, dev, cap)

    def _std_reduce(self, ls, std_rows, add=0.0):
        K.log_std_grad(std_rows, ls.numel(), ls.grad, add=add,
                       work=self._small("std_work", 4 * K.N.load().tg_log_std_grad_blocks(), torch.float64, ls.device))

    def _std_record(self, ls):
        """sum(log_std) BEFORE the coming optimizer step into the next row of this learn()'s [64] blocks (read by last_stats)."""
        torch.sum(ls.detach(), dim=0, keepdim=True, out=self._std_log.next_row(ls.device))

    def _logp_nograd(self, actor, xin, act, var, out=None):
        if out is None:
            out = torch.empty(xin.shape[0], dtype=torch.float32, device=xin.device)
        for lo in range(0, xin.shape[0], self.chunk_rows):
            hi = min(lo + self.chunk_rows, xin.shape[0])
            mean = self._forward(actor, xin[lo:hi], view=True)
            K.gaussian_logp(mean, act[lo:hi], var, out=out[lo:hi])
        return out

    # ---- kl_stats / desired_kl: how far this learn() moved the policy, measured ONCE after its last optimizer step, and rsl_rl's
    # adaptive learning rate from it ("KL-adaptive learning rate").  Off: nothing below runs ----
    # ---- target_kl / kl_every: the same measurement BETWEEN the optimizer steps of a learn() ("Per-update KL
    # control"): tg_kl_control acts on a device control block, the optimizer launches read it, and the host only ever follows ----
    _KL_BREAK_LAG = 1               # the host reads the check this many checks back before it enqueues more (None: it never breaks)
    _KL_LIST_KEYS = ("J", "kl_ref", "actor_loss", "critic_loss", "kl_div", "total_loss", "entropy", "grad_norm")     # one entry per step
    _kl_run = None

    def _kl_setup(self, kl_stats, desired_kl, lr_bounds, lr_factor, target_kl=None, kl_stop_factor=1.5, kl_every=None):
        def number(x):
            return not isinstance(x, bool) and isinstance(x, (int, float)) and math.isfinite(x)
        if not isinstance(kl_stats, bool):
            raise ValueError(f"kl_stats must be True or False, got {kl_stats!r}")
        if desired_kl is not None and not (number(desired_kl) and desired_kl > 0):
            raise ValueError(f"desired_kl must be None or a finite number > 0, got {desired_kl!r}")
        try:
            lo, hi = lr_bounds
        except (TypeError, ValueError):
            raise ValueError(f"lr_bounds must be a pair (lr_min, lr_max), got {lr_bounds!r}") from None
        if not (number(lo) and number(hi) and 0 < lo <= hi):
            raise ValueError(f"lr_bounds must be finite numbers with 0 < lr_min <= lr_max, got {lr_bounds!r}")
        if not (number(lr_factor) and lr_factor > 1):
            raise ValueError(f"lr_factor must be a finite number > 1, got {lr_factor!r}")
        if target_kl is not None and not (number(target_kl) and target_kl > 0):
            raise ValueError(f"target_kl must be None or a finite number > 0, got {target_kl!r}")
        if not (number(kl_stop_factor) and kl_stop_factor > 0):
            raise ValueError(f"kl_stop_factor must be a finite number > 0, got {kl_stop_factor!r}")
        if kl_every is not None and (isinstance(kl_every, bool) or not isinstance(kl_every, int) or kl_every < 1):
            raise ValueError(f"kl_every must be None or an integer >= 1, got {kl_every!r}")
        if kl_every is not None and target_kl is None and desired_kl is None:
            raise ValueError(f"kl_every = {kl_every!r} schedules checks that nothing acts on: give target_kl or desired_kl with it")
        self.kl_stats = kl_stats or desired_kl is not None or target_kl is not None
        self.desired_kl = None if desired_kl is None else float(desired_kl)
        self.lr_bounds, self.lr_factor = (float(lo), float(hi)), float(lr_factor)
        self.target_kl = None if target_kl is None else float(target_kl)
        self.kl_stop_factor, self.kl_every = float(kl_stop_factor), kl_every
        self._kl_ctl = target_kl is not None or kl_every is not None        # checks between the optimizer steps, a control block
        self._kl_adapt_checks = desired_kl is not None and kl_every is not None      # ... whose lr the optimizer launches read
        self._kl_rows = []                                                  # pinned f64 [64][8] blocks: one row per check of a learn()
        self._kl_pending = self._kl_pinned = self._kl_host = self._kl_run = None
        self._kl_bounds_checked = False
        if self.desired_kl is not None:
            self._kl_group_lr()

    def _kl_group_lr(self) -> float:
        """The one learning rate of the optimizer's param groups (desired_kl scales ONE number)."""
        lrs = [float(g["lr"]) for g in self.optimizer.param_groups]
        if any(lr != lrs[0] for lr in lrs):
            raise ValueError(f"desired_kl adapts one learning rate, the optimizer's param groups hold {sorted(set(lrs))}")
        return lrs[0]

    def _kl_entry_check(self):
        """First learn() with desired_kl: the optimizer's lr must lie inside lr_bounds (the rule clamps only what it changes)."""
        if self.desired_kl is None or self._kl_bounds_checked:
            return
        lr, (lo, hi) = self._kl_group_lr(), self.lr_bounds
        if not lo <= lr <= hi:
            raise ValueError(f"the optimizer's lr = {lr} lies outside lr_bounds = {self.lr_bounds}")
        self._kl_bounds_checked = True

    def _shift_sums(self, actor, xin, act, old_logp, var, ls, cap):
        """What a check and the end-of-learn() measurement share: one no-grad actor pass over this learn()'s rows, chunk by chunk, each
        chunk's means into tg_policy_shift with the actions and the old log-probabilities (a learned log_std stays on the device), the
        partials' sums, all-reduced.  Returns the device f64 buffer whose first four entries they are: sums [4] | tg_lr_adapt's {kl,
        clip_fraction, lr_in, lr_out} | with checks between the steps, the control block [8]."""
        dev, rows = xin.device, xin.shape[0]
        chunks = [(lo, min(lo + self.chunk_rows, rows)) for lo in range(0, rows, self.chunk_rows)]
        cap = max(cap, rows, 1)                                             # (sized for the largest iteration this buffer can bring)
        n_part = (cap // self.chunk_rows) * K.policy_shift_blocks(self.chunk_rows) + K.policy_shift_blocks(cap % self.chunk_rows)
        partials = self._small("shift_partials", 4 * n_part, torch.float64, dev).view(-1, 4)
        out = self._small("shift_out", 16 if self._kl_ctl else 8, torch.float64, dev)
        log_lo, log_hi = math.log1p(-float(self.epsilon)), math.log1p(float(self.epsilon))
        slot = 0
        for lo, hi in chunks:
            mean = self._forward(actor, xin[lo:hi], view=True)
            slot += K.policy_shift(mean, act[lo:hi], old_logp[lo:hi], var, log_lo, log_hi, partials, slot, log_std=ls)
        K.policy_shift_finish(partials, slot, out[:4])
        D.allreduce_sum_(out[:4], self.process_group, "policy_shift")
        return out

    def _measure_shift(self, actor, xin, act, old_logp, var, ls, cap):
        """After the last optimizer step, before old_policy <- policy: _shift_sums(), then tg_lr_adapt with the current lr BY VALUE;
        {sums, kl, clip fraction, lr_in, lr_out} to pinned memory behind an event.  Nothing here waits, and nothing it writes is read
        by an update.  With per-update adaptation (desired_kl and kl_every) the rate lives in the control block: tg_kl_control applies
        the rule there (target_kl = 0: nothing is left to stop; a latched block stays -- its last check measured these very weights)
        and tg_lr_adapt only measures.  The control block travels behind the eight numbers."""
        out = self._shift_sums(actor, xin, act, old_logp, var, ls, cap)
        dev, run = xin.device, self._kl_run
        adapt = self.desired_kl is not None
        if run is not None and self._kl_adapt_checks:
            K.kl_control(out[:4], 0.0, 1.0, self.desired_kl, self.lr_factor, *self.lr_bounds, max(run["enqueued"], 1), run["ctl"])
            K.lr_adapt(out[:4], 0.0, self.lr_factor, *self.lr_bounds, run["lr"], out[4:8])
        else:
            lr = self._kl_group_lr() if adapt else float(self.optimizer.param_groups[0]["lr"])
            K.lr_adapt(out[:4], self.desired_kl if adapt else 0.0, self.lr_factor, *self.lr_bounds, lr, out[4:8])
        if self._kl_pinned is None:
            self._kl_pinned = torch.empty(out.numel(), dtype=torch.float64).pin_memory()
        self._kl_pinned.copy_(out, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(dev))
        self._kl_pending, self._kl_run = (self._kl_pinned, ev, run), None

    def _kl_begin(self, actor, xin, act, old_logp, var, ls, cap):
        """target_kl / kl_every: this learn()'s control block {0, lr, 0, 0, nan, nan, 0, 0} -- one copy from pinned memory, no wait --
        and the arguments every check of it takes.  Called once the rows are prepared and the last learn()'s result has been applied."""
        if not self._kl_ctl:
            return
        dev = xin.device
        lr = self._kl_group_lr() if self._kl_adapt_checks else float(self.optimizer.param_groups[0]["lr"])
        ctl = self._small("shift_out", 16, torch.float64, dev)[8:]
        nan = float("nan")
        # (a new pinned tensor: the host allocator keeps its block until the copy has run)
        ctl.copy_(torch.tensor([0.0, lr, 0.0, 0.0, nan, nan, 0.0, 0.0], dtype=torch.float64).pin_memory(), non_blocking=True)
        self._kl_run = {"ctl": ctl, "lr": lr, "lr_host": lr, "enqueued": 0, "checks": [], "latched": False, "fused": True,
                        "args": (actor, xin, act, old_logp, var, ls, cap), "every": self.kl_every or 1}

    def _kl_check(self):
        """One check: _shift_sums(), tg_kl_control on the control block, the block to this check's own pinned row behind its own event."""
        run = self._kl_run
        out = self._shift_sums(*run["args"])
        K.kl_control(out[:4], self.target_kl or 0.0, self.kl_stop_factor, self.desired_kl if self._kl_adapt_checks else 0.0, self.lr_factor,
                     *self.lr_bounds, run["enqueued"], run["ctl"])
        i = len(run["checks"])
        if i // 64 >= len(self._kl_rows):
            self._kl_rows.append(torch.empty(64, 8, dtype=torch.float64).pin_memory())
        row = self._kl_rows[i // 64][i % 64]
        row.copy_(run["ctl"], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(out.device))
        run["checks"].append((row, ev))

    def _kl_read(self, i) -> bool:
        """Wait for check i of this learn() and read its row: True when the device has latched.  On the waiting path (an optimizer
        the fused step does not take) the row's lr goes into the param groups right here."""
        run = self._kl_run
        row, ev = run["checks"][i]
        ev.synchronize()
        if not run["fused"] and self._kl_adapt_checks:
            lr = float(row[1])
            for g in self.optimizer.param_groups:
                if float(g["lr"]) == run["lr_host"]:
                    g["lr"] = lr
            run["lr_host"] = lr
        run["latched"] = float(row[0]) != 0.0
        return run["latched"]

    def _kl_after_step(self, last) -> bool:
        """Called behind every optimizer step of a learn(); True: leave the update loop(s).  Enqueues the check that follows every
        kl_every-th step but the last, then reads the check _KL_BREAK_LAG checks back -- every rank the same all-reduced bits, so all
        ranks leave at the same step.  The device has decided long before: the steps enqueued behind a latch change nothing."""
        run = self._kl_run
        if run is None:
            return False
        if run["latched"]:                  # (the waiting path read the latch in front of this step and did not take it)
            return True
        if last or run["enqueued"] % run["every"]:
            return False
        self._kl_check()
        lag = self._KL_BREAK_LAG if run["fused"] else 0
        if lag is None or len(run["checks"]) <= lag:
            return False
        return self._kl_read(len(run["checks"]) - 1 - lag)

    def _kl_sync(self):
        """The last measurement, once its copy has landed (it was enqueued behind the updates of the learn() that made it; the next
        learn() asks only after it has waited for the next rollout's row count, which runs behind them): lr_out into every param group
        that still holds lr_in -- a group the user has changed since keeps the user's value.  With a control block: the CPU step
        counters, advanced per enqueued step, go back to steps at entry + steps applied, and the rate is the block's."""
        if self._kl_pending is None:
            return
        (host, ev, run), self._kl_pending = self._kl_pending, None
        ev.synchronize()
        vals = host.tolist()
        n, _, _, s_d, kl, clip_fraction, lr_in, lr_out = vals[:8]
        info = {}
        if run is not None:
            ctl = vals[8:16]
            stopped = ctl[0] != 0.0
            applied = int(ctl[2]) if stopped else run["enqueued"]
            if run["enqueued"] > applied:
                for g in self.optimizer.param_groups:
                    for p in g["params"]:
                        if "step" in self.optimizer.state.get(p, {}):
                            self.optimizer.state[p]["step"] -= run["enqueued"] - applied
            if self._kl_adapt_checks:
                lr_in, lr_out = run["lr_host"], ctl[1]
            kls, lrs = [], []
            for row, _ in run["checks"]:    # (the rows behind a latch repeat it)
                r = row.tolist()
                kls.append(r[4])
                lrs.append(r[1])
                if r[0] != 0.0:
                    break
            info = {"n_updates": applied, "kl_stopped": stopped, "kl_checks": kls, "lr_checks": lrs}
        if self.desired_kl is not None:
            for g in self.optimizer.param_groups:
                if float(g["lr"]) == lr_in:
                    g["lr"] = lr_out
        self._kl_host = {"approx_kl": kl, "clip_fraction": clip_fraction, "log_ratio_mean": s_d / n if n > 0 else float("nan"), **info}

    def _kl_stats_read(self) -> dict:
        self._kl_sync()
        return {**(self._kl_host or {}), "lr": float(self.optimizer.param_groups[0]["lr"])}

    def _kl_metadata(self) -> dict:
        if not self.kl_stats:
            return {}
        out = {}
        if self.target_kl is not None:
            out.update({"target_kl": self.target_kl, "kl_stop_factor": self.kl_stop_factor})
        if self.kl_every is not None:
            out["kl_every"] = self.kl_every
        if self.desired_kl is not None:
            out.update({"desired_kl": self.desired_kl, "lr_bounds": list(self.lr_bounds), "lr_factor": self.lr_factor})
        return out or {"kl_stats": True}


def _check_ref_model(ref_model, policy):
    """GRPO's reference policy: one of the project's Gaussian policies, on the policy's device, with the policy's input and output
    widths (its hidden shape is its own)."""
    if ref_model is None:
        return None
    if not isinstance(ref_model, (P.GaussianActor_NeuralNetwork, P.GaussianActorCritic_NeuralNetwork)):
        raise ValueError(f"ref_model must be a GaussianActor_NeuralNetwork or GaussianActorCritic_NeuralNetwork, got {type(ref_model).__name__}")
    def widths(net):
        lin = [m for m in net.network if isinstance(m, torch.nn.Linear)]
        return lin[0].in_features, lin[-1].out_features
    if widths(ref_model.actor) != widths(policy.actor):
        raise ValueError(f"ref_model's actor maps {widths(ref_model.actor)[0]} -> {widths(ref_model.actor)[1]}, the policy's "
                         f"{widths(policy.actor)[0]} -> {widths(policy.actor)[1]}: the widths must agree")
    d_ref, d_pol = next(ref_model.actor.parameters()).device, next(policy.actor.parameters()).device
    if d_ref != d_pol:
        raise ValueError(f"ref_model is on {d_ref}, the policy on {d_pol}: the reference pass runs on the policy's device")
    if (getattr(ref_model, "obs_norm", None) is None) != (getattr(policy, "obs_norm", None) is None):
        raise ValueError("ref_model and the policy must agree on normalize_obs: one of them reads normalised observations, the other raw "
                         "ones (the reference policy reads states through its OWN statistics, frozen)")
    if getattr(policy, "obs_norm", None) is not None and ref_model.obs_norm is policy.obs_norm:
        raise ValueError("ref_model shares the policy's obs_norm object: every learn() would update the reference policy's statistics.  "
                         "Give it its own (copy.deepcopy(policy) does)")
    return ref_model


class GRPO(_GpuLearner):
    """Group Relative Policy Optimization.  algorithms/grpo.py:12-169.

    ref_model (with beta != 0): the KL penalty to a frozen reference policy of DeepSeekMath's GRPO, as grpo.py:127-134 means it
    ("GRPO ref_model").  Per valid row, x = log pi_ref(a|s) - log pi(a|s) with each policy's own variance and
    D = exp(x) - x - 1; J = (sum min(rho A, clip(rho) A) - beta sum D) / G.  log pi_ref is computed once per learn() (no grad) on the
    same compacted rows the updates read; last_stats gains "kl_ref" (the mean D of each update).  Only valid rows count (the
    reference evaluates the reference policy on all rows: that form cannot be combined with the masked surrogate).  The sign is the
    reference's: with the default maximize=False (descent on J as grpo.py writes it) the beta term pushes the policy AWAY from the
    reference policy -- pass maximize=True for a penalty that keeps it close.  ref_model=None or beta == 0: no reference pass, the
    plain kernels, bit-identical to a GRPO without ref_model.

    max_grad_norm (a finite number > 0): `torch.nn.utils.clip_grad_norm_(policy.parameters(), max_grad_norm)` between backward() and
    optimizer.step() of every update, on the device ("Gradient clipping"): the norm of the all-reduced gradient
    bucket, the step on g * min(1, max_grad_norm / (norm + 1e-6)); last_stats gains "grad_norm" (the pre-clip norm of each update).
    None: no clipping, the launches of a learner without the keyword.

    desired_kl (a finite number > 0; lr_bounds, lr_factor): rsl_rl's adaptive learning rate, once per learn() (INTEGRATION.md,
    "KL-adaptive learning rate").  Behind the last optimizer step one no-grad actor pass measures, on this iteration's valid rows of
    all ranks, d = log pi(a|s) - logp_old: last_stats gains "approx_kl" (mean expm1(d) - d), "clip_fraction" (share of rows with
    exp(d) outside 1 -+ epsilon), "log_ratio_mean" and "lr"; kl > 2 desired_kl divides the optimizer's lr by lr_factor, kl <
    desired_kl / 2 multiplies it, inside lr_bounds, applied before the next learn()'s first optimizer step (and by last_stats and
    save()) without a stall.  kl_stats=True: measure and report only.  Off: no launch, allocation, collective or entry point more,
    and on, the updates themselves are those of a learner without the keywords, bit for bit.

    target_kl (a finite number > 0; kl_stop_factor, kl_every): early stopping of the updates of a learn() ("Per-update
    KL control").  Behind every kl_every-th optimizer step but the last (default: every one) a check runs the same measurement;
    once a check's approx_kl exceeds kl_stop_factor * target_kl, no further optimizer step of this learn() changes anything: the
    verdict lives in a device control block (tg_kl_control) that the optimizer launches read (tg_adam_step*_ctl), and the host
    follows _KL_BREAK_LAG checks behind.  desired_kl with an integer kl_every applies the lr rule at every check, on the device,
    instead of once per learn().  last_stats gains "n_updates", "kl_stopped", "kl_checks", "lr_checks" and its per-update lists end
    with the last update applied; .grad after an early stop holds whatever the last enqueued update left.  Off: nothing more runs.

    baseline="step" ("GRPO step baselines"): the advantage of a valid (episode, t) is its return-to-go minus the mean
    return-to-go of the episodes of ITS group that are alive at step t -- with restart groups a Monte-Carlo estimate of the value
    there -- in place of the reference's one mean over all of the group's (episode, t) (grpo.py:110-115, baseline="group", the
    default).  adv_scale="std" divides the residuals by one pooled within-step std per group (+ 1e-8), "none" leaves them as they
    are.  One entry point, tg_grpo_step_advantage (two launches), ahead of the row compaction; the groups are whole on a rank, so
    no collective per update is added.  last_stats gains "baseline" and "baseline_explained", the share of the return-to-go's
    within-group variance that the step means remove.  baseline="group": the launches of a learner without the keyword."""

    BASELINES, ADV_SCALES = ("group", "step"), ("std", "none")

    def __init__(self, epsilon: float, beta: float, gamma: float, policy, optimizer, ref_model=None,
                 updates_per_iter: int = 10, *, maximize: bool = False, chunk_rows=None, autocast_dtype=None,
                 process_group=None, fused_mlp: bool = True, max_grad_norm=None, kl_stats: bool = False, desired_kl=None,
                 lr_bounds=(1e-5, 1e-2), lr_factor: float = 1.5, baseline: str = "group", adv_scale: str = "std", target_kl=None,
                 kl_stop_factor: float = 1.5, kl_every=None):
        if baseline not in self.BASELINES:
            raise ValueError(f"baseline must be one of {self.BASELINES}, got {baseline!r}")
        if adv_scale not in self.ADV_SCALES:
            raise ValueError(f"adv_scale must be one of {self.ADV_SCALES}, got {adv_scale!r}")
        if baseline == "group" and adv_scale != "std":
            raise ValueError(f"baseline='group' divides by the group's std (adv_scale='std'), got adv_scale={adv_scale!r}: "
                             "adv_scale chooses the divisor of baseline='step'")
        self.baseline, self.adv_scale = baseline, adv_scale
        self._baseline_sums = None
        self.epsilon, self.beta, self.gamma = epsilon, beta, gamma
        self.ref_model = _check_ref_model(ref_model, policy)
        self.updates_per_iter = updates_per_iter
        self.maximize = maximize
        self._setup(policy, optimizer, chunk_rows, autocast_dtype, process_group, fused_mlp, max_grad_norm,
                    kl_stats, desired_kl, lr_bounds, lr_factor, target_kl, kl_stop_factor, kl_every)
        self.old_policy = self._make_old_policy()                           # grpo.py:48
        self._old_synced = self._actor_keys()

    def _ref_input(self, ref_actor, xin, in_dim, cap, traj=None, idx=None):
        """The reference actor's input rows: the policy's prepared `xin` itself when the reference net takes the same padded layout,
        else re-prepared from its first `in_dim` columns (a reference net of another shape / path).  A reference policy with a
        normaliser never shares `xin` (those rows went through the POLICY's table): its rows are the valid rows' raw observations
        through its own statistics."""
        m = self._mlp(ref_actor)
        ref_on = getattr(self.ref_model, "obs_norm", None)
        if ref_on is not None:
            X = traj.obs_rows().index_select(0, idx)
            if m is None:
                return ref_on.normalize(X)
            return m.prepare_input(X, out=self._ws.get("xin_ref", X.shape[0], m.in_pad, m.cd, X.device, cap), obs_norm=ref_on)
        if m is not None and m.in_pad == xin.shape[1] and m.cd == xin.dtype:
            return xin                                  # (a ones column at 31 meets zero weights in the forward pass)
        X = xin[:, :in_dim].float()
        if m is None:
            return X
        return m.prepare_input(X, out=self._ws.get("xin_ref", X.shape[0], m.in_pad, m.cd, X.device, cap))

    def _advantage_source(self, traj, rtg, moments):
        """(src0, moments or None, norm_mode) of the row compaction: the [T][n] array the valid rows' advantages are gathered from,
        and the group moments it is normalised with on the way (None: gathered as it is).  "group": the returns-to-go and their
        moments, grpo.py:110-115.  "step": tg_grpo_step_advantage's array, which is the advantage already; the two sums of
        baseline_explained (sum_g Q_g and sum_g (s2 - s1^2 / cnt), the within-group squared deviations after and before the step
        means) stay on the device for last_stats."""
        if self.baseline == "group":
            return rtg, moments, 0
        dev, G = rtg.device, traj.n // traj.E
        adv, group = K.grpo_step_advantage(rtg, traj.mask, traj.E, scale=self.adv_scale == "std",
                                           out=self._ws.get("step_adv", traj.T * traj.n, 1, torch.float32, dev, traj.T * traj.n).view(traj.T, traj.n),
                                           work=self._small("step_work", max(3 * G * traj.T, 1), torch.float64, dev),
                                           group=self._small("step_group", 3 * G, torch.float64, dev).view(G, 3))
        cnt, s1, s2 = moments.unbind(1)
        self._baseline_sums = torch.stack((group[:, 0].sum(), (s2 - s1 * (s1 / cnt.clamp_min(1.0))).sum()))
        return adv, None, 0

    def _learn(self, buffer) -> None:
        traj = device_trajectory(buffer, self.policy.device)
        var = self.policy.var
        rew = traj.rew if traj.rew.dtype == torch.float32 else traj.rew.float()
        if traj.n <= _SMALL_N_RETURNS and traj.T <= K.returns_moments_max_horizon():       # grpo.py:66-74; per group, :110-115
            rtg, moments = K.returns_moments(rew, traj.mask, self.gamma, traj.E)
        else:
            rtg = K.rtg_scan(rew, traj.mask, self.gamma)
            moments = K.masked_moments(rtg, traj.mask, traj.E)
        actor = self.policy.actor
        m_actor = self._mlp(actor)
        # the valid rows: index, padded input row, action and group-relative advantage (grpo.py:76-115) in one pass over the mask --
        # enqueued here; the host asks for the row count (and waits for the rollout's statistic) only after everything that does not
        # depend on it has been enqueued too
        src0, src_moments, norm_mode = self._advantage_source(traj, rtg, moments)
        handle = self._prepare_enqueue(traj, m_actor, src0=src0, moments=src_moments, norm_mode=norm_mode, group_size=traj.E)
        _, world = D.rank_world(self.process_group)
        G_global = traj.G * world
        coef = (-1.0 if self.maximize else 1.0) / G_global                  # J /= group_size, descent on J
        # the KL penalty to the reference policy (grpo.py:127-134): d loss / d (sum D) = -coef * beta
        ref_actor = self.ref_model.actor if (self.ref_model is not None and self.beta != 0 and self.updates_per_iter > 0) else None
        ref_coef = coef * float(self.beta) if ref_actor is not None else 0.0
        self._entry_refresh(actor)
        if ref_actor is not None:
            self._entry_refresh(ref_actor)                                  # (the caller may have refreshed the reference policy)
        self._refresh(self.old_policy.actor)
        _ = self.bucket                                                     # (the gradient windows exist before can_fuse_head() asks)
        ls = self._learned_std()                                            # (the old / reference passes keep their host `var`)
        # grpo.py:118-119.  When old_policy still IS the policy (the usual case: grpo.py:148 copied it at the end of the last learn()
        # and nothing has touched either since), its log-probabilities are the ones the first update's forward pass computes
        # anyway: that pass writes them (ratio exactly 1 there, as in the reference) and the no-grad pass is not run.
        fold_old = (_FOLD_OLD_LOGP and self.updates_per_iter > 0 and m_actor is not None and m_actor.can_write_old_logp()
                    and self._old_actor_is_current())
        if fold_old and not M.N.TRUST_KEYS:
            self._verify_old_is_current()
        all_sums = torch.zeros(max(self.updates_per_iter, 1), 4, dtype=torch.float64, device=traj.mask.device)
        if self.updates_per_iter > 0:
            self._zero_grads()                                              # (the first update's, ahead of the wait below)
        prepared = self._prepare_finish(handle)
        self._kl_sync()                                                     # (the last learn()'s adapted lr: landed long ago)
        if prepared is not None:
            idx, xin, act, adv, _ = prepared
        else:
            adv_full = src0 if src_moments is None else K.group_normalize(src0, traj.mask, src_moments, norm_mode, traj.E)
            idx, X, act = self._gather_valid(traj)
            adv = adv_full.reshape(-1).index_select(0, idx)
            xin = self._prep(actor, X, traj.T * traj.n)
        X = xin                                                             # (the loops below only ask for its row count and device)
        old_logp = (self._ws.get("old_logp", X.shape[0], 1, torch.float32, X.device, traj.T * traj.n).view(-1) if fold_old else
                    self._logp_nograd(self.old_policy.actor, xin, act, self.old_policy.var if ls is not None else var))
        ref_logp = None
        if ref_actor is not None:                                           # once per learn(): the reference policy is frozen
            in_dim = next(m for m in ref_actor.network if isinstance(m, torch.nn.Linear)).in_features
            ref_logp = self._logp_nograd(ref_actor, self._ref_input(ref_actor, xin, in_dim, traj.T * traj.n, traj, idx), act, self.ref_model.var,
                                         out=self._ws.get("ref_logp", X.shape[0], 1, torch.float32, X.device, traj.T * traj.n).view(-1))
        self._kl_begin(actor, xin, act, old_logp, var, ls, traj.T * traj.n)
        for u in range(self.updates_per_iter):
            if u > 0:
                self._zero_grads()
            sums = all_sums[u]
            fuse = m_actor is not None and m_actor.can_fuse_head()
            last = u == self.updates_per_iter - 1
            rider = None
            for lo in range(0, X.shape[0], self.chunk_rows):
                hi = min(lo + self.chunk_rows, X.shape[0])
                std_rows = self._std_rows(hi - lo, X.device, traj.T * traj.n) if ls is not None else None
                if fuse:        # loss head + head gradient inside the forward chain (tg_mlp_forward_chain_loss)
                    m_actor.forward_loss(xin[lo:hi], 0, act=act[lo:hi], logp_old=old_logp[lo:hi], adv=adv[lo:hi],
                                         var=None if ls is not None else var,
                                         epsilon=self.epsilon, surr_coef=coef, sums_out=sums,
                                         logp_old_out=old_logp[lo:hi] if (fold_old and u == 0) else None,
                                         logp_ref=ref_logp[lo:hi] if ref_logp is not None else None, ref_coef=ref_coef,
                                         log_std=ls, std_out=std_rows)
                    if ls is not None:
                        self._std_reduce(ls, std_rows)
                    # (asked for right before the launch it rides on: it marks the weight layouts as current; with a learned log_std
                    # the optimizer owns more than the net's parameters and the rider declines)
                    rider = self._adam_rider(actor, last, whole_update=lo == 0 and hi == X.shape[0])
                    m_actor.backward_fused(adam=rider)
                    continue
                else:
                    mean = self._forward(actor, xin[lo:hi], train=True, view=True)     # the loss kernel takes a row stride
                    _, s, g_mean, _ = K.surrogate_loss(mean.detach(), None, act[lo:hi], old_logp[lo:hi], adv[lo:hi], None,
                                                       None, None, var, self.epsilon, coef, 0.0, 0.0, want_total=False,
                                                       logp_ref=ref_logp[lo:hi] if ref_logp is not None else None, ref_coef=ref_coef,
                                                       log_std=ls, std_out=std_rows)
                    if ls is not None:
                        self._std_reduce(ls, std_rows)
                    self._backward(actor, mean, g_mean)
                sums += s
            if rider is not None:                                            # (one rank: no all-reduce; the step rode on the reduction)
                self._refresh(actor)                                         # (what the rider does not write -- "w", "dx" -- is stale now)
                continue
            self.bucket.allreduce(self.process_group)                        # one RCCL all-reduce / step
            self._optimizer_step(actor, last=last)
            if self._kl_after_step(last):                                   # (target_kl: the device has stopped, the host follows)
                break
        self._check_deferred()                                              # (this learn()'s own row count / fold flag: landed long ago)
        if self.kl_stats:
            self._measure_shift(actor, xin, act, old_logp, var, ls, traj.T * traj.n)
        self._copy_policy_to_old()                                          # grpo.py:148
        if self.updates_per_iter > 0:
            allJ = all_sums
            D.allreduce_sum_(allJ, self.process_group, "loss_stats")
            ls_end = ls.detach().clone() if ls is not None else None        # (after the last step; read when last_stats is)
            extra = (lambda: {"log_std": ls_end.tolist()}) if ls_end is not None else dict
            if ref_actor is None:
                self._stats_pending = lambda: {"J": (allJ[:, 0] / G_global).tolist(), "n_valid": allJ[0, 3].item(), **extra()}
            else:                                                           # slot 2: sum D (GRPO's heads have kl_coef = 0)
                beta = float(self.beta)
                self._stats_pending = lambda: {"J": ((allJ[:, 0] - beta * allJ[:, 2]) / G_global).tolist(), "n_valid": allJ[0, 3].item(),
                                               "kl_ref": (allJ[:, 2] / allJ[:, 3].clamp_min(1.0)).tolist(), **extra()}
        if self.baseline != "group":
            sums, self._baseline_sums = self._baseline_sums, None
            D.allreduce_sum_(sums, self.process_group, "baseline_explained")   # (the one collective of the feature: two f64 per learn())
            inner, name = self._stats_pending or dict, self.baseline

            def with_baseline():
                q, dev2 = sums.tolist()
                return {**inner(), "baseline": name, "baseline_explained": 1.0 - q / dev2 if dev2 > 0 else float("nan")}
            self._stats_pending = with_baseline

    def save(self, path: str) -> None:
        self._kl_sync()                                                     # (the checkpoint holds the adapted lr)
        torch.save(self.optimizer.state_dict(), os.path.join(path, "optimizer.pth"))   # grpo.py:154

    def load(self, path: str) -> None:
        self.optimizer.load_state_dict(torch.load(os.path.join(path, "optimizer.pth"), weights_only=True))

    def metadata(self):
        return {"algorithm": "GRPO", "epsilon": self.epsilon, "beta": self.beta,
                "updates_per_iter": self.updates_per_iter, **self._clip_metadata(), **self._kl_metadata(),
                **({} if self.baseline == "group" else {"baseline": self.baseline, "adv_scale": self.adv_scale})}


def _value_norm_stats(stat3, moments, eps, stat_a=None) -> dict:
    """last_stats' entries of a value-normalised PPO.learn(), from device copies of its {count, mean, m2} after the merge and of the
    all-reduced moments [2][3] = {n, sum, sum of squares} of the valid advantages and returns.  value_std is the table's sigma,
    sqrt(m2 / count + eps) (1 while count == 0); explained_variance = 1 - var(adv) / var(ret) with population variances
    (s2 - s1 (s1 / n)) / n clamped at 0 -- adv = ret - V on the valid rows in both modes -- and NaN when var(ret) == 0.
    stat_a (a PopArt policy: {count, mean, m2} before the merge): "popart_scale" = sigma_a / sigma_n and "popart_shift" = mean_a - mean_n
    of the rescale this learn() applied to the critic head, in the kernel's f64 operations; 1 and 0 where the head kept its bits."""
    count, mean, m2 = stat3.tolist()
    (na, a1, a2), (nr, r1, r2) = moments.tolist()
    var_a = max(a2 - a1 * (a1 / na), 0.0) / na if na > 0 else float("nan")
    var_r = max(r2 - r1 * (r1 / nr), 0.0) / nr if nr > 0 else float("nan")
    out = {"value_mean": mean if count > 0 else 0.0, "value_std": math.sqrt(m2 / count + eps) if count > 0 else 1.0, "value_count": count,
           "explained_variance": 1.0 - var_a / var_r if var_r > 0 else float("nan")}
    if stat_a is not None:
        count_a, mean_a, m2_a = stat_a.tolist()
        out["popart_scale"], out["popart_shift"] = 1.0, 0.0
        if count_a > 0 and count > count_a:                                 # (a batch was merged into statistics that were not empty)
            sigma_a, sigma_n = math.sqrt(m2_a / count_a + eps), math.sqrt(m2 / count + eps)
            if 0 < sigma_a < math.inf and 0 < sigma_n < math.inf:
                out["popart_scale"], out["popart_shift"] = sigma_a / sigma_n, mean_a - mean
    return out


def privileged_spec(policy, env, params=None) -> "K.N.PrivilegedSpec":
    """tg_privileged_spec of a policy's privileged_critic for `env`: column k is the mapping's k-th name (the mapping's order, not
    p[]'s), index[k] its p[] slot (env.parameter_slots()), nominal[k] the env's own value there (params: its tg_env_params, default
    env.native_params()), centre and scale the policy's.  ValueError names a parameter the env does not have."""
    want = policy.privileged_critic
    slots = env.parameter_slots()
    unknown = [name for name in want if name not in slots]
    if unknown:
        raise ValueError(f"privileged_critic names {unknown}, which {type(env).__name__} cannot randomise "
                         f"(randomisable: {', '.join(slots)})")
    if params is None:
        params = env.native_params()
    spec = K.N.PrivilegedSpec()
    spec.count = len(want)
    for k, name in enumerate(want):
        spec.index[k] = slots[name]
        spec.nominal[k] = float(params.p[spec.index[k]])
        spec.center[k], spec.scale[k] = policy.privileged_center[k], policy.privileged_scale[k]
    return spec


class PPO(_GpuLearner):
    """Proximal Policy Optimization.  algorithms/ppo.py:8-225.

    A policy built with privileged_critic={name: (lo, hi)} ("Privileged critic"): the critic also reads the physical
    parameters each env slot was rolled out with (Env.randomize with the same mapping; the buffer's rollout engine holds the table).
    The actor's rows are prepared as always; one tg_privileged_rows launch forms the critic's rows from them, and the two nets keep
    their own learners and input pads.  A plain policy: not one launch, allocation or entry point more.

    max_grad_norm: as GRPO's -- one norm over the actor's and the critic's gradients together (one optimizer), before every optimizer
    step (every minibatch's in minibatch mode); last_stats gains "grad_norm", one entry per step.

    bootstrap_truncated=True: an episode the CLOCK ended (not a failure, not Pendulum's balance terminal) has its cut return
    completed with the critic's value of the state its last step produced ("Time-limit bootstrapping"): returns and
    advantages are those of the rewards with gamma * V(s_final) added to the episode's last step, Monte Carlo and GAE alike, computed
    on the device in the prologue; the trajectory's rewards are not modified.  last_stats gains "n_bootstrapped" (episodes
    bootstrapped, over all ranks).  Needs the buffer's rollout engine (the env parameters); swarm envs are refused.  False: the
    launches of a learner without the keyword.

    A policy built with normalize_value=True (policy.value_norm; INTEGRATION.md, "Value normalisation"): the critic predicts returns
    standardised with RUNNING statistics.  Every critic value that enters a return -- the valid rows on the [T][n] grid, the bootstrap
    rows -- is denormalised on the device with the table as it stands at the entry of learn(); the returns' all-reduced moments are
    merged into the statistics (unless frozen) and the critic regresses onto (R - mean) / sigma of the merged statistics, in place of
    the batch's own mean and std.  last_stats gains "value_mean", "value_std", "value_count", "explained_variance".  GRPO ignores it.

    ... and with popart=True as well ("PopArt"): the launch that merges the statistics also rescales the critic's last
    layer, w' = w sigma / sigma', b' = (b sigma + mean - mean') / sigma', so that the critic read with the merged table predicts what
    it predicted with the old one; the critic's derived weight layouts are rebuilt from the rescaled masters before the first update,
    Adam's moments of the head are left alone.  last_stats gains "popart_scale" and "popart_shift".  Frozen statistics, and the
    first learn() (empty statistics): no rescale.  GRPO ignores it.

    kl_stats, desired_kl, lr_bounds, lr_factor: as GRPO's -- measured once per learn() behind its last optimizer step (the last
    minibatch's in minibatch mode), over all valid rows.  ("kl_div" stays the reference's own penalty term.)

    target_kl, kl_stop_factor, kl_every: as GRPO's -- in minibatch mode a check follows every kl_every-th minibatch step, a stop
    leaves both loops, and "n_updates" counts optimizer steps."""

    def __init__(self, epsilon: float, policy, optimizer, ref_model, updates_per_iter: int, c1: float = 0.5,
                 kl_coeff: float = 0.5, gamma: float = 0.99, lam: float = 0.95, entropy: float = 0.01,
                 batch_size: int = 64, monte_carlo: bool = True, *, chunk_rows=None, autocast_dtype=None,
                 process_group=None, seed: int = 0, fused_mlp: bool = True, max_grad_norm=None, bootstrap_truncated: bool = False,
                 kl_stats: bool = False, desired_kl=None, lr_bounds=(1e-5, 1e-2), lr_factor: float = 1.5, target_kl=None,
                 kl_stop_factor: float = 1.5, kl_every=None):
        if not isinstance(bootstrap_truncated, bool):
            raise ValueError(f"bootstrap_truncated must be True or False, got {bootstrap_truncated!r}")
        self.bootstrap_truncated = bootstrap_truncated
        self.epsilon, self.c1, self.ref_model = epsilon, c1, ref_model
        self.updates_per_iter = updates_per_iter
        self.gamma, self.lam, self.entropy = gamma, lam, entropy
        self.batch_size, self.kl_coeff, self.monte_carlo = batch_size, kl_coeff, monte_carlo
        self._setup(policy, optimizer, chunk_rows, autocast_dtype, process_group, fused_mlp, max_grad_norm,
                    kl_stats, desired_kl, lr_bounds, lr_factor, target_kl, kl_stop_factor, kl_every)
        self.old_policy = self._make_old_policy()                           # ppo.py:62 (never read in learn)
        self._seed = seed
        self._gen = None
        # minibatch mode: callable (n_rows, device) -> int64 permutation of this rank's valid rows (time-major order);
        # None = torch.randperm on the device from `seed` (the reference draws torch.randperm on the CPU, ppo.py:148)
        self.permutation_fn = None

    def _step(self, xin, act, adv, ret, old_logp, norm8, var, sums_out, host=None, last=True, write_old=False, xin_c=None):
        """One optimizer step on the given rows (all local rows, or one minibatch).  xin_c: the critic's own input rows (a privileged
        critic), None: the critic reads `xin`.  norm8: the device f32 [8] of tg_ppo_norm -- the
        normalisation constants of ppo.py:138-139 and the 1 / n of :165-179, read by the loss heads on the device.  host: minibatch
        mode only -- (the four normalisation constants as a list, this step's global row count): the 1 / n of a minibatch is its own.
        write_old: this is the first step of a full-batch learn() on a chain learner -- its forward pass WRITES `old_logp` (ppo.py:142-143
        takes the old log-probabilities from the current policy: the same numbers) instead of reading it."""
        actor, critic = self.policy.actor, self.policy.critic
        if xin_c is None:
            xin_c = xin
        self._zero_grads()
        ls = self._learned_std()
        # the entropy bonus (ppo.py:172,179): H = A/2 (1 + log 2 pi) + sum log_std, so -entropy * mean(H) adds exactly -entropy to every
        # component of d loss / d log_std -- once per optimizer step whatever the row count and the world size (rank 0 adds it
        # before the all-reduce), with the first chunk's reduction launch
        ent_add = -float(self.entropy) if (ls is not None and D.rank_world(self.process_group)[0] == 0) else 0.0
        if ls is not None:
            self._std_record(ls)
        # [actor | critic] loss sums: a row of the learn()'s pre-zeroed table when there is one (full batch: one fill per learn(), not per update)
        both = self._sum_rows.pop() if self._sum_rows else torch.zeros(2, 4, dtype=torch.float64, device=xin.device)
        sums = both[0]
        m_a, m_c = self._mlp(actor), self._mlp(critic)
        fuse = m_a is not None and m_c is not None and m_a.can_fuse_head() and m_c.can_fuse_head()
        if host is None:
            dev8, nh, coefs = norm8, (None,) * 4, (0.0, 0.0, 0.0)
        else:
            dev8, nh, n_global = None, host[0], host[1]
            coefs = (-1.0 / n_global, self.c1 / n_global, self.kl_coeff / n_global)
        for lo in range(0, xin.shape[0], self.chunk_rows):
            hi = min(lo + self.chunk_rows, xin.shape[0])
            std_rows = self._std_rows(hi - lo, xin.device, max(xin.shape[0], 1)) if ls is not None else None
            if fuse:            # both loss heads + head gradients inside the forward chains (tg_mlp_forward_chain_loss)
                m_a.forward_loss(xin[lo:hi], 0, act=act[lo:hi], logp_old=old_logp[lo:hi], adv=adv[lo:hi], norm=nh[0:2] if host else None,
                                 var=None if ls is not None else var, epsilon=self.epsilon, surr_coef=coefs[0], kl_coef=coefs[2],
                                 sums_out=both[0], logp_old_out=old_logp[lo:hi] if write_old else None, norm8=dev8,
                                 log_std=ls, std_out=std_rows)
                if ls is not None:
                    self._std_reduce(ls, std_rows, ent_add)
                    ent_add = 0.0
                m_a.backward_fused()
                m_c.forward_loss(xin_c[lo:hi], 1, ret=ret[lo:hi], norm=nh[2:4] if host else None, critic_coef=coefs[1], sums_out=both[1],
                                 norm8=dev8)
                m_c.backward_fused()
                continue
            mean = self._forward(actor, xin[lo:hi], train=True, view=True)         # the loss kernel takes a row stride
            vout = self._forward(critic, xin_c[lo:hi], train=True)
            value = vout.reshape(-1).contiguous()
            _, s, g_mean, g_val = K.surrogate_loss(mean.detach(), value.detach(), act[lo:hi], old_logp[lo:hi], adv[lo:hi],
                                                   ret[lo:hi], None, norm8[:4], var, self.epsilon, coefs[0], coefs[1], coefs[2],
                                                   want_total=False, coef=norm8[4:7] if host is None else None,
                                                   log_std=ls, std_out=std_rows)
            if ls is not None:
                self._std_reduce(ls, std_rows, ent_add)
                ent_add = 0.0
            self._backward(actor, mean, g_mean)
            self._backward(critic, vout, g_val.view_as(vout))
            sums += s
        if ent_add != 0.0:                                                   # (a rank-0 step without rows: an empty minibatch slice)
            ls.grad.add_(ent_add)
        self.bucket.allreduce(self.process_group)                            # one RCCL all-reduce / step
        self._optimizer_step(actor, critic, last=last)
        sums_out.append(both)

    # ---- a privileged critic (policies: privileged_critic={name: (lo, hi)}): the critic's input rows are the actor's prepared rows with
    # the env slot's randomised parameters behind them (tg_privileged_rows); every critic pass reads those rows, every actor pass its own
    def _privileged_setup(self, buffer, traj):
        """None for a plain policy (nothing below is touched); else (tg_privileged_spec, the parameter table f64 [12][n] of the rollout
        that filled `buffer`), after checking that the env draws exactly the parameters and ranges the critic was built for."""
        want = getattr(self.policy, "privileged_critic", None)
        if want is None:
            return None
        engine = getattr(getattr(buffer, "rollout_manager", None), "engine", None)
        if engine is None or getattr(engine, "params", None) is None:
            raise ValueError("a policy with privileged_critic reads each env slot's parameters from buffer.rollout_manager.engine.env_params: "
                             "this buffer has no rollout engine (hand-built tensors?)")
        have = engine.env.randomization
        if have != want:
            raise ValueError(f"the policy's privileged_critic {want} is not the env's randomisation {have}: "
                             f"{type(engine.env).__name__}.randomize() must draw exactly the parameters and ranges the critic was built for")
        table = engine.env_params
        if (not torch.is_tensor(table) or table.dtype != torch.float64 or tuple(table.shape) != (12, traj.n) or not table.is_contiguous()
                or table.device != traj.mask.device):
            raise ValueError(f"privileged_critic needs engine.env_params as a contiguous f64 [12][{traj.n}] table on {traj.mask.device} (the "
                             f"rollout's own), got {None if table is None else (table.dtype, tuple(table.shape), table.device)}")
        return privileged_spec(self.policy, engine.env, engine.params), table

    def _privileged_rows(self, priv, src, S, idx, n, out, ones_col):
        """The one launch that forms the critic's rows: `out` [rows][dst_pad] <- src's first S columns, the parameter features, padding."""
        spec, table = priv
        return K.privileged_rows(src, S, idx, n, table, spec, out, ones_col)

    def _critic_rows(self, priv, xin, idx, S, n, m_a, m_c, get):
        """What the critic's passes read for the actor's prepared rows `xin` (idx: their flat t * n + e, None: row i is env i).  A critic
        on a GemmMLP: [rows][m_c.in_pad] in its compute dtype with its own ones-column rule, marked as set_ones_column marks it; a
        critic on autograd: the [:, :S + P] view of f32 rows padded to a multiple of 4.  An actor without a GemmMLP (or of another
        compute dtype) first has its rows copied into rows padded the same way.  get(name, rows, cols, dtype): the workspace."""
        P, rows = priv[0].count, xin.shape[0]
        if m_c is not None:
            dt, pad = m_c.cd, m_c.in_pad
            ones = 31 if (pad == 32 and m_c.in_dim < 32 and m_c._f32 is None) else -1
        else:
            dt, pad, ones = torch.float32, M._round_up(S + P, 4), -1
        src = xin
        if m_a is None or xin.dtype != dt:
            src = get("priv_src", rows, M._round_up(S, 8 if dt == torch.bfloat16 else 4), dt).zero_()
            src[:, :S].copy_(xin[:, :S])
        xc = self._privileged_rows(priv, src, S, idx, n, get("xin_c", rows, pad, dt), ones)
        if m_c is None:
            return xc[:, :S + P]
        M.set_ones_column(xc, ones >= 0)
        return xc

    def _bootstrap_params(self, buffer):
        """The env parameters tg_rollout_final_state steps with: those of the engine that rolled the buffer's trajectory out."""
        engine = getattr(getattr(buffer, "rollout_manager", None), "engine", None)
        params = getattr(engine, "params", None)
        if params is None:
            raise ValueError("PPO(bootstrap_truncated=True) re-steps each episode's last transition with the env parameters of "
                             "buffer.rollout_manager.engine: this buffer has no rollout engine (hand-built tensors?)")
        if int(params.agents) > 1:
            raise ValueError(f"PPO(bootstrap_truncated=True) does not support swarm envs (agents={int(params.agents)}): a swarm episode "
                             "ends when any of its bodies does, which a body's own final state does not tell")
        return params

    @staticmethod
    def _bootstrap_table(buffer):
        """The per-env parameter table of the engine's last rollout (None unless it was randomised): the re-step must use the vehicle
        each slot was rolled out with."""
        return getattr(buffer.rollout_manager.engine, "env_params", None)

    @staticmethod
    def _bootstrap_substeps(buffer):
        """The physics steps per policy step the engine rolled out with (Env.substeps): the re-step runs the last CONTROL step."""
        return int(getattr(buffer.rollout_manager.engine, "substeps", 1))

    def _bootstrap_values(self, params, traj, critic, m_c, env_params=None, priv=None, substeps=1):
        """(b f32 [n], timeout u8 [n]): b[i] = V(s_final[i]) where the clock ended episode i, else 0 -- the re-step launch, the
        critic's input rows prepared as the valid rows are, one no-grad pass over n rows, one multiply.  Enqueued; no host read.
        priv (a privileged critic): the rows are prepared as the ACTOR's are and each gets its own env's parameters (row i is env i)."""
        n, dev = traj.n, traj.mask.device
        s_final, timeout = K.rollout_final_state(params, traj, self._small("boot_state", n * traj.S, torch.float32, dev).view(n, traj.S),
                                                 self._small("boot_timeout", n, torch.uint8, dev),
                                                 env_params=env_params, **({"substeps": substeps} if substeps != 1 else {}),
                                                 **({"motor": traj.motor} if getattr(traj, "motor", None) is not None else {}))
        on = getattr(self.policy, "obs_norm", None)        # (this learn()'s table: the update ran at the entry)
        if priv is not None:
            m_a = self._mlp(self.policy.actor)
            if m_a is not None:
                xa = m_a.prepare_input(s_final, out=self._small("boot_xin_a", n * m_a.in_pad, m_a.cd, dev).view(n, m_a.in_pad), obs_norm=on)
            else:
                xa = s_final if on is None else on.normalize(s_final)
            xc = self._critic_rows(priv, xa, None, traj.S, n, m_a, m_c,
                                   lambda name, r, c, dt: self._small("boot_" + name, r * c, dt, dev).view(r, c))
            v = m_c.forward(xc, keep=False, padded=True)[:, 0] if m_c is not None else self._forward(critic, xc).reshape(-1)
        elif m_c is not None:
            xin = m_c.prepare_input(s_final, out=self._small("boot_xin", n * m_c.in_pad, m_c.cd, dev).view(n, m_c.in_pad), obs_norm=on)
            v = m_c.forward(xin, keep=False, padded=True)[:, 0]
        else:
            v = self._forward(critic, s_final if on is None else on.normalize(s_final)).reshape(-1)
        vn = getattr(self.policy, "value_norm", None)
        if vn is not None:                                  # (V(s_final) in the returns' units: the table of this learn()'s entry)
            return K.boot_values_affine(v, timeout, vn.table, out=self._small("boot_value", n, torch.float32, dev)), timeout
        return torch.mul(v, timeout, out=self._small("boot_value", n, torch.float32, dev)), timeout

    def _learn(self, buffer) -> None:
        boot_params = self._bootstrap_params(buffer) if self.bootstrap_truncated else None
        boot_table = self._bootstrap_table(buffer) if self.bootstrap_truncated else None
        boot_substeps = self._bootstrap_substeps(buffer) if self.bootstrap_truncated else 1
        traj = device_trajectory(buffer, self.policy.device)
        var = self.policy.var
        T, n = traj.T, traj.n
        cap = T * n
        rew = traj.rew if traj.rew.dtype == torch.float32 else traj.rew.float()
        actor, critic = self.policy.actor, self.policy.critic
        m_a, m_c = self._mlp(actor), self._mlp(critic)
        # a privileged critic (policy.privileged_critic): (spec, parameter table) -- its input rows are the actor's plus the env's
        # parameters, formed by one launch into a workspace of their own; the two nets keep their own learners and pads.  None: off
        priv = self._privileged_setup(buffer, traj)
        if priv is None and m_a is not None and m_c is not None and m_a.in_pad != m_c.in_pad:
            # (only one of the two fits the fp32 chain learner: both take the per-layer path, so that they keep sharing ONE prepared
            # input -- a Tanh net has no per-layer path and goes back to torch autograd instead)
            for net, m in ((actor, m_a), (critic, m_c)):
                if not m.disable_f32_chain():
                    self._mlps[id(net)] = None
            m_a, m_c = self._mlp(actor), self._mlp(critic)
        # the valid rows (ppo.py:126-135): index, padded input row (actor and critic share input width / compute dtype), action --
        # enqueued on the buffers' capacity; the host asks for the row count (and waits for the rollout) only after everything that
        # does not depend on it has been enqueued too
        shared = priv is None and m_c is not None and m_a is not None and m_c.in_pad == m_a.in_pad and m_c.cd == m_a.cd
        handle = self._prepare_enqueue(traj, m_a) if (shared or priv is not None) else None
        self._entry_refresh(actor, critic)
        _ = self.bucket                                                     # (the gradient windows exist before can_fuse_head() asks)
        dev = traj.mask.device
        V = self._ws.get("V", cap, 1, torch.float32, dev, cap).view(T, n)
        V.zero_()                                                           # padded entries: V = 0 (they never reach a result)
        adv_full = self._ws.get("adv_full", cap, 1, torch.float32, dev, cap).view(T, n)
        ret_full = self._ws.get("ret_full", cap, 1, torch.float32, dev, cap).view(T, n)
        work = self._small("ppo_work", 6 * n, torch.float64, dev)
        prepared = self._prepare_finish(handle)
        self._kl_sync()                                                     # (the last learn()'s adapted lr: landed long ago)
        if prepared is not None:
            idx, xin, act, _, _ = prepared
        else:
            idx, X, act = self._gather_valid(traj)
            xin = self._prep(actor, X, cap)
        n_rows = xin.shape[0]
        xin_c = xin if priv is None else self._critic_rows(priv, xin, idx, traj.S, n, m_a, m_c,
                                                           lambda name, r, c, dt: self._ws.get(name, r, c, dt, dev, cap))
        # normalize_value: the critic's outputs are denormalised where they enter a return -- with the statistics the critic was last
        # trained against (the table as it stands here; the identity on the first call) -- and the table moves only after that
        vn = getattr(self.policy, "value_norm", None)
        if vn is not None and (not vn.table.is_cuda or vn.table.device != dev):
            raise ValueError(f"policy.value_norm lives on {vn.table.device}, the trajectory on {dev}")
        # ppo.py:93: V of the valid rows (padded rows are masked in both scans), scattered onto the [T][n] grid by the launch that
        # follows each chunk's no-grad pass
        for lo in range(0, n_rows, self.chunk_rows):
            hi = min(lo + self.chunk_rows, n_rows)
            out = m_c.forward(xin_c[lo:hi], keep=False, padded=True) if m_c is not None else self._forward(critic, xin_c[lo:hi])
            K.scatter_rows(out, idx[lo:hi], V, table=None if vn is None else vn.table)
        # ppo.py:100-124 + the masked moments of :138-139 in two launches; the ranks' sums in one all-reduce; the normalisation
        # constants and 1 / n on the device (tg_ppo_norm): nothing of this visits the host
        n_boot = None
        if boot_params is None:
            moments = K.ppo_returns(rew, V, traj.mask, self.gamma, self.lam, self.monte_carlo, adv_full, ret_full, work)
        else:
            # time-limit bootstrapping: the same two launches on r + gamma * V(s_final) at each clock-ended episode's last step
            boot, timeout = self._bootstrap_values(boot_params, traj, critic, m_c, env_params=boot_table, priv=priv, substeps=boot_substeps)
            moments = K.ppo_returns_boot(rew, V, traj.mask, traj.len, boot, self.gamma, self.lam, self.monte_carlo, adv_full, ret_full, work)
            n_boot = timeout.sum(dtype=torch.int64).reshape(1)              # (a new tensor: read when last_stats is)
            D.allreduce_sum_(n_boot, self.process_group, "n_bootstrapped")
        D.allreduce_sum_(moments, self.process_group, "ppo_moments")
        norm8 = K.ppo_norm(moments, self.c1, self.kl_coeff, out=self._small("norm8", 8, torch.float32, dev))
        self.norm8 = norm8                                                  # (diagnostics: this learn()'s constants, on the device)
        vn_stats = None
        if vn is not None:
            # the returns' moments (row 1, all-reduced above: no collective of its own) into the running statistics, the table in
            # place, and the critic's target constants norm8[2:4] <- {mean, 1 / sigma} of the merged statistics: one launch
            if not vn.popart:
                vn._merge(None if vn.frozen else moments[1], norm8)
                popart = ()
            else:
                # PopArt: the same launch also rescales the critic's last layer, so that the critic read with the merged table
                # predicts what it predicted with the old one.  Everything above read the old head with the old table, every update
                # below reads the new head with the new constants; frozen statistics: nothing is merged, nothing rescaled
                stat_a = torch.cat([vn.count, vn.mean, vn.m2])              # (the statistics before the merge: for last_stats)
                vn._merge(None if vn.frozen else moments[1], norm8, head=None if vn.frozen else critic.network[-1])
                if not vn.frozen:
                    self._masters_written(critic)
                popart = (stat_a,)
            vn_stats = (torch.cat([vn.count, vn.mean, vn.m2]), moments.clone(), vn.eps, *popart)    # (copies: read when last_stats is)
        adv = self._ws.get("row0", n_rows, 1, torch.float32, dev, cap).view(-1)
        ret = self._ws.get("row1", n_rows, 1, torch.float32, dev, cap).view(-1)
        K.gather_rows2(idx, adv_full, adv, ret_full, ret)
        # ppo.py:142-143: the old log-probabilities come from the CURRENT policy -- on a chain learner the first full-batch
        # update's own forward pass writes them (ratio exactly 1 there, as in the reference), no no-grad pass
        fold_old = (_FOLD_OLD_LOGP and self.batch_size is None and self.updates_per_iter > 0 and m_a is not None and m_c is not None
                    and m_a.can_write_old_logp() and m_c.can_fuse_head())
        old_logp = (self._ws.get("old_logp", n_rows, 1, torch.float32, dev, cap).view(-1) if fold_old else
                    self._logp_nograd(actor, xin, act, var))
        all_sums = []
        # full batch: the updates' [actor | critic] loss sums are the rows of ONE pre-zeroed table (update u <- row u): one fill, one
        # all-reduce, and the arithmetic that turns them into losses waits until somebody asks (last_stats)
        table = (torch.zeros(self.updates_per_iter, 2, 4, dtype=torch.float64, device=dev)
                 if self.batch_size is None and self.updates_per_iter > 0 else None)
        self._sum_rows = list(table.unbind(0))[::-1] if table is not None else None
        norm_host = None
        self._kl_begin(actor, xin, act, old_logp, var, self._learned_std(), cap)
        stop = False
        for u in range(self.updates_per_iter):
            final = u == self.updates_per_iter - 1
            if stop:
                break
            if self.batch_size is None:
                # full batch: the reference permutes and takes one "minibatch" of everything (ppo.py:147-150)
                self._step(xin, act, adv, ret, old_logp, norm8, var, all_sums, last=final, write_old=fold_old and u == 0,
                           xin_c=None if priv is None else xin_c)
                stop = self._kl_after_step(final)                           # (target_kl: the device has stopped, the host follows)
            else:
                if self.permutation_fn is not None:
                    perm = self.permutation_fn(n_rows, dev)
                else:
                    if self._gen is None:
                        self._gen = torch.Generator(device=dev)
                        self._gen.manual_seed(self._seed)
                    perm = torch.randperm(n_rows, device=dev, generator=self._gen)
                # every rank takes the same number of optimizer steps (each one is a collective); a rank that has run
                # out of rows joins the remaining ones with an empty slice
                local_bs, n_steps, sizes = D.minibatch_schedule(n_rows, self.batch_size, self.process_group, dev)
                if norm_host is None:
                    norm_host = norm8[:4].tolist()           # (a minibatch's 1 / n is its own: host numbers; one read per learn())
                for k in range(n_steps):
                    b = perm[k * local_bs:(k + 1) * local_bs]
                    # (the minibatch's rows are copies: they keep the prepared input's ones column, and say so)
                    self._step(M.inherit_ones_column(xin.index_select(0, b), xin), act.index_select(0, b), adv.index_select(0, b),
                               ret.index_select(0, b), old_logp.index_select(0, b), norm8, var, all_sums,
                               host=(norm_host, float(sizes[k])), last=final and k == n_steps - 1,
                               xin_c=None if priv is None else M.inherit_ones_column(xin_c.index_select(0, b), xin_c))
                    stop = self._kl_after_step(final and k == n_steps - 1)
                    if stop:
                        break
        self._check_deferred()                                              # (this learn()'s own row count: landed long ago)
        if self.kl_stats:
            self._measure_shift(actor, xin, act, old_logp, var, self._learned_std(), cap)
        self._copy_policy_to_old()                                          # ppo.py:186
        if all_sums:
            # [steps][actor | critic][4] (the steps that were enqueued: the host may have left the loop behind a target_kl stop)
            S2 = table[:len(all_sums)] if table is not None else torch.stack(all_sums)
            D.allreduce_sum_(S2, self.process_group, "loss_stats")
            ls = self._learned_std()
            ent = 0.5 * act.shape[1] * (1.0 + math.log(2 * math.pi)) + (0.0 if ls is not None else 0.5 * float(torch.log(var).sum()))
            std_log = self._std_log                                         # (sum log_std before each step, on the device)
            ls_end = ls.detach().clone() if ls is not None else None
            c1, ent_c, kl_c = self.c1, self.entropy, self.kl_coeff
            n_dev = moments[0, 0].clone()                                   # (the buffers above are re-used by the next learn())

            def stats():
                S = S2[:, 0].clone()
                S[:, 1] += S2[:, 1, 1]                                      # the critic's squared error
                nn = S[:, 3]
                a_loss, c_loss, kl = -S[:, 0] / nn, S[:, 1] / nn, S[:, 2] / nn
                if ls_end is None:
                    ent_out = ent_steps = ent
                else:                                                       # one entropy per optimizer step, taken before the step
                    ent_steps = ent + std_log.rows().double()
                    ent_out = ent_steps.tolist()
                total = a_loss + c1 * c_loss - ent_c * ent_steps + kl_c * kl
                out = {"actor_loss": a_loss.tolist(), "critic_loss": c_loss.tolist(), "kl_div": kl.tolist(),
                       "total_loss": total.tolist(), "entropy": ent_out, "n_valid": float(n_dev)}
                if ls_end is not None:
                    out["log_std"] = ls_end.tolist()
                if n_boot is not None:
                    out["n_bootstrapped"] = int(n_boot.item())
                if vn_stats is not None:
                    out.update(_value_norm_stats(*vn_stats))
                return out
            self._stats_pending = stats

    def metadata(self) -> dict:
        return {"algorithm": "PPO", "epsilon": self.epsilon, "c1": self.c1, "kl_coeff": self.kl_coeff,
                "gamma": self.gamma, "lam": self.lam, "entropy": self.entropy, "batch_size": self.batch_size,
                "updates_per_iter": self.updates_per_iter, **self._clip_metadata(), **self._kl_metadata(),
                **({"bootstrap_truncated": True} if self.bootstrap_truncated else {})}

    def save(self, path: str) -> None:
        self._kl_sync()                                                     # (the checkpoint holds the adapted lr)
        torch.save(self.optimizer.state_dict(), os.path.join(path, "optimizer.pt"))    # ppo.py:214

    def load(self, path: str) -> None:
        self.optimizer.load_state_dict(torch.load(os.path.join(path, "optimizer.pt"), weights_only=True))
