"""Hand-scheduled forward/backward of the reference's ReLU MLP on the MI355X matrix cores.

`models/neural_network.py:48-66` is `Sequential(Linear, ReLU, ..., Linear)`; under torch autograd (the reference,
algorithms/*.py `loss.backward()`) that costs ~12 launches per layer and, at the shapes of this path
(10^6..10^7 rows x 256 features), every pass is bound by HBM traffic (137 GFLOP per GB).  `GemmMLP` therefore
minimises bytes per row:
  * forward: ONE persistent chain kernel (tg_mlp_forward_chain) for bf16 nets Linear(S<=32, H) ReLU [Linear(H, H)
    ReLU]* Linear(H, A<=16), H in {128, 256}: activations stay on chip between layers and are written once
    (2.7 instead of 5.2 KB/row at 20-256x5-4).  Other shapes: per-layer GEMMs with bias + ReLU in the epilogue
    (`torch._addmm_activation`), K = 20 and N = 1 padded to 32 / 8 (slow hipBLASLt paths otherwise);
  * backward data: tg_dx_relu_bias fuses `dA = dZ W` with the ReLU backward and bias gradient of the layer below
    (1.5 instead of 2.5 KB/row) for square bf16 layers of width 64 / 128 / 256; the head's rank-A product is
    formed inside the top layer's pass (tg_head_bwd_relu_bias); otherwise a GEMM + tg_relu_bwd_bias;
  * backward data, chain shapes (bf16, H in {128, 256}, 3..6 hidden layers, <= 8 outputs): tg_mlp_backward_chain, the dZ of
    all hidden layers in one launch (2.7 KB/row at 5 x 256);
  * weight gradients, chain shapes: tg_mlp_weight_grad -- every weight and hidden bias gradient of the net in ONE persistent
    launch (each dZ and activation read once, the first hidden activation recomputed from the input row instead of stored);
    other shapes: dW = dZ^T A as a batched GEMM over row blocks with fp32 partials plus tg_dw_finish (a plain GEMM has 16
    output tiles on 256 CUs: 1.6-1.9 ms per 2^20 rows).
Gradients are accumulated in fp32 straight into `param.grad` (the learner's flat all-reduce bucket).

Only ReLU hidden activations take the bf16 and per-layer paths.  fp32 nets of the fp32 chain shapes (H in {64, 128}, 1-4 hidden
layers, <= 32 inputs, <= 4 outputs) may use Tanh instead: the fp32 chain learner (tg_mlp_f32_forward_act / _forward_backward_act /
_weight_grad) and the fp32 fused rollout take the activation as a compile-time kernel argument (`hidden_activation()`).  Any other
activation, a mix of activations, or a Tanh net outside those shapes stays on torch autograd.
"""
from __future__ import annotations

import ctypes as C
import logging

import torch

from . import _native as N
from . import hip_ops as K

_ROW_BLOCK = 8192


_LOG = logging.getLogger("trajopt_grpo_amd")
_LOGGED_SHAPES = set()

# "This input has a column of ones" is a property of the BYTES some GemmMLP.prepare_input() wrote, shared by the nets that read them
# (the learner's actor and critic take the same prepared input).  It is carried on the tensor's storage object -- torch keeps ONE
# Python object per live storage, so the mark is seen through every slice / view and dies with the allocation (a block the caching
# allocator hands out again is a new storage: no stale mark) -- as the byte range that was prepared.
def _mark_ones_column(xp: torch.Tensor) -> None:
    lo = xp.storage_offset() * xp.element_size()
    xp.untyped_storage()._tg_ones = (lo, lo + xp.numel() * xp.element_size(), xp.shape[1] * xp.element_size())


def set_ones_column(xp: torch.Tensor, has: bool) -> None:
    """`xp` was just written by a prepare kernel other than prepare_input() (tg_learn_compact): record whether it carries the ones column."""
    if has:
        _mark_ones_column(xp)
    elif getattr(xp.untyped_storage(), "_tg_ones", None) is not None:
        del xp.untyped_storage()._tg_ones


def has_ones_column(xin: torch.Tensor) -> bool:
    """`xin` is a contiguous run of whole rows of an input some prepare_input() gave the ones column."""
    if xin.dim() != 2 or not xin.is_contiguous():
        return False
    r = getattr(xin.untyped_storage(), "_tg_ones", None)
    lo = xin.storage_offset() * xin.element_size()
    return (r is not None and xin.shape[1] * xin.element_size() == r[2] and r[0] <= lo and lo + xin.numel() * xin.element_size() <= r[1]
            and (lo - r[0]) % r[2] == 0)


def inherit_ones_column(dst: torch.Tensor, src: torch.Tensor) -> torch.Tensor:
    """`dst` holds whole rows copied out of `src` (index_select of a minibatch): it has the ones column iff `src` has."""
    if dst.dim() == 2 and dst.is_contiguous() and dst.shape[1:] == src.shape[1:] and dst.dtype == src.dtype and has_ones_column(src):
        _mark_ones_column(dst)
    return dst


def _ref_penalty(kind, rows, logp_ref, ref_coef, kl_coef):
    """N.RefPenalty for forward_loss(logp_ref=..., ref_coef=...), or None: no penalty (the plain entry points)."""
    if logp_ref is None or float(ref_coef) == 0.0:
        return None
    if kind != 0:
        raise ValueError("the reference-policy penalty is a term of the actor's loss (kind 0)")
    if float(kl_coef) != 0.0:
        raise ValueError("kl_coef must be 0 beside the reference-policy penalty: both use the KL sum")
    return K.ref_penalty(logp_ref, ref_coef, rows)


# The training heads' four machines: the entry that runs forward + loss head (+ backward data), and whether it takes the hidden
# activation.  K.head_entry() appends the suffix of whatever optional arguments a call carries.
_LOSS_ENTRIES = {"bf16": ("tg_mlp_forward_chain_loss", False), "f32": ("tg_mlp_f32_forward_backward", True),
                 "f32w": ("tg_mlp_f32w_forward_backward", False), "f32r": ("tg_mlp_f32r_forward_backward", False)}


def loss_entry(machine: str, act: int, ref, std):
    """(entry name, tail arguments, the profiled kernel's trailing template arguments) of forward_loss() on `machine` (a key of
    _LOSS_ENTRIES) with hidden activation `act` (TG_ACT_*), reference penalty `ref` and learned log-std `std` (structs or None)."""
    base, takes_act = _LOSS_ENTRIES[machine]
    assert takes_act or act == N.TG_ACT_RELU, f"{base}: ReLU only"
    name, tail = K.head_entry(base, ref, std, act if takes_act else None)
    if machine == "bf16":
        targs = (",true,true" if ref else ",false,true") if std else (",true" if ref else "")
    else:
        targs = (",true" if ref is not None else (",false" if act else "")) + (f",{act}>" if act else ">")
    return name, tail, targs


def forward_entry(machine: str, act: int):
    """(entry name, tail arguments) of the fp32 learners' no-grad forward pass (machine: "f32", "f32w" or "f32r")."""
    base = _LOSS_ENTRIES[machine][0].replace("_forward_backward", "_forward")
    assert machine != "bf16" and (machine == "f32" or act == N.TG_ACT_RELU), f"{base}: ReLU only"
    return K.suffixed(base, "_act", None if act == N.TG_ACT_RELU else (act,))


def lin_ok(l) -> bool:
    return l.weight.grad is not None and l.weight.grad.dtype == torch.float32 and l.bias.grad is not None
_SPLIT_BATCHES = 128


def weight_grad(hidden: int, jobs, rows: int, workspace: torch.Tensor, w0frag: torch.Tensor = None, b0: torch.Tensor = None,
                whfrag: torch.Tensor = None, extra=(), loss_rider=None):
    """tg_mlp_weight_grad: every job's `wgrad += P^T Q` (and `bgrad += column sums of P`) in one persistent launch + one
    fixed-order reduction.  jobs = [(kind, P, Q, wgrad, bgrad or None[, aux])]; P / Q bf16 row-major [rows][*], wgrad a 2-D
    fp32 view with unit column stride (e.g. a window of the learner's flat gradient bucket).  Kind HR rebuilds its Q (the first
    hidden activation) from the net input with `w0frag` / `b0`; kind RH rebuilds its P (the top layer's dZ) from d loss / d head
    output, the layer's ReLU mask bits (`aux`) and `whfrag` (the backward chain's weight stream).  A seventh job element
    (N.DW_P_PANEL | N.DW_Q_PANEL) names the [rows][H] operands that are stored in panel order (whole 32-row tiles, see the header)
    instead of row-major."""
    arr = (N.DwJob * len(jobs))()
    for slot, job in zip(arr, jobs):
        kind, p, q, wgrad, bgrad = job[:5]
        aux = job[5] if len(job) > 5 else None
        slot.layout = job[6] if len(job) > 6 else 0
        assert not (slot.layout & N.DW_P_PANEL) or p.shape[0] >= _round_up(rows, 32)
        assert not (slot.layout & N.DW_Q_PANEL) or q.shape[0] >= _round_up(rows, 32)
        N.require_cuda(p, q, wgrad, bgrad, aux)
        assert (kind == N.TG_DW_RH) == (aux is not None)
        slot.d_aux = N.ptr(aux)
        assert p.dtype == torch.bfloat16 and q.dtype == torch.bfloat16 and p.is_contiguous() and q.is_contiguous()
        assert p.shape[0] >= rows and q.shape[0] >= rows
        assert wgrad.dtype == torch.float32 and wgrad.dim() == 2 and wgrad.stride(1) == 1
        assert bgrad is None or (bgrad.dtype == torch.float32 and bgrad.is_contiguous() and bgrad.numel() == wgrad.shape[0])
        slot.d_p, slot.d_q, slot.d_wgrad, slot.d_bgrad = p.data_ptr(), q.data_ptr(), wgrad.data_ptr(), N.ptr(bgrad)
        slot.wgrad_ld, slot.kind, slot.m_out, slot.n_out = wgrad.stride(0), kind, wgrad.shape[0], wgrad.shape[1]
    # extra = [(slab tensor, element offset, slab_stride, n_slabs, row_pitch, grad, m_out, n_out)]: the chain kernels' own partial
    # gradients, reduced by the same second launch (tg_mlp_weight_grad_ex); loss_rider = (f64 work [rows][4], n rows, f64 sums [4])
    ex = (N.SlabSum * max(len(extra), 1))()
    for slot, (slab, off, stride, n_slabs, pitch, grad, m_out, n_out) in zip(ex, extra):
        N.require_cuda(slab, grad)
        assert slab.dtype == grad.dtype == torch.float32 and slab.is_contiguous() and (grad.dim() == 1 or grad.stride(-1) == 1)
        assert off + (n_slabs - 1) * stride + (m_out - 1) * pitch + n_out <= slab.numel() or n_slabs == 0
        slot.d_slab, slot.slab_stride, slot.n_slabs, slot.row_pitch = slab.data_ptr() + 4 * off, stride, n_slabs, pitch
        slot.d_grad, slot.grad_ld, slot.m_out, slot.n_out = grad.data_ptr(), (grad.stride(0) if grad.dim() == 2 else 1), m_out, n_out
    lw, ln, ls = (loss_rider[0].data_ptr(), loss_rider[1], loss_rider[2].data_ptr()) if loss_rider else (None, 0, None)
    N.check(N.load().tg_mlp_weight_grad_ex(hidden, arr, len(jobs), rows, N.ptr(w0frag), N.ptr(b0), N.ptr(whfrag), workspace.data_ptr(),
                                           workspace.numel() * workspace.element_size(), ex, len(extra), lw, ln, ls,
                                           N.stream_ptr(workspace.device)), "tg_mlp_weight_grad_ex")


def weight_grad_workspace(hidden: int, device) -> torch.Tensor:
    return torch.empty(N.load().tg_mlp_weight_grad_workspace(hidden) // 4, dtype=torch.float32, device=device)


def per_layer_width_limits(compute_dtype, out_dim: int):
    """(widest hidden layer below the top one, widest top hidden layer) the per-layer backward can run in `compute_dtype`: the
    limits of tg_relu_bwd_bias (2048 columns in bf16, 1024 in fp32) and, for the top hidden layer of a net with <= 8 outputs, of
    tg_head_bwd_relu_bias (2048 in either dtype) -- asked of the library, which checks the same numbers at every launch."""
    lib = N.load()
    relu = lib.tg_relu_bwd_bias_max_cols(1 if compute_dtype == torch.bfloat16 else 0)
    return relu, (lib.tg_head_bwd_relu_bias_max_cols() if out_dim <= 8 else relu)


def supports(net, compute_dtype=torch.float32) -> bool:
    """`net` is Linear [ReLU Linear]+ with hidden widths that are multiples of 8 and within per_layer_width_limits(): every such net
    can run GemmMLP's per-layer path (the chain kernels take subsets of them).  A wider net stays on torch autograd."""
    mods = list(net.network)
    if len(mods) < 3 or len(mods) % 2 == 0:
        return False
    for i, m in enumerate(mods):
        if i % 2 == 0 and not isinstance(m, torch.nn.Linear):
            return False
        if i % 2 == 1 and not isinstance(m, torch.nn.ReLU):
            return False
    widths = [l.out_features for l in mods[0:-1:2]]
    if any(w % 8 != 0 for w in widths):
        return False
    below, top = per_layer_width_limits(compute_dtype, mods[-1].out_features)
    return widths[-1] <= top and all(w <= below for w in widths[:-1])


def log_too_wide(net, compute_dtype) -> None:
    """One INFO line (logger `trajopt_grpo_amd`) for a ReLU net that supports() turns away for its width alone."""
    if hidden_activation(net) != "ReLU":
        return
    lin = _linears(net)
    widths = [l.out_features for l in lin[:-1]]
    if any(w % 8 != 0 for w in widths) or supports(net, compute_dtype):
        return
    below, top = per_layer_width_limits(compute_dtype, lin[-1].out_features)
    shape = f"{lin[0].in_features}-" + "-".join(str(w) for w in widths) + f"-{lin[-1].out_features} {str(compute_dtype).replace('torch.', '')}"
    if (shape, "width") not in _LOGGED_SHAPES:
        _LOGGED_SHAPES.add((shape, "width"))
        _LOG.info("%s: a hidden layer is wider than the per-layer backward kernels take (%d, the top hidden layer %d) -- its update "
                  "runs on torch autograd", shape, below, top)


# hidden activations of the fp32 kernels' `_act` entry points (include/trajopt_grpo_hip.h TG_ACT_*)
ACTIVATIONS = {"ReLU": N.TG_ACT_RELU, "Tanh": N.TG_ACT_TANH}


def hidden_activation(net):
    """"ReLU" or "Tanh" if `net` is Linear [act Linear]+ with the SAME hidden activation after every hidden layer (exactly torch.nn.ReLU
    or torch.nn.Tanh modules), else None (mixed lists, Sigmoid, anything else).  Says nothing about the shape."""
    mods = list(getattr(net, "network", []))
    if len(mods) < 3 or len(mods) % 2 == 0:
        return None
    if any(not isinstance(m, torch.nn.Linear) for m in mods[0::2]):
        return None
    kinds = {type(m) for m in mods[1::2]}
    if kinds == {torch.nn.ReLU}:
        return "ReLU"
    if kinds == {torch.nn.Tanh}:
        return "Tanh"
    return None


def _linears(net):
    return [m for m in net.network if isinstance(m, torch.nn.Linear)]


def _mlp_shape(net):
    """(S, H, n_hidden, A, activation) if `net` is Linear(S, H) act [Linear(H, H) act]* Linear(H, A) with one hidden activation
    (hidden_activation(): "ReLU" or "Tanh") and equal hidden widths, else None.  Every `*_supported` predicate of a kernel family is
    a range check on this tuple."""
    act = hidden_activation(net)
    if act is None:
        return None
    lin = _linears(net)
    H = lin[0].out_features
    if any(l.out_features != H for l in lin[:-1]) or any(l.in_features != H for l in lin[1:]):
        return None
    return lin[0].in_features, H, len(lin) - 1, lin[-1].out_features, act


# forward_loss() of the bf16 chain learner stores its activations in panel order (the loss-head pass; False: that pass stays
# row-major, and so do the dZ unless GemmMLP.panel_mixed asks for them)
PANEL_ORDER_HEAD_PASS = True


def _round_up(x, m):
    return (x + m - 1) // m * m


class _Workspace:
    """Grow-only named device buffers for the per-chunk tensors of a forward/backward (activations, mask bits, dZ).
    Their size follows the number of valid rows, which changes every iteration; handed to the caching allocator, a
    GB-sized request that outgrows what is cached costs a hipMalloc (the update was measured up to 2x slower when the
    row count kept growing).  A buffer here is allocated once per name at the largest size seen and handed out as a view;
    with the learner's fixed first chunk that size is reached in the first update."""

    def __init__(self):
        self._buf = {}

    default_cap = 0     # rows every buffer is sized for when it is (re)allocated (the learner sets it to its chunk size: the
                        # row count of an iteration grows while a policy learns to survive, and a GB-sized buffer that is re-allocated
                        # a little larger every iteration costs tens of milliseconds of hipMalloc / hipFree with the GPU busy)

    def get(self, name: str, rows: int, cols: int, dtype, device, cap_rows: int = 0) -> torch.Tensor:
        """[rows][cols] view of buffer `name`; a (re)allocation sizes it for max(rows, cap_rows, default_cap) rows."""
        need = rows * cols
        b = self._buf.get(name)
        if b is None or b.numel() < need or b.dtype != dtype or b.device != device:
            self._buf[name] = b = torch.empty(max(rows, cap_rows, self.default_cap) * cols, dtype=dtype, device=device)
        return b[:need].view(rows, cols)


class GemmMLP:
    def __init__(self, net, compute_dtype=torch.bfloat16):
        # ReLU nets: every path below.  Tanh nets: the fp32 chain learner only (its kernels take the activation as an argument; the
        # per-layer GEMMs, the ReLU-backward kernels and the bf16 chains are ReLU by construction): forward(keep=True) and backward()
        # refuse them instead of applying ReLU
        self.act = hidden_activation(net)
        if self.act == "Tanh":
            if compute_dtype != torch.float32 or not f32_chain_supported(net):
                raise ValueError("GemmMLP runs a Tanh net only in float32 on the fp32 chain learner (Linear(S<=32, H) Tanh "
                                 "[Linear(H, H) Tanh]{0..3} Linear(H, A<=4), H in {64, 128})")
        else:
            assert supports(net, compute_dtype)
        self.net = net
        self.cd = compute_dtype
        self.linears = [m for m in net.network if isinstance(m, torch.nn.Linear)]
        dev = self.linears[0].weight.device
        self.in_dim, self.out_dim = self.linears[0].in_features, self.linears[-1].out_features
        # fp32 nets of the reference's own shapes: the fp32 chain learner (tg_mlp_f32_forward / _forward_backward / _weight_grad)
        self._f32 = None
        # (parity tests: every hidden activation and dZ of the fp32 chain learner written to HBM, so that each can be compared with
        # fp64; the product rebuilds the first activation and the top dZ on chip instead)
        self.f32_store_all = False
        # the bf16 chain learner (forward_loss() / backward_fused()) keeps its internal workspaces -- the stored activations and the
        # dZ, which only tg_mlp_weight_grad reads -- in panel order (include/trajopt_grpo_hip.h TG_LAYOUT_PANEL); False: row-major,
        # the same values at other addresses.  forward(keep=True) / backward() always store row-major: callers may read those.
        self.panel_order = True
        # ... the dZ only where the activations are (the plain loss head): a weight-gradient job with ONE operand in panel order ran
        # 6 % slower than with both or neither (profiles/r06_panel_order_ab.md).  True: the dZ regardless (tools/panel_order_probe.py)
        self.panel_mixed = False
        # the bf16 backward chain may take its depth-specialised kernel (H = 256, 5 hidden layers: the same results bit for bit from
        # fewer instructions, profiles/r19_chain_depth_ab.md); False: the run-time-depth kernel.  The native switch is process-wide
        # (tg_chain_depth_kernels), so it is set in front of the launch it governs.
        self.depth_kernels = N.chain_depth_kernels_default()
        # ... and the forward chain's training pass its block-structured kernel (H = 256, plain head, panel order, any depth: bit for
        # bit the same again, profiles/r22_fwd_chain_block_ab.md); a switch of its own (tg_chain_fwd_kernels), set the same way
        self.fwd_depth_kernels = N.chain_fwd_kernels_default()
        if self.act == "Tanh":
            # (the resident 16-row kernel and the H = 256 kernel are ReLU-only: a Tanh net of the resident shape runs the chain kernel;
            # nothing is rebuilt from mask bits, so every activation and dZ is stored)
            self._f32 = F32ChainStream(net, f32_chain_supported(net), activation="Tanh")
            self.f32_store_all = True
        elif compute_dtype == torch.float32 and f32_res_supported(net):
            self._f32 = F32ResStream(net)                       # H = 128, <= 2 hidden layers: the resident 16-row kernel (C2's shape)
        elif compute_dtype == torch.float32 and f32_chain_supported(net):
            self._f32 = F32ChainStream(net, f32_chain_supported(net))
        elif compute_dtype == torch.float32 and f32_wide_supported(net):
            self._f32 = F32WideStream(net)                      # H = 256: csrc/mlp_f32_wide.hip
        self.in_pad = _round_up(self.in_dim, 32) if self._f32 is None else self._f32.in_pad
        self.out_pad = _round_up(self.out_dim, 8)
        self.w, self.b = [], []
        for i, l in enumerate(self.linears):
            o = self.out_pad if i == len(self.linears) - 1 else l.out_features
            k = self.in_pad if i == 0 else l.in_features
            self.w.append(torch.zeros(o, k, dtype=compute_dtype, device=dev))
            self.b.append(torch.zeros(o, dtype=compute_dtype, device=dev))
        self._acts = None
        self._bits = None
        self._ws = _Workspace()
        self._partial = None
        # hidden layers whose backward-data product runs fused with the ReLU backward below it (tg_dx_relu_bias)
        self._dxfrag = [None] * len(self.linears)
        if compute_dtype == torch.bfloat16:
            lib = N.load()
            for i in range(1, len(self.linears) - 1):
                o, k = self.w[i].shape
                if lib.tg_dx_relu_bias_supported(o, k):
                    self._dxfrag[i] = torch.empty(o * k, dtype=torch.bfloat16, device=dev)
        self._dx_partial = None
        self._head_partial = None
        self._dw_ws = None
        self._w0_slabs = None
        self._head_ws = None
        self._dz_head = None
        self._tmask = None
        # like dx_events, for every tg_mlp_weight_grad launch / every training (keep=True) tg_mlp_forward_chain launch
        self.dw_events = None
        self.fwd_events = None
        # when set to a list, every backward-data launch (tg_mlp_backward_chain or tg_dx_relu_bias) is bracketed by HIP
        # events on the launch stream and (start, end, rows, algorithmic bytes per row, kernel name) is appended
        # (bench.py reads them back for that kernel's roofline)
        self.dx_events = None
        # all layers of the forward pass in one launch (tg_mlp_forward_chain) when the shape allows
        self._chain = None
        H = fused_rollout_supported(net, min(self.in_dim, 32), 1) if compute_dtype == torch.bfloat16 else 0
        self._bchain = None
        if H and self.in_dim <= 32 and self.out_pad <= 16 and len(self.linears) - 1 <= 8:
            self._chain = FragmentStream(net, H, layout="chain")
            # ... and the backward-data pass as one launch too (tg_mlp_backward_chain): dZ stays on chip from the head down
            if H in (128, 256) and self.out_pad == 8 and 3 <= len(self.linears) - 1 <= 6:     # 6: the kernel's LDS budget
                self._bchain = FragmentStream(net, H, layout="chain", transposed=True)
        self.bias_out_f32 = torch.zeros(self.out_pad, dtype=torch.float32, device=dev)
        self._log_path(net)
        self._built = {}            # derived operand -> the key (_key()) of the weights it was last built from
        self.refresh()

    def disable_f32_chain(self) -> bool:
        """Back to the per-layer path with the 32-wide padded input (a learner whose actor and critic would otherwise expect
        differently padded inputs: e.g. > 4 actions beside a 1-output critic).  False for a Tanh net, which has no per-layer path
        (nothing changes: the caller runs it on torch autograd instead)."""
        if self.act != "ReLU":
            return False
        if self._f32 is None:
            return True
        self._f32 = None
        self.in_pad = _round_up(self.in_dim, 32)
        w0 = self.w[0]
        self.w[0] = torch.zeros(w0.shape[0], self.in_pad, dtype=w0.dtype, device=w0.device)
        self._built.clear()                                         # (a re-allocated operand: nothing built counts any more)
        self.refresh()
        return True

    def _log_path(self, net):
        """One INFO line per net shape (logger `trajopt_grpo_amd`) saying which kernels run it, and a WARNING when a net falls off the
        hand-written chain kernels onto library GEMMs + per-layer glue (that used to be silent)."""
        lin = self.linears
        shape = f"{self.in_dim}-" + "-".join(str(l.out_features) for l in lin[:-1]) + f"-{self.out_dim} {str(self.cd).replace('torch.', '')}"
        if shape in _LOGGED_SHAPES:
            return
        _LOGGED_SHAPES.add(shape)
        if self._f32 is not None:
            _LOG.info("%s%s", shape, self._f32.log_line())
        elif self._chain is not None and self._bchain is not None:
            _LOG.info("%s: bf16 chain kernels (tg_mlp_forward_chain[_loss] / tg_mlp_backward_chain / tg_mlp_weight_grad)", shape)
        else:
            why = ("fp32 chain learners: hidden width 64 / 128 with 1-4 equal hidden layers or 256 with 1-5, <= 32 inputs, <= 4 outputs"
                   if self.cd == torch.float32 else
                   "bf16 chain kernels: hidden width 128 / 256, 3-6 equal hidden layers, <= 32 inputs, <= 8 outputs"
                   + ("; the forward chain alone covers this net" if self._chain is not None else ""))
            log = _LOG.warning if sum(l.weight.numel() for l in lin) >= 4096 else _LOG.info       # (scaffolding-sized nets: not worth a warning)
            log("%s is outside the hand-written learner kernels' shapes (%s): its update runs on hipBLASLt GEMMs + per-layer "
                         "HIP kernels, several times slower per row", shape, why)

    def refresh(self, force: bool = False):
        """The fp32 master weights changed: every derived operand (padded compute-dtype copies, chain streams, packed
        backward-data fragments) is rebuilt the next time the path that reads it runs -- with the chain kernels active
        the per-layer copies are never touched (17 of 36 tiny launches per update and net).  force=True: whatever the keys say
        (an entry point that cannot know who wrote the weights since its last call)."""
        k = self._key()
        self._stale = {w for w in ("w", "chain", "bchain", "dx", "f32") if force or N.ALWAYS_REBUILD or self._built.get(w) != k}

    def fresh_forward(self, force: bool = False):
        """Rebuild NOW what the no-grad forward() reads.  A captured hipGraph holds the forward launches only (a rebuild enqueued
        during the capture's warm-up leaves nothing stale for the capture itself to record), so the per-step rollout calls this
        eagerly in front of every replay: the graph then reads the rebuilt operands through the same buffers."""
        self.refresh(force)
        self._fresh("f32" if self._f32 is not None else ("chain" if self._chain is not None else "w"))

    def _key(self):
        """weights_key() of this net: refresh() marks stale only what was built from a different key, so a learn() that starts with
        the weights its last optimizer step left rebuilds nothing."""
        return weights_key(self.linears)

    def streams(self):
        """[(what, WeightStream)] of the derived layouts this net has -- `what` as refresh() and mark_built() name them."""
        return [ws for ws in (("chain", self._chain), ("bchain", self._bchain), ("f32", self._f32)) if ws[1] is not None]

    def mark_built(self, what: str) -> None:
        """`what` has just been rebuilt from the current weights by someone else (optim.StreamRefresher, a copy of an identical
        net's stream)."""
        self._stale.discard(what)
        self._built[what] = self._key()

    def _fresh(self, what: str):
        if what not in self._stale:
            return
        self.mark_built(what)
        with torch.no_grad():
            if what == "w":
                for w, b, l in zip(self.w, self.b, self.linears):
                    w[:l.out_features, :l.in_features].copy_(l.weight)
                    b[:l.out_features].copy_(l.bias)
                self.bias_out_f32[:self.out_dim].copy_(self.linears[-1].bias)
            elif what != "dx":
                dict(self.streams())[what].refresh()
            else:
                self._fresh("w")
                for w, frag in zip(self.w, self._dxfrag):
                    if frag is not None:
                        N.check(N.load().tg_dx_pack_weights(w.data_ptr(), frag.data_ptr(), w.shape[0], w.shape[1],
                                                            N.stream_ptr(w.device)), "tg_dx_pack_weights")

    def prepare_input(self, X: torch.Tensor, out: torch.Tensor = None, obs_norm=None) -> torch.Tensor:
        """[M][in_dim] (any float dtype, any strides) -> contiguous [M][in_pad] compute dtype, zero padded
        (into `out` when given: a [M][in_pad] buffer of the compute dtype).  obs_norm (a policy's ObsNorm): the rows hold the
        normalised observation -- one tg_obs_normalize_rows launch writes values, padding and the ones column."""
        if obs_norm is not None:
            from . import hip_ops as K
            xp = torch.empty(X.shape[0], self.in_pad, dtype=self.cd, device=X.device) if out is None else out
            ones = self.in_pad == 32 and self.in_dim < 32 and self._f32 is None
            if X.dtype not in (torch.float32, torch.float64):
                X = X.float()
            K.obs_normalize_rows(X, obs_norm, xp, 31 if ones else -1)
            set_ones_column(xp, ones)
            return xp
        xp = torch.zeros(X.shape[0], self.in_pad, dtype=self.cd, device=X.device) if out is None else out.zero_()
        xp[:, :self.in_dim].copy_(X)
        if self.in_pad == 32 and self.in_dim < 32 and self._f32 is None:
            # a padding column of ones: the first layer's weights are zero there (the forward pass does not see it), and
            # tg_mlp_backward_chain_w0 delivers the first layer's bias gradient as that column of dW0.  The prepared bytes are
            # marked on their storage: only inputs prepared HERE (slices of them, row copies registered with
            # inherit_ones_column) take that path -- a caller that pads its own input with zeros gets the HX job of
            # tg_mlp_weight_grad instead of a silently zero bias gradient.
            xp[:, 31] = 1.0
            _mark_ones_column(xp)
        elif getattr(xp.untyped_storage(), "_tg_ones", None) is not None:
            del xp.untyped_storage()._tg_ones                 # (a buffer re-prepared by a net that writes no ones column)
        return xp

    def _has_ones_column(self, xin: torch.Tensor) -> bool:
        return has_ones_column(xin)

    def _chain_backward_ok(self) -> bool:
        """backward() can take the chain path (tg_mlp_backward_chain + tg_mlp_weight_grad): fp32 gradients with unit column
        stride on every layer.  forward(keep=True) decides with the SAME predicate whether the first activation may be left out."""
        return self._bchain is not None and all(
            l.weight.grad is not None and l.bias.grad is not None and l.weight.grad.dtype == torch.float32
            and l.weight.grad.stride(1) == 1 and l.bias.grad.dtype == torch.float32 and l.bias.grad.is_contiguous()
            for l in self.linears)

    @torch.no_grad()
    def forward(self, xp: torch.Tensor, keep: bool = True, padded: bool = False) -> torch.Tensor:
        """-> fp32 [rows][out_dim] (contiguous), or the padded output buffer itself with padded=True
        (row stride >= out_dim -- read it from .stride(0); columns >= out_dim are zero).  keep=True stores the activations for backward().
        `xp`: [rows][in_pad] compute dtype, zero padded -- normally from prepare_input(), whose ones column (31) lets the
        backward chain form the first layer's bias gradient; a caller-padded input works too (kind HX job instead)."""
        L = len(self.linears)
        if self._f32 is not None and not keep and xp.shape[0] > 0:
            # the no-grad pass of an fp32 net (old log-probs, values, the per-step rollout's policy mean): one launch
            self._fresh("f32")
            f = self._f32
            assert xp.dtype == torch.float32 and xp.is_contiguous() and xp.shape[1] == f.in_pad
            out = torch.empty(xp.shape[0], 4, dtype=torch.float32, device=xp.device)
            name, tail = forward_entry(f.machine, f.act)
            N.check(getattr(N.load(), name)(xp.data_ptr(), f.in_pad, f.stream.data_ptr(), *f.forward_args(), xp.shape[0], out.data_ptr(),
                                            *tail, N.stream_ptr(xp.device)), name)
            self._acts = self._bits = None
            return out if padded else out[:, :self.out_dim].contiguous()
        if self._chain is not None and xp.shape[0] > 0:
            self._fresh("chain")
            rows, H = xp.shape[0], self._chain.H
            # with the backward chain active the first hidden activation is never read again: tg_mlp_weight_grad
            # recomputes it from the input row (kind HR), so it is not written either (its mask bits still are)
            skip_a0 = keep and L - 1 >= 2 and self._chain_backward_ok()
            hid = [None if (i == 0 and skip_a0) else self._ws.get(f"a{i}", rows, H, self.cd, xp.device)
                   for i in range(L - 1)] if keep else []
            # 1 bit per stored activation (its ReLU mask): all the backward-data kernels need of it
            bits = [self._ws.get(f"m{i}", rows, H // 32, torch.int32, xp.device) for i in range(L - 1)] if keep else []
            # (<= 4 outputs: a 16-B output row -- tg_rollout_step then reads the policy mean without padding)
            oc = 4 if self.out_dim <= 4 else self.out_pad
            out = torch.empty(rows, oc, dtype=torch.float32, device=xp.device)
            ptrs = (N.C.c_void_p * (L - 1))(*[N.ptr(t) or None for t in hid]) if keep else None
            mptrs = (N.C.c_void_p * (L - 1))(*[t.data_ptr() for t in bits]) if keep else None
            ev = None
            if keep and self.fwd_events is not None:
                ev = N.event_pair()
                ev[0].record()
            N.check(N.load().tg_mlp_forward_chain(xp.data_ptr(), self._chain.stream.data_ptr(), self._chain.bias.data_ptr(), H,
                                                  L - 1, rows, ptrs, mptrs, out.data_ptr(), oc,
                                                  N.stream_ptr(xp.device)), "tg_mlp_forward_chain")
            if ev is not None:
                ev[1].record()
                stored = sum(1 for t in hid if t is not None)
                self.fwd_events.append((ev[0], ev[1], rows, 2 * self.in_pad + stored * 2 * H + (L - 1) * (H // 8) + 4 * oc,
                                        f"tg::mlp_fwd_chain_kernel<{H},8,true,4,{'true' if stored == L - 1 else 'false'}>"))
            self._acts = [xp] + hid if keep else None
            self._bits = [None] + bits if keep else None
            self._acts_panel = False
            return out if padded else out[:, :self.out_dim].contiguous()
        if self.act != "ReLU":
            raise NotImplementedError(f"GemmMLP.forward(keep={keep}) of a {self.act} net: the per-layer GEMM path applies ReLU; a {self.act} net "
                                      "trains through forward_loss() / backward_fused() (fp32 chain learner) only")
        self._fresh("w")
        acts = [xp]
        h = xp
        for i in range(L - 1):
            h = torch._addmm_activation(self.b[i], h, self.w[i].t())       # bias + ReLU in the GEMM epilogue
            acts.append(h)
        if self.cd == torch.float32:
            out = torch.addmm(self.b[-1], h, self.w[-1].t())
        else:                                                              # fp32 accumulate AND fp32 output for the head
            out = torch.mm(h, self.w[-1].t(), out_dtype=torch.float32)
            out += self.bias_out_f32
        self._acts = acts if keep else None
        self._bits = None
        return out if padded else out[:, :self.out_dim].contiguous()

    def can_fuse_head(self) -> bool:
        """The loss head + the head's weight gradient inside the forward chain (tg_mlp_forward_chain_loss): chain shapes with the
        backward chain active, at most 4 outputs, fp32 gradient windows."""
        if self._f32 is not None:
            return all(lin_ok(l) and l.weight.grad.stride(1) == 1 and l.bias.grad.is_contiguous() for l in self.linears)
        return (self._chain is not None and self._bchain is not None and self.cd == torch.bfloat16
                and len(self.linears) - 1 >= 3 and self.out_dim <= 4 and all(lin_ok(l) for l in self.linears)
                and self.linears[-1].weight.grad.stride(1) == 1)

    @torch.no_grad()
    def forward_loss(self, xp: torch.Tensor, kind: int, *, act=None, logp_old=None, adv=None, ret=None, norm=None, var=None,
                     epsilon=0.0, surr_coef=0.0, critic_coef=0.0, kl_coef=0.0, sums_out=None, logp_old_out=None, norm8=None,
                     logp_ref=None, ref_coef=0.0, log_std=None, std_out=None) -> torch.Tensor:
        """Training forward pass with the loss head inside it (kind 0: actor, clipped surrogate; kind 1: critic, squared error).
        Stores what backward_fused() needs, adds the head's weight / bias gradient into their windows and returns the f64 sums
        [surrogate, squared error, KL, count] of these rows -- or, given `sums_out` (f64 [4] on the device), ADDS them there and
        returns None; on the fp32 chain learner that addition rides on backward_fused()'s reduction launch (no launches of its own),
        so `sums_out` is complete once backward_fused() has been enqueued.
        norm8: device f32 [8] (hip_ops.ppo_norm): the normalisation pair and the three coefficients are read from it on the device;
        `norm` and the `*_coef` arguments are then ignored.
        logp_ref (f32 [rows], kind 0) with ref_coef != 0: GRPO's KL penalty to a frozen reference policy in the head (the `_ref` entry
        points): D = exp(x) - x - 1, x = logp_ref - logp, joins the KL sum (slot 2; kl_coef must be 0) and d loss / d logp gains
        ref_coef (exp(x) - 1).  Otherwise the plain entry points run.
        log_std (device f32 [A], kind 0) with std_out (f32 [rows][4]): the policy's learned log-std (the `_std` entry points): the head
        reads it on the device (`var` is ignored) and writes each row's contribution to d loss / d log_std into std_out
        (hip_ops.log_std_grad sums it into the gradient window)."""
        lib = N.load()
        ref = _ref_penalty(kind, xp.shape[0], logp_ref, ref_coef, kl_coef)
        std = None
        if log_std is not None:
            if kind != 0:
                raise ValueError("the learned log-std is a term of the actor's loss (kind 0)")
            std = K.learned_std(log_std, std_out, xp.shape[0], self.out_dim)
        if self._f32 is not None:
            return self._forward_loss_f32(xp, kind, act, logp_old, adv, ret, norm, var, epsilon, surr_coef, critic_coef, kl_coef, sums_out,
                                          logp_old_out, norm8, ref, std)
        assert self.act == "ReLU"
        self._flush_riders()                 # (a forward_loss() that was never followed by backward_fused(): its head gradient is due)
        self._fresh("chain")
        L = len(self.linears)
        rows, H, dev = xp.shape[0], self._chain.H, xp.device
        # (panel order: whole 32-row tiles; built for the plain head -- the reference-penalty and learned-std heads store row-major)
        panel = bool(self.panel_order) and PANEL_ORDER_HEAD_PASS and ref is None and std is None
        hid = [None if i in (0, L - 2) else self._ws.get(f"a{i}", _round_up(rows, 32) if panel else rows, H, self.cd, dev)
               for i in range(L - 1)]
        bits = [self._ws.get(f"m{i}", rows, H // 32, torch.int32, dev) for i in range(L - 1)]
        dz_head = self._ws.get("z_head", rows, self.out_pad, self.cd, dev)
        nblk = lib.tg_mlp_forward_chain_blocks()
        if self._head_ws is None:
            self._head_ws = (torch.empty(nblk * 4 * 16 * H, dtype=torch.float32, device=dev),
                             torch.empty(nblk * 4, dtype=torch.float64, device=dev),
                             torch.empty(nblk * 4, dtype=torch.float32, device=dev))
        slabs, work, bpart = self._head_ws
        # (norm = host pair (mean, 1 / (std + eps)) of the advantage / return, or None; logp_old_out: the old policy is the current
        # one -- this pass writes the old log-probabilities instead of reading them)
        a = self._loss_args(kind, rows, act, logp_old, adv, ret, norm, var, epsilon, surr_coef, critic_coef, kl_coef, logp_old_out, norm8)
        a.d_dout8, a.d_head_slabs, a.d_work, a.d_bias_partial = dz_head.data_ptr(), slabs.data_ptr(), work.data_ptr(), bpart.data_ptr()
        ptrs = (N.C.c_void_p * (L - 1))(*[N.ptr(t) or None for t in hid])
        mptrs = (N.C.c_void_p * (L - 1))(*[t.data_ptr() for t in bits])
        name, tail, targs = loss_entry("bf16", N.TG_ACT_RELU, ref, std)
        if panel:
            name, tail, targs = "tg_mlp_forward_chain_loss_ex", (None, None, N.TG_LAYOUT_PANEL), ",false,false,true"
            if self._set_fwd_depth_kernels(lib) and H == 256:             # (what the launcher picks: the events' label)
                targs += ",true"
        ev = None
        if self.fwd_events is not None:
            ev = N.event_pair()
            ev[0].record()
        N.check(getattr(lib, name)(xp.data_ptr(), self._chain.stream.data_ptr(), self._chain.bias.data_ptr(), H, L - 1, rows, ptrs, mptrs,
                                   N.C.byref(a), *tail, N.stream_ptr(dev)), name)
        self._acts_panel = panel
        if ev is not None:
            ev[1].record()
            stored = sum(1 for t in hid if t is not None)
            per_row = (2 * self.in_pad + stored * 2 * H + (L - 1) * (H // 8) + 16 + (4 * self.out_dim + 8 if kind == 0 else 4) + (4 if ref else 0)
                       + (16 if std else 0))
            self.fwd_events.append((ev[0], ev[1], rows, per_row, f"tg::mlp_fwd_chain_kernel<{H},8,true,4,false,true{targs}>"))
        grid = min(nblk, -(-rows // 256))
        lin = self.linears[-1]
        # the head's partial weight / bias gradients (rows >= 4 of a slab are never written) and -- with sums_out -- the loss sums are
        # added by backward_fused()'s weight-gradient reduction launch, in a fixed order (three torch launches each before)
        self._riders = ([(slabs, 0, 16 * H, grid * 4, H, lin.weight.grad, self.out_dim, H),
                         (bpart, 0, 4, grid, 4, lin.bias.grad, 1, self.out_dim)],
                        (work, grid, sums_out) if sums_out is not None else None)
        if sums_out is not None:
            assert sums_out.dtype == torch.float64 and sums_out.is_cuda and sums_out.numel() == 4 and sums_out.is_contiguous()
        self._acts = [xp] + hid
        self._bits = [None] + bits
        self._dz_head = dz_head
        return None if sums_out is not None else work[:grid * 4].view(grid, 4).sum(0)

    def _set_depth_kernels(self, lib):
        """Carries GemmMLP.depth_kernels to the native switch in front of a chain launch; -> the value set."""
        on = bool(self.depth_kernels)
        lib.tg_chain_depth_kernels(int(on))
        return on

    def _set_fwd_depth_kernels(self, lib):
        """Carries GemmMLP.fwd_depth_kernels to the native switch in front of the forward chain's training launch; -> the value set."""
        on = bool(self.fwd_depth_kernels)
        lib.tg_chain_fwd_kernels(int(on))
        return on

    def _flush_riders(self):
        """The partial gradients / loss sums a forward_loss() left for backward_fused()'s reduction launch, added here by torch instead
        (same sums, torch's order): only when that backward_fused() never came."""
        riders, loss_rider = getattr(self, "_riders", None) or ([], None)
        self._riders = None
        for slab, off, stride, n_slabs, pitch, grad, m_out, n_out in riders:
            if n_slabs > 0:
                v = torch.as_strided(slab, (n_slabs, m_out, n_out), (stride, pitch, 1), off).sum(0)
                grad.add_(v.view_as(grad))
        if loss_rider is not None:
            work, n, sums = loss_rider
            sums += work[:n * 4].view(n, 4).sum(0)

    def _loss_args(self, kind, rows, act, logp_old, adv, ret, norm, var, epsilon, surr_coef, critic_coef, kl_coef, logp_old_out=None,
                   norm8=None) -> "N.ChainLoss":
        a = N.ChainLoss()
        if norm8 is not None:
            N.require_cuda(norm8)
            assert norm8.dtype == torch.float32 and norm8.is_contiguous() and norm8.numel() == 8
            a.d_norm8 = norm8.data_ptr()
        a.kind, a.act_dim = kind, self.out_dim
        if kind == 0:
            N.require_cuda(act, logp_old, adv, logp_old_out)
            assert act.dtype == torch.float32 and adv.dtype == torch.float32
            assert adv.is_contiguous() and act.shape == (rows, self.out_dim) and act.is_contiguous()
            a.d_act, a.act_row_stride, a.act_col_stride = act.data_ptr(), act.stride(0), act.stride(1)
            if logp_old_out is not None:                 # the old policy is the current one: this pass WRITES the old log-probabilities
                assert logp_old_out.dtype == torch.float32 and logp_old_out.is_contiguous() and logp_old_out.numel() == rows
                a.d_logp_old_out = logp_old_out.data_ptr()
            else:
                assert logp_old.dtype == torch.float32 and logp_old.is_contiguous()
                a.d_logp_old = logp_old.data_ptr()
            a.d_adv = adv.data_ptr()
            if var is not None:                          # (None: a learned log-std, read by the head on the device)
                va = [float(v) for v in (var.tolist() if isinstance(var, torch.Tensor) else var)]
                for i in range(self.out_dim):
                    a.var[i] = va[i]
        else:
            N.require_cuda(ret)
            assert ret.dtype == torch.float32 and ret.is_contiguous() and self.out_dim == 1
            a.d_ret = ret.data_ptr()
            a.var[0] = 1.0
        a.norm_mean, a.norm_inv = (0.0, 1.0) if norm is None else (float(norm[0]), float(norm[1]))
        a.epsilon, a.surr_coef, a.critic_coef, a.kl_coef = float(epsilon), float(surr_coef), float(critic_coef), float(kl_coef)
        return a

    def can_write_old_logp(self) -> bool:
        """forward_loss(logp_old_out=...) is available: the loss head runs inside the forward chain (bf16 or fp32)."""
        return self.can_fuse_head()

    def _forward_loss_f32(self, xp, kind, act, logp_old, adv, ret, norm, var, epsilon, surr_coef, critic_coef, kl_coef, sums_out=None,
                          logp_old_out=None, norm8=None, ref=None, std=None):
        """forward_loss() of an fp32 net: forward + loss head + backward-data pass in ONE launch (tg_mlp_f32_forward_backward);
        every hidden layer's activation and dZ is written for backward_fused() (tg_mlp_f32_weight_grad)."""
        lib = N.load()
        self._fresh("f32")
        f = self._f32
        rows, H, dev, nh = xp.shape[0], f.H, xp.device, f.n_hidden
        assert xp.dtype == torch.float32 and xp.is_contiguous() and xp.shape[1] == f.in_pad
        # with >= 2 hidden layers the first activation and the top layer's dZ are neither written nor read: the weight-gradient job
        # that needs them rebuilds them from the input row / from d loss / d output + the top layer's mask bits (16 B per row)
        rec = nh >= 2 and not self.f32_store_all and f.rebuilds_on_chip
        acts = [None if (rec and i == 0) else self._ws.get(f"fa{i}", rows, H, torch.float32, dev) for i in range(nh)]
        dzs = [None if (rec and i == nh - 1) else self._ws.get(f"fz{i}", rows, H, torch.float32, dev) for i in range(nh)]
        tmask = self._ws.get("fmask", rows, 4, torch.int32, dev) if rec else None
        dout = self._ws.get("fz_head", rows, 4, torch.float32, dev)
        if self._head_ws is None:
            self._head_ws = torch.empty(f.blocks() * 4, dtype=torch.float64, device=dev)
        a = self._loss_args(kind, rows, act, logp_old, adv, ret, norm, var, epsilon, surr_coef, critic_coef, kl_coef, logp_old_out, norm8)
        a.d_dout8, a.d_work = dout.data_ptr(), self._head_ws.data_ptr()
        ptrs = (N.C.c_void_p * nh)(*[N.ptr(t) for t in acts])
        zptrs = (N.C.c_void_p * nh)(*[N.ptr(t) for t in dzs])
        if f.act != N.TG_ACT_RELU:          # Tanh: everything stored, no mask bits
            assert tmask is None and all(t is not None for t in acts + dzs)
        name, tail, targs = loss_entry(f.machine, f.act, ref, std)
        ev = None
        if self.fwd_events is not None:
            ev = N.event_pair()
            ev[0].record()
        N.check(getattr(lib, name)(xp.data_ptr(), f.in_pad, f.stream.data_ptr(), *f.loss_args(), rows, ptrs, zptrs,
                                   *((N.ptr(tmask),) if f.takes_mask_bits else ()), N.C.byref(a), *tail, N.stream_ptr(dev)), name)
        if ev is not None:
            ev[1].record()
            # matrix-core flops per row: first layer + forward and backward products of the H x H layers (head: vector unit)
            # algorithmic flops per row (un-padded): forward first layer + H x H layers + head, backward head + H x H layers
            self.fwd_events.append((ev[0], ev[1], rows, 2 * H * self.in_dim + 4 * (nh - 1) * H * H + 4 * H * self.out_dim,
                                    f.kernel_prefix() + targs))
        grid = f.grid(rows)
        self._acts, self._bits, self._dz_head, self._tmask = [xp] + acts, dzs, dout, tmask
        assert getattr(self, "_loss_rider", None) is None, "forward_loss(sums_out=...) must be followed by backward_fused()"
        if sums_out is not None:
            assert sums_out.dtype == torch.float64 and sums_out.is_cuda and sums_out.numel() == 4 and sums_out.is_contiguous()
            self._loss_rider = (grid, sums_out)             # added by tg_mlp_f32_weight_grad's reduction launch
            return None
        return self._head_ws[:grid * 4].view(grid, 4).sum(0)

    def _backward_fused_f32(self, adam=None):
        f = self._f32
        xp, acts, dzs, dout = self._acts[0], self._acts[1:], self._bits, self._dz_head
        rows, H, nh, lin = xp.shape[0], f.H, f.n_hidden, self.linears
        if nh == 1:
            assert acts[0] is not None and dzs[0] is not None
        if self._dw_ws is None:
            self._dw_ws = torch.empty(N.load().tg_mlp_f32_weight_grad_workspace(H) // 4, dtype=torch.float32, device=xp.device)
        # (kind, P, Q, columns of Q, weight window, bias window, rows x columns of the window, rebuild bits)
        specs = []
        fused = False
        for i in range(nh - 1, 0, -1):
            rp, rq = dzs[i] is None, acts[i - 1] is None           # top layer's dZ / first activation rebuilt on chip
            fused = fused or rp or rq
            specs.append((N.TG_F32DW_MM, dout if rp else dzs[i], xp if rq else acts[i - 1], H, lin[i].weight.grad, lin[i].bias.grad, H, H,
                          (2 if rp else 0) | (1 if rq else 0)))
        if not fused:                                               # (the rebuilding jobs carry these two as riders)
            specs.append((N.TG_F32DW_MM, dzs[0], xp, f.in_pad, lin[0].weight.grad, lin[0].bias.grad, H, self.in_dim, 0))
            specs.append((N.TG_F32DW_HEAD, dout, acts[nh - 1], H, lin[nh].weight.grad, lin[nh].bias.grad, self.out_dim, H, 0))
        arr = (N.F32DwJob * len(specs))()
        for slot, (kind, p, q, ncols, wg, bg, m_out, n_out, rebuild) in zip(arr, specs):
            assert wg.dtype == torch.float32 and wg.stride(1) == 1 and bg.dtype == torch.float32 and bg.is_contiguous()
            slot.d_p, slot.d_q, slot.d_wgrad, slot.d_bgrad = p.data_ptr(), q.data_ptr(), wg.data_ptr(), bg.data_ptr()
            slot.wgrad_ld, slot.kind, slot.n_cols, slot.m_out, slot.n_out = wg.stride(0), kind, ncols, m_out, n_out
            slot.recompute, slot.in_pad, slot.in_dim, slot.act_dim = rebuild, f.in_pad, self.in_dim, self.out_dim
            if rebuild & 1:                                         # rider: the first layer's gradient
                w0, b0 = lin[0].weight, lin[0].bias
                assert w0.is_contiguous() and w0.dtype == torch.float32 and w0.grad.stride(1) == 1 and b0.grad.is_contiguous()
                slot.d_w0, slot.d_b0, slot.d_dz0 = w0.data_ptr(), b0.data_ptr(), dzs[0].data_ptr()
                slot.d_w0grad, slot.d_b0grad, slot.w0grad_ld = w0.grad.data_ptr(), b0.grad.data_ptr(), w0.grad.stride(0)
            if rebuild & 2:                                         # rider: the head's gradient
                wh, bh = lin[nh].weight, lin[nh].bias
                assert wh.is_contiguous() and wh.dtype == torch.float32 and wh.grad.stride(1) == 1 and bh.grad.is_contiguous()
                slot.d_wh, slot.d_maskbits, slot.d_a_top = wh.data_ptr(), self._tmask.data_ptr(), acts[nh - 1].data_ptr()
                slot.d_whgrad, slot.d_bhgrad, slot.whgrad_ld = wh.grad.data_ptr(), bh.grad.data_ptr(), wh.grad.stride(0)
        ev = None
        if self.dw_events is not None:
            ev = N.event_pair()
            ev[0].record()
        rider = getattr(self, "_loss_rider", None)
        self._loss_rider = None
        N.check(N.load().tg_mlp_f32_weight_grad_adam(H, arr, len(specs), rows, self._dw_ws.data_ptr(), self._dw_ws.numel() * 4,
                                                     self._head_ws.data_ptr() if rider else None, rider[0] if rider else 0,
                                                     rider[1].data_ptr() if rider else None, C.byref(adam) if adam is not None else None,
                                                     N.stream_ptr(xp.device)), "tg_mlp_f32_weight_grad")
        if adam is not None:
            adam.commit()                # (the launch was accepted: now the optimizer's step counters and the layouts' marks move)
        if ev is not None:
            ev[1].record()
            # algorithmic flops per row (un-padded): every layer's dZ^T A
            self.dw_events.append((ev[0], ev[1], rows, 2 * (nh - 1) * H * H + 2 * H * self.in_dim + 2 * H * self.out_dim, f.dw_kernel()))
        self._acts = self._bits = self._dz_head = self._tmask = None

    @torch.no_grad()
    def backward_fused(self, adam=None):
        """The rest of the backward pass after forward_loss(): the backward chain and the weight gradients (no head job).
        adam (fp32 chain learner only): an optim.FusedAdam.rider() -- the optimizer step rides on the gradient reduction."""
        if self._f32 is not None:
            assert self._acts is not None and self._dz_head is not None, "backward_fused() needs forward_loss()"
            return self._backward_fused_f32(adam)
        assert adam is None, "the optimizer step rides only on the fp32 chain learner's reduction"
        acts, bits = self._acts, self._bits
        assert acts is not None and self._dz_head is not None, "backward_fused() needs forward_loss()"
        self._backward_chain(self._dz_head, acts, bits, acts[0].shape[0], acts[0].device, acts_panel=getattr(self, "_acts_panel", False),
                             dz_panel=bool(self.panel_order) and (getattr(self, "_acts_panel", False) or self.panel_mixed))
        self._dz_head = None

    def _dw(self, dz: torch.Tensor, a: torch.Tensor) -> torch.Tensor:
        """dz^T a in fp32 via a batched GEMM over row blocks (split-K with fp32 partials)."""
        rows = dz.shape[0]
        if rows >= _SPLIT_BATCHES * 4096:
            # big batches: a fixed number of row blocks (2 output tiles each: every CU busy) keeps the fp32 partials --
            # written once, read once by the reduction -- at 128 x 256 KB whatever the row count (3 % at 4 M rows)
            nb, bs = _SPLIT_BATCHES, rows // _SPLIT_BATCHES            # any block length: the tail is < 128 rows
        else:
            nb, bs = rows // _ROW_BLOCK, _ROW_BLOCK
        out = None
        main = nb * bs
        if nb > 0:
            p = torch.bmm(dz[:main].view(nb, bs, dz.shape[1]).transpose(1, 2), a[:main].view(nb, bs, a.shape[1]),
                          out_dtype=torch.float32)
            out = p.sum(0)
        if rows - main > 0:
            tail = torch.mm(dz[main:].t(), a[main:], out_dtype=torch.float32) if self.cd != torch.float32 else dz[main:].t() @ a[main:]
            out = tail if out is None else out + tail
        return out

    def _bias_into(self, grads, partial: torch.Tensor):
        """grads[v] += partial[:, v, :].sum(0) for all v in ONE launch (tg_colsum_finish); partial f32 [blocks][len(grads)][width]
        or [blocks][width] for a single gradient."""
        width = partial.shape[-1]
        if len(grads) > 8 or any(g.dtype != torch.float32 or not g.is_contiguous() or g.numel() != width for g in grads):
            p3 = partial.view(partial.shape[0], len(grads), width).sum(0)
            for v, g in enumerate(grads):
                g.add_(p3[v])
            return
        ptrs = (N.C.c_void_p * len(grads))(*[g.data_ptr() for g in grads])
        N.check(N.load().tg_colsum_finish(partial.data_ptr(), partial.shape[0], len(grads), width, ptrs,
                                          N.stream_ptr(partial.device)), "tg_colsum_finish")

    def _dw_into(self, grad: torch.Tensor, dz: torch.Tensor, a: torch.Tensor):
        """grad += (dz^T a)[:grad.shape[0], :grad.shape[1]].  Big batches: the split-K batched GEMM, then ONE launch of
        tg_dw_finish (partial sums + the < 128-row tail product + the accumulation) instead of a reduction, a tail
        GEMM and two additions."""
        rows = dz.shape[0]
        if (rows < _SPLIT_BATCHES * 4096 or grad.stride(1) != 1 or grad.dtype != torch.float32
                or self.cd not in (torch.bfloat16, torch.float32)):
            grad.add_(self._dw(dz, a)[:grad.shape[0], :grad.shape[1]])
            return
        nb, bs = _SPLIT_BATCHES, rows // _SPLIT_BATCHES
        main = nb * bs
        M, K = dz.shape[1], a.shape[1]
        p = torch.bmm(dz[:main].view(nb, bs, M).transpose(1, 2), a[:main].view(nb, bs, K), out_dtype=torch.float32) \
            if self.cd != torch.float32 else torch.bmm(dz[:main].view(nb, bs, M).transpose(1, 2), a[:main].view(nb, bs, K))
        tail = rows - main
        N.check(N.load().tg_dw_finish(p.data_ptr(), nb, M, K, dz[main:].data_ptr() if tail else None,
                                      a[main:].data_ptr() if tail else None, tail, 1 if self.cd == torch.bfloat16 else 0,
                                      grad.data_ptr(), grad.stride(0), grad.shape[0], grad.shape[1], N.stream_ptr(dz.device)),
                "tg_dw_finish")

    def _backward_chain(self, dz_head, acts, bits, rows, device, acts_panel=False, dz_panel=False):
        """All hidden layers' dZ in one launch (tg_mlp_backward_chain), then every weight and hidden bias gradient in one
        more (tg_mlp_weight_grad: each dZ and activation is read once; the bias sums ride in the same contraction).
        acts_panel: the stored activations are in panel order; dz_panel: the dZ are written (and read) in panel order."""
        lib = N.load()
        self._fresh("bchain")
        L = len(self.linears)
        nh = L - 1                                             # hidden layers; chain order = top (i = L-2) down to i = 0
        H = self._bchain.H
        # the top layer's dZ is neither written nor read: tg_mlp_weight_grad rebuilds it from dz_head and the mask bits (kind RH)
        dzs = [self._ws.get(f"z{j}", _round_up(rows, 32) if dz_panel else rows, H, self.cd, device) if j > 0 else None for j in range(nh)]
        dz_ptrs = (N.C.c_void_p * nh)(*[N.ptr(t) for t in dzs])
        m_ptrs = (N.C.c_void_p * nh)(*[bits[L - 1 - j].data_ptr() for j in range(nh)])     # bits[i + 1] masks hidden layer i
        # the first layer's weight (and, through the ones column of the input, bias) gradient is formed inside the backward chain
        # from the bottom dZ it holds in registers: that dZ is neither written nor read (an input without the ones column -- padded by
        # the caller, not by prepare_input() / tg_learn_compact -- takes the stored form, kind HX)
        xin = acts[0]
        fuse0 = (xin is not None and xin.shape[1] == 32 and self.in_dim < 32 and lin_ok(self.linears[0])
                 and self._has_ones_column(xin))
        if fuse0:
            dzs[nh - 1] = None
            dz_ptrs = (N.C.c_void_p * nh)(*[N.ptr(t) for t in dzs])
            if self._w0_slabs is None:
                self._w0_slabs = torch.empty(2 * lib.tg_mlp_backward_chain_blocks() * H * 32, dtype=torch.float32, device=device)
        depth = self._set_depth_kernels(lib) and dz_panel and fuse0 and H == 256 and nh == 5      # (what the launcher picks: the events' label)
        ev = None
        if self.dx_events is not None:
            ev = N.event_pair()
            ev[0].record()
        n_slabs = N.C.c_int32(0)
        if dz_panel:
            N.check(lib.tg_mlp_backward_chain_ex(dz_head.data_ptr(), self._bchain.stream.data_ptr(), H, nh, rows, dz_ptrs, m_ptrs,
                                                 xin.data_ptr() if fuse0 else None, N.ptr(self._w0_slabs) if fuse0 else None,
                                                 self._w0_slabs.numel() if fuse0 else 0, N.C.byref(n_slabs), N.TG_LAYOUT_PANEL,
                                                 N.stream_ptr(device)), "tg_mlp_backward_chain_ex")
        elif fuse0:
            N.check(lib.tg_mlp_backward_chain_w0(dz_head.data_ptr(), self._bchain.stream.data_ptr(), H, nh, rows, dz_ptrs, m_ptrs,
                                                 xin.data_ptr(), self._w0_slabs.data_ptr(), self._w0_slabs.numel(),
                                                 N.C.byref(n_slabs), N.stream_ptr(device)), "tg_mlp_backward_chain_w0")
        else:
            N.check(lib.tg_mlp_backward_chain(dz_head.data_ptr(), self._bchain.stream.data_ptr(), H, nh, rows, dz_ptrs, m_ptrs,
                                              None, N.stream_ptr(device)), "tg_mlp_backward_chain")
        if ev is not None:
            ev[1].record()
            n_stored = nh - 1 - (1 if fuse0 else 0)
            self.dx_events.append((ev[0], ev[1], rows, 16 + nh * (H // 8) + n_stored * 2 * H + (64 if fuse0 else 0),
                                   f"tg::mlp_bwd_chain_kernel<{H},8,{'true' if fuse0 else 'false'}{',true' if dz_panel else ''}{',5' if depth else ''}>"))
        riders, loss_rider = getattr(self, "_riders", None) or ([], None)
        self._riders = None
        if fuse0 and rows > 0:
            # the first layer's partial gradients ([H][32] per slab; column 31 = the bias): added by the weight-gradient reduction launch
            l0 = self.linears[0]
            riders = riders + [(self._w0_slabs, 0, H * 32, n_slabs.value, 32, l0.weight.grad, H, self.in_dim),
                               (self._w0_slabs, 31, H * 32, n_slabs.value, 32, l0.bias.grad, H, 1)]
        if self._dw_ws is None:
            self._dw_ws = weight_grad_workspace(H, device)
        lin = self.linears
        # head (bias: tg_head_prep) -- unless forward_loss() already formed its gradient and did not store the top activation
        jobs = [(N.TG_DW_DH, dz_head, acts[L - 1], lin[L - 1].weight.grad, None)] if acts[L - 1] is not None else []
        lp, lq = (N.DW_P_PANEL if dz_panel else 0), (N.DW_Q_PANEL if acts_panel else 0)      # layout of the [rows][H] operands
        assert not (acts_panel and jobs), "the head job reads a row-major top activation"
        for j in range(nh - 1):
            i = L - 2 - j                                                                      # hidden-to-hidden layer i
            if j == 0:                                                                         # top layer: dZ not stored
                assert acts[i] is not None
                jobs.append((N.TG_DW_RH, dz_head, acts[i], lin[i].weight.grad, lin[i].bias.grad, bits[L - 1], lq))
            elif acts[i] is None:                                                              # i == 1: input not stored
                jobs.append((N.TG_DW_HR, dzs[j], acts[0], lin[i].weight.grad, lin[i].bias.grad, None, lp))
            else:
                jobs.append((N.TG_DW_HH, dzs[j], acts[i], lin[i].weight.grad, lin[i].bias.grad, None, lp | lq))
        if not fuse0:
            jobs.append((N.TG_DW_HX, dzs[nh - 1], acts[0], lin[0].weight.grad, lin[0].bias.grad, None, lp))
        ev = None
        if self.dw_events is not None:
            ev = N.event_pair()
            ev[0].record()
        weight_grad(H, jobs, rows, self._dw_ws, self._chain.stream, self._chain.bias[0], self._bchain.stream, riders, loss_rider)
        if ev is not None:
            ev[1].record()
            per_row = sum({N.TG_DW_HH: 4 * H, N.TG_DW_HX: 2 * H + 64, N.TG_DW_HR: 2 * H + 64, N.TG_DW_DH: 2 * H + 16,
                           N.TG_DW_RH: 2 * H + 16 + H // 8}[jb[0]] for jb in jobs)
            self.dw_events.append((ev[0], ev[1], rows, per_row, f"tg::dw_kernel<{H}>"))
        self._acts = self._bits = None

    @torch.no_grad()
    def backward(self, dout: torch.Tensor):
        if self.act != "ReLU":
            raise NotImplementedError(f"GemmMLP.backward() of a {self.act} net: the per-layer backward kernels apply the ReLU mask; a "
                                      f"{self.act} net trains through forward_loss() / backward_fused() (fp32 chain learner) only")
        return self._backward_relu(dout)

    def _backward_relu(self, dout: torch.Tensor):
        """dout fp32 [rows][out_dim] = d loss / d output.  Accumulates into weight.grad / bias.grad (fp32)."""
        acts = self._acts
        assert acts is not None, "backward() needs forward(keep=True)"
        bits = self._bits if self._bits is not None else [None] * len(acts)      # ReLU mask bits of acts[i] (chain forward)
        lib = N.load()
        rows = dout.shape[0]
        L = len(self.linears)
        dout = dout.contiguous()
        dz = self._ws.get("z_head", rows, self.out_pad, self.cd, dout.device)
        lin = self.linears[-1]
        if (self.out_dim <= 8 and self.out_pad <= 16 and self.cd in (torch.bfloat16, torch.float32) and dout.dtype == torch.float32
                and lin.bias.grad.dtype == torch.float32 and lin.bias.grad.is_contiguous()):
            # padded compute-dtype copy of dout + the head's bias gradient: two launches instead of four
            if self._head_partial is None:
                self._head_partial = torch.empty(lib.tg_head_prep_blocks(), self.out_dim, dtype=torch.float32, device=dout.device)
            N.check(lib.tg_head_prep(dout.data_ptr(), rows, self.out_dim, self.out_pad, 1 if self.cd == torch.bfloat16 else 0,
                                     dz.data_ptr(), self._head_partial.data_ptr(), N.stream_ptr(dout.device)), "tg_head_prep")
            self._bias_into([lin.bias.grad], self._head_partial)
        else:
            dz.zero_()
            dz[:, :self.out_dim].copy_(dout)
            lin.bias.grad.add_(dout.sum(0))
        if self._bits is not None and self._chain_backward_ok():
            self._backward_chain(dz, acts, bits, rows, dout.device)
            return
        assert all(a is not None for a in acts), "the gradient buffers changed between forward(keep=True) and backward()"
        self._dw_into(lin.weight.grad, dz, acts[L - 1])
        self._fresh("dx")
        is_bf16 = 1 if self.cd == torch.bfloat16 else 0
        nblk = lib.tg_relu_bwd_bias_blocks()
        fuse_head = self.out_dim <= 8
        st = N.stream_ptr(dout.device)
        for i in range(L - 2, -1, -1):
            a = acts[i + 1]                                    # post-ReLU output of hidden layer i
            cols = a.shape[1]
            frag = self._dxfrag[i + 1] if i < L - 2 else None
            if frag is not None:
                # dZ_i = (dZ_{i+1} W_{i+1}) * (a > 0) and its column sums in one pass on the matrix cores
                if self._dx_partial is None or self._dx_partial.shape[1] != cols:
                    self._dx_partial = torch.empty(lib.tg_dx_relu_bias_blocks(), cols, dtype=torch.float32, device=dout.device)
                partial = self._dx_partial
                dz_below = torch.empty_like(a)
                ev = None
                if self.dx_events is not None:
                    ev = N.event_pair()
                    ev[0].record()
                mb = bits[i + 1]
                N.check(lib.tg_dx_relu_bias(dz.data_ptr(), frag.data_ptr(), a.data_ptr(), None if mb is None else mb.data_ptr(),
                                            dz_below.data_ptr(), rows, dz.shape[1], cols, partial.data_ptr(), st),
                        "tg_dx_relu_bias")
                if ev is not None:
                    ev[1].record()
                    self.dx_events.append((ev[0], ev[1], rows, 2 * (dz.shape[1] + cols) + (cols // 8 if mb is not None else 2 * cols),
                                           "tg::dx_relu_bias_kernel<%d,%d>" % (cols, dz.shape[1])))
                dz = dz_below
            else:
                if self._partial is None or self._partial.shape[1] != cols:
                    self._partial = torch.empty(nblk, cols, dtype=torch.float32, device=dout.device)
                partial = self._partial
                if i == L - 2 and fuse_head:
                    # top hidden layer: dA = dout . W_head is a rank-A product, formed inside the ReLU-backward kernel
                    da = torch.empty_like(a)
                    mb = bits[i + 1]
                    N.check(lib.tg_head_bwd_relu_bias(dout.data_ptr(), self.out_dim, self.linears[-1].weight.data_ptr(),
                                                      a.data_ptr(), None if mb is None else mb.data_ptr(), da.data_ptr(), rows,
                                                      cols, is_bf16, partial.data_ptr(), st), "tg_head_bwd_relu_bias")
                else:
                    da = dz @ self.w[i + 1]
                    N.check(lib.tg_relu_bwd_bias(da.data_ptr(), a.data_ptr(), rows, cols, is_bf16, partial.data_ptr(), st),
                            "tg_relu_bwd_bias")
                dz = da
            lin = self.linears[i]
            self._bias_into([lin.bias.grad], partial)
            self._dw_into(lin.weight.grad, dz, acts[i])
        self._acts = self._bits = None


# ---------------------------------------------------------------------------------------------
# weight stream of the fused rollout kernel (csrc/fused_rollout.hip)
# ---------------------------------------------------------------------------------------------
def fused_rollout_supported(net, obs_dim: int, act_dim: int) -> int:
    """Hidden width H if `net` is Linear(S,H) ReLU [Linear(H,H) ReLU]* Linear(H,A) with H in {128,256}, else 0."""
    s = _mlp_shape(net)
    return s[1] if s and s[4] == "ReLU" and s[1] in (128, 256) and obs_dim <= 32 and act_dim <= 4 else 0


def weights_key(lin):
    """What every derived operand is a function of: the master tensors' storage and torch version counters, and the count of
    raw-pointer parameter writes (the fused Adam launch bypasses the version counters)."""
    return (tuple((p.data_ptr(), p._version) for l in lin for p in (l.weight, l.bias)), N.RAW_PARAM_WRITES[0])


class WeightStream:
    """A kernel family's weights in the order its lanes read them, kept current from the fp32 masters by ONE gather.
    Source: the masters of `self.lin` laid end to end -- every weight row-major, then every bias, then one zero that every padded
    position points at.  A subclass sets `lin` (and what its kernels ask of it), says in _layout() which source element each
    position of each buffer holds, and calls _build(); the refresh, the gather codes of optim.StreamRefresher and the freshness key
    are written here once.
      outputs: [(destination, is_bf16)] -- one flat buffer per allocation, in the order of `_idx`, whose sizes partition it."""
    rides_on_optimizer_step = False     # a rollout engine's stream that joins the learner's gather (StreamRefresher extra_streams)
                                        # and is then trusted as fresh at the next rollout's entry: the fp32 fused rollout's only

    def _layout(self, woff, boff, zero_at, dev):
        """[(is_bf16, [(attribute, [index pieces]), ...])], one entry per allocation: the first attribute names the whole buffer,
        every later one a view of its own range.  woff[i] / boff[i]: where weight / bias i of `lin` starts in the source."""
        raise NotImplementedError

    def _build(self):
        lin = self.lin
        dev = lin[0].weight.device
        sizes = [l.weight.numel() for l in lin] + [l.bias.numel() for l in lin]
        starts = [sum(sizes[:i]) for i in range(len(sizes) + 1)]
        idx, self.outputs, self._stage = [], [], []
        for is_bf16, parts in self._layout(starts[:len(lin)], starts[len(lin):-1], starts[-1], dev):
            flat = [torch.cat([p.reshape(-1) for p in pieces] + [torch.empty(0, dtype=torch.int64, device=dev)]) for _, pieces in parts]
            buf = torch.empty(sum(f.numel() for f in flat), dtype=torch.bfloat16 if is_bf16 else torch.float32, device=dev)
            setattr(self, parts[0][0], buf)
            at = flat[0].numel()
            for (attr, _), f in zip(parts[1:], flat[1:]):
                setattr(self, attr, buf[at:at + f.numel()])
                at += f.numel()
            idx += flat
            self.outputs.append((buf, is_bf16))
            self._stage.append(torch.empty(buf.numel(), dtype=torch.float32, device=dev) if is_bf16 else None)
        self._idx = torch.cat(idx)
        self._zero = torch.zeros(1, dtype=torch.float32, device=dev)
        self._fresh_key = None

    def refresh(self):
        self._refresh()
        self.mark_fresh()

    @torch.no_grad()
    def _refresh(self):
        """Concatenate the masters, then one gather per buffer (+ the conversion of a bf16 one): 2 launches for one fp32 buffer."""
        src = torch.cat([l.weight.reshape(-1) for l in self.lin] + [l.bias for l in self.lin] + [self._zero])
        src = src if src.dtype == torch.float32 else src.float()
        at = 0
        for (dst, is_bf16), stage in zip(self.outputs, self._stage):
            torch.index_select(src, 0, self._idx[at:at + dst.numel()], out=stage if is_bf16 else dst)
            if is_bf16:
                dst.copy_(stage)
            at += dst.numel()

    def segments(self, tensor_ids):
        """The buffers as tg_gather_streams segments: [(dst, int32 code per element, is_bf16)], code = master tensor << 24 | offset,
        -1 = zero.  tensor_ids: optim.FusedAdam's id(param) -> (group, tensor); a master outside group 0 is an AssertionError and one
        the optimizer does not hold a KeyError (optim.StreamRefresher remembers either as a layout its launch cannot cover)."""
        codes = []
        for p in [l.weight for l in self.lin] + [l.bias for l in self.lin]:
            gi, ti = tensor_ids[id(p)]
            assert gi == 0
            codes.append((ti << 24) + torch.arange(p.numel(), dtype=torch.int64))
        codes.append(torch.tensor([-1], dtype=torch.int64))
        codes = torch.cat(codes).to(self._idx.device)[self._idx].to(torch.int32)
        segs, at = [], 0
        for dst, is_bf16 in self.outputs:
            segs.append((dst, codes[at:at + dst.numel()].contiguous(), int(is_bf16)))
            at += dst.numel()
        return segs

    def mark_fresh(self) -> None:
        self._fresh_key = weights_key(self.lin)

    def is_fresh(self) -> bool:
        return not N.ALWAYS_REBUILD and self._fresh_key == weights_key(self.lin)


def _head_table(lin, woff, boff, zero_at, dev, bias_rows: int, head_rows: int, head_bias: int):
    """Index pieces of the fp32 kernels' table [bias_rows][H] hidden biases | [head_rows][H] head weights | [head_bias] head bias;
    rows and entries the net does not have are zero."""
    H, nh, A = lin[0].out_features, len(lin) - 1, lin[-1].out_features
    j, zeros = torch.arange(H, device=dev), torch.full((H,), zero_at, device=dev)
    return ([boff[l] + j if l < nh else zeros for l in range(bias_rows)]
            + [woff[nh] + a * H + j if a < A else zeros for a in range(head_rows)]
            + [torch.tensor([boff[nh] + a if a < A else zero_at for a in range(head_bias)], device=dev)])


def _fragment_index(k_pad: int, device):
    """[k_pad/16][64 lanes][8]: column of W that element j of lane (r, h) holds at k-step ks:
    16*ks + 8*(j>>2) + 4*h + (j&3)  (the order in which an MFMA accumulator tile hands its rows over)."""
    ks = torch.arange(k_pad // 16, device=device).view(-1, 1, 1)
    lane = torch.arange(64, device=device).view(1, -1, 1)
    j = torch.arange(8, device=device).view(1, 1, -1)
    return 16 * ks + 8 * (j >> 2) + 4 * (lane >> 5) + (j & 3)


def _chain_fragment_index(k_pad: int, device):
    """[k_pad/32 k-steps][2 feature halves f][64 lanes][8] -> (row within the 32-row block, column) of W for the chain kernels'
    `v_mfma_f32_16x16x32_bf16` A fragments.  Lane (i = lane & 15, g = lane >> 4) of half f holds, for k-step ks, the 8 weights
    W[rowmap(f, i)][32 ks + 8 g + j]: the k order is natural (the B operand of the next layer is the packed accumulator of this
    one, whose lane (col, g) holds the 8 CONSECUTIVE features 8 g .. 8 g + 7 of a block -- that is what the row map arranges:
    accumulator register r of lane group g in half f is output feature 8 g + 4 f + r)."""
    ks = torch.arange(k_pad // 32, device=device).view(-1, 1, 1, 1)
    f = torch.arange(2, device=device).view(1, -1, 1, 1)
    lane = torch.arange(64, device=device).view(1, 1, -1, 1)
    j = torch.arange(8, device=device).view(1, 1, 1, -1)
    i = lane & 15
    chain_row = (8 * (i >> 2) + 4 * f + (i & 3)).expand(k_pad // 32, 2, 64, 8)      # outputs that feed another layer / are stored
    natural_row = (16 * f + i).expand(k_pad // 32, 2, 64, 8)                          # the forward head: outputs 0..15 in half 0
    col = (32 * ks + 8 * (lane >> 4) + j).expand(k_pad // 32, 2, 64, 8)
    return chain_row, natural_row, col


class FragmentStream(WeightStream):
    """bf16 weight stream + f32 bias table in the layout tg_fused_rollout (layout="rollout", 32x32x16 MFMA) or the chain
    kernels (layout="chain", 16x16x32 MFMA: tg_mlp_forward_chain, tg_mlp_backward_chain, tg_mlp_weight_grad's recompute)
    consume (refresh: three launches + one for the bias table).
    rollout: blocks = the first layer's output tiles (2 k-steps each), then one block per 32-row output tile of every later
      layer; a block = its k-steps x 64 lanes x 8 bf16 (1 KiB per k-step); lane (m, h) holds 8 weights of output row 32*tile + m.
    chain: every block is H/16 pieces of 1 KiB.  A matrix with K <= 32 (the first layer; the backward stream's W_head^T) is ONE
      block [output block mt][half f]; a matrix with K = H is one block per 32 output features, [k-step ks][half f]
      (_chain_fragment_index documents the lane map); the forward head keeps its <= 16 outputs in half 0, natural order.
    bias: [layers][H], zero padded."""

    def __init__(self, net, H: int, layout: str = "rollout", transposed: bool = False):
        """transposed=True: the stream of the backward chain (tg_mlp_backward_chain): the head first, then the
        hidden-to-hidden layers from the top down, every matrix transposed ([in][out]); no bias table (`bias` stays zero)."""
        assert layout in ("rollout", "chain")
        lin = _linears(net)
        self.H, self.layout, self.transposed = H, layout, transposed
        self.lin = lin[:0:-1] if transposed else lin            # head, L-2, ..., 1  |  0, 1, ..., head
        self._build()
        self.bias = (torch.zeros(len(self.lin), H, dtype=torch.float32, device=self.stream.device) if transposed else
                     self.bias.view(len(self.lin), H))
        self.refresh()

    def _layout(self, woff, boff, zero_at, dev):
        transposed = self.transposed
        m = torch.arange(64, device=dev) & 31
        stream = []
        for li, l in enumerate(self.lin):
            rows_, cols_ = (l.in_features, l.out_features) if transposed else (l.out_features, l.in_features)
            m_pad, k_pad = _round_up(rows_, 32), _round_up(cols_, 32)
            if self.layout == "rollout":
                kidx = _fragment_index(k_pad, dev)
                rmap = m.view(1, -1, 1).expand_as(kidx)
            else:
                chain_row, natural_row, kidx = _chain_fragment_index(k_pad, dev)
                rmap = natural_row if (not transposed and li == len(self.lin) - 1) else chain_row
            for mo in range(m_pad // 32):
                r = 32 * mo + rmap                                             # row / column of the (transposed) padded matrix
                c = kidx
                src = woff[li] + (c * l.in_features + r if transposed else r * l.in_features + c)   # weight is [out][in]
                stream.append(torch.where((r < rows_) & (c < cols_), src, torch.full_like(src, zero_at)))
        if transposed:
            return [(True, [("stream", stream)])]
        j = torch.arange(self.H, device=dev)
        bias = [torch.where(j < l.out_features, boff[li] + j, torch.full_like(j, zero_at)) for li, l in enumerate(self.lin)]
        return [(True, [("stream", stream)]), (False, [("bias", bias)])]


def fragment_stream(net, H: int):
    """(bf16 weight stream, f32 bias table) in the layout tg_fused_rollout consumes (one-shot form of FragmentStream)."""
    fs = FragmentStream(net, H)
    return fs.stream, fs.bias


# ---------------------------------------------------------------------------------------------
# register-resident fp32 weights of the fp32 fused rollout kernel (csrc/fused_rollout_f32.hip)
# ---------------------------------------------------------------------------------------------
def fused_rollout_f32_supported(net, obs_dim: int, act_dim: int, activations=("ReLU",)) -> int:
    """Hidden width H if `net` is Linear(S,H) act [Linear(H,H) act]* Linear(H,A) with act in `activations` (hidden_activation();
    the kernels have "ReLU" and "Tanh": DeviceRollout asks for both, the default keeps the ReLU-only meaning of tg_fused_rollout_f32),
    H in {64,128} and 1..4 hidden layers (what tg_fused_rollout_f32[_act] has kernels for), else 0."""
    s = _mlp_shape(net)
    return s[1] if (s and s[4] in activations and s[4] in ACTIVATIONS and s[1] in (64, 128) and 1 <= s[2] <= 4
                    and obs_dim <= 32 and act_dim <= 4) else 0


class RegisterStreamF32(WeightStream):
    """fp32 weights in the order tg_fused_rollout_f32 loads them into registers:
    [H/32 waves][K1/2 + n_hh*H/2 registers][64 lanes] (first layer: K1 = in_features rounded up to 8, zero beyond).
    block_envs 32: register 4q + j of lane (m, kh) of wave w holds W[32w + m][8q + 4kh + j];
    block_envs 16: register tt * (k / 4) + s of lane (i, g) holds W[32w + 16 tt + i][first layer: 4 s + g; H x H: 16 (s >> 2) + 4 g + (s & 3)].
    `table` = [n_hidden*H hidden biases][4*H head weights][4 head biases].  Refresh: three launches (two buffers)."""
    rides_on_optimizer_step = True

    def __init__(self, net, H: int, block_envs: int = 32):
        assert block_envs in (16, 32)
        self.block_envs = block_envs
        self.lin, self.H = _linears(net), H
        self._build()
        self.refresh()

    def _layout(self, woff, boff, zero_at, dev):
        H, lin = self.H, self.lin
        lane = torch.arange(64, device=dev).view(1, 1, -1)
        wave = torch.arange(H // 32, device=dev).view(-1, 1, 1)
        regs = []
        for li, l in enumerate(lin[:-1]):
            k = _round_up(l.in_features, 8)
            r = torch.arange(k // 2, device=dev).view(1, -1, 1)
            if self.block_envs == 32:
                row = 32 * wave + (lane & 31)
                colk = 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3)
            else:
                tt, s_ = r // (k // 4), r % (k // 4)
                row = 32 * wave + 16 * tt + (lane & 15)
                colk = 4 * s_ + (lane >> 4) if li == 0 else 16 * (s_ >> 2) + 4 * (lane >> 4) + (s_ & 3)
            src = woff[li] + row * l.in_features + colk                               # [waves][k/2][64]
            regs.append(torch.where(colk < l.in_features, src, torch.full_like(src, zero_at)))
        return [(False, [("stream", [torch.cat(regs, dim=1)])]),
                (False, [("table", _head_table(lin, woff, boff, zero_at, dev, len(lin) - 1, 4, 4))])]


# ---------------------------------------------------------------------------------------------
# fp32 chain learner (csrc/mlp_f32_chain.hip): weight stream of tg_mlp_f32_forward / _forward_backward
# ---------------------------------------------------------------------------------------------
def f32_chain_supported(net) -> int:
    """Hidden width H if `net` is Linear(S<=32, H) act [Linear(H, H) act]{0..3} Linear(H, A<=4), act = ReLU or Tanh
    (hidden_activation()), with H in {64, 128} -- the reference's own policy shapes (pipelines/cartpole_pipeline_grpo.py:54-76,
    cartpole_pipeline_ppo.py:54-79) -- else 0."""
    s = _mlp_shape(net)
    return s[1] if s and s[1] in (64, 128) and 1 <= s[2] <= 4 and s[0] <= 32 and s[3] <= 4 else 0


def f32_res_supported(net) -> int:
    """128 if `net` is Linear(S<=32, 128) ReLU [Linear(128, 128) ReLU]{0..1} Linear(128, A<=4) -- BASELINE configs[1]'s policy
    (5-128-128-1) and its like: the whole weight stream fits the LDS beside the tables -- else 0."""
    s = _mlp_shape(net)
    ok = s and s[4] == "ReLU" and s[1] == 128 and 1 <= s[2] <= 2 and s[0] <= 32 and s[3] <= 4
    return 128 if ok and N.load().tg_mlp_f32r_supported(128, s[2], _round_up(s[0], 8)) else 0


def f32_wide_supported(net) -> int:
    """256 if `net` is Linear(S<=32, 256) ReLU [Linear(256, 256) ReLU]{0..4} Linear(256, A<=4) -- the reference's QuadPole factory
    (pipelines/quadpole_pipeline_ppo.py:54-58: 20-256x5-{4,1}) -- else 0."""
    s = _mlp_shape(net)
    return 256 if s and s[4] == "ReLU" and s[1] == 256 and 1 <= s[2] <= 5 and s[0] <= 32 and s[3] <= 4 else 0


class F32ChainStream(WeightStream):
    """The fp32 weight stream of the chain learner (refresh: two launches):
      [first layer, MFMA fragment order: H/32 tiles x k2/4 groups x 64 lanes x 4]  lane (i, kk), step s = 4 g + e of tile mo holds
                                                                                 W0[32 mo + i][s + kk k2]   (k2 = in_pad / 2)
      [hidden biases: n_hidden x H]  [head weights: 4 x H, rows >= A zero]  [head bias: 4]          (natural order)
      [forward blocks]   layer l = 1..n_hh, output tile mo: H/8 groups x 64 lanes x 4; step s = 16 mt + t holds
                         W_l[32 mo + i][32 mt + F(t, kk)],  F(t, kk) = (t & 3) + 8 (t >> 2) + 4 kk  -- register t of the two lane
                         halves of the previous layer's accumulator tile mt (v_mfma_f32_32x32x2_f32: see the kernel's header)
      [backward blocks]  layer l = n_hh..1 (top first), output tile ko over the layer's INPUT features:
                         W_l[32 mt + F(t, kk)][32 ko + i]
    The methods say what GemmMLP needs to know of an fp32 learner machine besides its weights; F32ResStream and F32WideStream
    override what differs on theirs."""
    wide, res, machine = False, False, "f32"
    tile_rows = 256                 # rows per workgroup pass: the launchers' grid is min(blocks(), ceil(rows / tile_rows))
    takes_mask_bits = True          # the training entry takes the pointer of the top layer's ReLU mask bits ...
    rebuilds_on_chip = True         # ... for the weight-gradient jobs that rebuild the first activation and the top dZ on chip

    def __init__(self, net, H: int, activation: str = "ReLU"):
        self.act = ACTIVATIONS[activation]          # the kernels' hidden activation (TG_ACT_*): the stream itself does not depend on it
        self._dims(net, H)
        self._build()
        n = N.load().tg_mlp_f32_stream_floats(H, self.n_hidden, self.in_pad)
        assert self.stream.numel() == n, (self.stream.numel(), n)
        self.refresh()

    def _dims(self, net, H):
        self.lin, self.H = _linears(net), H
        self.n_hidden, self.in_dim, self.out_dim = len(self.lin) - 1, self.lin[0].in_features, self.lin[-1].out_features
        self.in_pad = _round_up(self.in_dim, 8)

    def _layout(self, woff, boff, zero_at, dev):
        H, nh = self.H, self.n_hidden
        K2, MT = self.in_pad // 2, H // 32
        lane = torch.arange(64, device=dev).view(1, 64, 1)
        i, kk = lane & 31, lane >> 5
        e = torch.arange(4, device=dev).view(1, 1, 4)
        idx = []
        # first layer
        g = torch.arange(K2 // 4, device=dev).view(-1, 1, 1)
        col = (4 * g + e) + kk * K2
        for mo in range(MT):
            row = (32 * mo + i).expand(K2 // 4, 64, 4)
            src = woff[0] + row * self.in_dim + col
            idx.append(torch.where(col.expand_as(src) < self.in_dim, src, torch.full_like(src, zero_at)))
        idx += _head_table(self.lin, woff, boff, zero_at, dev, nh, 4, 4)
        # H x H blocks
        g = torch.arange(H // 8, device=dev).view(-1, 1, 1)
        s = 4 * g + e
        mt, t = s // 16, s % 16
        feat = (32 * mt + (t & 3) + 8 * (t >> 2) + 4 * kk).expand(H // 8, 64, 4)      # the contraction index of step s, lane half kk
        for l in range(1, nh):                                                          # forward: W_l[32 mo + i][feat]
            for mo in range(MT):
                idx.append(woff[l] + (32 * mo + i) * H + feat)
        for l in range(nh - 1, 0, -1):                                                  # backward: W_l[feat][32 ko + i]
            for ko in range(MT):
                idx.append(woff[l] + feat * H + (32 * ko + i))
        return [(False, [("stream", idx)])]

    # (common to every entry: input, its padding, weight stream; then these; then rows and the buffers)
    def forward_args(self):
        """What the no-grad entry (forward_entry) takes of this machine's weights and shape."""
        return self.H, self.n_hidden

    def loss_args(self):
        """... and the training entry (loss_entry)."""
        return self.H, self.n_hidden

    def blocks(self) -> int:
        return N.load().tg_mlp_f32_blocks()

    def grid(self, rows: int) -> int:
        """Workgroups of the training entry at `rows` (the launcher's own grid): the partial loss sums it leaves."""
        return min(self.blocks(), -(-rows // self.tile_rows))

    def kernel_prefix(self) -> str:
        """The training kernel as the profiler names it, up to loss_entry()'s trailing template arguments."""
        return f"tg::mlp_f32_chain_kernel<{self.H},true"

    def dw_kernel(self) -> str:
        """The weight-gradient launch as the profiler names it."""
        one_job = self.H == 128 and self.n_hidden == 2
        return f"tg::mlp_f32_dw_fused8_kernel<{self.H},...> + finish" if one_job else f"tg::mlp_f32_dw_kernel<{self.H}> + finish"

    def log_line(self) -> str:
        if self.act == N.TG_ACT_TANH:
            return " Tanh: fp32 chain learner (tg_mlp_f32_forward_act / _forward_backward_act / _weight_grad)"
        return ": fp32 chain learner (tg_mlp_f32_forward / _forward_backward / _weight_grad)"


def _f32_16x16_blocks(woff, nh, H, dev):
    """Index pieces of the H x H blocks the 16x16x4 fp32 MFMA kernels (resident, H = 256) share, lane = (i = lane & 15, g = lane >> 4),
    [H/16 pieces t][64 lanes][4 e] per block: forward, layer l = 1 .. nh - 1, block mo: W_l[16 mo + i][16 t + 4 g + e]; then
    backward, layer l = nh - 1 .. 1, block ko: W_l[16 t + 4 g + e][16 ko + i]."""
    NT = H // 16
    lane = torch.arange(64, device=dev).view(1, 64, 1)
    i, g = lane & 15, lane >> 4
    e = torch.arange(4, device=dev).view(1, 1, 4)
    t = torch.arange(NT, device=dev).view(NT, 1, 1)
    k = (16 * t + 4 * g + e).expand(NT, 64, 4)                                       # the contraction index of piece t, lane group g
    return ([woff[l] + (16 * mo + i) * H + k for l in range(1, nh) for mo in range(NT)]
            + [woff[l] + k * H + (16 * ko + i) for l in range(nh - 1, 0, -1) for ko in range(NT)])


class F32ResStream(F32ChainStream):
    """Weight stream, first-layer table and bias / head table of the resident 16-row kernel (csrc/mlp_f32_wide.hip, mlp_f32_res_kernel),
    ONE buffer (refresh: two launches): lane = (i = lane & 15, g = lane >> 4)
      stream: forward blocks [8 mo][8 t][64 lanes][4]: W_1[16 mo + i][16 t + 4 g + e]; backward blocks [8 ko][8 t][64][4]:
              W_1[16 t + 4 g + e][16 ko + i]            (nothing with one hidden layer)
      w0:     [8 mo][in_pad / 4 steps s][64 lanes]: W0[16 mo + i][4 s + g]              (zero beyond the inputs)
      table:  [2][128] hidden biases | [4][128] head weights (rows >= A zero) | [4] head bias | 12 zeros
    `stream` is the whole buffer, `w0` and `table` are views of it."""
    wide, res, act, machine = False, True, 0, "f32r"        # (act: TG_ACT_RELU -- the resident kernel is ReLU-only)

    def __init__(self, net):
        self._dims(net, 128)
        self._build()
        lib, H, nh = N.load(), 128, self.n_hidden
        assert self.stream.numel() - self.w0.numel() - self.table.numel() == lib.tg_mlp_f32r_stream_floats(H, nh)
        assert self.w0.numel() == lib.tg_mlp_f32r_w0_floats(H, self.in_pad) and self.table.numel() == lib.tg_mlp_f32r_table_floats(H)
        self.refresh()

    def _layout(self, woff, boff, zero_at, dev):
        K4 = self.in_pad // 4
        blocks = _f32_16x16_blocks(woff, self.n_hidden, 128, dev)
        s4 = torch.arange(K4, device=dev).view(K4, 1)
        ln = torch.arange(64, device=dev).view(1, 64)
        col = (4 * s4 + (ln >> 4)).expand(K4, 64)
        w0 = []
        for mo in range(8):
            src = woff[0] + (16 * mo + (ln & 15)).expand(K4, 64) * self.in_dim + col
            w0.append(torch.where(col < self.in_dim, src, torch.full_like(src, zero_at)))
        # (with one hidden layer there are no blocks: the buffer then starts with the first-layer table)
        parts = [("stream", blocks), ("w0", w0), ("table", _head_table(self.lin, woff, boff, zero_at, dev, 2, 4, 16))]
        return [(False, parts)]

    def forward_args(self):
        return self.w0.data_ptr(), self.table.data_ptr(), self.H, self.n_hidden, self.out_dim

    def loss_args(self):
        return self.w0.data_ptr(), self.table.data_ptr(), self.H, self.n_hidden

    def grid(self, rows: int) -> int:
        return N.load().tg_mlp_f32r_grid(rows)

    def kernel_prefix(self) -> str:
        return f"tg::mlp_f32_res_kernel<{self.H},{self.in_pad // 4},true"


class F32WideStream(F32ChainStream):
    """The fp32 weight stream + tables of the H = 256 chain learner (csrc/mlp_f32_wide.hip), ONE buffer (refresh: two launches).
    16-KiB blocks of 16 pieces x 64 lanes x 16 B, lane = (i = lane & 15, g = lane >> 4); a lane's 16 B are four consecutive
    floats of a weight row (forward) or of a weight column (backward):
      first layer, 2 blocks: block b, piece 2 tt + q:     W0[16 (8 b + tt) + i][8 g + 4 q + e]      (zero beyond the inputs)
      forward, layer l = 1 .. nh - 1, block mo, piece t:  W_l[16 mo + i][16 t + 4 g + e]
      backward, layer l = nh - 1 .. 1, block ko, piece t: W_l[16 t + 4 g + e][16 ko + i]
    then the tables (`table`, a view): [5][256] hidden biases | [4][256] head weights (rows >= A zero) | [4] head bias | 12 zeros."""
    wide, res, act, machine = True, False, 0, "f32w"        # (act: TG_ACT_RELU -- the H = 256 kernel is ReLU-only)
    tile_rows = 64
    takes_mask_bits = False         # (the H = 256 learner's weight-gradient jobs read every operand back: nothing is rebuilt there yet)
    rebuilds_on_chip = False

    def __init__(self, net):
        self._dims(net, 256)
        self._build()
        lib = N.load()
        assert self.stream.numel() - self.table.numel() == lib.tg_mlp_f32w_stream_floats(self.n_hidden)
        assert self.table.numel() == lib.tg_mlp_f32w_table_floats()
        self.refresh()

    def _layout(self, woff, boff, zero_at, dev):
        lane = torch.arange(64, device=dev).view(1, 64, 1)
        i, g = lane & 15, lane >> 4
        e = torch.arange(4, device=dev).view(1, 1, 4)
        q = torch.arange(2, device=dev).view(2, 1, 1)
        col = (8 * g + 4 * q + e).expand(2, 64, 4)
        first = []
        for mo in range(16):                                                         # first layer: 16 tiles x 2 pieces
            src = woff[0] + (16 * mo + i) * self.in_dim + col
            first.append(torch.where(col < self.in_dim, src, torch.full_like(src, zero_at)))
        blocks = _f32_16x16_blocks(woff, self.n_hidden, 256, dev)
        return [(False, [("stream", first + blocks), ("table", _head_table(self.lin, woff, boff, zero_at, dev, 5, 4, 16))])]

    def forward_args(self):
        return self.table.data_ptr(), self.n_hidden

    def loss_args(self):
        return self.table.data_ptr(), self.n_hidden

    def blocks(self) -> int:
        return N.load().tg_mlp_f32w_blocks()

    def kernel_prefix(self) -> str:
        return "tg::mlp_f32_wide_kernel<true"

    def dw_kernel(self) -> str:
        return "tg::mlp_f32_wide_dw_kernel + finish"

    def log_line(self) -> str:
        return ": fp32 chain learner at H = 256 (tg_mlp_f32w_forward / _forward_backward / tg_mlp_f32_weight_grad)"
