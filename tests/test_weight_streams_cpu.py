"""The five derived weight layouts (mlp.WeightStream and its subclasses) against bytes recorded before they shared a base class.

tests/golden/weight_streams.json holds sha256 digests of every destination buffer and of every tg_gather_streams code tensor, and
the values of the five `*_supported` predicates over a grid of nets, all recorded from the per-class implementations this base
replaced (the codes through optim.StreamRefresher._codes for the classes that had no segments() of their own).  The nets'
parameters are a closed-form integer pattern that is exact in fp32: nothing here depends on an RNG.  No GPU is needed: the streams
are built on the CPU, which runs the same index arithmetic."""
import hashlib
import json
import os

import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

import trajopt_grpo_amd as tg
from trajopt_grpo_amd import mlp as M
from conftest import GOLDEN

with open(os.path.join(GOLDEN, "weight_streams.json")) as _f:
    RECORDED = json.load(_f)

CHAIN_SHAPES = [(5, 1, (64,)), (20, 4, (128,) * 3), (9, 2, (64,) * 4)]
BF16_SHAPES = [(20, 4, (256,) * 5), (5, 1, (128,) * 3)]
# (class tag of the fixture, constructor, shapes, the tensors of the "tensors" digest, those of the "views" digest or None,
#  is_bf16 of each output, launches of one refresh())
CASES = [
    ("F32ChainStream", lambda net, H: M.F32ChainStream(net, H), CHAIN_SHAPES, ("stream",), None, [0], 2),
    ("RegisterStreamF32.16", lambda net, H: M.RegisterStreamF32(net, H, 16), CHAIN_SHAPES, ("stream", "table"), None, [0, 0], 3),
    ("RegisterStreamF32.32", lambda net, H: M.RegisterStreamF32(net, H, 32), CHAIN_SHAPES, ("stream", "table"), None, [0, 0], 3),
    ("F32ResStream", lambda net, H: M.F32ResStream(net), [(5, 1, (128,)), (20, 4, (128, 128))], ("stream",), ("w0", "table"), [0], 2),
    ("F32WideStream", lambda net, H: M.F32WideStream(net), [(20, 4, (256,) * 5), (5, 1, (256,))], ("stream",), ("table",), [0], 2),
    ("FragmentStream.rollout", lambda net, H: M.FragmentStream(net, H), BF16_SHAPES, ("stream", "bias"), None, [1, 0], 4),
    ("FragmentStream.chain", lambda net, H: M.FragmentStream(net, H, layout="chain"), BF16_SHAPES, ("stream", "bias"), None, [1, 0], 4),
    ("FragmentStream.transposed", lambda net, H: M.FragmentStream(net, H, layout="chain", transposed=True), BF16_SHAPES,
     ("stream", "bias"), None, [1], 3),
]


def patterned_net(S, A, hidden):
    """The net whose parameter `ti` (weight, bias per layer) holds v[i] = (((i * 2654435761 + ti * 40503) % 65536) - 32768) / 256,
    and the optimizer's tensor table for it: id(p) -> (group 0, ti)."""
    net = tg.NeuralNetwork(S, A, list(hidden), "ReLU")
    ids = {}
    with torch.no_grad():
        for ti, p in enumerate(p for l in net.network if isinstance(l, torch.nn.Linear) for p in (l.weight, l.bias)):
            i = torch.arange(p.numel(), dtype=torch.int64)
            p.copy_(((((i * 2654435761 + ti * 40503) % 65536) - 32768).double() / 256).float().view_as(p))
            ids[id(p)] = (0, ti)
    return net, ids


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


class _Launches(TorchDispatchMode):
    """Counts what would be a kernel launch on the device: every op that writes a tensor (views and slices write nothing)."""
    WRITES = ("cat", "index_select", "copy_", "_to_copy", "index", "zeros", "fill_", "zero_")

    def __init__(self):
        super().__init__()
        self.ops = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        if func.overloadpacket.__name__ in self.WRITES:
            self.ops.append(func.overloadpacket.__name__)
        return func(*args, **(kwargs or {}))


@pytest.mark.parametrize("tag,make,shapes,fields,views,flags,launches", CASES, ids=[c[0] for c in CASES])
def test_streams_hold_the_recorded_bytes_and_gather_codes(tag, make, shapes, fields, views, flags, launches):
    for S, A, hidden in shapes:
        key = f"{tag}/{S}-{A}-{'x'.join(map(str, hidden))}"
        net, ids = patterned_net(S, A, hidden)
        fs = make(net, hidden[0])
        assert sha(*[getattr(fs, f) for f in fields]) == RECORDED["digests"][key + "/tensors"], key
        if views is not None:
            assert sha(*[getattr(fs, f) for f in views]) == RECORDED["digests"][key + "/views"], key
            # what was a view stays a view: the tail of the one buffer, in this order
            at = fs.stream.numel() - sum(getattr(fs, f).numel() for f in views)
            for f in views:
                v = getattr(fs, f)
                assert v.data_ptr() == fs.stream.data_ptr() + 4 * at and v.dtype == torch.float32, (key, f)
                at += v.numel()
        # the outputs partition the index, keep their dtype and are allocations of their own, named by the attributes
        assert [int(b) for _, b in fs.outputs] == flags and sum(d.numel() for d, _ in fs.outputs) == fs._idx.numel()
        assert [d.dtype for d, _ in fs.outputs] == [torch.bfloat16 if b else torch.float32 for b in flags]
        assert [d.data_ptr() for d, _ in fs.outputs] == [getattr(fs, f).data_ptr() for f in fields[:len(flags)]]
        assert len({d.untyped_storage().data_ptr() for d, _ in fs.outputs}) == len(flags)
        segs = fs.segments(ids)
        assert [(d.data_ptr(), int(b)) for d, _, b in segs] == [(d.data_ptr(), int(b)) for d, b in fs.outputs]
        assert all(c.dtype == torch.int32 and c.is_contiguous() and c.numel() == d.numel() for d, c, _ in segs)
        assert sha(*[c for _, c, _ in segs]) == RECORDED["digests"][key + "/codes"], key
        # a refresh rebuilds the same bytes from scratch, in no more launches than the class took before
        for d, _ in fs.outputs:
            d.zero_()
        with _Launches() as count:
            fs.refresh()
        assert sha(*[getattr(fs, f) for f in fields]) == RECORDED["digests"][key + "/tensors"], key
        assert len(count.ops) == launches, (key, count.ops)


def test_freshness_and_who_rides_on_the_optimizer_step():
    """Every stream has the key bookkeeping; only the fp32 fused rollout's stream joins the learner's gather and is trusted as fresh
    (the bf16 rollout stream keeps refreshing itself at every rollout entry)."""
    from trajopt_grpo_amd import _native as N
    net, ids = patterned_net(5, 1, (128, 128, 128))
    streams = [M.F32ChainStream(net, 128), M.RegisterStreamF32(net, 128, 16), M.FragmentStream(net, 128),
               M.FragmentStream(net, 128, layout="chain", transposed=True)]
    streams += [M.F32ResStream(patterned_net(5, 1, (128,))[0]), M.F32WideStream(patterned_net(5, 1, (256,))[0])]
    assert [s.rides_on_optimizer_step for s in streams] == [False, True, False, False, False, False]
    for s in streams[:4]:
        s.refresh()                                             # (the four share one net: the writes below reach every one of them)
        assert s.is_fresh() or N.ALWAYS_REBUILD
        with torch.no_grad():
            s.lin[0].bias.add_(1.0)
        assert not s.is_fresh()
        s.mark_fresh()
        assert s.is_fresh() or N.ALWAYS_REBUILD
        N.RAW_PARAM_WRITES[0] += 1
        assert not s.is_fresh()
    # a master the optimizer does not hold, or holds outside its first group: the errors StreamRefresher remembers a layout by
    for s in streams[:4]:
        with pytest.raises(KeyError):
            s.segments({})
        with pytest.raises(AssertionError):
            s.segments({k: (1, ti) for k, (_, ti) in ids.items()})


def test_shape_predicates_return_what_they_returned_per_class():
    """fused_rollout_supported, fused_rollout_f32_supported (ReLU only / ReLU and Tanh), f32_chain_supported, f32_res_supported and
    f32_wide_supported over ReLU, Tanh and mixed nets, H in {32, 64, 128, 256, 100}, 0..6 hidden layers, S in {5, 32, 40},
    A in {1, 4, 5, 8}: the fixture lists every net with a non-zero answer, all others answer 0."""
    want, seen = RECORDED["predicates"]["nonzero"], 0
    assert RECORDED["predicates"]["order"] == ["fused_rollout_supported", "fused_rollout_f32_supported", "fused_rollout_f32_supported+Tanh",
                                               "f32_chain_supported", "f32_res_supported", "f32_wide_supported"]
    for kind in ("ReLU", "Tanh", "mixed"):
        for H in (32, 64, 128, 256, 100):
            for nh in range(7):
                acts = [("ReLU", "Tanh")[i % 2] for i in range(nh)] if kind == "mixed" else [kind] * nh
                for S in (5, 32, 40):
                    for A in (1, 4, 5, 8):
                        with torch.device("meta"):                                  # (only the module list is read)
                            net = tg.NeuralNetwork(S, A, [H] * nh, acts)
                        got = [M.fused_rollout_supported(net, S, A), M.fused_rollout_f32_supported(net, S, A),
                               M.fused_rollout_f32_supported(net, S, A, activations=("ReLU", "Tanh")), M.f32_chain_supported(net),
                               M.f32_res_supported(net), M.f32_wide_supported(net)]
                        key = f"{kind}/{H}/{nh}/{S}/{A}"
                        assert [int(v) for v in got] == want.get(key, [0] * 6), key
                        assert all(isinstance(v, int) for v in got), key
                        seen += key in want
    assert seen == len(want) == 108
