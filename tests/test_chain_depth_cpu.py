"""The switch of the depth-specialised bf16 backward chain, without a device: the native setter tg_chain_depth_kernels (process-wide,
returns the previous value), its environment default TG_CHAIN_DEPTH_KERNELS, and GemmMLP.depth_kernels on its way to the launch it
governs.  What the kernel computes is test_chain_depth_gpu.py's."""
import inspect
import re

import pytest
import torch


@pytest.fixture()
def native():
    from trajopt_grpo_amd import _native as N
    lib = N.load()
    before = lib.tg_chain_depth_kernels(1)
    yield N, lib
    lib.tg_chain_depth_kernels(before)


def _mlp(N):
    import trajopt_grpo_amd as tg
    from trajopt_grpo_amd import mlp as M
    return M, M.GemmMLP(tg.NeuralNetwork(20, 4, (256,) * 5, "ReLU"), torch.bfloat16)


def test_the_setter_round_trips(native):
    N, lib = native
    assert "tg_chain_depth_kernels" in N.SIGNATURES
    assert lib.tg_chain_depth_kernels(0) == 1          # (the fixture set 1)
    assert lib.tg_chain_depth_kernels(0) == 0
    assert lib.tg_chain_depth_kernels(7) == 0          # any nonzero value is "on" ...
    assert lib.tg_chain_depth_kernels(1) == 1          # ... and reads back as 1
    assert lib.tg_chain_depth_kernels(-1) == 1
    assert lib.tg_chain_depth_kernels(1) == 1


@pytest.mark.parametrize("value,want", [(None, True), ("1", True), ("0", False), ("2", True)])
def test_the_environment_default_is_read(native, monkeypatch, value, want):
    N, _ = native
    if value is None:
        monkeypatch.delenv("TG_CHAIN_DEPTH_KERNELS", raising=False)
    else:
        monkeypatch.setenv("TG_CHAIN_DEPTH_KERNELS", value)
    assert N.chain_depth_kernels_default() is want
    assert _mlp(N)[1].depth_kernels is want


def test_the_attribute_reaches_the_native_switch(native):
    N, lib = native
    M, m = _mlp(N)

    class Recorder:
        calls = []

        def tg_chain_depth_kernels(self, on):
            self.calls.append(on)
            return 1

    for on in (False, True, 0, 1):
        m.depth_kernels = on
        assert m._set_depth_kernels(Recorder()) is bool(on) and Recorder.calls[-1] == int(bool(on))
        assert m._set_depth_kernels(lib) is bool(on)
        assert lib.tg_chain_depth_kernels(int(bool(on))) == int(bool(on))          # (reads the value back, leaves it)


def test_the_switch_is_set_in_front_of_the_launch_it_governs(native):
    """_backward_chain() sets the process-wide switch from its own GemmMLP before it launches (two GemmMLPs with different settings
    may alternate)."""
    N, _ = native
    M, _ = _mlp(N)
    src = inspect.getsource(M.GemmMLP._backward_chain)
    set_at, launch_at = src.find("self._set_depth_kernels(lib)"), re.search(r"lib\.tg_mlp_backward_chain_ex\(", src)
    assert set_at >= 0 and launch_at is not None and set_at < launch_at.start()
