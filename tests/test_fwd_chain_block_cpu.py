"""The switch of the block-structured bf16 forward chain, without a device: the native setter tg_chain_fwd_kernels (process-wide,
returns the previous value, independent of tg_chain_depth_kernels), its environment default TG_CHAIN_FWD_KERNELS, and
GemmMLP.fwd_depth_kernels on its way to the launch it governs.  What the kernel computes is test_fwd_chain_block_gpu.py's."""
import inspect
import re

import pytest
import torch


@pytest.fixture()
def native():
    from trajopt_grpo_amd import _native as N
    lib = N.load()
    before = lib.tg_chain_fwd_kernels(1)
    yield N, lib
    lib.tg_chain_fwd_kernels(before)


def _mlp(N):
    import trajopt_grpo_amd as tg
    from trajopt_grpo_amd import mlp as M
    return M, M.GemmMLP(tg.NeuralNetwork(20, 4, (256,) * 5, "ReLU"), torch.bfloat16)


def test_the_setter_round_trips(native):
    N, lib = native
    assert "tg_chain_fwd_kernels" in N.SIGNATURES
    assert lib.tg_chain_fwd_kernels(0) == 1            # (the fixture set 1)
    assert lib.tg_chain_fwd_kernels(0) == 0
    assert lib.tg_chain_fwd_kernels(7) == 0            # any nonzero value is "on" ...
    assert lib.tg_chain_fwd_kernels(1) == 1            # ... and reads back as 1
    assert lib.tg_chain_fwd_kernels(-1) == 1
    assert lib.tg_chain_fwd_kernels(1) == 1


def test_the_two_chain_switches_are_independent(native):
    """tg_chain_depth_kernels governs the backward chain alone, tg_chain_fwd_kernels the forward chain alone."""
    N, lib = native
    depth_before = lib.tg_chain_depth_kernels(1)
    try:
        lib.tg_chain_fwd_kernels(0)
        assert lib.tg_chain_depth_kernels(1) == 1      # untouched by the forward switch
        lib.tg_chain_depth_kernels(0)
        assert lib.tg_chain_fwd_kernels(0) == 0        # ... and the other way round
        lib.tg_chain_fwd_kernels(1)
        assert lib.tg_chain_depth_kernels(0) == 0
    finally:
        lib.tg_chain_depth_kernels(depth_before)


@pytest.mark.parametrize("value,want", [(None, True), ("1", True), ("0", False), ("2", True)])
def test_the_environment_default_is_read(native, monkeypatch, value, want):
    N, _ = native
    if value is None:
        monkeypatch.delenv("TG_CHAIN_FWD_KERNELS", raising=False)
    else:
        monkeypatch.setenv("TG_CHAIN_FWD_KERNELS", value)
    assert N.chain_fwd_kernels_default() is want
    m = _mlp(N)[1]
    assert m.fwd_depth_kernels is want
    assert m.depth_kernels is N.chain_depth_kernels_default()        # (the backward chain's default has its own variable)


def test_the_attribute_reaches_the_native_switch(native):
    N, lib = native
    M, m = _mlp(N)

    class Recorder:
        calls = []

        def tg_chain_fwd_kernels(self, on):
            self.calls.append(on)
            return 1

    for on in (False, True, 0, 1):
        m.fwd_depth_kernels = on
        assert m._set_fwd_depth_kernels(Recorder()) is bool(on) and Recorder.calls[-1] == int(bool(on))
        assert m._set_fwd_depth_kernels(lib) is bool(on)
        assert lib.tg_chain_fwd_kernels(int(bool(on))) == int(bool(on))            # (reads the value back, leaves it)


def test_the_switch_is_set_in_front_of_the_launch_it_governs(native):
    """forward_loss() sets the process-wide switch from its own GemmMLP before it launches (two GemmMLPs with different settings may
    alternate), and the launch it sets it for is tg_mlp_forward_chain_loss_ex."""
    N, _ = native
    M, _ = _mlp(N)
    src = inspect.getsource(M.GemmMLP.forward_loss)
    set_at = src.find("self._set_fwd_depth_kernels(lib)")
    named_at = src.find('"tg_mlp_forward_chain_loss_ex"')
    launch_at = re.search(r"N\.check\(getattr\(lib, name\)\(", src)
    assert 0 <= named_at < set_at and launch_at is not None and set_at < launch_at.start()
