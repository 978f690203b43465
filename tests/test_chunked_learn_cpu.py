"""The comparison behind tests/test_chunked_learn_gpu.py can fail: chunked_learn.gradients_agree() on a gradient formed as a sum of N
float32 outer products (a weight gradient dZ^T A and its bias gradient) -- it must accept the same rows summed in another order and
reject the sum with one row left out, at the smallest and the largest row count the GPU tests allow.  Runs without a GPU."""
import pytest
import torch

import chunked_learn as CL


def _operands(rows, seed):
    """dZ [rows][48] and A [rows][40] shaped like a learner's: dZ carries the 1 / rows of a mean loss and a ReLU mask, A is a ReLU
    activation; every row has entries on both sides (an all-zero row could be dropped unnoticed, here as in the learner)."""
    g = torch.Generator().manual_seed(seed)
    dz = torch.randn(rows, 48, generator=g) * (torch.rand(rows, 48, generator=g) < 0.6) / rows
    a = torch.randn(rows, 40, generator=g).clamp_min(0.0)
    dz[:, 0] = torch.randn(rows, generator=g) / rows
    a[:, 0] = 1.0 + torch.rand(rows, generator=g)
    return dz, a


def _gradient(dz, a, order):
    """{weight, bias} accumulated row by row in float32 in the given order (rank-one updates: one rounding per row and element)."""
    w, b = torch.zeros(dz.shape[1], a.shape[1]), torch.zeros(dz.shape[1])
    for i in order:
        w += torch.outer(dz[i], a[i])
        b += dz[i]
    return {"weight": w, "bias": b}


@pytest.mark.parametrize("rows", [600, 3000])
def test_the_comparison_accepts_a_reordered_sum_and_rejects_a_missing_row(rows):
    dz, a = _operands(rows, seed=rows)
    forward = _gradient(dz, a, range(rows))
    # the chunked learner's order: per-chunk sums added chunk by chunk; and the rows back to front
    chunked = {"weight": torch.zeros(48, 40), "bias": torch.zeros(48)}
    for lo, hi in CL.chunk_bounds(rows, 257):
        part = _gradient(dz, a, range(lo, hi))
        chunked["weight"] += part["weight"]
        chunked["bias"] += part["bias"]
    backward = _gradient(dz, a, range(rows - 1, -1, -1))
    assert not torch.equal(forward["weight"], backward["weight"]), "the two orders must differ somewhere, or nothing is shown"
    for other in (chunked, backward):
        dists = CL.grad_distances(forward, other, rows)
        print(rows, [(n, f"{d:.3e}", f"{bar:.3e}") for n, d, bar in dists])
        assert CL.gradients_agree(forward, other, rows)
    # one row left out: the last (a tail chunk of one row dropped), the first, and the row with the smallest contribution
    contribution = dz.abs().max(1).values * a.abs().max(1).values
    for missing in (rows - 1, 0, int(contribution.argmin())):
        short = _gradient(dz, a, [i for i in range(rows) if i != missing])
        dists = CL.grad_distances(forward, short, rows)
        print(rows, "without row", missing, [(n, f"{d:.3e}", f"{bar:.3e}") for n, d, bar in dists])
        assert not CL.gradients_agree(forward, short, rows), missing
        assert dists[0][1] > dists[0][2] and dists[1][1] > dists[1][2], "weight and bias gradient must each notice"
    # a row counted twice is a missing row's mirror image
    twice = _gradient(dz, a, list(range(rows)) + [rows - 1])
    assert not CL.gradients_agree(forward, twice, rows)


def test_the_bar_and_the_statistics_distance():
    g = {"w": torch.tensor([1.0, -4.0])}
    assert CL.grad_bar(g["w"], 500) == pytest.approx(2e-5 * 4.0) and CL.grad_bar(g["w"], 4000) == pytest.approx(2e-5 * 4.0 * 2.0)
    assert CL.gradients_agree(g, {"w": torch.tensor([1.0 + 7e-5, -4.0])}, 1000)
    assert not CL.gradients_agree(g, {"w": torch.tensor([1.0 + 9e-5, -4.0])}, 1000)
    assert not CL.gradients_agree(g, {"w": torch.tensor([float("nan"), -4.0])}, 1000)
    # the measured yardstick of the library-GEMM learners raises the bar to 4 x itself, never lowers it
    assert CL.gradients_agree(g, {"w": torch.tensor([1.0 + 3e-4, -4.0])}, 1000, yardstick={"w": 1e-4})
    assert not CL.gradients_agree(g, {"w": torch.tensor([1.0 + 9e-5, -4.0])}, 1000, yardstick={"w": 1e-9})
    a = {"J": [1.0, 2.0], "n_valid": 700.0}
    assert CL.stats_distance(a, {"J": [1.0, 2.0], "n_valid": 700.0}) == (0.0, None)
    ratio, key = CL.stats_distance(a, {"J": [1.0, 2.0 + 4e-5], "n_valid": 700.0})
    assert key == "J" and ratio > 1.0
    assert CL.stats_distance(a, {"J": [1.0 + 5e-6, 2.0], "n_valid": 700.0})[0] < 1.0
    with pytest.raises(AssertionError):
        CL.stats_distance(a, {"J": [1.0, float("nan")], "n_valid": 700.0})
    assert CL.chunk_bounds(600, 257) == [(0, 257), (257, 514), (514, 600)] and CL.chunk_bounds(600, 599)[-1] == (599, 600)
    assert [CL.resolve_arm(x, 600) for x in CL.ARMS] == [None, 600, 601, 599, 257, 96]
    assert CL.expected_calls("ppo_bf16_256x5", "minibatch", 1056, 96) == 3 * 2 * (6 + 6 + 1)
    assert CL.expected_calls("grpo_f32_chain_64x1", None, 700, 257) == 9 and CL.expected_calls("ppo_per_layer_40x2", None, 700, None) == 3
