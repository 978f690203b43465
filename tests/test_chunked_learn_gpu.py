"""learn() in several chunks (`chunk_rows`) against the one-chunk learn() of the same learner, on every learner family and optional
feature (tests/chunked_learn.py: the cases, the arms, the comparison).  The one-chunk arm is what the rest of the suite ties to fp64
and to the reference's goldens; against it bf16 rounding cancels and only fp32 summation order is left.

Every arm: a deep copy of one policy, plain Adam at lr = 0 (the fused step, and the rider of the one-chunk fp32 GRPO update, with weights
that never move), updates_per_iter = 3, chunk_rows in {None, N, N + 1, N - 1, 257, 96} for N valid rows (600 <= N <= 3000).  Asserted
against the None arm:
  * N and N + 1 make the same launches: everything is bit-equal, last_stats included;
  * the per-row outputs (folded / no-grad old log-probabilities, reference log-probabilities, V on the [T][n] grid, gathered advantages
    and returns, norm8) are bit-equal on the hand-written learners;
  * n_valid and slot 3 of every loss-sum row equal N;
  * every entry of last_stats within rtol 1e-5, atol 1e-7;
  * every gradient tensor (log_std's too) within 2e-5 (max |g| + 1e-9) max(1, sqrt(N / 1000)); the learners on library GEMMs (per-layer,
    autograd): within 4 x the distance of torch's own float32 autograd over all rows from its sum over the same chunks, floored at that bar;
  * within an arm the three updates give equal loss-sum rows and a one-update learn() leaves the same .grad, bit for bit;
  * a learner that first ran a smaller buffer gives the bits of a fresh one;
  * a control arm whose last chunk is launched one row short is rejected by the gradient comparison alone.

Measured on an MI355X, worst arm of each run (N; the worst gradient tensor's distance / its bar, and the arm):
  ppo_bf16_256x5             1056  critic head bias 1.2e-7 / 5.3e-6 (96)    grpo_bf16_128x3            2048  7.2e-7 / 8.5e-5 (96)
  ppo_f32_wide_256x2         1056  1.7e-8 / 5.2e-7 (257)                    grpo_f32_resident_128x2    2048  4.8e-7 / 4.1e-5 (96)
  grpo_f32_chain_64x1        2048  1.6e-6 / 5.1e-5 (96)                     grpo_f32_chain_128x4       2048  2.2e-7 / 7.5e-6 (96)
  grpo_f32_chain_tanh_128x3  2048  5.4e-7 / 2.0e-5 (96)
  ref: bf16 1.8e-7 / 1.8e-5, fp32 7.6e-6 / 2.6e-4    learn_std: bf16 1.2e-7 / 5.3e-6, fp32 1.7e-8 / 5.2e-7    privileged 1.5e-8 / 7.1e-7
  clip: bf16 3.7e-9 / 4.6e-7 (grad_norm at 1e-2 of the statistics' bound), fp32 1.1e-8 / 3.3e-7
  minibatch (every one of the 9 steps): bf16 5.2e-8 / 2.3e-6, fp32 3.7e-9 / 2.2e-7    stale_old: bf16 1.8e-7 / 2.4e-5, fp32 1.6e-7 / 7.1e-6
  loss statistics: equal to the last bit on every hand-written learner (the f64 sums of bit-equal float32 rows are exact)
  ppo_per_layer_40x2         2048  7.5e-9 / 1.2e-7; torch's own all-rows-against-chunks distance 6.0e-8 at the most;
                                   statistics at 8e-4 of their bound; V differs from the one-chunk arm in chunks of 257 and 96 (library GEMMs)
  ppo_autograd_sigmoid_32x2  2048  3.6e-9 / 3.2e-8; torch's distance 6.7e-8; statistics at 7e-5 of their bound (V differs in chunks of 2047)
  one row short (chunks of 257): every tensor off by 3e+2 .. 8e+3 bars (bf16 PPO), 30 .. 120 bars (fp32 GRPO)
  the PPO critics' output bias starts at 0.25 (chunked_learn.setup says why): with a fresh critic that scalar is 2.2e-3, the remainder
  of terms that cancel, and chunks of 96 sat 1.5e-7 from it (one rounding of the partial sums) against a bar of 4.4e-8."""
import pytest
import torch

import chunked_learn as CL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tg():
    import trajopt_grpo_amd as tg
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return tg


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


_RECORDS = {}


def _arm(tg, dev, case, feature, arm, updates=3):
    """The record of one arm, computed once per module and left unchanged."""
    rows = CL.setup(tg, dev, case, feature)[2]
    key = (case, feature, arm, updates)
    if key not in _RECORDS:
        _RECORDS[key] = CL.run_arm(tg, dev, case, feature, CL.resolve_arm(arm, rows), updates)
    return _RECORDS[key]


def _bit_equal(a, b, what):
    assert sorted(a) == sorted(b), (what, sorted(a), sorted(b))
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k, float((a[k].double() - b[k].double()).abs().max()))


def _ids(run):
    return run[0] if run[1] is None else f"{run[0]}-{run[1]}"


@pytest.mark.parametrize("case,feature", CL.RUNS, ids=[_ids(r) for r in CL.RUNS])
def test_a_chunked_learn_reproduces_the_one_chunk_learn(tg, dev, case, feature):
    base, buf, N, _ = CL.setup(tg, dev, case, feature)
    learner, family = CL.CASES[case][0], CL.CASES[case][-1]
    assert 600 <= N <= 3000, N
    arms = (None, 96) if feature == "minibatch" else CL.ARMS
    one = _arm(tg, dev, case, feature, None)
    print(f"{case} {feature}: N = {N}, entries {one['calls']}")
    worst_stats, worst_grad = (0.0, None, None), (None, -1.0, 1.0, None)
    for arm in arms:
        rec = _arm(tg, dev, case, feature, arm)
        chunk = rec["chunk"]
        CL.check_family(rec, case, feature)
        assert rec["weights_kept"], "lr = 0: the weights must keep their bits"
        # counts
        assert rec["stats"]["n_valid"] == N
        sums = rec["sums"].reshape(-1, rec["sums"].shape[-2] if rec["sums"].dim() == 3 else 1, 4)
        assert bool((sums[:, 0, 3] == N).all()) or feature == "minibatch", sums[:, :, 3]
        if learner == "PPO" and family in CL.HAND_WRITTEN and feature != "minibatch":
            assert bool((sums[:, 1, 3] == N).all()), sums[:, :, 3]
        if feature == "minibatch":
            per_step = [hi - lo for lo, hi in CL.chunk_bounds(N, CL.MINIBATCH)] * 3
            assert sums[:, :, 3].tolist() == [[float(r)] * 2 for r in per_step], sums[:, :, 3]
            by_update = sums.reshape(3, -1, 2, 4)
            assert bool((by_update == by_update[0:1]).all()), sums
        else:
            # the weights do not move: every update of a learn() gives the same loss sums, bit for bit
            assert bool((sums == sums[0:1]).all()), sums
        # per-row outputs
        hand = family in CL.HAND_WRITTEN
        same_launches = arm in (None, "N", "N+1")
        if hand or same_launches:
            _bit_equal(one["per_row"], rec["per_row"], (case, feature, arm))
            assert len(one["logps"]) == len(rec["logps"]) and all(torch.equal(a, b) for a, b in zip(one["logps"], rec["logps"]))
        else:
            print(f"  chunk {chunk}: per-row outputs bit-equal:",
                  {k: bool(torch.equal(v, rec['per_row'][k])) for k, v in one["per_row"].items()})
        assert "V" in rec["per_row"] or learner == "GRPO"
        assert "old_logp" in rec["per_row"] or not hand or feature in ("minibatch", "stale_old")
        assert ("ref_logp" in rec["per_row"]) == (feature == "ref")
        # loss statistics, gradients
        ratio, key = CL.stats_distance(one["stats"], rec["stats"])
        yard = None
        if not hand and not same_launches:
            yard = CL.torch_chunk_yardstick(base, buf, one, chunk)
        dists = CL.grad_distances(one["grads"], rec["grads"], N, yard)
        if "grad_norm" in one["stats"]:
            gn = {"grad_norm": torch.tensor(one["stats"]["grad_norm"])}
            dists += CL.grad_distances(gn, {"grad_norm": torch.tensor(rec["stats"]["grad_norm"])}, N)
        if feature == "minibatch":                                 # 3 x (512, 512, N - 1024 rows): every step's gradients
            assert len(rec["step_grads"]) == len(one["step_grads"]) == 3 * len(CL.chunk_bounds(N, CL.MINIBATCH))
            for k, (a, b) in enumerate(zip(one["step_grads"], rec["step_grads"])):
                dists += [(f"step {k} {n}", d_, bar_) for n, d_, bar_ in CL.grad_distances(a, b, min(CL.MINIBATCH, N))]
        name, d, bar = CL.worst(dists)
        print(f"  chunk {chunk} ({rec['n_chunks']} chunks): stats distance / bound {ratio:.3e} ({key}); worst gradient {name} "
              f"{d:.3e} bar {bar:.3e}" + (f"; torch yardstick {max(yard.values()):.3e}" if yard else ""))
        if same_launches:
            assert rec["stats"] == one["stats"], (arm, rec["stats"], one["stats"])
            _bit_equal(one["grads"], rec["grads"], (case, feature, arm))
            assert torch.equal(one["sums"], rec["sums"])
        assert ratio <= 1.0, (case, feature, arm, key, one["stats"][key], rec["stats"][key])
        assert all(d_ <= bar_ for _, d_, bar_ in dists), (case, feature, arm, [t for t in dists if t[1] > t[2]])
        if ratio > worst_stats[0]:
            worst_stats = (ratio, key, chunk)
        if d / bar > worst_grad[1] / worst_grad[2]:
            worst_grad = (name, d, bar, chunk)
        # a one-update learn() from the same state leaves the same gradients as the third update of three
        # (minibatch mode: the fixed permutation gives every update the same minibatches)
        if arm not in ("N", "N+1"):
            single = _arm(tg, dev, case, feature, arm, updates=1)
            CL.check_family(single, case, feature, updates=1)
            _bit_equal(rec["grads"], single["grads"], (case, feature, arm, "one update"))
            assert torch.equal(single["sums"], rec["sums"][:single["sums"].shape[0]])
    print(f"  WORST {case} {feature}: stats {worst_stats[0]:.2e} of the bound ({worst_stats[1]}, chunk {worst_stats[2]}); gradient "
          f"{worst_grad[0]} {worst_grad[1]:.2e} / bar {worst_grad[2]:.2e} (chunk {worst_grad[3]})")


@pytest.mark.parametrize("case", ["ppo_bf16_256x5", "grpo_f32_chain_128x4"])
def test_the_gradient_comparison_rejects_a_last_chunk_one_row_short(tg, dev, case):
    """The control arm: chunks of 257 with the last chunk of every update launched on rows - 1 (an ordinary launch).  The count notices;
    the gradient comparison alone must, too -- else the inputs are too large for a row to show."""
    N = CL.setup(tg, dev, case)[2]
    one, honest = _arm(tg, dev, case, None, None), _arm(tg, dev, case, None, 257)
    short = CL.run_arm(tg, dev, case, None, 257, control=True)
    CL.check_family(short, case, None)
    assert bool((short["sums"].reshape(-1, 4)[:, 3] == N - 1).all())
    dists = CL.grad_distances(one["grads"], short["grads"], N)
    print(case, "one row short:", [(n, f"{d:.3e}", f"{b:.3e}") for n, d, b in dists])
    assert CL.gradients_agree(one["grads"], honest["grads"], N)
    assert not CL.gradients_agree(one["grads"], short["grads"], N)
    # (every net notices, not one stray tensor)
    for net in ("actor", "critic") if case.startswith("ppo") else ("actor",):
        assert any(d > bar for n, d, bar in dists if n.startswith(net)), net


@pytest.mark.parametrize("case", ["ppo_bf16_256x5", "grpo_f32_chain_128x4"])
def test_the_workspaces_of_a_smaller_buffer_leave_no_trace(tg, dev, case):
    """learn(small buffer) then learn(the case's buffer), chunks of 257, against a fresh learner given only the latter: the row
    workspaces are sized once and re-viewed per chunk, and nothing of the first buffer may reach the second's results."""
    fresh = _arm(tg, dev, case, None, 257)
    used = CL.run_arm(tg, dev, case, None, 257, history=True)
    CL.check_family(used, case, None)
    assert used["stats"] == fresh["stats"], (used["stats"], fresh["stats"])
    _bit_equal(fresh["grads"], used["grads"], (case, "history"))
    _bit_equal(fresh["per_row"], used["per_row"], (case, "history"))
    assert torch.equal(fresh["sums"], used["sums"]) and used["weights_kept"]
