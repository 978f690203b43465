"""bench.py's two kinds of run: a plain run is the headline alone (set-up, warm-up, timed steps, the JSON line); --full adds
the measurements that take work of their own.  Small shards (--envs) so that both runs take seconds."""
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*extra):
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--envs", "1024", *extra]
    p = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-4000:]
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_other_configs_on_needs_full():
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--other-configs", "on"], cwd=REPO, capture_output=True,
                       text=True, timeout=120)
    assert p.returncode == 2 and "--other-configs on needs --full" in p.stderr and p.stdout == ""


@pytest.mark.gpu
def test_plain_run_is_the_headline_alone():
    out = _bench()
    assert out["unit"] == "env-steps/s" and out["higher_is_better"] is True and out["value"] > 0 and out["ms_per_step"] > 0
    assert out["steps"] == 2 and out["warmup"] == 1 and out["full"] is False and out["dtype"].startswith("bf16")
    assert out["rollout_path"].startswith("fused") and out["rollout_kernel"]["all_alive"] is None
    assert out["kernels"] and out["roofline"]["launches"] > 0           # (from the launch events of the timed steps)
    for key in ("cpu_baseline", "fixed_work_ms_per_step", "sustained_matrix_rate"):
        assert key not in out, key
    assert out["dynamics_kernel"] is None and "other_configs" not in out["roofline"]
    assert all("frac_of_sustained" not in k for k in out["kernels"].values())


@pytest.mark.gpu
def test_full_run_keeps_the_extra_measurements():
    out = _bench("--full", "--no-cpu-baseline", "--other-configs", "on")
    assert out["full"] is True and out["value"] > 0 and "cpu_baseline" not in out
    assert out["fixed_work_ms_per_step"] > 0 and out["fixed_work_env_steps_per_s"] > 0
    dyn = out["dynamics_kernel"]
    assert dyn["us_per_launch"] > 0 and dyn["at_4194304_envs"]["us_per_launch"] > 0 and dyn["one_launch_form"]["ms_per_launch"] > 0
    assert out["rollout_kernel"]["all_alive"]["env_steps"] > 0
    assert out["sustained_matrix_rate"]["TFLOPs"] > 0
    assert out["kernels"] and all(k["frac_of_sustained"] > 0 for k in out["kernels"].values())
    others = out["roofline"]["other_configs"]
    assert set(others) == {"c2", "c4", "c5"}
    for name, o in others.items():
        assert "error" not in o and o["value"] > 0 and o["ms_per_step"] > 0, name
