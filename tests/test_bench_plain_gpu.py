"""GPU: a plain `bench.py --gpus 1 --steps N --warmup W` does what its headline figure needs and nothing else -- set-up,
warm-up, the N timed steps, the line -- so that it can be run several times in a row; what takes runs of its own (CPU
baselines, torch-placed buffers, secondary figures) is measured under `--full` only."""
import json
import os
import subprocess
import sys
import time

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
OUTSIDE_STEPS_LIMIT_S = 30.0  # whole process, start to exit, less (N + W) * ms_per_step


def test_plain_run_is_lean():
    steps, warmup = 20, 5
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    t0 = time.perf_counter()
    p = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)],
                       capture_output=True, text=True, timeout=600, env=env)
    wall = time.perf_counter() - t0
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["full"] is False and line["steps"] == steps and line["warmup"] == warmup and line["n_gpus"] == 1
    assert line["metric"] == "agent-steps/sec (whole node), 64-agent 64x64 grid, batch=8192 envs"
    assert line["unit"] == "agent-steps/s" and line["higher_is_better"] is True and line["dtype"] == "u32"
    assert line["value"] == pytest.approx(8192 * 64 / (line["ms_per_step"] * 1e-3), rel=1e-6)
    assert "secondary" not in line and "cpu_baseline" not in line
    assert line["roofline"]["default_placement_kernel_ms"] is None
    assert line["roofline"]["zone_walks_in_process"]["walks"] <= 1
    outside = wall - (steps + warmup) * line["ms_per_step"] * 1e-3
    print(f"plain bench run: {wall:.1f} s wall, {outside:.1f} s outside its {steps} + {warmup} steps")
    assert outside <= OUTSIDE_STEPS_LIMIT_S, f"{outside:.1f} s outside the steps"
