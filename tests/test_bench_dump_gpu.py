"""GPU: bench.py --dump-outputs -- what the last timed step returned, the same from run to run (seeded inputs), so that
two builds can be compared output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
# 1024 envs of configs[2]: 95 MB of float32 observations, so the dump has to sample them
ARGS = ["--gpus", "1", "--batch", "1024", "--steps", "20", "--warmup", "3", "--no-extras", "--no-cpu-baseline",
        "--no-default-placement"]


def _bench(out_dir):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    p = subprocess.run([sys.executable, BENCH] + ARGS + ["--dump-outputs", str(out_dir)], capture_output=True, text=True,
                       timeout=600, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])


def _replay(steps):
    """The engine bench.py times for ARGS, stepped `steps` times outside bench.py with the same seeds (reset seed 0, a
    pool of 32 action tensors from a device generator seeded 1 + rank) -> the outputs of the last two steps, on the host."""
    import torch
    import bench
    from pogema_amd import VecPogema
    args = bench.make_parser().parse_args(ARGS)
    _, size, agents, r = bench.WORKLOADS[args.workload]
    env = VecPogema(bench.workload_grid_config(args, size, agents, r), batch=args.batch, device="cuda:0", auto_reset=True,
                    reuse_buffers=False, placement_probe=False)
    env.reset(seed=0)
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(1)
    pool = [torch.randint(0, 5, (args.batch, agents), generator=gen, device="cuda:0").to(torch.int8) for _ in range(32)]
    outs = []
    for t in range(steps):
        obs, rewards, terminated, truncated, infos = env.step(pool[t % len(pool)])
        if t >= steps - 2:
            got = {"obs": obs, "rewards": rewards, "terminated": terminated, "truncated": truncated,
                   "is_active": infos["is_active"], "episode_done": infos["episode_done"], "metrics": infos["metrics"]}
            outs.append({k: v.to(torch.float32).cpu().numpy() for k, v in got.items()})
    env.close()
    return outs


def test_dumped_outputs_are_reproducible(tmp_path):
    lines = [_bench(tmp_path / name) for name in ("a", "b")]
    files = lines[0]["dump_outputs"]["files"]
    assert lines[1]["dump_outputs"]["files"] == files and lines[0]["steps"] == 20 and lines[0]["windows"]["n"] == 1
    assert sorted(files) == ["episode_done", "is_active", "metrics", "obs", "obs_env_index", "rewards", "terminated", "truncated"]
    assert files["rewards"] == [1024, 64] and files["obs"][1:] == [64, 3, 11, 11] and 0 < files["obs"][0] < 1024
    sizes = [os.path.getsize(tmp_path / "a" / f"{n}.npy") for n in files]
    assert sum(sizes) <= 64_000_000
    for name in files:
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), name
    obs = np.load(tmp_path / "a" / "obs.npy")
    assert np.all((obs == 0) | (obs == 1)) and obs.any(), "observation planes are 0/1 maps"
    # ... and they are the outputs of the LAST timed step: warm-up 3 + 20 timed steps of the same engine outside bench.py
    prev, last = _replay(3 + 20)
    rows = np.load(tmp_path / "a" / "obs_env_index.npy").astype(np.int64)
    for name in files:
        if name == "obs_env_index":
            continue
        got = np.load(tmp_path / "a" / f"{name}.npy")
        assert np.array_equal(got, last[name][rows] if name == "obs" else last[name]), name
    assert not np.array_equal(prev["obs"][rows], last["obs"][rows]), "step 22 and step 23 must be told apart"
