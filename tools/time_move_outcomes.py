#!/usr/bin/env python
"""Per-call device time (HIP events) of move_outcomes() next to step(actions, compute_obs=False) on the same engine, in
one process, under each collision system: the query does the step's resolve work without its state write-back.

    python tools/time_move_outcomes.py --batch 1024 --size 16 --agents 8  [--reps 200] [--rounds 5]
    python tools/time_move_outcomes.py --batch 8192 --size 64 --agents 64
Prints one JSON line per collision system.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pogema_amd import NUM_OUTCOMES, GridConfig, VecPogema  # noqa: E402


def timed(fn, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1000.0 / reps


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--size", type=int, default=16)
    ap.add_argument("--agents", type=int, default=8)
    ap.add_argument("--density", type=float, default=0.3)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    B, A = args.batch, args.agents
    for collision in ("priority", "block_both", "soft"):
        gc = GridConfig(size=args.size, num_agents=A, density=args.density, obs_radius=5, seed=1,
                        collision_system=collision, on_target="restart", max_episode_steps=1 << 20)
        env = VecPogema(gc, batch=B)
        env.reset(seed=1)
        actions = torch.randint(0, 5, (B, A), dtype=torch.int64, device=env.device)
        out = (torch.empty((B, A, 2), dtype=torch.int32, device=env.device), torch.empty((B, A), dtype=torch.uint8, device=env.device),
               torch.empty((B, A), dtype=torch.int32, device=env.device), torch.empty((B, NUM_OUTCOMES), dtype=torch.int32, device=env.device))
        calls = {
            "move_outcomes_us": lambda: env.move_outcomes(actions, out=out),
            "step_no_obs_us": lambda: env.step(actions, compute_obs=False),
        }
        for fn in calls.values():
            for _ in range(20):
                fn()
        torch.cuda.synchronize()
        samples = {k: [] for k in calls}
        for _ in range(args.rounds):            # alternate, so that drift hits both calls alike
            for k, fn in calls.items():
                samples[k].append(timed(fn, args.reps))
        counts = out[3].sum(dim=0).tolist()
        res = {"collision_system": collision, "batch": B, "size": args.size, "agents": A, "reps": args.reps,
               "rounds": args.rounds, "outcome_counts": counts}
        for k, v in samples.items():
            res[k] = round(sorted(v)[len(v) // 2], 2)
            res[k.replace("_us", "_minmax_us")] = [round(min(v), 2), round(max(v), 2)]
        print(json.dumps(res))
        env.close()


if __name__ == "__main__":
    main()
