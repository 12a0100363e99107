#!/usr/bin/env python
"""Per-call device time (HIP events) of shield_actions() next to pibt_actions() on the same state, in one process:
shield_actions in its default form (no distance field) and with tie_break="distance", float32 and bfloat16 scores,
alternating with the planner on a warm distance-field cache.

    python tools/time_shield.py --batch 1024 --size 16 --agents 8  [--reps 200] [--rounds 5]
    python tools/time_shield.py --batch 8192 --size 64 --agents 64
Prints one JSON line.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pogema_amd import GridConfig, VecPogema  # noqa: E402


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
    gc = GridConfig(size=args.size, num_agents=args.agents, density=args.density, obs_radius=5, seed=1,
                    collision_system="soft", on_target="finish", max_episode_steps=256)
    env = VecPogema(gc, batch=args.batch)
    env.reset(seed=1)
    B, A = args.batch, args.agents
    prio = torch.randint(-3, 4, (B, A), dtype=torch.int32, device=env.device)
    scores = torch.randn((B, A, 5), device=env.device)
    narrow = scores.to(torch.bfloat16)
    out_p = (torch.empty((B, A), dtype=torch.int64, device=env.device), torch.empty((B, A, 2), dtype=torch.int32, device=env.device))
    out_s = out_p + (torch.empty((B, A), dtype=torch.uint8, device=env.device),)
    calls = {
        "pibt_actions_us": lambda: env.pibt_actions(priority=prio, out=out_p),
        "shield_actions_us": lambda: env.shield_actions(scores, priority=prio, out=out_s),
        "shield_actions_bf16_us": lambda: env.shield_actions(narrow, priority=prio, out=out_s),
        "shield_actions_distance_us": lambda: env.shield_actions(scores, priority=prio, tie_break="distance", out=out_s),
    }
    for _ in range(4):                      # a few steps, so that the state is not the reset's; then warm every call
        env.step(env.pibt_actions(priority=prio)[0])
    for fn in calls.values():
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    builds = env.cost_to_go_builds
    samples = {k: [] for k in calls}
    for _ in range(args.rounds):            # alternate, so that drift hits every call alike
        for k, fn in calls.items():
            samples[k].append(timed(fn, args.reps))
    assert env.cost_to_go_builds == builds, "a timed call built distance fields"
    res = {"batch": B, "size": args.size, "agents": A, "reps": args.reps, "rounds": args.rounds,
           "overridden_mean": round(float(out_s[2].float().mean()), 4)}
    for k, v in samples.items():
        res[k] = round(sorted(v)[len(v) // 2], 2)
        res[k.replace("_us", "_minmax_us")] = [round(min(v), 2), round(max(v), 2)]
    print(json.dumps(res))
    env.close()


if __name__ == "__main__":
    main()
