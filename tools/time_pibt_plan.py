#!/usr/bin/env python3
"""Per-call device time (HIP events) of pibt_plan(K) for K = 1, 8, 32 on a warm distance-field cache, next to
pibt_actions() on the same state in the same process, plus a 32-step episode segment driven two ways from the same
reset: PibtPolicy.act() + step() + update() per step against one PibtPolicy.plan(32) + one rollout().  One JSON line
per run; one process per shape.

    python tools/time_pibt_plan.py --batch 1024 --size 16 --agents 8  [--reps 200] [--once]
    python tools/time_pibt_plan.py --batch 8192 --size 64 --agents 64
`--once`: a few calls of each kind and nothing else (for a kernel trace).
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from pogema_amd import GridConfig, PibtPolicy, VecPogema  # noqa: E402

HORIZONS = (1, 8, 32)
EPISODE = 32


def timed(fn, reps):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    rounds = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        rounds.append(a.elapsed_time(b) * 1000.0 / reps)
    rounds.sort()
    return {"median_us": round(rounds[2], 2), "min_us": round(rounds[0], 2), "max_us": round(rounds[-1], 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, required=True)
    ap.add_argument("--size", type=int, required=True)
    ap.add_argument("--agents", type=int, required=True)
    ap.add_argument("--radius", type=int, default=5)
    ap.add_argument("--density", type=float, default=0.3)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    gc = GridConfig(size=args.size, num_agents=args.agents, obs_radius=args.radius, density=args.density, seed=0,
                    collision_system="soft", on_target="finish", max_episode_steps=4 * EPISODE)
    env = VecPogema(gc, batch=args.batch, auto_reset=False)
    env.reset(seed=0)
    B, A, dev = env.batch, env.num_agents, env.device
    prio = torch.zeros((B, A), dtype=torch.int32, device=dev)
    out_p = (torch.empty((B, A), dtype=torch.int64, device=dev), torch.empty((B, A, 2), dtype=torch.int32, device=dev))
    outs = {K: (torch.empty((K, B, A), dtype=torch.int64, device=dev), torch.empty((K, B, A, 2), dtype=torch.int32, device=dev),
                torch.empty((B, A), dtype=torch.int32, device=dev), torch.empty((B, A), dtype=torch.int32, device=dev))
            for K in HORIZONS}
    env.pibt_actions(priority=prio, out=out_p)      # allocates and fills the cache
    torch.cuda.synchronize()
    if args.once:
        for _ in range(3):
            env.pibt_actions(priority=prio, out=out_p)
            for K in HORIZONS:
                env.pibt_plan(K, priority=prio, out=outs[K])
        torch.cuda.synchronize()
        env.close()
        return
    res = {"shape": {"batch": B, "size": args.size, "agents": A, "obs_radius": args.radius, "density": args.density},
           "builds_before": env.cost_to_go_builds}
    res["pibt_actions_us"] = timed(lambda: env.pibt_actions(priority=prio, out=out_p), args.reps)
    for K in HORIZONS:
        t = timed(lambda: env.pibt_plan(K, priority=prio, out=outs[K]), max(args.reps // K, 10))
        t["per_step_us"] = round(t["median_us"] / K, 2)
        res[f"pibt_plan_{K}_us"] = t
    res["pibt_actions_again_us"] = timed(lambda: env.pibt_actions(priority=prio, out=out_p), args.reps)
    res["builds_after"] = env.cost_to_go_builds         # equal: every timed planner call ran on a warm cache

    # the first EPISODE steps of an episode, both ways, from the same reset; the reset is outside the timed span
    policy = PibtPolicy(env)

    def per_step():
        for _ in range(EPISODE):
            _, rewards, _, _, infos = env.step(policy.act()[0], compute_obs=False)
            policy.update(rewards, infos["episode_done"])

    def planned():
        actions, _, _ = policy.plan(EPISODE)
        env.rollout(actions, obs_slots=0)

    for name, fn in (("episode_per_step_us", per_step), ("episode_planned_us", planned)):
        rounds = []
        for _ in range(7):
            env.reset(seed=1)
            policy.reset()
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            rounds.append(a.elapsed_time(b) * 1000.0)
        rounds = sorted(rounds[2:])                      # the first two warm the paths up
        res[name] = {"median_us": round(rounds[2], 1), "min_us": round(rounds[0], 1), "max_us": round(rounds[-1], 1),
                     "per_step_us": round(rounds[2] / EPISODE, 2)}
        res[name.replace("_us", "_final_xy_sum")] = int(env.get_state()["agents_xy"].sum())
    env.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
