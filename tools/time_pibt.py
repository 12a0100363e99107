#!/usr/bin/env python3
"""Per-call device time (HIP events) of pibt_actions() on a warm distance-field cache, next to expert_actions(),
cost_to_go() and one step() on the same state in the same process, plus the ISR of planner-driven against
expert-driven episodes (soft / finish) on the same seeded instances.  One JSON line per run; one process per shape.

    python tools/time_pibt.py --batch 1024 --size 16 --agents 8  [--reps 200] [--episode-steps 64] [--once]
    python tools/time_pibt.py --batch 8192 --size 64 --agents 64
`--once`: a few calls of each kind and nothing else (for a kernel trace).
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from pogema_amd import GridConfig, PibtPolicy, VecPogema  # noqa: E402


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


def episode_isr(env, act, after_step, steps, seed):
    env.reset(seed=seed)
    isr = torch.zeros(env.batch, dtype=torch.float32, device=env.device)
    seen = torch.zeros(env.batch, dtype=torch.bool, device=env.device)   # the metrics row counts where the episode ENDS
    for _ in range(steps):
        _, rewards, _, _, infos = env.step(act(), compute_obs=False)
        after_step(rewards, infos["episode_done"])
        done = infos["episode_done"].to(torch.bool) & ~seen
        isr = torch.where(done, infos["metrics"][:, 0], isr)
        seen |= done
    return round(float(isr.mean()), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, required=True)
    ap.add_argument("--size", type=int, required=True)
    ap.add_argument("--agents", type=int, required=True)
    ap.add_argument("--radius", type=int, default=5)
    ap.add_argument("--density", type=float, default=0.3)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--episode-steps", type=int, default=64)
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    gc = GridConfig(size=args.size, num_agents=args.agents, obs_radius=args.radius, density=args.density, seed=0,
                    collision_system="soft", on_target="finish", max_episode_steps=args.episode_steps)
    env = VecPogema(gc, batch=args.batch, auto_reset=False)
    env.reset(seed=0)
    B, A = env.batch, env.num_agents
    prio = torch.zeros((B, A), dtype=torch.int32, device=env.device)
    out_p = (torch.empty((B, A), dtype=torch.int64, device=env.device), torch.empty((B, A, 2), dtype=torch.int32, device=env.device))
    out_e = (torch.empty((B, A), dtype=torch.int64, device=env.device), torch.empty((B, A), dtype=torch.int32, device=env.device))
    out_c = torch.empty((B, A, env.window, env.window), dtype=torch.int32, device=env.device)
    env.pibt_actions(priority=prio, out=out_p)      # allocates and fills the cache
    torch.cuda.synchronize()
    if args.once:
        for _ in range(3):
            env.pibt_actions(priority=prio, out=out_p)
            env.expert_actions(out=out_e)
            env.cost_to_go(out=out_c)
        torch.cuda.synchronize()
        env.close()
        return
    stay = torch.zeros((B, A), dtype=torch.int64, device=env.device)   # step() that leaves the state as it is
    res = {"shape": {"batch": B, "size": args.size, "agents": A, "obs_radius": args.radius, "density": args.density},
           "builds_before": env.cost_to_go_builds}
    res["pibt_actions_us"] = timed(lambda: env.pibt_actions(priority=prio, out=out_p), args.reps)
    res["expert_actions_us"] = timed(lambda: env.expert_actions(out=out_e), args.reps)
    res["cost_to_go_us"] = timed(lambda: env.cost_to_go(out=out_c), args.reps)
    res["step_us"] = timed(lambda: env.step(stay), args.reps)
    res["step_no_obs_us"] = timed(lambda: env.step(stay, compute_obs=False), args.reps)
    res["builds_after"] = env.cost_to_go_builds         # equal: every timed planner call ran on a warm cache
    policy = PibtPolicy(env)
    res["isr_pibt"] = episode_isr(env, lambda: policy.act()[0], policy.update, args.episode_steps, 1)
    res["isr_expert"] = episode_isr(env, lambda: env.expert_actions()[0], lambda *_: None, args.episode_steps, 1)
    env.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
