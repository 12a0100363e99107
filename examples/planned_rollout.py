#!/usr/bin/env python3
"""Planner-driven episodes in chunks: PibtPolicy.plan(K) looks K steps ahead in one launch (pibt_plan(), docs/SPEC.md
S16), rollout(actions) runs the K steps in one launch, and the next plan starts from where the rollout ended -- two
calls per K steps.  The individual success rate (ISR) is printed next to that of examples/pibt_rollout.py's loop (one
pibt_actions(), one step() and one priority update per step) on the same seeded instances; under `soft` / `finish` the
two follow the same trajectories, so the rates are equal.

    python examples/planned_rollout.py [--envs 1024] [--agents 32] [--size 32] [--density 0.3] [--steps 128] [--horizon 16]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from pogema_amd import GridConfig, PibtPolicy, VecPogema  # noqa: E402
from pibt_rollout import episode_isr  # noqa: E402  (the per-step loop, next to this file)


def planned_episode_isr(env, policy, steps, horizon, seed):
    """Mean ISR over the envs after one episode of `steps` steps, planned and rolled out `horizon` steps at a time."""
    env.reset(seed=seed)
    policy.reset()
    isr = torch.zeros(env.batch, dtype=torch.float32, device=env.device)
    seen = torch.zeros(env.batch, dtype=torch.bool, device=env.device)   # the metrics row counts where the episode ENDS
    for t0 in range(0, steps, horizon):
        actions, _, _ = policy.plan(min(horizon, steps - t0))
        out = env.rollout(actions, obs_slots=0)
        for done, metrics in zip(out["episode_done"], out["metrics"]):
            first = done & ~seen
            isr = torch.where(first, metrics[:, 0], isr)
            seen |= first
        # the plan does not know that an episode ended: those envs start over with equal priorities
        policy.priority[out["episode_done"].any(dim=0)] = 0
    return float(isr.mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--agents", type=int, default=32)
    ap.add_argument("--size", type=int, default=32)
    ap.add_argument("--density", type=float, default=0.3)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--horizon", type=int, default=16)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    gc = GridConfig(size=args.size, num_agents=args.agents, obs_radius=5, density=args.density, seed=args.seed,
                    collision_system="soft", on_target="finish", max_episode_steps=args.steps)
    env = VecPogema(gc, batch=args.envs, auto_reset=False)
    policy = PibtPolicy(env)
    planned = planned_episode_isr(env, policy, args.steps, args.horizon, args.seed)
    policy.reset()
    stepped = episode_isr(env, lambda: policy.act()[0], policy.update, args.steps, args.seed)
    calls = 2 * -(-args.steps // args.horizon)
    print(f"{args.envs} envs, {args.agents} agents on {args.size}x{args.size}, density {args.density}, {args.steps} steps")
    print(f"ISR plan({args.horizon}) + rollout(): {planned:.4f} in {calls} calls   "
          f"ISR pibt_actions() + step() per step: {stepped:.4f} in {3 * args.steps} calls")
    env.close()


if __name__ == "__main__":
    main()
