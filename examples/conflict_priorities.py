#!/usr/bin/env python
"""Conflict-based priorities (path_conflicts(), docs/SPEC.md S26) for the collision shield, next to no priorities.

A stand-in policy scores the four moves by goal_directions()' centre cell and samples with Gumbel noise, as in
examples/shielded_policy.py; shield_actions() makes the sampled actions jointly collision-free.  One rollout shields
with `priority=None` (all agents equal), one with `priority=count`: the number of conflicts the agent's own shortest path
has with the other agents' over the next K steps -- path_conflicts() on agent_forecasts()' cells, one launch each.  Both
run on seeded twin instances with the same noise; the script prints how many agents and episodes each solves and claims
nothing about which is better.

    python examples/conflict_priorities.py [--envs 256] [--agents 32] [--size 16] [--density 0.2] [--steps 64] [--ahead 8]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pogema_amd import GridConfig, VecPogema  # noqa: E402


def sampled_scores(env, gen, temperature):
    """[batch, agents, 5] float32: logits (2 for a move towards the target, 0 otherwise) plus Gumbel noise."""
    r = env.window // 2
    towards = env.goal_directions(format="float32")[:, :, :, r, r]                 # [B, A, 4]
    logits = torch.cat([torch.zeros_like(towards[..., :1]), 2.0 * towards], dim=-1)
    u = torch.rand(logits.shape, generator=gen, device=env.device).clamp_(1e-9, 1.0 - 1e-7)
    return logits / temperature - torch.log(-torch.log(u))


def rollout(gc, args, by_conflicts):
    env = VecPogema(gc, batch=args.envs, auto_reset=False)
    env.reset(seed=args.seed)
    gen = torch.Generator(device=env.device).manual_seed(args.seed)        # the same noise in both rollouts
    conflicts = torch.zeros((), dtype=torch.int64, device=env.device)
    for _ in range(args.steps):
        scores = sampled_scores(env, gen, args.temperature)
        first_step, partner, kind, count = env.path_conflicts(steps=args.ahead)
        conflicts += count.sum()
        actions, _, _ = env.shield_actions(scores, priority=count if by_conflicts else None)
        env.step(actions)
    active = env.get_state()["is_active"]
    finished, solved = int((~active).sum()), int((~active).all(1).sum())
    env.close()
    return finished, solved, int(conflicts) / args.steps


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--agents", type=int, default=32)
    ap.add_argument("--size", type=int, default=16)
    ap.add_argument("--density", type=float, default=0.2)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--ahead", type=int, default=8)
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    gc = GridConfig(size=args.size, num_agents=args.agents, density=args.density, obs_radius=5, seed=args.seed,
                    collision_system="soft", on_target="finish", max_episode_steps=args.steps)
    total = args.envs * args.agents
    for name, by_conflicts in (("priority=None", False), ("priority=count", True)):
        finished, solved, conflicts = rollout(gc, args, by_conflicts)
        print(f"{name:15s} finished agents {finished:6d} / {total}   solved envs {solved:5d} / {args.envs}   "
              f"conflicts ahead per step {conflicts:9.1f}")


if __name__ == "__main__":
    main()
